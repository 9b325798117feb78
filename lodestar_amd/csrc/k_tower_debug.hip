// The field tower's raw-limb test hooks on the device (blsgpu_debug_op ops 32..68, tower_debug.hpp): one element per
// lane, in = k x 56 bytes of limb words, out = m x 56 bytes, the predicate / flag in status.  A translation unit of its
// own with the default flags, so it checks the shared source and the device call boundary (fp_mul_r, fp_sqr_r,
// fp2_mul_r, fp2_sqr_r, fp2_mul_fp_r and the per-lane LDS slot) under the product's compiler -- not the code objects
// of the stage kernels' units, which the whole-operation parity tests cover.
#include "k_common.hpp"
#include "tower_debug.hpp"

// 128-lane workgroups: the full width bls_fp2_arg is sized for, so lanes 64..127 of the slot carry live operands too
#define TWR_LANES 128
#ifdef BLS_FP2_LDS_LANES  // (the slot exists only in the device pass of the default build: tower.hpp)
static_assert(TWR_LANES == BLS_FP2_LDS_LANES, "the tower hooks run at the Fp2 argument slot's full width");
#endif
__global__ __launch_bounds__(TWR_LANES) void k_debug_tower(int op, uint32_t n, const uint8_t* in,
                                                                  uint32_t in_stride, uint8_t* out, uint32_t out_stride,
                                                                  int32_t* status) {
  const uint32_t i = blockIdx.x * TWR_LANES + threadIdx.x;
  if (i >= n) return;
  // strides are multiples of 4 and at least the op's element (checked in blsgpu_debug_op)
  status[i] = tower_debug_op(op, reinterpret_cast<const uint32_t*>(in + (size_t)i * in_stride),
                             reinterpret_cast<uint32_t*>(out + (size_t)i * out_stride));
}

void launch_debug_tower(int op, uint32_t n, const uint8_t* in, uint32_t in_stride, uint8_t* out, uint32_t out_stride,
                        int32_t* status, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_debug_tower, dim3((n + TWR_LANES - 1) / TWR_LANES), dim3(TWR_LANES), 0, s,
                     op, n, in, in_stride, out, out_stride, status);
}
