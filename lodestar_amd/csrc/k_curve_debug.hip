// The point formulas' raw-limb test hooks on the device (blsgpu_debug_op ops 69..107, curve_debug.hpp): one record per
// lane, in = k x 56 bytes of limb words, out = m x 56 bytes, the predicate / flag in status.  A translation unit of its
// own beside k_tower_debug.hip (the two compile in parallel), with the default flags: it checks the shared source, the
// register-ABI product calls and the per-lane LDS slot under lanes of one wave that take different branches of
// jac_add / jac_add_aff (a nested jac_dbl next to the generic path) -- not the code objects of the stage kernels' units.
#include "k_common.hpp"
#include "curve_debug.hpp"

// 128-lane workgroups: the full width bls_fp2_arg is sized for
#define CRV_LANES 128
#ifdef BLS_FP2_LDS_LANES  // (the slot exists only in the device pass of the default build: tower.hpp)
static_assert(CRV_LANES == BLS_FP2_LDS_LANES, "the curve hooks run at the Fp2 argument slot's full width");
#endif
__global__ __launch_bounds__(CRV_LANES) void k_debug_curve(int op, uint32_t n, const uint8_t* in, uint32_t in_stride,
                                                           uint8_t* out, uint32_t out_stride, int32_t* status) {
  const uint32_t i = blockIdx.x * CRV_LANES + threadIdx.x;
  if (i >= n) return;
  // strides are multiples of 4 and at least the op's element (checked in blsgpu_debug_op)
  status[i] = curve_debug_op(op, reinterpret_cast<const uint32_t*>(in + (size_t)i * in_stride),
                             reinterpret_cast<uint32_t*>(out + (size_t)i * out_stride));
}

void launch_debug_curve(int op, uint32_t n, const uint8_t* in, uint32_t in_stride, uint8_t* out, uint32_t out_stride,
                        int32_t* status, hipStream_t s) {
  if (!n) return;
  hipLaunchKernelGGL(k_debug_curve, dim3((n + CRV_LANES - 1) / CRV_LANES), dim3(CRV_LANES), 0, s,
                     op, n, in, in_stride, out, out_stride, status);
}
