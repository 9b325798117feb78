// The multi-lane engines' raw-limb test hooks on the device (blsgpu_debug_op ops 108..157 and 160..162, coop_debug.hpp).  One kernel
// per engine, each in the launch shape its production kernels use -- that shape is what these hooks are for:
//   k_coop_lane   op 108        128-lane blocks, one record per lane (lacc_fin)
//   k_coop_pair   ops 109..131, 160..162  128-lane blocks, one element per lane PAIR (k_miller, k_sig, k_msm); exit per pair
//   k_coop_g6     ops 132..141  one wave, ten groups of six lanes, lanes 60-63 leave at once (k_group_check6)
//   k_coop_g2c    ops 142..144  one wave, four 16-lane groups with their LDS areas (k_hash_clear_coop); a group whose
//                               element is flagged off runs every phase on arbitrary words and writes nothing
//   k_coop_gtw    ops 145..157  one element per 128-lane block, 192 lanes for the Miller loop (k_group's engine)
// A translation unit of its own with the default flags, like k_tower_debug.hip and k_curve_debug.hip: it checks the
// shared source, not the code objects of the stage kernels' units.
#include "k_common.hpp"
#include "coop_debug.hpp"

#define COOP_LANES 128
__global__ __launch_bounds__(COOP_LANES) void k_coop_lane(uint32_t n, const uint8_t* in, uint32_t in_stride,
                                                          uint8_t* out, uint32_t out_stride, int32_t* status) {
  const uint32_t i = blockIdx.x * COOP_LANES + threadIdx.x;
  if (i >= n) return;
  twr_st(reinterpret_cast<uint32_t*>(out + (size_t)i * out_stride), 0,
         coop_lacc_fin(reinterpret_cast<const uint32_t*>(in + (size_t)i * in_stride)));
  status[i] = 0;
}

__global__ __launch_bounds__(COOP_LANES) void k_coop_pair(int op, uint32_t n, const uint8_t* in, uint32_t in_stride,
                                                          uint8_t* out, uint32_t out_stride, int32_t* status) {
  const uint32_t q = blockIdx.x * COOP_LANES + threadIdx.x, i = q >> 1;
  if (i >= n) return;  // per pair: both lanes of an element leave together
  const int st = coop_pair_op(op, reinterpret_cast<const uint32_t*>(in + (size_t)i * in_stride),
                              reinterpret_cast<uint32_t*>(out + (size_t)i * out_stride));
  if ((q & 1) == 0) status[i] = st;
}

__global__ __launch_bounds__(WAVE) void k_coop_g6(int op, uint32_t n, const uint8_t* in, uint32_t in_stride,
                                                  uint8_t* out, uint32_t out_stride, int32_t* status) {
  __shared__ uint32_t ln[W_LINE * ACC6_GROUPS];
  const uint32_t lane = threadIdx.x, grp = lane / 6, k = lane % 6;
  const uint32_t q = blockIdx.x * ACC6_GROUPS + grp;
  if (grp >= ACC6_GROUPS || q >= n) return;  // whole groups leave together; lanes 60-63 always
  const G6 g{(int)(grp * 6), k};
  const int st = coop_g6_op(op, reinterpret_cast<const uint32_t*>(in + (size_t)q * in_stride),
                            reinterpret_cast<uint32_t*>(out + (size_t)q * out_stride), ln, grp, g);
  if (k == 0) status[q] = st;
}

#define COOP_G2C_GROUPS (WAVE / G2C_LANES)  // k_hash.hip's HC_GROUPS
__global__ __launch_bounds__(WAVE) void k_coop_g2c(int op, uint32_t n, const uint8_t* in, uint32_t in_stride,
                                                   uint8_t* out, uint32_t out_stride, int32_t* status) {
  __shared__ uint32_t lds[COOP_G2C_GROUPS * G2C_WORDS];
  const uint32_t tg = threadIdx.x % G2C_LANES, grp = threadIdx.x / G2C_LANES;
  const uint32_t u = blockIdx.x * COOP_G2C_GROUPS + grp;
  const bool inb = u < n;
  // (an element past the end reads element 0's words: in bounds, and never live)
  const uint32_t* w = reinterpret_cast<const uint32_t*>(in + (size_t)(inb ? u : 0) * in_stride);
  const bool on = inb && w[0] != 0;
  uint32_t* g = lds + grp * G2C_WORDS;
  const uint32_t* pw = w + BLS_NL;  // the point, then the addend
  // an off group's whole area holds the element's input words (whatever the record put there), over and over
  if (!on)
    for (uint32_t i = tg; i < G2C_WORDS; i += G2C_LANES) g[i] = w[i % (COOP_G2C_IN_FPS * BLS_NL)];
  if (on && tg == 0) {
    g2c_st_point(g, crv_ldj<fp2>(pw, 0));
    if (op == 143) g2c_st_q(g, crv_ldj<fp2>(pw, 3));
  }
  g2c_sync();
  coop_g2c_op(op, g, tg, on, pw);
  if (on && tg == 0) {
    crv_stj(reinterpret_cast<uint32_t*>(out + (size_t)u * out_stride), g2c_ld_point(g));
    status[u] = 0;
  }
}

__global__ __launch_bounds__(GTW_MILLER_LANES) void k_coop_gtw(int op, const uint8_t* in, uint32_t in_stride, uint8_t* out,
                                                               uint32_t out_stride, int32_t* status) {
  __shared__ GtwLds sh;
  const uint32_t i = blockIdx.x, t = threadIdx.x;
  const uint32_t* w = reinterpret_cast<const uint32_t*>(in + (size_t)i * in_stride);
  uint32_t* o = reinterpret_cast<uint32_t*>(out + (size_t)i * out_stride);
  uint32_t* res = sh.F;
  if (op == COOP_OP_GTW_MILLER) {  // P = (x, y), Q = (x0, x1, y0, y1)
    if (t < 4) lds_st(sh.QA, (int)t, twr_ld(w, 2 + (int)t));
    gtw_sync();
    gtw_miller_loop(sh.F, sh.QA, twr_ld(w, 0), twr_ld(w, 1), sh.TB, sh.L, sh.L1, sh.S, sh.S2, t);
  } else {
    // operands into LDS in the w-basis by the lanes t < 12 (gtw_from_reg's mapping)
    if (t < 12) {
      lds_st(sh.F, (int)t, twr_ld(w, coop_tower_fp((int)t)));
      if (op >= 145 && op <= 147) lds_st(sh.G, (int)t, twr_ld(w, 12 + coop_tower_fp((int)t)));
      if (op == 149) {  // a line: w-coefficients 0, 2, 3; the others hold words nothing may read
        const int k = (int)t >> 1, c = (int)t & 1;
        fp v;
#pragma unroll
        for (int l = 0; l < BLS_NL; l++) v.l[l] = 0xFFFFFFFFu;
        if (k == 0 || k == 2 || k == 3) v = twr_ld(w, 12 + (k == 0 ? 0 : k == 2 ? 2 : 4) + c);
        lds_st(sh.G, (int)t, v);
      }
    }
    gtw_sync();
    res = coop_gtw_op(op, sh.F, sh.G, sh.L, sh.W, sh.S, t);
  }
  if (t < 12) twr_st(o, coop_tower_fp((int)t), lds_ld(res, (int)t));
  if (t == 0) status[i] = 0;
}

void launch_debug_coop(int op, uint32_t n, const uint8_t* in, uint32_t in_stride, uint8_t* out, uint32_t out_stride,
                       int32_t* status, hipStream_t s) {
  if (!n) return;
  if (op == COOP_OP_LACC)
    hipLaunchKernelGGL(k_coop_lane, dim3((n + COOP_LANES - 1) / COOP_LANES), dim3(COOP_LANES), 0, s, n, in, in_stride,
                       out, out_stride, status);
  else if (op <= COOP_OP_PAIR_LAST || (op >= COOP_OP_PAIR2 && op <= COOP_OP_PAIR2_LAST))
    hipLaunchKernelGGL(k_coop_pair, dim3((2 * n + COOP_LANES - 1) / COOP_LANES), dim3(COOP_LANES), 0, s, op, n, in,
                       in_stride, out, out_stride, status);
  else if (op <= COOP_OP_G6_LAST)
    hipLaunchKernelGGL(k_coop_g6, dim3((n + ACC6_GROUPS - 1) / ACC6_GROUPS), dim3(WAVE), 0, s, op, n, in, in_stride, out,
                       out_stride, status);
  else if (op <= COOP_OP_G2C_LAST)
    hipLaunchKernelGGL(k_coop_g2c, dim3((n + COOP_G2C_GROUPS - 1) / COOP_G2C_GROUPS), dim3(WAVE), 0, s, op, n, in,
                       in_stride, out, out_stride, status);
  else
    hipLaunchKernelGGL(k_coop_gtw, dim3(n), dim3(op == COOP_OP_GTW_MILLER ? GTW_MILLER_LANES : GTW_LANES), 0, s, op, in,
                       in_stride, out, out_stride, status);
}
