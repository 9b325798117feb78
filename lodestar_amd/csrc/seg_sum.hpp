// Combiners of the segmented sums (k_sigagg.hip: signatures in G2; k_awr.hip: r pk in G1 and r sig in G2): the lanes
// of a group each hold a Jacobian partial sum and the first error they met (lowest element index, its code); these
// fold them into lane 0 of the group.  Templated over the coordinate field F (fp: G1, fp2: G2).
#pragma once
#include "k_common.hpp"

#define SEG_SLOTS (WAVE / 2)

// The group's first error of a wave-per-group kernel: the lowest index over the wave's lanes, taken by lane 0 through
// LDS (err_k / err_c: WAVE entries each; the barrier also orders them before the tree's slots).
BLS_INL void seg_wave_first_error(uint32_t* err_k, int32_t* err_c, uint32_t lane, uint32_t my_err_k, int my_err,
                                  uint32_t& bk, int& bc) {
  err_k[lane] = my_err_k;
  err_c[lane] = my_err;
  __syncthreads();
  bk = 0xffffffffu;
  bc = 0;
  if (lane == 0) {
    for (int l = 0; l < WAVE; l++)
      if (err_k[l] < bk) {
        bk = err_k[l];
        bc = err_c[l];
      }
  }
}

// One wave per group, LDS tree: level s, lanes [s, 2s) hand their sum to lanes [0, s), so SEG_SLOTS slots of
// sizeof(jac<F>) / 4 words (G2: 10.5 KB, G1: 5.25 KB).  Lane 0 ends with the sum.  Every lane of the wave calls it.
template <class F>
BLS_INL void seg_wave_tree(jac<F>& acc, uint32_t* red, uint32_t lane) {
  constexpr int W = sizeof(jac<F>) / 4;
#pragma unroll 1
  for (int s = WAVE / 2; s >= 1; s >>= 1) {
    if (lane >= (uint32_t)s && lane < (uint32_t)(2 * s)) {
      uint32_t* o = red + (lane - s) * W;
      const uint32_t* a = reinterpret_cast<const uint32_t*>(&acc);
#pragma unroll
      for (int w = 0; w < W; w++) o[w] = a[w];
    }
    __syncthreads();
    if (lane < (uint32_t)s) {
      jac<F> o;
      uint32_t* d = reinterpret_cast<uint32_t*>(&o);
      const uint32_t* a = red + lane * W;
#pragma unroll
      for (int w = 0; w < W; w++) d[w] = a[w];
      acc = jac_add(acc, o);
    }
    __syncthreads();
  }
}

// L lanes per group (L = 32, 16, 8 or 1 divides WAVE, so a group never straddles a wave): an in-register butterfly
// (__shfl_xor inside the lane group: one point per level, no LDS, no barrier).  After log2 L levels every lane of the
// group holds the sum and the first error by element index.  L = 1 does nothing.
template <class F>
BLS_INL jac<F> jac_shfl_xor(const jac<F>& p, int m) {
  constexpr int W = sizeof(jac<F>) / 4;
  jac<F> r;
  const uint32_t* a = reinterpret_cast<const uint32_t*>(&p);
  uint32_t* d = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int w = 0; w < W; w++) d[w] = (uint32_t)__shfl_xor((int)a[w], m);
  return r;
}
template <class F, int L>
BLS_INL void seg_butterfly(jac<F>& acc, uint32_t& my_err_k, int& my_err) {
#pragma unroll 1
  for (int m = L / 2; m >= 1; m >>= 1) {
    const jac<F> o = jac_shfl_xor(acc, m);
    const uint32_t ok = (uint32_t)__shfl_xor((int)my_err_k, m);
    const int oc = __shfl_xor(my_err, m);
    if (ok < my_err_k) {
      my_err_k = ok;
      my_err = oc;
    }
    acc = jac_add(acc, o);
  }
}
