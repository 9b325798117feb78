// TEST HARNESS ONLY (tests/test_miller_segments.py): the step segments of the Miller accumulation on the host, from
// the device headers.  A chunk's segment values are computed as k_miller_acc computes them -- miller_acc_step over each
// segment's step range from f = 1, the stored lines of every item, conj(f) kept -- and folded by the Horner pass
// k_f_fold runs (pairing.hpp miller_seg_fold); the reference is the product of miller_loop over the chunk's pairs.
// Byte formats as tests/native/emu.cpp: canonical big-endian 48-byte Fp, P = x || y, Q = x.c1 || x.c0 || y.c1 || y.c0.
// With -DMILLER_SEGMENTS_MAIN it is a program over fixed multiples of the generators (for a sanitizer build).
#include <string.h>

#include "../../lodestar_amd/csrc/ops.hpp"
#include "../../lodestar_amd/csrc/miller_plan.hpp"

static_assert(miller_plan::kSteps == 68 && miller_plan::kZAbs == BLS_Z_ABS, "miller_plan.hpp follows the device loop");

static fp load_mont(const uint8_t* b) {
  fp x;
  fp_from_be48_plain(b, x, 0xff);
  return fp_to_mont(x);
}
static fp2 load2(const uint8_t* b) { return fp2_make(load_mont(b + 48), load_mont(b)); }
static void store12(const fp12& f, uint8_t* b) {  // canonical: fp_to_be48 leaves Montgomery form and reduces below p
  const fp2* t[6] = {&f.c0.c0, &f.c0.c1, &f.c0.c2, &f.c1.c0, &f.c1.c1, &f.c1.c2};
  for (int j = 0; j < 6; j++) {
    fp_to_be48(t[j]->c0, b + 96 * j);
    fp_to_be48(t[j]->c1, b + 96 * j + 48);
  }
}

extern "C" {

// pairs: n x (96-byte P, 192-byte Q); active[i] = 0 leaves item i out (as an excluded set of a chunk does).
// out_segs: J x 576 bytes, the stored segment values conj(g_j); out_fold / out_ref: 576 bytes each.
// Returns 0, or -1 for bad arguments.
int seg_chunk(const uint8_t* pairs, const uint8_t* active, uint32_t n, uint32_t J, uint8_t* out_segs, uint8_t* out_fold,
              uint8_t* out_ref) {
  if (n == 0 || n > 8 || J == 0 || J > miller_plan::kMaxSegments) return -1;
  static line3 L[8][MILLER_STEPS];
  g1a P[8];
  fp12 ref = fp12_one();
  for (uint32_t i = 0; i < n; i++) {
    const uint8_t* b = pairs + 288 * (size_t)i;
    P[i].x = load_mont(b);
    P[i].y = load_mont(b + 48);
    g2a Q;
    Q.x = load2(b + 96);
    Q.y = load2(b + 192);
    g2proj T;
    T.x = Q.x;
    T.y = Q.y;
    T.z = fp2_one();
    for (int s = 0; s < MILLER_STEPS; s++) {
      if (miller_step_is_add(s))
        miller_add_line(T, Q, L[i][s]);
      else
        miller_dbl_line(T, L[i][s]);
    }
    if (active[i]) ref = fp12_mul(ref, miller_loop(P[i], Q));
  }
  const miller_plan::Segments sg = miller_plan::segments(J);
  fp12 g[miller_plan::kMaxSegments];
  for (uint32_t j = 0; j < sg.n; j++) {
    fp12 f = fp12_one();
    const int s0 = (int)sg.first[j];
    for (int s = s0; s < (int)sg.first[j + 1]; s++) {
      const bool add = miller_step_is_add(s);
      if (!add && s != s0) f = fp12_sqr(f);  // one squaring per doubling step for the whole chunk, none at the first
      for (uint32_t i = 0; i < n; i++)
        if (active[i]) f = miller_acc_step(f, 0, true, L[i][s], P[i].x, P[i].y);  // the line product alone
    }
    g[j] = fp12_conj(f);
    store12(g[j], out_segs + 576 * (size_t)j);
  }
  store12(miller_seg_fold(sg.n, sg.dbl, [&](uint32_t j) { return g[j]; }), out_fold);
  store12(ref, out_ref);
  return 0;
}

// the same single pairing by miller_acc_step alone, as the issue states it (its own squaring rule, s relative to the
// segment's first step): one item, every J
int seg_single(const uint8_t* pair, uint32_t J, uint8_t* out_fold) {
  if (J == 0 || J > miller_plan::kMaxSegments) return -1;
  static line3 L[MILLER_STEPS];
  g1a P;
  P.x = load_mont(pair);
  P.y = load_mont(pair + 48);
  g2a Q;
  Q.x = load2(pair + 96);
  Q.y = load2(pair + 192);
  g2proj T;
  T.x = Q.x;
  T.y = Q.y;
  T.z = fp2_one();
  for (int s = 0; s < MILLER_STEPS; s++) {
    if (miller_step_is_add(s))
      miller_add_line(T, Q, L[s]);
    else
      miller_dbl_line(T, L[s]);
  }
  const miller_plan::Segments sg = miller_plan::segments(J);
  fp12 g[miller_plan::kMaxSegments];
  for (uint32_t j = 0; j < sg.n; j++) {
    fp12 f = fp12_one();
    for (int s = (int)sg.first[j]; s < (int)sg.first[j + 1]; s++)
      f = miller_acc_step(f, s - (int)sg.first[j], miller_step_is_add(s), L[s], P.x, P.y);
    g[j] = fp12_conj(f);
  }
  store12(miller_seg_fold(sg.n, sg.dbl, [&](uint32_t j) { return g[j]; }), out_fold);
  return 0;
}
}

#ifdef MILLER_SEGMENTS_MAIN
#include <stdio.h>
int main() {
  // P_i = (i + 2) g1, Q_i = H(32 bytes of i + 1)
  uint8_t pairs[3 * 288], active[3] = {1, 1, 1};
  for (int i = 0; i < 3; i++) {
    g1a g;
    g.x = G1_GEN_X;
    g.y = G1_GEN_Y;
    g1a Pa;
    g2a Qa;
    uint8_t msg[32];
    memset(msg, i + 1, sizeof msg);
    if (!jac_to_aff(jac_mul_u64(g, (uint64_t)i + 2), Pa)) return 2;
    if (!jac_to_aff(hash_to_g2_jac(msg), Qa)) return 2;
    g1a_to_be96(Pa, pairs + 288 * i);
    g2a_to_be192(Qa, pairs + 288 * i + 96);
  }
  static uint8_t segs[8 * 576], fold[576], ref[576];
  for (uint32_t J = 1; J <= 8; J++)
    for (uint32_t n = 1; n <= 3; n++) {
      if (seg_chunk(pairs, active, n, J, segs, fold, ref) || memcmp(fold, ref, 576)) {
        printf("mismatch at J = %u, %u pairs\n", J, n);
        return 1;
      }
    }
  printf("ok\n");
  return 0;
}
#endif
