// Raw-limb test hooks for the field tower (fp.hpp, tower.hpp, pairing.hpp's fp12_pow_zabs): one operation per op
// code on operands given as 14 little-endian 28-bit limb words per Fp value, results written the same way.  Nothing
// is converted, reduced or range-checked on the way in, so a test can hand every function the edges of its operand
// contract: redundant representatives above p, un-normalized limb sums, the lazy subtraction's borrowed limbs.
// ONE dispatch for both builds: the device kernel (k_tower_debug.hip, blsgpu_debug_op ops 32..68) and the host build
// (tests/native/emu.cpp emu_tower_op) run this same function, so the records of tests/tower_vectors.py mean the same
// on both.
// Fp2 = (c0, c1), Fp6 = (c0, c1, c2), Fp12 = (c0, c1) in tower order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...).
#pragma once
#include "pairing.hpp"

#define TWR_OP_FIRST 32
#define TWR_OP_LAST 68

BLS_INL fp twr_ld(const uint32_t* w, int k) {
  fp x;
#pragma unroll
  for (int i = 0; i < BLS_NL; i++) x.l[i] = w[BLS_NL * k + i];
  return x;
}
BLS_INL fp2 twr_ld2(const uint32_t* w, int k) { return fp2_make(twr_ld(w, k), twr_ld(w, k + 1)); }
BLS_INL fp6 twr_ld6(const uint32_t* w, int k) { return fp6_make(twr_ld2(w, k), twr_ld2(w, k + 2), twr_ld2(w, k + 4)); }
BLS_INL fp12 twr_ld12(const uint32_t* w, int k) { return fp12_make(twr_ld6(w, k), twr_ld6(w, k + 6)); }
BLS_INL void twr_st(uint32_t* o, int k, const fp& x) {
#pragma unroll
  for (int i = 0; i < BLS_NL; i++) o[BLS_NL * k + i] = x.l[i];
}
BLS_INL void twr_st2(uint32_t* o, int k, const fp2& x) {
  twr_st(o, k, x.c0);
  twr_st(o, k + 1, x.c1);
}
BLS_INL void twr_st6(uint32_t* o, int k, const fp6& x) {
  twr_st2(o, k, x.c0);
  twr_st2(o, k + 2, x.c1);
  twr_st2(o, k + 4, x.c2);
}
BLS_INL void twr_st12(uint32_t* o, int k, const fp12& x) {
  twr_st6(o, k, x.c0);
  twr_st6(o, k + 6, x.c1);
}

// in: the op's operands; out: its results; returns the status word (a predicate's answer, fp2_sqrt's flag, else 0;
// -2 for an unknown op).  `op` is uniform over a launch, so the switch does not diverge.
BLS_INL int tower_debug_op(int op, const uint32_t* w, uint32_t* o) {
  int st = 0;
  switch (op) {
    // ---- Montgomery products at their operand contracts
    case 32: twr_st(o, 0, fp_mul(twr_ld(w, 0), twr_ld(w, 1))); break;
    case 33: twr_st(o, 0, fp_sqr(twr_ld(w, 0))); break;
    case 34: twr_st2(o, 0, fp2_mul(twr_ld2(w, 0), twr_ld2(w, 2))); break;
    case 35: twr_st2(o, 0, fp2_sqr(twr_ld2(w, 0))); break;
    case 36: twr_st2(o, 0, fp2_mul_fp(twr_ld2(w, 0), twr_ld(w, 2))); break;
    // ---- additive glue on stored values in [0, 2p]
    case 37: twr_st(o, 0, fp_add(twr_ld(w, 0), twr_ld(w, 1))); break;
    case 38: twr_st(o, 0, fp_sub(twr_ld(w, 0), twr_ld(w, 1))); break;
    case 39: twr_st(o, 0, fp_neg(twr_ld(w, 0))); break;
    case 40: twr_st(o, 0, fp_dbl(twr_ld(w, 0))); break;
    case 41: twr_st(o, 0, fp_half(twr_ld(w, 0))); break;
    case 42: twr_st(o, 0, fp_mul3(twr_ld(w, 0))); break;
    case 43: twr_st(o, 0, fp_mul4(twr_ld(w, 0))); break;
    case 44: twr_st(o, 0, fp_mul8(twr_ld(w, 0))); break;
    case 45: twr_st(o, 0, fp_canon(twr_ld(w, 0))); break;
    case 46: twr_st(o, 0, fp_add_norm(twr_ld(w, 0), twr_ld(w, 1))); break;
    case 47: twr_st2(o, 0, fp2_mul_xi(twr_ld2(w, 0))); break;
    // ---- predicates (answer in the status word)
    case 48: st = fp_is_zero(twr_ld(w, 0)) ? 1 : 0; break;
    case 49: st = fp_eq(twr_ld(w, 0), twr_ld(w, 1)) ? 1 : 0; break;
    case 50: st = fp12_is_one(twr_ld12(w, 0)) ? 1 : 0; break;
    // ---- inversions and roots
    case 51: twr_st(o, 0, fp_inv(twr_ld(w, 0))); break;
    case 52: twr_st(o, 0, fp_pow_p34(twr_ld(w, 0))); break;
    case 53: twr_st2(o, 0, fp2_inv(twr_ld2(w, 0))); break;
    case 54: twr_st6(o, 0, fp6_inv(twr_ld6(w, 0))); break;
    case 55: twr_st12(o, 0, fp12_inv(twr_ld12(w, 0))); break;
    case 56: {
      fp2 r;
      st = fp2_sqrt(twr_ld2(w, 0), r) ? 1 : 0;
      twr_st2(o, 0, r);
      break;
    }
    // ---- Fp6 / Fp12
    case 57: twr_st6(o, 0, fp6_mul(twr_ld6(w, 0), twr_ld6(w, 6))); break;
    case 58: twr_st6(o, 0, fp6_mul_by_01(twr_ld6(w, 0), twr_ld2(w, 6), twr_ld2(w, 8))); break;
    case 59: twr_st6(o, 0, fp6_mul_by_12(twr_ld6(w, 0), twr_ld2(w, 6), twr_ld2(w, 8))); break;
    case 60: twr_st12(o, 0, fp12_mul(twr_ld12(w, 0), twr_ld12(w, 12))); break;
    case 61: twr_st12(o, 0, fp12_sqr(twr_ld12(w, 0))); break;
    case 62: twr_st12(o, 0, fp12_mul_by_014(twr_ld12(w, 0), twr_ld2(w, 12), twr_ld2(w, 14), twr_ld2(w, 16))); break;
    case 63:  // f, then the two lines (a0, a1, a4), (b0, b1, b4)
      twr_st12(o, 0, fp12_mul_by_line2(twr_ld12(w, 0), line_pair(twr_ld2(w, 12), twr_ld2(w, 14), twr_ld2(w, 16),
                                                                 twr_ld2(w, 18), twr_ld2(w, 20), twr_ld2(w, 22))));
      break;
    case 64: twr_st12(o, 0, fp12_frob1(twr_ld12(w, 0))); break;
    case 65: twr_st12(o, 0, fp12_frob2(twr_ld12(w, 0))); break;
    case 66: twr_st12(o, 0, fp12_conj(twr_ld12(w, 0))); break;
    case 67: twr_st12(o, 0, fp12_pow_zabs(twr_ld12(w, 0))); break;
    case 68: twr_st12(o, 0, fp12_cyclotomic_sqr(twr_ld12(w, 0))); break;
    default: st = -2;
  }
  return st;
}
