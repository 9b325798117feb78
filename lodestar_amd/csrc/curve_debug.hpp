// Raw-limb test hooks for the point formulas (curve.hpp, ops.hpp's g1_in_subgroup): one function per op code on
// operands given as 14 limb words per Fp value, exactly as tower_debug.hpp takes them -- nothing is converted, reduced
// or range-checked on the way in, so a test can hand the formulas Z != 1, redundant representatives, infinity as
// z = p or 2p, and points that drive them through the branches only adversarial inputs take (P = Q, P = -Q, infinity).
// ONE dispatch for both builds: the device kernel (k_curve_debug.hip, blsgpu_debug_op ops 69..107) and the host build
// (tests/native/emu.cpp emu_curve_op) run this same function on the records of tests/curve_vectors.py.
// A Jacobian point is (x, y, z), an affine point (x, y): 3 / 2 Fp values on G1, 6 / 4 on G2 (Fp2 = (c0, c1)).
// Every body is called by name, so one build tests the lazy and the eager formulas whatever BLS_LAZY_CURVE selects.
#pragma once
#include "ops.hpp"
#include "tower_debug.hpp"

#define CRV_OP_FIRST 69
#define CRV_OP_G1 69  // + the group-generic sub-op below
#define CRV_OP_G2 86
#define CRV_OP_LAST 107

// Fp values per coordinate, and the coordinate loads / stores, per field
template <class F>
struct crv_io;
template <>
struct crv_io<fp> {
  static constexpr int N = 1;
};
template <>
struct crv_io<fp2> {
  static constexpr int N = 2;
};
BLS_INL void crv_ld(const uint32_t* w, int k, fp& x) { x = twr_ld(w, k); }
BLS_INL void crv_ld(const uint32_t* w, int k, fp2& x) { x = twr_ld2(w, k); }
BLS_INL void crv_st(uint32_t* o, int k, const fp& x) { twr_st(o, k, x); }
BLS_INL void crv_st(uint32_t* o, int k, const fp2& x) { twr_st2(o, k, x); }
// k counts coordinates, not Fp values
template <class F>
BLS_INL jac<F> crv_ldj(const uint32_t* w, int k) {
  jac<F> p;
  crv_ld(w, crv_io<F>::N * k, p.x);
  crv_ld(w, crv_io<F>::N * (k + 1), p.y);
  crv_ld(w, crv_io<F>::N * (k + 2), p.z);
  return p;
}
template <class F>
BLS_INL aff<F> crv_lda(const uint32_t* w, int k) {
  aff<F> p;
  crv_ld(w, crv_io<F>::N * k, p.x);
  crv_ld(w, crv_io<F>::N * (k + 1), p.y);
  return p;
}
template <class F>
BLS_INL void crv_stj(uint32_t* o, const jac<F>& p) {
  crv_st(o, 0, p.x);
  crv_st(o, crv_io<F>::N, p.y);
  crv_st(o, crv_io<F>::N * 2, p.z);
}
template <class F>
BLS_INL void crv_sta(uint32_t* o, const aff<F>& p) {
  crv_st(o, 0, p.x);
  crv_st(o, crv_io<F>::N, p.y);
}

// the sub-ops both groups have: G1 at 69 + sub, G2 at 86 + sub
template <class F>
BLS_INL int curve_group_op(int sub, const uint32_t* w, uint32_t* o) {
  int st = 0;
  switch (sub) {
    case 0: crv_stj(o, jac_dbl(crv_ldj<F>(w, 0))); break;
    case 1: crv_stj(o, jac_dbl_lazy(crv_ldj<F>(w, 0))); break;
    case 2: crv_stj(o, jac_dbl_eager(crv_ldj<F>(w, 0))); break;
    case 3: crv_stj(o, jac_add(crv_ldj<F>(w, 0), crv_ldj<F>(w, 3))); break;
    case 4: crv_stj(o, jac_add_lazy(crv_ldj<F>(w, 0), crv_ldj<F>(w, 3))); break;
    case 5: crv_stj(o, jac_add_eager(crv_ldj<F>(w, 0), crv_ldj<F>(w, 3))); break;
    case 6: crv_stj(o, jac_add_aff(crv_ldj<F>(w, 0), crv_lda<F>(w, 3))); break;
    case 7: crv_stj(o, jac_add_aff_lazy(crv_ldj<F>(w, 0), crv_lda<F>(w, 3))); break;
    case 8: crv_stj(o, jac_add_aff_eager(crv_ldj<F>(w, 0), crv_lda<F>(w, 3))); break;
    case 9: crv_stj(o, jac_neg(crv_ldj<F>(w, 0))); break;
    case 10: st = jac_is_inf(crv_ldj<F>(w, 0)) ? 1 : 0; break;
    case 11: st = jac_eq(crv_ldj<F>(w, 0), crv_ldj<F>(w, 3)) ? 1 : 0; break;
    case 12: {  // status = the returned flag; the affine point is written only when it is set
      aff<F> a;
      st = jac_to_aff(crv_ldj<F>(w, 0), a) ? 1 : 0;
      if (st) crv_sta(o, a);
      break;
    }
    case 13: crv_stj(o, endo_lambda(crv_ldj<F>(w, 0))); break;
    case 14: crv_stj(o, jac_mul_zabs(crv_ldj<F>(w, 0))); break;
    default: st = -2;
  }
  return st;
}

// in: the op's operands; out: its results; returns the status word (a predicate's answer, jac_to_aff's flag, else 0;
// -2 for an unknown op).  `op` is uniform over a launch; the branches inside the formulas are not.
BLS_INL int curve_debug_op(int op, const uint32_t* w, uint32_t* o) {
  if (op >= CRV_OP_G1 && op < CRV_OP_G1 + 15) return curve_group_op<fp>(op - CRV_OP_G1, w, o);
  if (op >= CRV_OP_G2 && op < CRV_OP_G2 + 15) return curve_group_op<fp2>(op - CRV_OP_G2, w, o);
  int st = 0;
  switch (op) {
    case 84: st = g1_on_curve(crv_lda<fp>(w, 0)) ? 1 : 0; break;
    case 85: st = g1_in_subgroup(crv_lda<fp>(w, 0)) ? 1 : 0; break;
    case 101: crv_stj(o, g2_psi(crv_ldj<fp2>(w, 0))); break;
    case 102: crv_stj(o, g2_psi2(crv_ldj<fp2>(w, 0))); break;
    // the loaders read the record's input words at every call, as the kernels' loaders read their SoA buffers
    case 103: crv_stj(o, jac_mul_zabs_ld<fp2>([&]() { return crv_ldj<fp2>(w, 0); })); break;
    case 104: crv_stj(o, jac_mul_zabs_lda<fp2>([&]() { return crv_lda<fp2>(w, 0); })); break;
    case 105: st = g2_on_curve(crv_lda<fp2>(w, 0)) ? 1 : 0; break;
    case 106: st = g2_in_subgroup(crv_lda<fp2>(w, 0)) ? 1 : 0; break;
    case 107: st = g2_in_subgroup_ld([&]() { return crv_lda<fp2>(w, 0); }) ? 1 : 0; break;
    default: st = -2;
  }
  return st;
}
