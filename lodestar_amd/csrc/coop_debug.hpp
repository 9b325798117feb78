// Raw-limb test hooks for the multi-lane engines: lacc_fin (lacc.hpp), the lane-pair forms (fp2x.hpp, gtx.hpp), the
// six-lane GT engine (gt6.hpp), the 16-lane cooperative G2 chains (g2_coop.hpp) and the workgroup GT engine
// (gt_wave.hpp).  Operands are 14 limb words per Fp value, exactly as tower_debug.hpp / curve_debug.hpp take them:
// nothing is converted, reduced or range-checked on the way in.  What differs from those hooks is the launch shape:
// every engine runs in the shape its production kernels use (k_coop_debug.hip), an element per lane PAIR, per group of
// SIX lanes, per group of 16 lanes (four per block) or per 128 / 192-lane block, so the cross-lane exchanges, the
// lane-dependent select tables, the pair-combined branch conditions, the LDS slots other lanes wrote and the barrier
// schedules are what is tested (blsgpu_debug_op ops 108..157 and 160..162; records: tests/coop_vectors.py).
// The host build (tests/native/emu.cpp emu_coop_op) runs the host-compilable subset lane by lane: lacc_fin, the g2c
// phases, gtw_mul_prod / gtw_mul_rec and the Miller schedule.  The lane-pair and six-lane ops are device-only.
//
// Fp2 = (c0, c1), Fp12 in tower order (c0.c0.c0, c0.c0.c1, c0.c1.c0, ...), Jacobian (x, y, z), affine (x, y).
#pragma once
#include "curve_debug.hpp"
#include "g2_coop.hpp"
#include "gt_wave.hpp"

#define COOP_OP_FIRST 108
#define COOP_OP_LACC 108      // lacc_fin: pos, neg limb sums (28 words) -> 14, one record per lane
#define COOP_OP_PAIR 109      // 109..131: lane pairs
#define COOP_OP_PAIR_LAST 131
#define COOP_OP_G6 132        // 132..141: six-lane groups
#define COOP_OP_G6_LAST 141
#define COOP_OP_G2C 142       // 142..144: 16-lane groups; element = flag slot (word 0: on), point, addend
#define COOP_OP_G2C_LAST 144
#define COOP_OP_GTW 145       // 145..157: one element per block
#define COOP_OP_GTW_MILLER 157
#define COOP_OP_LAST 157
// lane pairs again, for the chains' hot loop (158 and 159 stay unassigned: refused like every unknown op)
#define COOP_OP_PAIR2 160       // 160: jac_dbl n times (in: x, y, z, then a slot whose word 0 is n <= 64; uniform over a launch)
#define COOP_OP_PAIR2_LAST 162  // 161 / 162: the [|z|] chain, jac_mul_zabs_ld (Jacobian in) / jac_mul_zabs_lda (affine in)
#define COOP_G2C_IN_FPS 13    // Fp slots of a g2c element

BLS_INL fp coop_lacc_fin(const uint32_t* w) {
  lacc a;
#pragma unroll
  for (int i = 0; i < BLS_NL; i++) {
    a.pos[i] = w[i];
    a.neg[i] = w[BLS_NL + i];
  }
  return lacc_fin(a);
}

// tower Fp index of w-basis Fp index q = 2k + comp (gt_wave.hpp / gt6.hpp: coefficient k is the tower's Fp2 slot
// (c0.c0, c1.c0, c0.c1, c1.c1, c0.c2, c1.c2)[k])
BLS_INL int coop_tower_fp(int q) {
  const int k = q >> 1;
  return 2 * (((k & 1) ? 3 : 0) + (k >> 1)) + (q & 1);
}

// ---- the host-compilable subset, lane by lane (also what the device kernels' results are compared with on the host)
#if !defined(__HIPCC__)
static void coop_host_g2c_dbl(uint32_t* g) {
  for (uint32_t t = 0; t < G2C_LANES; t++) g2c_dbl_p1(g, t);
  for (uint32_t t = 0; t < G2C_LANES; t++) g2c_dbl_p2(g, t);
  for (uint32_t t = 0; t < G2C_LANES; t++) g2c_dbl_r1(g, t);
  for (uint32_t t = 0; t < G2C_LANES; t++) g2c_dbl_p3(g, t);
  for (uint32_t t = 0; t < G2C_LANES; t++) g2c_dbl_r2(g, t);
}
// C = A * B with the pointers as given (the aliasings of ops 145..148); S: 108 products
template <bool SPARSE>
static void coop_host_gtw_mul(uint32_t* C, const uint32_t* A, const uint32_t* B, uint32_t* S) {
  for (uint32_t t = 0; t < GTW_LANES; t++) gtw_mul_prod<SPARSE>(A, B, S, t);
  for (uint32_t t = 0; t < GTW_LANES; t++) gtw_mul_rec<SPARSE>(C, S, t);
}
static void coop_host_ld12(uint32_t* A, const uint32_t* w, int k0) {
  for (int q = 0; q < 12; q++) lds_st(A, q, twr_ld(w, k0 + coop_tower_fp(q)));
}
static void coop_host_st12(uint32_t* o, const uint32_t* A) {
  for (int q = 0; q < 12; q++) twr_st(o, coop_tower_fp(q), lds_ld(A, q));
}
// returns 0, or -2 for an op the host build does not have
static int coop_host_op(int op, const uint32_t* w, uint32_t* o) {
  static uint32_t A[GTW_FP12], B[GTW_FP12], C[GTW_FP12], S[108 * BLS_NL];
  switch (op) {
    case COOP_OP_LACC: twr_st(o, 0, coop_lacc_fin(w)); return 0;
    case 142:
    case 143:
    case 144: {
      uint32_t g[G2C_WORDS] = {};
      const uint32_t* pw = w + BLS_NL;  // (the flag slot first)
      g2c_st_point(g, crv_ldj<fp2>(pw, 0));
      if (op == 142) {
        coop_host_g2c_dbl(g);
      } else if (op == 143) {
        g2c_st_q(g, crv_ldj<fp2>(pw, 3));
        g2c_host_add(g);
      } else {
        const g2j r = g2c_host_mul_zabs(g2c_ld_point(g), [&] { return crv_ldj<fp2>(pw, 0); });
        g2c_st_point(g, r);
      }
      crv_stj(o, g2c_ld_point(g));
      return 0;
    }
    case 145:
    case 146:
    case 147:
    case 148: {
      coop_host_ld12(A, w, 0);
      if (op != 148) coop_host_ld12(B, w, 12);
      uint32_t* c = op == 145 ? C : (op == 147 ? B : A);
      coop_host_gtw_mul<false>(c, A, op == 148 ? A : B, S);
      coop_host_st12(o, c);
      return 0;
    }
    case 149: {
      coop_host_ld12(A, w, 0);
      for (int i = 0; i < GTW_FP12; i++) B[i] = 0xFFFFFFFFu;  // the w-coefficients a line does not have: never read
      for (int c = 0; c < 2; c++) {
        lds_st(B, 0 + c, twr_ld(w, 12 + c));
        lds_st(B, 4 + c, twr_ld(w, 14 + c));
        lds_st(B, 6 + c, twr_ld(w, 16 + c));
      }
      coop_host_gtw_mul<true>(C, A, B, S);
      coop_host_st12(o, C);
      return 0;
    }
    case COOP_OP_GTW_MILLER: {
      static uint32_t QA[4 * BLS_NL], TB[20 * BLS_NL], L0[GTW_FP12], L1[GTW_FP12], S2[28 * BLS_NL];
      for (int q = 0; q < 4; q++) lds_st(QA, q, twr_ld(w, 2 + q));
      gtw_miller_schedule(
          [&](auto&& phase) {
            for (uint32_t t = 0; t < GTW_MILLER_LANES; t++) phase(t);
          },
          A, QA, twr_ld(w, 0), twr_ld(w, 1), TB, L0, L1, S, S2);
      coop_host_st12(o, A);
      return 0;
    }
    default: return -2;
  }
}
#endif

// ---- device bodies -------------------------------------------------------------------------------------------
#if defined(__HIPCC__)
#include "gt6.hpp"
#include "gtx.hpp"

// lane pairs: Fp2 value j of the element, this lane's coefficient (fp2x_of's selection, from raw words)
BLS_INL fp2x px_ld(const uint32_t* w, int j) { return fp2x{twr_ld(w, 2 * j + (int)fp2x_k())}; }
BLS_INL void px_st(uint32_t* o, int j, const fp2x& v) { twr_st(o, 2 * j + (int)fp2x_k(), v.v); }
BLS_INL g2jx px_ldj(const uint32_t* w, int j) {
  g2jx p;
  p.x = px_ld(w, j);
  p.y = px_ld(w, j + 1);
  p.z = px_ld(w, j + 2);
  return p;
}
BLS_INL void px_stj(uint32_t* o, const g2jx& p) {
  px_st(o, 0, p.x);
  px_st(o, 1, p.y);
  px_st(o, 2, p.z);
}
BLS_INL fp6x px_ld6(const uint32_t* w, int j) {
  fp6x r;
  r.c0 = px_ld(w, j);
  r.c1 = px_ld(w, j + 1);
  r.c2 = px_ld(w, j + 2);
  return r;
}
BLS_INL void px_st6(uint32_t* o, int j, const fp6x& v) {
  px_st(o, j, v.c0);
  px_st(o, j + 1, v.c1);
  px_st(o, j + 2, v.c2);
}
// a predicate's answer on both lanes of the pair: bit 0 = lane 0's, bit 1 = lane 1's (0 or 3 when they agree)
BLS_INL int px_both(bool mine) {
  const uint32_t m = mine ? 1u : 0u, other = dpp_swap(m);
  return (int)(fp2x_k() ? (other | (m << 1)) : (m | (other << 1)));
}

// every lane of the pair calls it; each lane stores its own coefficient; returns the status word (the same on both)
BLS_INL int coop_pair_op(int op, const uint32_t* w, uint32_t* o) {
  int st = 0;
  switch (op) {
    case 109: px_st(o, 0, fp2x_mul(px_ld(w, 0), px_ld(w, 1))); break;
    case 110: px_st(o, 0, fp2x_sqr(px_ld(w, 0))); break;
    case 111: px_st(o, 0, fp2x_mul_xi(px_ld(w, 0))); break;
    case 112: px_st(o, 0, fp2x{fp2x_norm(px_ld(w, 0))}); break;  // (both lanes hold N(a): out = (N, N))
    case 113: st = px_both(F_is_zero(px_ld(w, 0))); break;
    // lc_xi as gtx.hpp instantiates it (d first, then the terms), and one at total weight 15
    case 114: px_st(o, 0, lc_xi<1>(px_ld(w, 0), L<1>(px_ld(w, 1)))); break;
    case 115: px_st(o, 0, lc_xi<1>(px_ld(w, 0), L<1>(px_ld(w, 1)), L<-1>(px_ld(w, 2)), L<-1>(px_ld(w, 3)))); break;
    case 116: px_st(o, 0, lc_xi<-1>(px_ld(w, 0), L<1>(px_ld(w, 1)), L<-1>(px_ld(w, 2)))); break;
    case 117: px_st(o, 0, lc_xi<1>(px_ld(w, 0), L<1>(px_ld(w, 1)), L<-1>(px_ld(w, 2)))); break;
    case 118: px_st(o, 0, lc_xi<3>(px_ld(w, 0), L<4>(px_ld(w, 1)), L<-5>(px_ld(w, 2)))); break;
    case 119: px_st6(o, 0, fp6x_mul(px_ld6(w, 0), px_ld6(w, 3))); break;
    case 120: {
      fp12x a;
      a.c0 = px_ld6(w, 0);
      a.c1 = px_ld6(w, 3);
      const fp12x r = fp12x_sqr(a);
      px_st6(o, 0, r.c0);
      px_st6(o, 3, r.c1);
      break;
    }
    case 121: {
      fp12x a;
      a.c0 = px_ld6(w, 0);
      a.c1 = px_ld6(w, 3);
      const fp12x r = fp12x_mul_by_014(a, px_ld(w, 6), px_ld(w, 7), px_ld(w, 8));
      px_st6(o, 0, r.c0);
      px_st6(o, 3, r.c1);
      break;
    }
    case 122:
    case 123: {  // out: R (x, y, z), then the line (l0, c1, c4)
      g2projx R;
      R.x = px_ld(w, 0);
      R.y = px_ld(w, 1);
      R.z = px_ld(w, 2);
      line3x Ln;
      if (op == 122) {
        miller_dbl_line(R, Ln);
      } else {
        aff<fp2x> Q;
        Q.x = px_ld(w, 3);
        Q.y = px_ld(w, 4);
        miller_add_line(R, Q, Ln);
      }
      px_st(o, 0, R.x);
      px_st(o, 1, R.y);
      px_st(o, 2, R.z);
      px_st(o, 3, Ln.l0);
      px_st(o, 4, Ln.c1);
      px_st(o, 5, Ln.c4);
      break;
    }
    case 124: px_stj(o, jac_dbl(px_ldj(w, 0))); break;
    case 125: px_stj(o, jac_add(px_ldj(w, 0), px_ldj(w, 3))); break;
    case 126: {
      aff<fp2x> Q;
      Q.x = px_ld(w, 3);
      Q.y = px_ld(w, 4);
      px_stj(o, jac_add_aff(px_ldj(w, 0), Q));
      break;
    }
    case 127: px_stj(o, jac_neg(px_ldj(w, 0))); break;
    case 128: st = px_both(jac_is_inf(px_ldj(w, 0))); break;
    case 129: px_stj(o, g2_psi(px_ldj(w, 0))); break;
    case 130: px_stj(o, g2_psi2(px_ldj(w, 0))); break;
    case 131: px_stj(o, jac_mul_zabs(px_ldj(w, 0))); break;
    case 160: {
      g2jx r = px_ldj(w, 0);
      const uint32_t n = w[6 * BLS_NL] < 64u ? w[6 * BLS_NL] : 64u;
#pragma unroll 1
      for (uint32_t i = 0; i < n; i++) r = jac_dbl(r);
      px_stj(o, r);
      break;
    }
    // the loaders read the record's input words at every call, as the kernels' loaders read their SoA buffers
    case 161: px_stj(o, jac_mul_zabs_ld<fp2x>([&]() { return px_ldj(w, 0); })); break;
    case 162:
      px_stj(o, jac_mul_zabs_lda<fp2x>([&]() {
               aff<fp2x> Q;
               Q.x = px_ld(w, 0);
               Q.y = px_ld(w, 1);
               return Q;
             }));
      break;
    default: st = -2;
  }
  return st;
}

// six lanes: lane g.k loads and stores w-coefficient k of the Fp12 whose first Fp is k0
BLS_INL fp2 g6_ld(const uint32_t* w, int k0, const G6& g) { return twr_ld2(w, k0 + coop_tower_fp(2 * (int)g.k)); }
// every lane of the group calls it; `ln`: an LDS area of W_LINE * ACC6_GROUPS words for g6_line_mul's line records;
// returns the status word (the same on the six lanes)
BLS_INL int coop_g6_op(int op, const uint32_t* w, uint32_t* o, uint32_t* ln, uint32_t grp, const G6& g) {
  int st = 0;
  const fp2 f = g6_ld(w, 0, g);
  fp2 r = f;
  switch (op) {
    case 132: r = g6_mul(f, g6_ld(w, 12, g), g); break;
    case 133: r = g6_sqr(f, g); break;
    case 134: r = g6_cyc_sqr(f, g); break;
    case 135: r = g6_frob(f, 1, g); break;
    case 136: r = g6_frob(f, 2, g); break;
    case 137: r = g6_conj(f, g); break;
    case 138: {
      // the line record (l0, c1, c4: 6 Fp) as column grp of an ACC6_GROUPS-column SoA, the layout ld_fp / ld_fp2 read
      // (the production lines buffer: nm columns, this message's column m); lane k moves Fp k.  The block is one wave
      // and `op` is uniform, so the barrier is met by every lane still running
      st_fp(ln, ACC6_GROUPS, grp, (int)g.k * W_FP, twr_ld(w, 12 + (int)g.k));
      __syncthreads();
      r = g6_line_mul(f, ln, ACC6_GROUPS, grp, twr_ld(w, 18), twr_ld(w, 19), g);
      break;
    }
    case 139: return g6_is_one(f, g) ? 1 : 0;
    case 140: r = g6_pow_z(f, g); break;
    case 141: r = g6_final_exp(f, g); break;
    default: return -2;
  }
  twr_st2(o, coop_tower_fp(2 * (int)g.k), r);
  return st;
}

// a g2c group's op (every lane of the block calls it: the barriers).  `g`: the group's LDS area, holding the point
// (and the addend) of a live group, arbitrary words of an off one; `pw`: the element's point words
__device__ __forceinline__ void coop_g2c_op(int op, uint32_t* g, uint32_t tg, bool on, const uint32_t* pw) {
  if (op == 142)
    g2c_dbl(g, tg);
  else if (op == 143)
    g2c_add(g, tg, on);
  else  // the loader reads the element's input words at every call (ops 103 / 104)
    g2c_mul_zabs(g, tg, on, [&] { return crv_ldj<fp2>(pw, 0); });
}

// the workgroup engine's op on LDS buffers A, B (operands, w-basis), C (a third Fp12), W (5 Fp12), S (108 products);
// returns the buffer that holds the result.  Every lane of the block calls it.
__device__ __forceinline__ uint32_t* coop_gtw_op(int op, uint32_t* A, uint32_t* B, uint32_t* C, uint32_t* W,
                                                 uint32_t* S, uint32_t t) {
  switch (op) {
    case 145: gtw_mul<false>(C, A, B, S, t); return C;
    case 146: gtw_mul<false>(A, A, B, S, t); return A;
    case 147: gtw_mul<false>(B, A, B, S, t); return B;
    case 148: gtw_mul<false>(A, A, A, S, t); return A;
    case 149: gtw_mul<true>(C, A, B, S, t); return C;
    case 150: gtw_cyc_sqr(A, A, S, t); return A;
    case 151: gtw_cyc_sqr(C, A, S, t); return C;
    case 152: gtw_conj(C, A, t); return C;
    case 153: gtw_frob(C, A, 1, t); return C;
    case 154: gtw_frob(C, A, 2, t); return C;
    case 155: gtw_pow_z(C, A, S, t); return C;
    default: gtw_final_exp(A, W, S, t); return A;  // 156
  }
}
#endif  // __HIPCC__
