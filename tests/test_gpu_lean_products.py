"""The Montgomery products in their single-chain form, the lane-pair doubling step and the lane-pair [|z|] chains, on
raw limbs on the device (blsgpu_debug_op): every product routine whose column sums were rewritten (fp_mul 32, fp_sqr 33,
fp2_mul 34, fp2_sqr 35, fp2_mul_fp 36, the lane-pair fp2x_mul 109 / fp2x_sqr 110, and the inlined bodies under
fp_pow_p34 52), n doublings of a lane pair (160) and the chains jac_mul_zabs_ld / jac_mul_zabs_lda over lane pairs
(161 / 162).  One launch of one or two waves per case.

References, none of them the code under test:
  * a product's output is an exact integer, not only a residue: Redc(t) = (t + m p) / 2^392 with m = -t / p mod 2^392,
    whatever the order the columns are summed in, and the routines store it in normalized limbs -- so the expected
    limbs come from Python integers and the comparison is limb for limb, before any canonicalisation;
  * the doublings against the oracle's jac_double (the same dbl-2009-l formula, so the Jacobian coordinates agree as
    residues), the chains against the oracle's [|z|]P in affine coordinates; canonical values compared exactly.
Run on the MI355X box:  timeout -k 10 300 python -u -m pytest tests/test_gpu_lean_products.py -q --durations=0"""
import random

import numpy as np
import pytest

from oracle import bls12_381 as bls
from tests import tower_vectors as tv

pytestmark = pytest.mark.gpu

P, R, RM, RINV, NL = tv.P, tv.R, tv.RM, tv.RINV, tv.NL
NPINV = (-pow(P, -1, R)) % R
F2 = bls.Fp2Ops
# tower.hpp FP_16P_K: 16p with limbs 0..12 borrowed up into [2^29, 2^30)
FP_16P_K = [0x3ffaaab0, 0x3efffffc, 0x3ffffb9c, 0x3ffeb150, 0x3241eabc, 0x30f6b0f3, 0x36730d27, 0x338512bc,
            0x3774b84c, 0x3bacd761, 0x3a7b6431, 0x369a4b18, 0x3ea397fb, 0x001a010e]
assert tv.val(FP_16P_K) == 16 * P


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd.native import Context

    c = Context()
    yield c
    c.close()


def redc(t):
    """the Montgomery reduction's exact output integer"""
    m = (t % R) * NPINV % R
    assert (t + m * P) % R == 0
    return (t + m * P) >> (tv.LB * NL)


def run(ctx, op, rows, n_out):
    """rows: per record the list of its operands' limb lists -> per record n_out limb lists, and the status words"""
    n_in = len(rows[0])
    a = np.array([[x for l in r for x in l] for r in rows], dtype=np.uint32)
    out, st = ctx.debug_op(op, a.tobytes(), 56 * n_in, 56 * n_out)
    o = np.frombuffer(out, np.uint32).reshape(len(rows), n_out, NL)
    return [[[int(x) for x in l] for l in rec] for rec in o], [int(s) for s in st]


def operand_pool(rng, bits, vmax):
    """64 operands of a product whose contract is limbs < 2^bits, value <= vmax: zero, one (plain and Montgomery),
    p - 1, p and values in [p, 1.003 p), every limb at the contract's maximum, random values with the deepest
    un-normalisation the limb bound allows and with a random one, random stored values"""
    hi = tv.lt_frac(1003, 1000)
    vals = [0, 1, RM, P - 1, P, P + 1, hi] + [rng.randint(P, hi) for _ in range(5)]
    pool = [tv.limbs(v) for v in vals]
    if bits > tv.LB:
        pool.append(tv.saturated(bits, vmax))
        pool += [tv.borrowed(rng.randint(vmax // 2, vmax), rng, bits, full=True) for _ in range(6)]
        pool += [tv.borrowed(rng.randint(0, vmax), rng, bits) for _ in range(12)]
    else:
        pool += [tv.limbs(vmax), tv.limbs(vmax - 1)]
        pool += [tv.limbs(rng.randint(vmax // 2, vmax)) for _ in range(12)]
    while len(pool) < 64:
        pool.append(tv.limbs(rng.randint(0, 2 * P)))
    assert all(0 <= x < (1 << bits) for l in pool for x in l[:-1]) and all(tv.val(l) <= vmax for l in pool)
    return pool


def tuples(rng, pools):
    """64 operand tuples, one operand per pool: position i of every pool together (zero with zero, the all-maximum
    operands with each other), then each position against random ones of the other pools"""
    n = len(pools[0])
    out = [tuple(p[i] for p in pools) for i in range(n // 2)]
    while len(out) < 64:
        out.append(tuple(p[rng.randrange(n)] for p in pools))
    return out


def expect_limbs(got, want_value, what):
    assert got == tv.limbs(want_value), "%s: got %s, want %s" % (what, got, tv.limbs(want_value))


# ------------------------------------------------------------------------------------------------ the products
def test_fp_mul(ctx):
    """fp_mul: operands up to limbs 2^30 - 1 (every limb at it: value < 16p)"""
    rng = random.Random(0x1ea1)
    recs = tuples(rng, [operand_pool(rng, 30, 16 * P - 1), operand_pool(rng, 30, 16 * P - 1)])
    assert any(max(a[:-1]) == (1 << 30) - 1 == max(b[:-1]) for a, b in recs)
    outs, _ = run(ctx, 32, recs, 1)
    for i, ((a, b), (o,)) in enumerate(zip(recs, outs)):
        expect_limbs(o, redc(tv.val(a) * tv.val(b)), "fp_mul record %d" % i)


def test_fp_sqr(ctx):
    """fp_sqr: limbs up to 2^29 - 1 (one fp_add_nr level of stored values: <= 4p)"""
    rng = random.Random(0x1ea2)
    recs = [(a,) for a in operand_pool(rng, 29, 4 * P)]
    assert any(min(a[:-1]) == (1 << 29) - 1 for a, in recs)
    outs, _ = run(ctx, 33, recs, 1)
    for i, ((a,), (o,)) in enumerate(zip(recs, outs)):
        expect_limbs(o, redc(tv.val(a) ** 2), "fp_sqr record %d" % i)


def _fp2_mul_records(rng):
    """(a0, a1, b0, b1), limbs < 2^29 and values <= 8p; with them the two extremes of the 16p - b1 operand: b1 = 0
    (16p - b1 = FP_16P_K itself, every limb at its maximum, next to all-maximum a0, a1, b0) and the all-maximum b1"""
    pools = [operand_pool(rng, 29, 8 * P) for _ in range(4)]
    recs = tuples(rng, pools)
    sat = tv.saturated(29, 8 * P)
    recs[-1] = (sat, sat, sat, tv.limbs(0))
    recs[-2] = (sat, sat, sat, sat)
    return recs


def _fp2_mul_want(a0, a1, b0, b1):
    nb = [k - x for k, x in zip(FP_16P_K, b1)]
    assert all(0 <= x < (1 << 30) for x in nb)
    v = tv.val
    return redc(v(a0) * v(b0) + v(a1) * v(nb)), redc(v(a0) * v(b1) + v(a1) * v(b0))


@pytest.mark.parametrize("op,name", [(34, "fp2_mul"), (109, "fp2x_mul")])
def test_fp2_mul(ctx, op, name):
    """c0 = Redc(a0 b0 + a1 (16p - b1)), c1 = Redc(a0 b1 + a1 b0): one lane (two accumulators) and a lane pair"""
    recs = _fp2_mul_records(random.Random(0x1ea3))
    outs, _ = run(ctx, op, recs, 2)
    for i, (r, o) in enumerate(zip(recs, outs)):
        w0, w1 = _fp2_mul_want(*r)
        expect_limbs(o[0], w0, "%s record %d c0" % (name, i))
        expect_limbs(o[1], w1, "%s record %d c1" % (name, i))


@pytest.mark.parametrize("op,name", [(35, "fp2_sqr"), (110, "fp2x_sqr")])
def test_fp2_sqr(ctx, op, name):
    """c0 = Redc((a0 + a1)(a0 + 8p - a1)), c1 = Redc((a0 + a0) a1); normalized operands, values <= 4p"""
    rng = random.Random(0x1ea4)
    recs = tuples(rng, [operand_pool(rng, 28, 4 * P), operand_pool(rng, 28, 4 * P)])
    # every limb at the contract's maximum (2^28 - 1, the top limb the largest within 4p): both coefficients (the limbs
    # of a0 + a1 at 2^29 - 2 next to a0 + 8p - a1), and each against zero
    sat, zero = tv.saturated(28, 4 * P), tv.limbs(0)
    recs[-3:] = [(sat, sat), (sat, zero), (zero, sat)]
    assert all(any(min(a0[:-1]) == tv.MASK and (min(a1[:-1]) == tv.MASK) == both for a0, a1 in recs)
               for both in (True, False))
    assert (zero, sat) in recs and len(recs) == 64
    outs, _ = run(ctx, op, recs, 2)
    for i, ((a0, a1), o) in enumerate(zip(recs, outs)):
        v0, v1 = tv.val(a0), tv.val(a1)
        expect_limbs(o[0], redc((v0 + v1) * (v0 + 8 * P - v1)), "%s record %d c0" % (name, i))
        expect_limbs(o[1], redc(2 * v0 * v1), "%s record %d c1" % (name, i))


def test_fp2_mul_fp(ctx):
    """(Redc(a0 s), Redc(a1 s)): fp_mul operands"""
    rng = random.Random(0x1ea5)
    recs = tuples(rng, [operand_pool(rng, 30, 16 * P - 1) for _ in range(3)])
    outs, _ = run(ctx, 36, recs, 2)
    for i, ((a0, a1, s), o) in enumerate(zip(recs, outs)):
        expect_limbs(o[0], redc(tv.val(a0) * tv.val(s)), "fp2_mul_fp record %d c0" % i)
        expect_limbs(o[1], redc(tv.val(a1) * tv.val(s)), "fp2_mul_fp record %d c1" % i)


def test_fp_pow_inlined_bodies(ctx):
    """fp_pow_p34 runs the inlined product bodies (378 squarings, ~80 multiplications): the residue of a^((p-3)/4)"""
    rng = random.Random(0x1ea6)
    recs = [(a,) for a in operand_pool(rng, 28, 2 * P)]
    outs, _ = run(ctx, 52, recs, 1)
    for i, ((a,), (o,)) in enumerate(zip(recs, outs)):
        plain = tv.val(a) * RINV % P
        assert tv.val(o) % P == pow(plain, (P - 3) // 4, P) * R % P, "fp_pow_p34 record %d" % i
        assert all(x <= tv.MASK for x in o[:-1]) and tv.val(o) < 2 * P


# ------------------------------------------------------------------------------------ the doubling step, the chains
def mont2(a):
    """an Fp2 value's two Montgomery-form limb lists"""
    return [tv.limbs(a[0] * R % P), tv.limbs(a[1] * R % P)]


def plain2(l0, l1):
    return (tv.val(l0) * RINV % P, tv.val(l1) * RINV % P)


def curve_point(rng):
    """a random point of E'(Fp2): y^2 = x^3 + 4 (1 + u) (outside G2 but for a chance of 2^-256)"""
    while True:
        x = (rng.randrange(P), rng.randrange(P))
        y = bls.f2sqrt(F2.add(F2.mul(F2.sqr(x), x), bls.B2))
        if y is not None:
            pt = (x, y if rng.random() < 0.5 else F2.neg(y))
            assert bls.on_curve(F2, pt)
            return pt


def jac_of(rng, pt):
    """Jacobian coordinates with a random Z"""
    z = (rng.randrange(1, P), rng.randrange(P))
    z2 = F2.sqr(z)
    return (F2.mul(pt[0], z2), F2.mul(pt[1], F2.mul(z2, z)), z)


def jac_rows(J):
    return mont2(J[0]) + mont2(J[1]) + mont2(J[2])


def jac_plain(o):
    return (plain2(o[0], o[1]), plain2(o[2], o[3]), plain2(o[4], o[5]))


def _dbl_inputs():
    """32 lane pairs: random points of E'(Fp2) with random Z and with Z = 1, the identity (Z = 0 as zero limbs and as
    the limbs of p, X and Y arbitrary), and points whose Z comes un-normalised (limbs up to 2^29 - 1, the value
    unchanged and the value plus p)"""
    rng = random.Random(0xdb1)
    rows, ref = [], []
    for i in range(32):
        J = jac_of(rng, curve_point(rng))
        if i % 8 == 1:
            J = (J[0], J[1], (0, 0))
        if i % 8 == 2:
            J = bls.jac_from_affine(F2, curve_point(rng))
        r = jac_rows(J)
        if i == 9:  # zero as the limbs of p
            r[4], r[5] = tv.limbs(P), tv.limbs(P)
        if i % 8 == 3:
            r[4] = tv.borrowed(tv.val(r[4]), rng, 29, full=True)
            r[5] = tv.borrowed(tv.val(r[5]) + P, rng, 29, full=(i == 3))
        rows.append(r)
        ref.append(J)
    return rows, ref


@pytest.fixture(scope="module")
def dbl_inputs():
    return _dbl_inputs()


@pytest.mark.parametrize("n", [1, 2, 63])
def test_lane_pair_doubling(ctx, dbl_inputs, n):
    rows, ref = dbl_inputs
    outs, st = run(ctx, 160, [r + [[n] + [0] * (NL - 1)] for r in rows], 6)
    assert st == [0] * len(rows)
    for i, (J, o) in enumerate(zip(ref, outs)):
        assert all(x <= tv.MASK for l in o for x in l[:-1]) and all(tv.val(l) <= 2 * P for l in o), "record %d" % i
        for _ in range(n):
            J = bls.jac_double(F2, J)
        got = jac_plain(o)
        if F2.is_zero(J[2]):
            assert got[2] == (0, 0), "record %d: the identity must stay at Z = 0" % i
        else:
            assert got == J, "record %d after %d doublings" % (i, n)


def _chain_points():
    """32 points of G2 and 32 of E'(Fp2) outside it, interleaved (neighbouring lane pairs on different data), with
    [|z|]P from the oracle"""
    rng = random.Random(0xc4a1)
    pts = []
    for i in range(32):
        g = bls.g2_mul(bls.G2_GEN, rng.randrange(1, bls.R))
        c = curve_point(rng)
        assert bls.g2_in_subgroup_psi(g) and not bls.g2_in_subgroup_psi(c)
        pts += [g, c]
    return pts, [bls.g2_mul(p, bls.BLS_X_ABS) for p in pts]


@pytest.fixture(scope="module")
def chain_points():
    return _chain_points()


@pytest.mark.parametrize("op,name", [(161, "jac_mul_zabs_ld"), (162, "jac_mul_zabs_lda")])
def test_lane_pair_zabs_chain(ctx, chain_points, op, name):
    pts, want = chain_points
    rng = random.Random(0xc4a2)
    if op == 161:  # Jacobian in: a random Z for every other point
        rows = [jac_rows(jac_of(rng, p) if i % 4 < 2 else bls.jac_from_affine(F2, p)) for i, p in enumerate(pts)]
    else:
        rows = [mont2(p[0]) + mont2(p[1]) for p in pts]
    outs, st = run(ctx, op, rows, 6)
    assert st == [0] * len(rows)
    verdicts = []
    for i, (p, w, o) in enumerate(zip(pts, want, outs)):
        got = bls.jac_to_affine(F2, jac_plain(o))
        assert got == w, "%s record %d" % (name, i)
        # what the subgroup check compares: psi(P) against [z]P = -[|z|]P
        verdicts.append(bls.g2_psi(p) == bls.g2_neg(got))
    assert verdicts == [True, False] * 32
