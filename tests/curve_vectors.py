"""Test vectors for the one-lane point formulas (lodestar_amd/csrc/curve.hpp, ops.hpp g1_in_subgroup) on raw limbs,
exceptional branches included, shared by the host test (tests/test_curve_contracts.py, through tests/native/emu.cpp
emu_curve_op) and the device test (tests/test_gpu_curve_contracts.py, blsgpu_debug_op ops 69..107).  Plain Python,
fixed seeds; built on tests/tower_vectors.py (limbs, Rec, Op, _finish, check).  The only reference is the oracle
(oracle/bls12_381.py: g1_add, g2_add, g1_mul, g2_mul, g2_psi, on_curve, [r]P == O) and Python integers; for inputs the
oracle's API cannot take (pairs that are not on the curve) the affine chord-and-tangent law aff_add() below, which
tests/test_curve_contracts.py compares with the oracle.  Nothing here calls the code under test.

Operands are raw Montgomery values as the code holds them (14 limbs of 28 bits per Fp value): a Jacobian point is
(x, y, z), 3 Fp values on G1 and 6 on G2 (Fp2 = (c0, c1)), an affine point (x, y).  Every point is given through several
Jacobian lifts (x l^2, y l^3, l): l = the Montgomery one, small values, random, -1 and, on G2, l with a zero component;
every coordinate residue v as v and as v + p, a zero residue as 0, p and 2p (per component on G2).  Infinity is z in
{0, p, 2p} (every mix of the two components on G2) under x, y = (one, one), (0, 0), arbitrary values and what the
doubling formula leaves behind.

A Jacobian result is checked by value: Z == 0 (mod p) exactly when the reference is infinity, else X == x Z^2 and
Y == y Z^3; every output coordinate has limbs 0..12 below 2^28 and a value within the bound the headers state for
the operation that produced it (F_lc < 1.003 p; fp2_mul < 1.1 p; an fp_mul of operands <= 4p and <= 2p
< p + 8 p^2 / 2^392; everything else <= 2p).  The un-suffixed jac_dbl / jac_add / jac_add_aff, and the nested jac_dbl
of an addition's P = Q branch, run whichever body the build selects, so their sums get the eager bound 2p.  Where a
branch returns an operand unchanged (inf + Q, P + inf, mixed addition onto infinity with z = the Montgomery one), the
exact input limbs are expected.

Points: multiples of the generators; curve points outside the subgroups (random x, y solved); points of small order
derived from the cofactors h1 = (z - 1)^2 / 3 = 3 * 11^2 * 10177^2 * .. and h2 = 13^2 * 23^2 * 2713 * 11953 * ..
([n / m^k] A for a random A, m^k the full power of m in the group order n: the squared parts are Z_m x Z_m); E has
(0, +-2) of order 3, the x = 0 edge (E' has no point with x = 0).  For jac_add* also Fp2 pairs that need not lie on the
curve: x equal in exactly one component (still the generic chord), and the same x with y equal in exactly one
component (a vertical chord: infinity) -- a zero test that looks at half an Fp2 fails these.

The [|z|] chain (jac_mul_zabs, _ld, _lda and the subgroup predicates built on them) takes its exceptional branches only
on points of tiny order; chain_branches(m) mirrors it over Z / m (the accumulator's multiple of P at every step):
    order 3            inf + P, P + P, -P + P, doubling of infinity
    order 11           P + P
    order 13           inf + P, -P + P, doubling of infinity
    order 23, 2713, 10177   only generic steps
The module asserts that table, and that every such branch is taken by a record of each chain op that can reach it.
Not reachable with any available order: P + P inside the chain on G2 (orders 13, 23, 2713, 11953 never bring the
accumulator to P before an addition), so jac_mul_zabs / _ld / _lda / g2_in_subgroup / g2_in_subgroup_ld on G2 never
run the nested doubling -- the G2 doubling branch is covered by the jac_add* records only; on G1 order 3 reaches all
four branches."""
import functools
import itertools
import random

from oracle import bls12_381 as bls
from tests import tower_vectors as tv
from tests.tower_vectors import (BOUND_2P, BOUND_LC, P, RM, Z_ABS, Op, Rec, _finish, _mont_bound, limbs, lt_frac, m_,
                                 s_)

BOUND_F2MUL = lt_frac(11, 10)
BOUND_Z1 = _mont_bound(4 * P, 2 * P)  # fp_mul of an operand <= 4p (F_add_nr(y, y)) and a stored one
BOUND_M1 = _mont_bound(2 * P, 2 * P)  # fp_mul of two stored values
_Z = bls.BLS_X
H1 = (_Z - 1) ** 2 // 3
H2 = (_Z**8 - 4 * _Z**7 + 5 * _Z**6 - 4 * _Z**4 + 6 * _Z**3 - 4 * _Z**2 - 4 * _Z + 13) // 9
assert (_Z - 1) ** 2 % 3 == 0 and H2 * 9 == _Z**8 - 4 * _Z**7 + 5 * _Z**6 - 4 * _Z**4 + 6 * _Z**3 - 4 * _Z**2 - 4 * _Z + 13
assert H1 % (3 * 11**2 * 10177**2) == 0 and H2 % (13**2 * 23**2 * 2713 * 11953) == 0
LAMBDA = (-_Z * _Z) % bls.R  # the eigenvalue of endo_lambda on both groups


class Grp:
    """one of the two groups: its field (the oracle's ops), Fp values per coordinate, and the oracle's point API"""

    def __init__(self, tag, F, n, gen, mul, add, neg, order):
        self.tag, self.F, self.n, self.gen, self.mul, self.add, self.neg, self.order = (
            tag, F, n, gen, mul, add, neg, order)

    def comps(self, e):
        return [e] if self.n == 1 else list(e)

    def elem(self, c):
        return c[0] % P if self.n == 1 else tuple(x % P for x in c)

    def rand(self, rng):
        return self.elem([rng.randrange(P) for _ in range(self.n)])

    def rhs(self, x):
        return self.F.add(self.F.mul(self.F.sqr(x), x), self.F.b)

    def sqrt(self, a):
        return bls.fsqrt(a) if self.n == 1 else bls.f2sqrt(a)

    def one_raw(self):
        return [RM] + [0] * (self.n - 1)


G1 = Grp("g1", bls.Fp1Ops, 1, bls.G1_GEN, bls.g1_mul, bls.g1_add, bls.g1_neg, H1 * bls.R)
G2 = Grp("g2", bls.Fp2Ops, 2, bls.G2_GEN, bls.g2_mul, bls.g2_add, bls.g2_neg, H2 * bls.R)
GRP = {"g1": G1, "g2": G2}


def aff_add(G, a, b):
    """The affine chord-and-tangent law (a = 0), written out: None is infinity.  It uses no curve equation, so it is
    also what the Jacobian formulas compute on pairs that are not on the curve; there, equal x with y neither equal
    nor opposite is a vertical chord."""
    F = G.F
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2:
        if y1 != y2 or F.is_zero(y1):
            return None
        lam = F.mul(F.mul(F.sqr(x1), G.elem([3] + [0] * (G.n - 1))), F.inv(F.add(y1, y1)))
    else:
        lam = F.mul(F.sub(y2, y1), F.inv(F.sub(x2, x1)))
    x3 = F.sub(F.sub(F.sqr(lam), x1), x2)
    return (x3, F.sub(F.mul(lam, F.sub(x1, x3)), y1))


def chain_branches(m):
    """the exceptional branches jac_mul_zabs / _ld / _lda take on a point of order m: the accumulator's multiple of P
    mod m before every doubling and addition of the chain (left to right over |z|, starting from P)"""
    acc, out = 1 % m, set()
    for i in range(62, -1, -1):
        if acc == 0:
            out.add("dbl inf")
        acc = 2 * acc % m
        if (Z_ABS >> i) & 1:
            if acc in (0, 1, m - 1):
                out.add({0: "inf+P", 1: "P+P"}.get(acc, "-P+P"))
            acc = (acc + 1) % m
    return out


assert chain_branches(3) == {"inf+P", "P+P", "-P+P", "dbl inf"}
assert chain_branches(11) == {"P+P"}
assert chain_branches(13) == {"inf+P", "-P+P", "dbl inf"}
assert not any(chain_branches(m) for m in (23, 2713, 10177, 11953, bls.R))
CHAIN_REACHABLE = {"g1": chain_branches(3) | chain_branches(11), "g2": chain_branches(13)}


class Pt:
    """a pool point: affine residues (standard form), its order where that is small, whether [r]P == O"""

    def __init__(self, name, aff, order, in_subgroup):
        self.name, self.aff, self.order, self.in_subgroup = name, aff, order, in_subgroup

    @property
    def chain_cls(self):
        b = chain_branches(self.order) if self.order else set()
        return "order %d: %s" % (self.order, ", ".join(sorted(b)) or "generic") if self.order else "generic"


def _curve_point(G, rng):
    while True:
        x = G.rand(rng)
        y = G.sqrt(G.rhs(x))
        if y is not None:
            assert bls.on_curve(G.F, (x, y))
            return (x, y)


def _small_order(G, m, rng):
    """a point of order m (prime): [n / m^k] A for random A, m^k the full power of m in the group order n"""
    mk = m
    while G.order % (mk * m) == 0:
        mk *= m
    while True:
        t = G.mul(_curve_point(G, rng), G.order // mk)
        if t is not None:
            assert G.mul(t, m) is None and bls.on_curve(G.F, t)
            return t


@functools.lru_cache(maxsize=None)
def pool(tag):
    """small-order points first, then subgroup points, then curve points outside the subgroup"""
    G = GRP[tag]
    rng = random.Random(7001 if tag == "g1" else 7002)
    assert G.mul(_curve_point(G, rng), G.order) is None  # [h r] annihilates the whole curve group
    pts = []
    if tag == "g1":
        for y in (2, P - 2):
            assert bls.on_curve(G.F, (0, y)) and G.mul((0, y), 3) is None
            pts.append(Pt("order 3 (0, %s2)" % ("+" if y == 2 else "-"), (0, y), 3, False))
        small, n_sub, n_out = ((11, 4), (10177, 3)), 14, 10
    else:
        small, n_sub, n_out = ((13, 1), (23, 1), (2713, 1), (11953, 1)), 3, 2
    for m, k in small:
        t = _small_order(G, m, rng)
        for j in range(1, k + 1):
            pts.append(Pt("order %d #%d" % (m, j), G.mul(t, j), m, False))
    pts.append(Pt("generator", G.gen, None, True))
    for i in range(n_sub):
        pts.append(Pt("[k]G #%d" % i, G.mul(G.gen, rng.randrange(1, bls.R)), None, True))
    while n_out:
        a = _curve_point(G, rng)
        if G.mul(a, bls.R) is not None:
            n_out -= 1
            pts.append(Pt("outside #%d" % n_out, a, None, False))
    for pt in pts:
        assert bls.on_curve(G.F, pt.aff) and (G.mul(pt.aff, bls.R) is None) == pt.in_subgroup, pt.name
        assert tag == "g1" or not G.F.is_zero(pt.aff[0])
    return pts


def pool_core(tag):
    """one point of each kind and order (the additions' P = +-Q cases go through these)"""
    out, seen = [], {}
    for pt in pool(tag):
        kind = pt.order or pt.name.split(" #")[0]
        if seen.get(kind, 0) < (2 if kind in (3, "[k]G", "outside") else 1):
            seen[kind] = seen.get(kind, 0) + 1
            out.append(pt)
    return out


# ------------------------------------------------------------------------------------------------ representations
MODES = ("canon", "+p", "mixed")


def rep(m, mode, rng):
    """a representative in [0, 2p] of the residue m: m, m + p; zero as 0, p, 2p"""
    if m == 0:
        return {"canon": 0, "+p": P, "2p": 2 * P}.get(mode) if mode != "mixed" else rng.choice([0, P, 2 * P])
    return {"canon": m, "+p": m + P}.get(mode) if mode != "mixed" else rng.choice([m, m + P])


def raw_of(G, e, mode, rng):
    """the raw Montgomery values of a field element (standard-form residues in)"""
    return [rep(m_(c), mode, rng) for c in G.comps(e)]


def lams(G, rng):
    """the Jacobian lifts' l, as (label, standard-form element)"""
    F = G.F
    pad = [0] * (G.n - 1)
    out = [("one", F.one), ("two", G.elem([2] + pad)), ("raw3", G.elem([s_(3)] + [s_(5)] * (G.n - 1))),
           ("random", G.rand(rng)), ("-1", F.neg(F.one))]
    if G.n == 2:
        out += [("(0,a)", (0, rng.randrange(1, P))), ("(a,0)", (rng.randrange(1, P), 0))]
    return out


def jac_raw(G, aff, lam, mode, rng):
    F = G.F
    l2 = F.sqr(lam)
    return (raw_of(G, F.mul(aff[0], l2), mode, rng) + raw_of(G, F.mul(aff[1], F.mul(l2, lam)), mode, rng) +
            raw_of(G, lam, mode, rng))


def aff_raw(G, aff, mode, rng):
    return raw_of(G, aff[0], mode, rng) + raw_of(G, aff[1], mode, rng)


def aff_raw_all(G, aff):
    """every representative combination of an affine point's coordinates"""
    choices = [[m_(c), m_(c) + P] + ([2 * P] if c == 0 else []) for e in aff for c in G.comps(e)]
    return [list(t) for t in itertools.product(*choices)]


def _dbl_left(G, x, y):
    """what dbl-2009-l leaves in X3, Y3 for the input (x, y, z = 0)"""
    F = G.F
    A, B = F.sqr(x), F.sqr(y)
    C = F.sqr(B)
    D = F.sub(F.sqr(F.add(x, B)), F.add(A, C))
    D = F.add(D, D)
    E = F.add(F.add(A, A), A)
    X3 = F.sub(F.sqr(E), F.add(D, D))
    C8 = F.add(C, C)
    C8 = F.add(C8, C8)
    return X3, F.sub(F.mul(E, F.sub(D, X3)), F.add(C8, C8))


@functools.lru_cache(maxsize=None)
def infs(tag):
    """infinity's encodings as (label, raw values)"""
    G = GRP[tag]
    rng = random.Random(7101 if tag == "g1" else 7102)
    gx, gy = G.gen
    xys = [("one,one", G.one_raw() * 2), ("0,0", [0] * (2 * G.n)),
           ("arbitrary", [rng.randrange(2 * P + 1) for _ in range(2 * G.n)]),
           ("after dbl", aff_raw(G, _dbl_left(G, G.F.mul(gx, G.rand(rng)), G.F.mul(gy, G.rand(rng))), "mixed", rng))]
    out = []
    for z in itertools.product((0, P, 2 * P), repeat=G.n):
        for n, xy in xys:
            out.append(("inf[%s; z=%s]" % (n, ",".join(tv._vname(c) for c in z)), xy + list(z)))
    return out


class CRec(Rec):
    """a record with its branch class (the launch orders of the device test group and interleave by it)"""
    __slots__ = ("cls",)

    def __init__(self, name, cls, raw, want, bound, **kw):
        Rec.__init__(self, name, [limbs(v) for v in raw], want, bound, **kw)
        assert all(0 <= v <= 2 * P for v in raw), name
        self.cls = cls


def _jac_post(G, ref):
    """the by-value check of a Jacobian output against the affine reference (None = infinity)"""
    n, F = G.n, G.F

    def post(vals):
        X, Y, Z = (G.elem([s_(v) for v in vals[n * k:n * k + n]]) for k in range(3))
        if F.is_zero(Z):
            return True if ref is None else "Z == 0 (infinity) for a finite sum"
        if ref is None:
            return "Z != 0 where the reference is infinity"
        Z2 = F.sqr(Z)
        if X != F.mul(ref[0], Z2):
            return "X != x Z^2"
        if Y != F.mul(ref[1], F.mul(Z2, Z)):
            return "Y != y Z^3"
        return True
    return post


def _b(G, bx, by, bz):
    return [bx] * G.n + [by] * G.n + [bz] * G.n


def _zp(G):
    return BOUND_Z1 if G.n == 1 else BOUND_F2MUL


def _jrec(G, name, cls, raw, ref, bound, exact=None):
    return CRec(name, cls, raw, [None] * (3 * G.n), bound, exact=exact, post=_jac_post(G, ref))


def _points_lifted(G, rng, n_min):
    """(name, point, raw Jacobian) over the pool, every lift and the representative modes, small orders first;
    at least n_min of them"""
    out = []
    for k in itertools.count():
        for pt in pool(G.tag):
            for j, (ln, lam) in enumerate(lams(G, rng)):
                mode = MODES[(j + k) % 3]
                out.append(("%s l=%s %s" % (pt.name, ln, mode), pt, jac_raw(G, pt.aff, lam, mode, rng)))
        if len(out) >= n_min:
            return out


# ------------------------------------------------------------------------------------------------ doubling
def _gen_dbl(tag, body):
    def gen():
        G = GRP[tag]
        rng = random.Random(7201)
        xy = BOUND_LC if body == "lazy" else BOUND_2P
        recs = []
        for n, raw in infs(tag):
            recs.append(_jrec(G, "jac_dbl %s" % n, "inf", raw, None, _b(G, xy, xy, _zp(G))))
        for n, pt, raw in _points_lifted(G, rng, 150):
            recs.append(_jrec(G, "jac_dbl %s" % n, "finite", raw, G.add(pt.aff, pt.aff), _b(G, xy, xy, _zp(G))))
        return recs
    return gen


# ------------------------------------------------------------------------------------------------ additions
@functools.lru_cache(maxsize=None)
def _add_protos(tag, kind):
    """body-independent records of P + Q (kind "jac": Q Jacobian, "aff": Q affine) as
    (name, class, raw operands, reference, exact output or None)"""
    G, F = GRP[tag], GRP[tag].F
    rng = random.Random({"g1jac": 7301, "g1aff": 7302, "g2jac": 7303, "g2aff": 7304}[tag + kind])
    pts = pool(tag)
    out = []

    def second(aff, lam, mode):
        return jac_raw(G, aff, lam, mode, rng) if kind == "jac" else aff_raw(G, aff, mode, rng)

    def lam_pairs():
        ls = lams(G, rng)
        return [(a, b) for a in ls for b in (ls if kind == "jac" else ls[:1])]

    # generic P + Q: every pair of lifts, the points and the representatives at random
    for rnd in range((5 - G.n) if kind == "jac" else 12):
        for (la, a), (lb, b) in lam_pairs():
            p, q = rng.sample(pts, 2)
            while p.aff[0] == q.aff[0]:
                p, q = rng.sample(pts, 2)
            ma, mb = rng.choice(MODES), rng.choice(MODES)
            out.append(("%s l=%s %s + %s l=%s %s" % (p.name, la, ma, q.name, lb, mb), "generic",
                        jac_raw(G, p.aff, a, ma, rng) + second(q.aff, b, mb), G.add(p.aff, q.aff), None))
    # P + P and P + (-P): the same lift and representatives, the same lift with x (y) against x + p, other lifts
    for sign, cls in ((1, "P+P"), (-1, "P-P")):
        for pt in pool_core(tag):
            q = pt.aff if sign == 1 else G.neg(pt.aff)  # (-y canonical is p - y, + p is 2p - y)
            ref = G.add(pt.aff, q)
            assert (ref is None) == (sign == -1)
            tagn = "%s %s" % (pt.name, cls)
            ls = lams(G, rng)
            for j, (ln, lam) in enumerate(ls):
                for mp, mq in (("canon", "canon"), (("canon", "+p"), ("+p", "canon"), ("mixed", "mixed"))[j % 3]):
                    rp = jac_raw(G, pt.aff, lam, mp, rng)
                    rq = second(q, lam if kind == "jac" else F.one, mq)
                    if sign == 1 and kind == "jac" and mp == mq:
                        rq = list(rp)  # the very same limbs on both sides
                    out.append(("%s: l=%s %s / %s" % (tagn, ln, mp, mq), cls, rp + rq, ref, None))
            if kind == "jac":
                for (la, a), (lb, b) in rng.sample([(x, y) for x in ls for y in ls if x is not y], 3):
                    ma, mb = rng.choice(MODES), rng.choice(MODES)
                    out.append(("%s: l=%s %s / l=%s %s" % (tagn, la, ma, lb, mb), cls,
                                jac_raw(G, pt.aff, a, ma, rng) + jac_raw(G, q, b, mb, rng), ref, None))
    # infinity on either side: the other operand comes back limb for limb
    lifted = _points_lifted(G, rng, 1)
    for i, (n, inf) in enumerate(infs(tag)):
        qn, pt, rq = lifted[(5 * i) % len(lifted)]
        if kind == "jac":
            out.append(("%s + %s" % (n, qn), "inf+Q", inf + rq, pt.aff, list(rq)))
            pn, pt2, rp = lifted[(5 * i + 2) % len(lifted)]
            out.append(("%s + %s" % (pn, n), "P+inf", rp + inf, pt2.aff, list(rp)))
            n2, inf2 = infs(tag)[(7 * i + 3) % len(infs(tag))]
            out.append(("%s + %s" % (n, n2), "inf+inf", inf + inf2, None, None))
        else:
            pt = pts[i % len(pts)]
            mode = MODES[i % 3]
            rq = aff_raw(G, pt.aff, mode, rng)
            out.append(("%s + affine %s %s" % (n, pt.name, mode), "inf+Q", inf + rq, pt.aff, rq + G.one_raw()))
    # Fp2 pairs off the curve that agree in exactly one component of x (generic chord) or, at the same x, of y
    if tag == "g2":
        for i in range(36):
            a, b, c, y1, y2 = (rng.randrange(1, P) for _ in range(5))
            k = i % 2
            if i % 3 < 2:
                x1, x2 = (a, b), ((a, c) if k == 0 else (c, b))
                p, q, cls = (x1, (y1, y2)), (x2, G.rand(rng)), "generic, x half-equal"
            else:
                p, q, cls = ((a, b), (y1, y2)), ((a, b), ((y1, c) if k == 0 else (c, y2))), "P-P, y half-equal"
            ref = aff_add(G, p, q)
            assert (ref is None) == (i % 3 == 2)
            ls = lams(G, rng)
            (la, a_), (lb, b_) = rng.choice(ls), rng.choice(ls)
            ma, mb = rng.choice(MODES), rng.choice(MODES)
            out.append(("off-curve #%d %s c%d: l=%s %s / l=%s %s" % (i, cls, k, la, ma, lb, mb), cls,
                        jac_raw(G, p, a_, ma, rng) + second(q, b_, mb), ref, None))
    return out


def _add_bound(G, kind, body, cls):
    if cls in ("inf+Q", "P+inf", "inf+inf") or cls.startswith("P-P"):
        return _b(G, BOUND_2P, BOUND_2P, BOUND_2P)
    if cls == "P+P":  # the nested jac_dbl, whichever body the build selects
        return _b(G, BOUND_2P, BOUND_2P, _zp(G))
    xy = BOUND_LC if body == "lazy" else BOUND_2P
    return _b(G, xy, xy, _zp(G) if kind == "jac" else xy)


def _gen_add(tag, kind, body):
    def gen():
        G = GRP[tag]
        fn = "jac_add" if kind == "jac" else "jac_add_aff"
        return [_jrec(G, "%s %s" % (fn, n), cls, raw, ref, _add_bound(G, kind, body, cls),
                      exact=exact) for n, cls, raw, ref, exact in _add_protos(tag, kind)]
    return gen


# ------------------------------------------------------------------------------------------------ neg, predicates
def _gen_neg(tag):
    def gen():
        G = GRP[tag]
        rng = random.Random(7401)
        n = G.n
        recs = []
        items = [(nm, "inf", raw, None) for nm, raw in infs(tag)]
        items += [(nm, "finite", raw, G.neg(pt.aff)) for nm, pt, raw in _points_lifted(G, rng, 130)]
        for nm, cls, raw, ref in items:
            want = [None] * n + [-v % P for v in raw[n:2 * n]] + [None] * n
            recs.append(CRec("jac_neg %s" % nm, cls, raw, want, [BOUND_2P] * (3 * n),
                             exact=raw[:n] + [None] * n + raw[2 * n:], post=_jac_post(G, ref)))
        return recs
    return gen


def _z_near_misses(G):
    """z values that are not zero but look like it to a test that is off by one, or reads one component of two"""
    if G.n == 1:
        return [[v] for v in (1, P - 1, P + 1, 2 * P - 1)]
    out = []
    for z in (0, P, 2 * P):
        for v in (1, P - 1, P + 1, 2 * P - 1, RM):
            out += [[z, v], [v, z]]
    return out


def _gen_is_inf(tag):
    def gen():
        G = GRP[tag]
        rng = random.Random(7501)
        recs = [CRec("jac_is_inf %s" % n, "inf", raw, [], [], status=1) for n, raw in infs(tag)]
        for z in _z_near_misses(G):
            xy = [rng.randrange(2 * P + 1) for _ in range(2 * G.n)]
            recs.append(CRec("jac_is_inf z=%s" % ",".join(tv._vname(c) for c in z), "near miss", xy + z, [], [],
                             status=0))
        for n, pt, raw in _points_lifted(G, rng, 130):
            recs.append(CRec("jac_is_inf %s" % n, "finite", raw, [], [], status=0))
        return recs
    return gen


def _gen_eq(tag):
    def gen():
        G = GRP[tag]
        rng = random.Random(7601)
        pts = pool(tag)
        recs = []

        def rec(name, cls, raw, st):
            recs.append(CRec("jac_eq %s" % name, cls, raw, [], [], status=st))

        def lifted(aff):
            ln, lam = rng.choice(lams(G, rng))
            mode = rng.choice(MODES)
            return "l=%s %s" % (ln, mode), jac_raw(G, aff, lam, mode, rng)

        for rnd in range(4 if G.n == 1 else 7):  # (a class of more than 64 records: a uniform wave)
            for i, pt in enumerate(pts):
                (na, a), (nb, b) = lifted(pt.aff), lifted(pt.aff)
                rec("%s %s == itself %s" % (pt.name, na, nb), "equal", a + b, 1)
                (na, a), (nb, b) = lifted(pt.aff), lifted(G.neg(pt.aff))
                rec("%s %s vs its negative %s" % (pt.name, na, nb), "negative", a + b, 0)
                q = pts[(i + 1 + rnd) % len(pts)]
                if q.aff[0] != pt.aff[0]:
                    (na, a), (nb, b) = lifted(pt.aff), lifted(q.aff)
                    rec("%s %s vs %s %s" % (pt.name, na, q.name, nb), "different", a + b, 0)
        ii = infs(tag)
        for i, (n, inf) in enumerate(ii):
            n2, inf2 = ii[(7 * i + 3) % len(ii)]
            rec("%s == %s" % (n, n2), "inf, inf", inf + inf2, 1)
            pt = pts[i % len(pts)]
            na, a = lifted(pt.aff)
            rec("%s vs %s %s" % (n, pt.name, na), "inf, P", inf + a, 0)
            na, a = lifted(pt.aff)
            rec("%s %s vs %s" % (pt.name, na, n), "P, inf", a + inf, 0)
        if tag == "g2":  # differing in exactly one component of x, or of y at the same x
            for i in range(24):
                a, b, c, y1, y2 = (rng.randrange(1, P) for _ in range(5))
                k = i % 2
                if i % 4 < 2:
                    p, q = ((a, b), (y1, y2)), (((a, c) if k == 0 else (c, b)), (y1, y2))
                else:
                    p, q = ((a, b), (y1, y2)), ((a, b), ((y1, c) if k == 0 else (c, y2)))
                (na, ra), (nb, rb) = lifted(p), lifted(q)
                rec("off-curve #%d, %s differs in c%d only: %s / %s" % (i, "x" if i % 4 < 2 else "y", 1 - k, na, nb),
                    "half-equal", ra + rb, 0)
        return recs
    return gen


def _gen_to_aff(tag):
    def gen():
        G = GRP[tag]
        rng = random.Random(7701)
        n = G.n
        bound = [BOUND_M1 if n == 1 else BOUND_F2MUL] * (2 * n)
        recs = [CRec("jac_to_aff %s" % nm, "inf", raw, [None] * (2 * n), [BOUND_2P] * (2 * n), status=0)
                for nm, raw in infs(tag)]
        for nm, pt, raw in _points_lifted(G, rng, 130):
            want = [m_(c) for e in pt.aff for c in G.comps(e)]
            recs.append(CRec("jac_to_aff %s" % nm, "finite", raw, want, bound, status=1))
        return recs
    return gen


# ------------------------------------------------------------------------------------------------ endomorphisms
def _g1_beta():
    """beta with [lambda](x, y) = (beta x, y) on G1, from the oracle's scalar multiplication"""
    lx, ly = bls.g1_mul(bls.G1_GEN, LAMBDA)
    assert ly == bls.G1_Y
    beta = lx * pow(bls.G1_X, -1, P) % P
    assert pow(beta, 3, P) == 1 and beta != 1
    return beta


def _endo_ref(tag):
    if tag == "g1":
        beta = _g1_beta()
        return lambda a: (beta * a[0] % P, a[1])
    assert bls.g2_neg(bls.g2_psi(bls.g2_psi(bls.G2_GEN))) == bls.g2_mul(bls.G2_GEN, LAMBDA)
    return lambda a: bls.g2_neg(bls.g2_psi(bls.g2_psi(a)))


def _gen_map(tag, fname, ref_of, bound_of, exact_of):
    """a map on Jacobian coordinates: `ref_of` the affine reference, `bound_of(G)` the bounds, `exact_of(G, raw)` the
    coordinates that pass through unchanged"""
    def gen():
        G = GRP[tag]
        rng = random.Random(7801)
        f = ref_of(tag)
        recs = [_jrec(G, "%s %s" % (fname, nm), "inf", raw, None, bound_of(G), exact=exact_of(G, raw))
                for nm, raw in infs(tag)]
        for nm, pt, raw in _points_lifted(G, rng, 130):
            ref = f(pt.aff)
            if pt.in_subgroup and fname == "endo_lambda":
                assert ref == G.mul(pt.aff, LAMBDA)
            recs.append(_jrec(G, "%s %s" % (fname, nm), "finite", raw, ref, bound_of(G), exact=exact_of(G, raw)))
        return recs
    return gen


def _keep(*coords):
    """exact_of: the listed coordinates (0 = x, 1 = y, 2 = z) come back limb for limb"""
    def exact_of(G, raw):
        return [raw[i] if i // G.n in coords else None for i in range(3 * G.n)]
    return exact_of


def _psi_exact(G, raw):  # z = conj(z): c0 unchanged
    return [None] * 4 + [raw[4], None]


# ------------------------------------------------------------------------------------------------ chains, predicates
def _assert_chain_coverage(tag, recs):
    """from the mirror alone: every exceptional branch an available order reaches is taken by some record"""
    seen = set()
    for r in recs:
        seen |= getattr(r, "branches", set())
    assert seen >= CHAIN_REACHABLE[tag], (tag, seen)


class ChainRec(CRec):
    __slots__ = ("branches",)


def _chain_rec(G, name, pt, raw, ref):
    r = ChainRec(name, pt.chain_cls, raw, [None] * (3 * G.n), _b(G, BOUND_2P, BOUND_2P, _zp(G)),
                 post=_jac_post(G, ref))  # the chain ends on a doubling (|z| is even)
    r.branches = chain_branches(pt.order) if pt.order else set()
    return r


@functools.lru_cache(maxsize=None)
def _zabs_ref(tag, aff):
    return GRP[tag].mul(aff, Z_ABS)


def _gen_zabs(tag, fname):
    def gen():
        G = GRP[tag]
        rng = random.Random(7901)
        recs = []
        for nm, pt, raw in _points_lifted(G, rng, 132)[:150]:
            recs.append(_chain_rec(G, "%s %s" % (fname, nm), pt, raw, _zabs_ref(tag, pt.aff)))
        inf = Pt("infinity", None, None, True)
        for nm, raw in infs(tag)[::5][:4]:
            recs.append(_chain_rec(G, "%s %s" % (fname, nm), inf, raw, None))
            recs[-1].cls = "inf in"
        _assert_chain_coverage(tag, recs)
        return recs
    return gen


def _gen_zabs_lda():
    G = G2
    recs = []
    for pt in pool("g2"):
        for i, raw in enumerate(aff_raw_all(G, pt.aff)):
            if pt.order or i % 5 != 4:  # (trim: some representative mixes of the points that take no branch)
                recs.append(_chain_rec(G, "jac_mul_zabs_lda %s reps %s" % (pt.name, format(i, "04b")), pt, raw,
                                       _zabs_ref("g2", pt.aff)))
    _assert_chain_coverage("g2", recs)
    return recs


def _gen_on_curve(tag):
    def gen():
        G = GRP[tag]
        recs = []
        for pt in pool(tag):
            for i, raw in enumerate(aff_raw_all(G, pt.aff)):
                recs.append(CRec("%s_on_curve %s reps #%d" % (tag, pt.name, i), "on", raw, [], [], status=1))
            base = aff_raw_all(G, pt.aff)[0]
            for k in range(2 * G.n):  # one Fp value off by one: for G2 the other component of the coordinate is right
                for j, d in enumerate((1, -1)):
                    off = list(base)
                    off[k] = (off[k] + d) % P + (P if (k + j) % 2 else 0)
                    st = int(bls.on_curve(G.F, (G.elem([s_(v) for v in off[:G.n]]),
                                                G.elem([s_(v) for v in off[G.n:]]))))
                    assert st == 0
                    recs.append(CRec("%s_on_curve %s value %d off by one #%d" % (tag, pt.name, k, j), "off", off, [],
                                     [], status=st))
        return recs
    return gen


def _gen_in_subgroup(tag, fname):
    def gen():
        G = GRP[tag]
        recs = []
        for pt in pool(tag):
            for i, raw in enumerate(aff_raw_all(G, pt.aff)):
                if tag == "g2" and not pt.order and i % 5 == 4:
                    continue
                r = ChainRec("%s %s reps #%d" % (fname, pt.name, i),
                             pt.chain_cls + (" (in)" if pt.in_subgroup else " (out)"), raw, [], [],
                             status=int(pt.in_subgroup))
                r.branches = chain_branches(pt.order) if pt.order else set()
                recs.append(r)
        assert any(r.status for r in recs) and not any(r.status for r in recs if r.branches or "order" in r.cls)
        _assert_chain_coverage(tag, recs)
        return recs
    return gen


# ------------------------------------------------------------------------------------------------ the op table
def _group_ops(tag, base):
    G = GRP[tag]
    n = G.n
    endo_bound = (lambda G_: _b(G_, _mont_bound(2 * P, P), BOUND_2P, BOUND_2P)) if n == 1 else (
        lambda G_: _b(G_, BOUND_F2MUL, BOUND_2P, BOUND_2P))
    ops = []
    for k, body in enumerate(("", "_lazy", "_eager")):
        b = body[1:] or "any"
        ops.append(Op("%s_jac_dbl%s" % (tag, body), base + k, 3 * n, 3 * n, _gen_dbl(tag, b)))
        ops.append(Op("%s_jac_add%s" % (tag, body), base + 3 + k, 6 * n, 3 * n, _gen_add(tag, "jac", b)))
        ops.append(Op("%s_jac_add_aff%s" % (tag, body), base + 6 + k, 5 * n, 3 * n, _gen_add(tag, "aff", b)))
    ops += [
        Op("%s_jac_neg" % tag, base + 9, 3 * n, 3 * n, _gen_neg(tag)),
        Op("%s_jac_is_inf" % tag, base + 10, 3 * n, 0, _gen_is_inf(tag)),
        Op("%s_jac_eq" % tag, base + 11, 6 * n, 0, _gen_eq(tag)),
        Op("%s_jac_to_aff" % tag, base + 12, 3 * n, 2 * n, _gen_to_aff(tag)),
        Op("%s_endo_lambda" % tag, base + 13, 3 * n, 3 * n,
           _gen_map(tag, "endo_lambda", _endo_ref, endo_bound, _keep(1, 2) if n == 1 else _keep(2))),
        Op("%s_jac_mul_zabs" % tag, base + 14, 3 * n, 3 * n, _gen_zabs(tag, "jac_mul_zabs")),
    ]
    return ops


def _psi_ref(k):
    def ref_of(tag):
        return bls.g2_psi if k == 1 else (lambda a: bls.g2_psi(bls.g2_psi(a)))
    return ref_of


OPS = sorted(
    _group_ops("g1", 69) + [
        Op("g1_on_curve", 84, 2, 0, _gen_on_curve("g1")),
        Op("g1_in_subgroup", 85, 2, 0, _gen_in_subgroup("g1", "g1_in_subgroup")),
    ] + _group_ops("g2", 86) + [
        Op("g2_psi", 101, 6, 6, _gen_map("g2", "g2_psi", _psi_ref(1),
                                         lambda G: _b(G, BOUND_F2MUL, BOUND_F2MUL, BOUND_2P), _psi_exact)),
        Op("g2_psi2", 102, 6, 6, _gen_map("g2", "g2_psi2", _psi_ref(2),
                                          lambda G: _b(G, BOUND_F2MUL, BOUND_F2MUL, BOUND_2P), _keep(2))),
        Op("g2_jac_mul_zabs_ld", 103, 6, 6, _gen_zabs("g2", "jac_mul_zabs_ld")),
        Op("g2_jac_mul_zabs_lda", 104, 4, 6, _gen_zabs_lda),
        Op("g2_on_curve", 105, 4, 0, _gen_on_curve("g2")),
        Op("g2_in_subgroup", 106, 4, 0, _gen_in_subgroup("g2", "g2_in_subgroup")),
        Op("g2_in_subgroup_ld", 107, 4, 0, _gen_in_subgroup("g2", "g2_in_subgroup_ld")),
    ], key=lambda o: o.code)
OP_NAMES = [o.name for o in OPS]
BY_NAME = {o.name: o for o in OPS}
assert [o.code for o in OPS] == list(range(69, 108))
CHAIN_OPS = {"g1": ["g1_jac_mul_zabs", "g1_in_subgroup"],
             "g2": ["g2_jac_mul_zabs", "g2_jac_mul_zabs_ld", "g2_jac_mul_zabs_lda", "g2_in_subgroup",
                    "g2_in_subgroup_ld"]}


@functools.lru_cache(maxsize=None)
def records(name):
    """the op's records (computed once per process; shared, not to be modified)"""
    op = BY_NAME[name]
    recs = _finish(op.gen())
    for r in recs:
        assert len(r.ins) == op.n_in and len(r.want) == len(r.bound) == op.n_out, r.name
    return recs


def check(name, outs, statuses):
    """tower_vectors.check on this module's records"""
    return tv.check(name, outs, statuses, op=BY_NAME[name], recs=records(name))


def format_failures(name, bad, limit=12):
    return tv.format_failures(name, bad, limit, total=len(records(name)))


def launch_orders(name):
    """Two orders of the op's records, as index lists.  `interleaved`: every branch class spread evenly over the whole
    launch, so each 64-lane wave holds lanes on different branches; `grouped`: class by class, the largest first, so
    waves are uniform wherever a class fills one."""
    recs = records(name)
    by_cls = {}
    for i, r in enumerate(recs):
        by_cls.setdefault(r.cls, []).append(i)
    groups = sorted(by_cls.values(), key=len, reverse=True)
    grouped = [i for g in groups for i in g]
    keyed = sorted(((k + 0.5) / len(g), gi, i) for gi, g in enumerate(groups) for k, i in enumerate(g))
    return [i for _, _, i in keyed], grouped


def wave_classes(name, order):
    """the set of branch classes in each 64-lane wave of a launch in `order`"""
    recs = records(name)
    return [{recs[i].cls for i in order[w:w + 64]} for w in range(0, len(order), 64)]
