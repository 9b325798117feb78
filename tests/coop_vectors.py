"""Test vectors for the multi-lane engines on raw limbs, at the edges of their operand contracts: lacc_fin (lacc.hpp),
the lane-pair forms (fp2x.hpp, gtx.hpp), the six-lane GT engine (gt6.hpp), the 16-lane cooperative G2 chains
(g2_coop.hpp) and the workgroup GT engine (gt_wave.hpp).  Shared by the host test (tests/test_coop_contracts.py,
through tests/native/emu.cpp emu_coop_op: the host-compilable subset, lane by lane) and the device test
(tests/test_gpu_coop_contracts.py, blsgpu_debug_op ops 108..157, every engine in its production launch shape).
Plain Python, fixed seeds; built on tests/tower_vectors.py and tests/curve_vectors.py (their encoders, edge sets,
pools and per-op generators); the only reference is the oracle (oracle/bls12_381.py) and Python integers.

Per op the inputs are the one-lane generators' of the same operation plus what the multi-lane forms add:
  fp2x_mul       one fp_add_nr level per coefficient (limbs < 2^29), values up to 8p - 1 independently per coefficient,
                 and 8p itself (fp2x.hpp says `<= 8p` since this module: its derivation is there)
  fp2x_sqr, fp6x_mul   normalized values <= 4p
  fp12x_sqr      stored values <= 2p: it feeds a0 + a1 (fp_add_norm) to fp6x_mul, whose operands end at 4p
  every field op patterns with ONE coefficient at 0, p, 2p or 1 and the rest random -- the two coefficients of one Fp2
                 in different classes, which is what a pair-combined predicate or a lane-indexed select table gets wrong
  F_is_zero, g6_is_one   every mix of {0, p, 2p} (1, 1 + p) per coefficient and near misses in exactly one
  pair points, g2c       curve_vectors' G2 records: lifts with Z != 1, redundant representatives, every infinity
                 encoding, P + P, P - P, P + O, O + Q, the small orders (the chain's exceptional branches), the
                 off-curve pairs equal in one component
  g2c            also elements flagged off: arbitrary words (all-ones among them) that the group runs every phase on
                 and must not write out
  lacc users     the all-2p operand and 2p on one half of the coefficients only (gtw_mul, g6_mul: pairs of such
                 operands; g2c_dbl, g2c_add: such points; the cyclotomic squarings: zero in such representatives)
  the [|z|] chains   every multiple of the order-13 point as well, so the in-chain branches fill a wave of lane pairs
Each record has a branch class; launch_orders() gives two record orders (classes interleaved / grouped) in which every
record sits at two different positions of its block, and the grouped one has whole waves on one class."""
import functools
import itertools
import random

from oracle import bls12_381 as bls
from tests import curve_vectors as cv
from tests import tower_vectors as tv
from tests.tower_vectors import (BOUND_2P, BOUND_LC, E2, E4, E8, LIMB_EDGES, NL, P, RM, Rec, _f2, _f6, _f12, _flat,
                                 _mont, _std, _vname, add_nr, borrowed, limbs, lt_frac, m_, s_, saturated, stored,
                                 val)

BOUND_DOT = lt_frac(11, 10)    # fp_dot_body / fp2_mul outputs
BOUND_SQRX = lt_frac(104, 100)  # fp2x_sqr (fp2x.hpp: derived there)
# elements per block of each engine's kernel (k_coop_debug.hip) and per 64-lane wave
BLOCK = {"lane": 128, "pair": 64, "g6": 10, "g2c": 4, "gtw": 1}
WAVE = {"lane": 64, "pair": 32, "g6": 10, "g2c": 4, "gtw": 1}


class KRec(Rec):
    """a record with its branch class"""
    __slots__ = ("cls",)

    def __init__(self, name, cls, ins, want, bound, **kw):
        Rec.__init__(self, name, ins, want, bound, **kw)
        self.cls = cls


def _of(r, cls, bound=None, want=None, status=None, ins=None):
    """a one-lane record as a record of this module"""
    return KRec(r.name, cls, r.ins if ins is None else ins, r.want if want is None else want,
                [bound] * len(r.bound) if bound is not None else r.bound, exact=r.exact,
                status=r.status if status is None else status, post=r.post)


def _edge_cls(name):
    return "random" if ("#" in name and "sparse" not in name) else "edge"


class Op:
    def __init__(self, name, code, engine, n_in, n_out, gen, host=False):
        self.name, self.code, self.engine, self.n_in, self.n_out, self.gen, self.host = (
            name, code, engine, n_in, n_out, gen, host)


# ------------------------------------------------------------------------------------------------ lacc_fin
def gen_lacc_fin():
    """test_lacc_fin_and_lazy_operands' edge list (0..15 terms per side from {0, p, p - 1, 2p, random}, the limb sums
    at their maxima) plus 15 x 2p on either side and on both"""
    rng = random.Random(10801)
    recs = []

    def rec(name, cls, terms_p, terms_n, pos=None):
        pos = pos or [sum(limbs(t)[i] for t in terms_p) for i in range(NL)]
        neg = [sum(limbs(t)[i] for t in terms_n) for i in range(NL)]
        recs.append(KRec(name, cls, [pos, neg], [(val(pos) - val(neg)) % P], [BOUND_2P]))

    full = [2 * P] * 15
    for np_, nn in ((15, 0), (0, 15), (15, 15)):
        rec("lacc_fin %d x 2p - %d x 2p" % (np_, nn), "15 x 2p", full[:np_], full[:nn])
    for k in range(1, 15):
        rec("lacc_fin 15 x 2p - %d x 2p" % k, "15 x 2p", full, full[:k])
        rec("lacc_fin %d x 2p - 15 x 2p" % k, "15 x 2p", full[:k], full)
        rec("lacc_fin 15 x 2p - %d x (p - 1)" % k, "15 x 2p", full, [P - 1] * k)
    maxpos = [15 * tv.MASK if i < 13 else 15 * limbs(2 * P)[13] for i in range(NL)]
    for i in range(300):
        npos, nneg = rng.randint(0, 15), rng.randint(0, 15)
        tp = [rng.choice([0, 2 * P, P, rng.randrange(2 * P + 1)]) for _ in range(npos)]
        tn = [rng.choice([0, 2 * P, P - 1, rng.randrange(2 * P + 1)]) for _ in range(nneg)]
        if i % 7 == 0:
            rec("lacc_fin limb sums at their maxima - %d terms #%d" % (nneg, i), "max limbs", [], tn, pos=maxpos)
        else:
            rec("lacc_fin %d - %d terms #%d" % (npos, nneg, i), "random", tp, tn)
    return recs


# ------------------------------------------------------------------------------------------------ lane pairs, field
def _single_coef(rng, n_coef, other, tag):
    """patterns with ONE coefficient at 0, p, 2p, 1 (the Montgomery one too) and everything else drawn by `other`"""
    out = []
    for k in range(n_coef):
        for e in (0, P, 2 * P, 1, RM):
            v = [other(rng) for _ in range(n_coef)]
            v[k] = e
            out.append((("%s coefficient %d = %s, rest random" % (tag, k, _vname(e))).strip(), v))
    return out


def _fp2_mul_rec(name, cls, ls):
    a0, a1, b0, b1 = (val(l) for l in ls)
    return KRec(name, cls, list(ls), [(a0 * b0 - a1 * b1) * tv.RINV % P, (a0 * b1 + a1 * b0) * tv.RINV % P],
                [BOUND_DOT] * 2)


def gen_fp2x_mul():
    rng = random.Random(10901)
    recs = [_of(r, _edge_cls(r.name), bound=BOUND_DOT) for r in tv.records("fp2_mul")]
    top = 8 * P - 1
    z = limbs(0)
    forms = {"4p+(4p-1)": add_nr(limbs(4 * P), limbs(4 * P - 1)), "8p-1": limbs(top),
             "full-borrow(8p-1)": borrowed(top, rng, 29, True), "saturated29": saturated(29, top)}
    for n, l in forms.items():
        recs.append(_fp2_mul_rec("fp2x_mul all four at %s" % n, "edge", [l] * 4))
    for mask in range(1, 16):  # every corner of {0, 8p - 1}^4, independently per coefficient
        ls = [forms["4p+(4p-1)"] if (mask >> k) & 1 else z for k in range(4)]
        recs.append(_fp2_mul_rec("fp2x_mul corner %s of {0, 8p-1}" % format(mask, "04b"), "edge", ls))
    lt8 = [e for e in E8 if e < 8 * P]
    half = [e for e in E4 if e <= top // 2]
    for n, v in _single_coef(rng, 4, lambda r: None, "fp2x_mul"):
        ls = [limbs(x) if x is not None else tv.sqr_operand(rng, lt8, top, half)[0] for x in v]
        recs.append(_fp2_mul_rec(n, "one coefficient fixed", ls))
    for i in range(300):
        ops = [tv.sqr_operand(rng, lt8, top, half) for _ in range(4)]
        recs.append(_fp2_mul_rec("fp2x_mul <8p #%d %s" % (i, " ".join(n for _, n in ops)), "random",
                                 [l for l, _ in ops]))
    return recs


def gen_fp2x_sqr():
    rng = random.Random(11001)
    recs = [_of(r, _edge_cls(r.name), bound=BOUND_SQRX) for r in tv.records("fp2_sqr")]
    for n, (a0, a1) in _single_coef(rng, 2, tv._le4, "fp2x_sqr"):
        recs.append(KRec(n, "one coefficient fixed", [limbs(a0), limbs(a1)],
                         [(a0 * a0 - a1 * a1) * tv.RINV % P, 2 * a0 * a1 * tv.RINV % P], [BOUND_SQRX] * 2))
    return recs


def _stored_pairs(rng, n):
    ed = E2 + LIMB_EDGES
    return [(a, b) for a in ed for b in ed] + [(stored(rng), stored(rng)) for _ in range(n)]


def gen_fp2x_mul_xi():
    recs = [_of(r, _edge_cls("#" if i >= (len(E2 + LIMB_EDGES)) ** 2 else ""), bound=BOUND_LC)
            for i, r in enumerate(tv.records("fp2_mul_xi"))]
    return recs


def gen_fp2x_norm():
    rng = random.Random(11201)
    n_ed = len(E2 + LIMB_EDGES) ** 2
    recs = []
    for i, (a, b) in enumerate(_stored_pairs(rng, 600)):
        n = (a * a + b * b) * tv.RINV % P
        recs.append(KRec("fp2x_norm(%s, %s)" % (_vname(a), _vname(b)), "edge" if i < n_ed else "random",
                         [limbs(a), limbs(b)], [n, n], [BOUND_2P] * 2))
    return recs


def _zeroish(v):
    return v % P == 0


def gen_f_is_zero():
    """every mix of {0, p, 2p} on the two coefficients (zero: both lanes answer 1, status 3), near misses in exactly
    one coefficient, and pairs with neither zero"""
    rng = random.Random(11301)
    recs = []

    def rec(name, cls, a0, a1):
        st = 3 if _zeroish(a0) and _zeroish(a1) else 0
        recs.append(KRec("F_is_zero(%s, %s) %s" % (_vname(a0), _vname(a1), name), cls, [limbs(a0), limbs(a1)], [], [],
                         status=st))

    zs = (0, P, 2 * P)
    for a0 in zs:
        for a1 in zs:
            rec("zero", "zero", a0, a1)
    near = [1, P - 1, P + 1, 2 * P - 1, RM, RM + P, 1 << 28, 1 << (28 * 13)] + [rng.randrange(1, P) for _ in range(8)]
    for z_ in zs:
        for v in near:
            rec("c1 not zero", "c0 zero only", z_, v)
            rec("c0 not zero", "c1 zero only", v, z_)
    for i in range(60):
        rec("#%d" % i, "neither zero", rng.randrange(1, P) + P * (i % 2), rng.randrange(1, P) + P * (i // 2 % 2))
    return recs


def _gen_lc_xi(tag, wd, ws):
    """this pair's coefficients of sum W_t t + WD xi d: inputs d, then the terms; stored values (fp_lc's contract)"""
    def gen():
        rng = random.Random(11400 + 7 * wd + sum(ws))
        n = 2 * (1 + len(ws))
        pats = [("all %s" % _vname(e), [e] * n) for e in E2 + LIMB_EDGES]
        pats += [("c0 all 2p, c1 all 0", [2 * P, 0] * (n // 2)), ("c0 all 0, c1 all 2p", [0, 2 * P] * (n // 2))]
        # the largest positive and the largest negative sum: 2p where the weight's sign says so, 0 elsewhere
        for sgn in (1, -1):
            for lane in (0, 1):
                v = []
                sd = wd * sgn
                v += [2 * P if sd > 0 else 0, 2 * P if (sd > 0) == (lane == 1) else 0]
                for w in ws:
                    v += [2 * P if w * sgn > 0 else 0] * 2
                pats.append(("%s sum of lane %d" % ("largest" if sgn > 0 else "most negative", lane), v))
        pats += _single_coef(rng, n, stored, "")
        pats += [("stored #%d" % i, [stored(rng) for _ in range(n)]) for i in range(150)]
        recs = []
        for pn, v in pats:
            d0, d1 = v[0], v[1]
            w0 = wd * (d0 - d1) + sum(w * v[2 + 2 * j] for j, w in enumerate(ws))
            w1 = wd * (d1 + d0) + sum(w * v[3 + 2 * j] for j, w in enumerate(ws))
            cls = "random" if pn.startswith("stored") else ("one coefficient fixed" if "coefficient" in pn else "edge")
            recs.append(KRec("%s %s" % (tag, pn), cls, [limbs(x) for x in v], [w0 % P, w1 % P], [BOUND_LC] * 2))
        return recs
    return gen


def _tower_krec(name, cls, vals, want, bound):
    return KRec(name, cls, [limbs(v) for v in vals], want, [bound] * len(want))


def gen_fp6x_mul():
    rng = random.Random(11901)
    recs = [_of(r, _edge_cls(r.name.replace("<=4p #", "#")), bound=BOUND_LC) for r in tv.records("fp6_mul")]
    for n, v in _single_coef(rng, 12, tv._le4, "fp6x_mul"):
        recs.append(_tower_krec(n, "one coefficient fixed", v,
                                _mont(bls.f6mul(_f6(_std(v[:6])), _f6(_std(v[6:])))), BOUND_LC))
    return recs


def _fp12_single(rng, tag):
    return _single_coef(rng, 12, stored, tag)


def gen_fp12x_sqr():
    rng = random.Random(12001)
    recs = [_of(r, _edge_cls(r.name), bound=BOUND_LC) for r in tv.records("fp12_sqr")]
    for n, v in _fp12_single(rng, "fp12x_sqr"):
        recs.append(_tower_krec(n, "one coefficient fixed", v, _mont(bls.f12sqr(_f12(_std(v)))), BOUND_LC))
    return recs


def gen_fp12x_mul_by_014():
    return [_of(r, _edge_cls(r.name), bound=BOUND_LC) for r in tv.records("fp12_mul_by_014")]


def _g2_proj_inputs(rng, n_random, with_q):
    """(name, class, raw values): projective lifts (x l, y l, l) of the G2 pool's points in the three representative
    modes, [+ an affine pool point], then stored-value patterns -- the line steps are polynomial, so any values will do"""
    G, F = cv.G2, cv.G2.F
    out = []
    pts = cv.pool("g2")
    for k, pt in enumerate(pts):
        for j, (ln, lam) in enumerate(cv.lams(G, rng)):
            mode = cv.MODES[(j + k) % 3]
            raw = (cv.raw_of(G, F.mul(pt.aff[0], lam), mode, rng) + cv.raw_of(G, F.mul(pt.aff[1], lam), mode, rng) +
                   cv.raw_of(G, lam, mode, rng))
            nm = "%s l=%s %s" % (pt.name, ln, mode)
            if with_q:
                q = pts[(k + 1 + j) % len(pts)] if j % 3 else pt  # T == Q too: the chord through one point
                raw += cv.aff_raw(G, q.aff, cv.MODES[(j + 1) % 3], rng)
                nm += " + %s" % q.name
            out.append((nm, "curve point", raw))
    n = 10 if with_q else 6
    for pn, v in tv._stored_patterns(rng, n, n_random):
        out.append((pn, _edge_cls(pn), v))
    for pn, v in _single_coef(rng, n, stored, "line step"):
        out.append((pn, "one coefficient fixed", v))
    return out


def _line_bounds():
    return [BOUND_DOT] * 2 + [BOUND_LC] * 2 + [BOUND_DOT] * 2 + [BOUND_LC] * 6


def gen_miller_dbl_line():
    rng = random.Random(12201)
    recs = []
    for nm, cls, raw in _g2_proj_inputs(rng, 60, False):
        s = _std(raw)
        T, line = bls.dbl_step((_f2(s[0:2]), _f2(s[2:4]), _f2(s[4:6])), 1, 1)
        recs.append(KRec("miller_dbl_line %s" % nm, cls, [limbs(v) for v in raw], _mont(T) + _mont(line),
                         _line_bounds()))
    return recs


def gen_miller_add_line():
    rng = random.Random(12301)
    recs = []
    for nm, cls, raw in _g2_proj_inputs(rng, 60, True):
        s = _std(raw)
        T, line = bls.add_step((_f2(s[0:2]), _f2(s[2:4]), _f2(s[4:6])), (_f2(s[6:8]), _f2(s[8:10])), 1, 1)
        recs.append(KRec("miller_add_line %s" % nm, cls, [limbs(v) for v in raw], _mont(T) + _mont(line),
                         _line_bounds()))
    return recs


# ------------------------------------------------------------------------------------------------ lane pairs, points
@functools.lru_cache(maxsize=None)
def _order13_chain_recs():
    """more [|z|] chain inputs on the branches inside the chain (inf + P, -P + P, the doubling of infinity): every
    multiple of the pool's point of order 13 in three lifts, enough of them to fill a wave of lane pairs"""
    G = cv.G2
    rng = random.Random(13101)
    t = next(pt for pt in cv.pool("g2") if pt.order == 13)
    recs = []
    for j in range(2, 13):
        pt = cv.Pt("order 13 #1 x %d" % j, G.mul(t.aff, j), 13, False)
        assert pt.chain_cls == t.chain_cls and cv.chain_branches(13) >= {"inf+P", "-P+P", "dbl inf"}
        for k, (ln, lam) in enumerate(rng.sample(cv.lams(G, rng), 3)):
            mode = cv.MODES[(j + k) % 3]
            recs.append(cv._chain_rec(G, "jac_mul_zabs %s l=%s %s" % (pt.name, ln, mode), pt,
                                      cv.jac_raw(G, pt.aff, lam, mode, rng), cv._zabs_ref("g2", pt.aff)))
    return recs


def _gen_pair_point(cv_name):
    """the one-lane G2 records of the same formula; a predicate's answer comes back from both lanes (status 3)"""
    def gen():
        extra = _order13_chain_recs() if cv_name == "g2_jac_mul_zabs" else []
        return [_of(r, r.cls, status=3 * r.status) for r in list(cv.records(cv_name)) + extra]
    return gen


# ------------------------------------------------------------------------------------------------ six lanes
def _fp12_one_fixed_recs(tag, seed, ref, bound):
    rng = random.Random(seed)
    return [_tower_krec(n, "one coefficient fixed", v, ref(v), bound) for n, v in _fp12_single(rng, tag)]


def _gen_fp12_from(tv_name, tag, seed, ref, bound):
    def gen():
        recs = [_of(r, _edge_cls(r.name), bound=bound) for r in tv.records(tv_name)]
        return recs + (_fp12_one_fixed_recs(tag, seed, ref, bound) if ref else [])
    return gen


def _sqr_ref(v):
    return _mont(bls.f12sqr(_f12(_std(v))))


def gen_fp12_mul_pairs(tag, seed, bound):
    """the one-lane fp12_mul records, one-coefficient patterns, and the lacc users' operands: everything at 2p, and 2p
    on one half of the coefficients only (the even / odd w-coefficients: tower c0 / c1; the real / imaginary parts)"""
    def gen():
        rng = random.Random(seed)
        recs = [_of(r, _edge_cls(r.name), bound=bound) for r in tv.records("fp12_mul")]
        halves = {"all 2p": [2 * P] * 12, "c0 2p, c1 0": [2 * P] * 6 + [0] * 6, "c0 0, c1 2p": [0] * 6 + [2 * P] * 6,
                  "real 2p, imaginary 0": [2 * P, 0] * 6, "real 0, imaginary 2p": [0, 2 * P] * 6}
        seen = {tuple(tuple(l) for l in r.ins) for r in recs}
        for (na, a), (nb, b) in itertools.product(halves.items(), repeat=2):
            if tuple(tuple(limbs(x)) for x in a + b) not in seen:
                recs.append(_tower_krec("%s [%s] * [%s]" % (tag, na, nb), "edge", a + b,
                                        _mont(bls.f12mul(_f12(_std(a)), _f12(_std(b)))), bound))
        for n, v in _single_coef(rng, 24, stored, tag)[::2]:
            recs.append(_tower_krec(n, "one coefficient fixed", v,
                                    _mont(bls.f12mul(_f12(_std(v[:12])), _f12(_std(v[12:])))), bound))
        return recs
    return gen


def _conj_m(want):
    """the conjugate of a flat tower-order residue list"""
    return [x % P for x in want[:6]] + [-x % P for x in want[6:]]


def _gen_pow_z(bound):
    def gen():  # x^z = conj(x^|z|): the one-lane chain's records, the expectation conjugated
        return [_of(r, "cyclotomic" if "cyclotomic #" in r.name else "zero / one", bound=bound, want=_conj_m(r.want))
                for r in tv.records("fp12_pow_zabs")]
    return gen


def _one_sided_zeros():
    """zero (x -> x^2 holds on it, like the one-lane records' uniform zeros) with 2p on one half of the coefficients
    only and 0 or p on the other: the tower halves c0 / c1 (the even / odd w-coefficients), the real / imaginary
    parts, and the first / second member of every squaring pair (w^k, w^(k+3)) -- a recombination's positive side
    at its largest next to an empty negative side, and the reverse"""
    first = [0, 3, 1]  # the tower Fp2 slots of w^0, w^1, w^2 (w^k sits in slot (k odd ? 3 : 0) + k / 2)
    shapes = {"c0 2p, c1 %s": lambda q: q < 6, "c0 %s, c1 2p": lambda q: q >= 6,
              "real 2p, imaginary %s": lambda q: q % 2 == 0, "real %s, imaginary 2p": lambda q: q % 2 == 1,
              "w^k 2p, w^(k+3) %s": lambda q: q // 2 in first, "w^k %s, w^(k+3) 2p": lambda q: q // 2 not in first}
    return [("zero: " + n % _vname(lo), [2 * P if hi(q) else lo for q in range(12)])
            for n, hi in shapes.items() for lo in (0, P)]


def _gen_cyc_sqr(bound):
    def gen():
        recs = [_of(r, "cyclotomic" if "cyclotomic #" in r.name else "zero / one", bound=bound)
                for r in tv.records("fp12_cyclotomic_sqr")]
        return recs + [_tower_krec("cyc_sqr %s" % n, "zero, one-sided 2p", v, [0] * 12, bound)
                       for n, v in _one_sided_zeros()]
    return gen


def gen_g6_is_one():
    return [_of(r, "one" if r.status else ("near miss" if "off by one" in r.name else "not one"))
            for r in tv.records("fp12_is_one")]


def gen_g6_line_mul():
    """f, the line record (l0, c1, c4) and P = (xP, yP): f (l0 + c1 xP w^2 + c4 yP w^3)"""
    rng = random.Random(13801)
    recs = []
    pats = [(n, _edge_cls(n), f + [stored(rng) for _ in range(8)]) for n, f in tv._fp12_patterns(rng, 90)]
    pats += [("all %s" % _vname(e), "edge", [e] * 20) for e in E2]
    pats += [(n, "one coefficient fixed", v) for n, v in _single_coef(rng, 20, stored, "")]
    for n, cls, v in pats:
        s = _std(v)
        xp, yp = s[18], s[19]
        l1 = bls.f2muls(_f2(s[14:16]), xp)
        l4 = bls.f2muls(_f2(s[16:18]), yp)
        want = bls.f12mul(_f12(s[:12]), tv._line12(_f2(s[12:14]), l1, l4))
        recs.append(_tower_krec("g6_line_mul %s" % n, cls, v, _mont(want), BOUND_LC))
    return recs


@functools.lru_cache(maxsize=None)
def _final_exp_inputs():
    """a handful of Fp12 values in redundant representation with the oracle's final exponentiation (e^3): Miller values
    of pool points and random elements; canonical, + p and mixed"""
    rng = random.Random(14101)
    out = []
    g1, g2 = cv.pool("g1"), cv.pool("g2")
    vals = [("miller(%s, %s)" % (g1[-1 - i].name, g2[-1 - i].name), bls.miller_loop(g1[-1 - i].aff, g2[-1 - i].aff))
            for i in range(4)]
    vals += [("random #%d" % i, _f12([rng.randrange(P) for _ in range(12)])) for i in range(4)]
    vals.append(("one", bls.F12_ONE))
    for i, (n, f) in enumerate(vals):
        mode = cv.MODES[i % 3]
        out.append(("%s %s" % (n, mode), tv._reps(rng, _mont(f), mode), _mont(bls.final_exp(f))))
    f = vals[0][1]
    out.append(("%s + p, zeros 2p" % vals[0][0], [x + P for x in _mont(f)], _mont(bls.final_exp(f))))
    return out


def _gen_final_exp(tag, bound):
    def gen():
        return [_tower_krec("%s %s" % (tag, n), "miller value" if "miller" in n else "other", raw, want, bound)
                for n, raw, want in _final_exp_inputs()]
    return gen


# ------------------------------------------------------------------------------------------------ g2c
def _g2c_rec(rng, r, raw_addend=None):
    """a live g2c element from a one-lane G2 record: the flag slot (word 0 set, the rest arbitrary), the point, the
    addend (the record's, or arbitrary stored values the op does not read); every output a lacc_fin result: <= 2p"""
    flag = [1 + rng.randrange(1 << 32 - 1)] + [rng.randrange(1 << 32) for _ in range(NL - 1)]
    ins = list(r.ins)
    if len(ins) == 6:
        ins = ins + [limbs(stored(rng)) for _ in range(6)]
    return KRec(r.name, r.cls, [flag] + ins, r.want, [BOUND_2P] * 6, exact=r.exact, post=r.post)


def _g2c_off(rng, i):
    """an element flagged off: word 0 of the flag slot is zero, everything else arbitrary words (no valid limbs), whole
    slots of all-ones among them; the group must run every phase on them and write nothing (the output stays zero)"""
    kind = i % 4
    slots = []
    for k in range(13):
        if kind == 0 or (kind == 2 and k % 2):
            slots.append([0xFFFFFFFF] * NL)
        elif kind == 3 and k % 3 == 0:
            slots.append([0] * NL)
        else:
            slots.append([rng.randrange(1 << 32) for _ in range(NL)])
    if kind == 0 and i:  # (distinct records: one all-ones element, the others differ in a word)
        slots[1 + i % 12][i % NL] = rng.randrange(1 << 32)
    slots[0][0] = 0
    return KRec("off #%d (%s)" % (i, ("all-ones", "random words", "all-ones / random", "zeros / random")[kind]), "off",
                slots, [None] * 6, [0] * 6, exact=[0] * 6)


def _g2c_2p_points(rng, with_q):
    """the lacc users' operands: every coordinate at 2p, and 2p in the real / the imaginary parts only (points by
    value, off the curve: the reference is the affine law on x = X / Z^2, y = Y / Z^3)"""
    G = cv.G2
    out = []
    shapes = {"all 2p": lambda c: 2 * P, "real parts 2p": lambda c: 2 * P if c == 0 else None,
              "imaginary parts 2p": lambda c: 2 * P if c == 1 else None}

    def point(f):
        return [f(k % 2) if f(k % 2) is not None else rng.randrange(1, P) + P * rng.randrange(2) for k in range(6)]

    def aff_of(raw):
        X, Y, Z = (G.elem([s_(v) for v in raw[2 * k:2 * k + 2]]) for k in range(3))
        if G.F.is_zero(Z):
            return None
        zi = G.F.inv(Z)
        zi2 = G.F.sqr(zi)
        return (G.F.mul(X, zi2), G.F.mul(Y, G.F.mul(zi2, zi)))

    for (na, fa), (nb, fb) in itertools.product(shapes.items(), repeat=2):
        a, b = point(fa), point(fb)
        if with_q:
            ref = cv.aff_add(G, aff_of(a), aff_of(b))
            out.append(("[%s] + [%s]" % (na, nb), a + b, ref))
        elif na == nb:
            pa = aff_of(a)
            out.append(("[%s]" % na, a, cv.aff_add(G, pa, pa)))
    return out


def _gen_g2c(cv_name, tag, with_q):
    def gen():
        rng = random.Random(14200 + len(tag))
        extra = _order13_chain_recs() if tag == "g2c_mul_zabs" else []
        recs = [_g2c_rec(rng, r) for r in list(cv.records(cv_name)) + extra]
        if tag != "g2c_mul_zabs":
            for n, raw, ref in _g2c_2p_points(rng, with_q):
                r = cv._jrec(cv.G2, "%s %s" % (tag, n), "2p operands", raw, ref, [BOUND_2P] * 6)
                recs.append(_g2c_rec(rng, r))
        for i in range(max(24, len(recs) // 4)):
            recs.append(_g2c_off(rng, i))
        return recs
    return gen


# ------------------------------------------------------------------------------------------------ gtw
def gen_gtw_sqr_alias():  # A = B = C: the square, from one operand
    rng = random.Random(14801)
    recs = [_of(r, _edge_cls(r.name), bound=BOUND_2P) for r in tv.records("fp12_sqr")]
    for n, v in [("real 2p, imaginary 0", [2 * P, 0] * 6), ("real 0, imaginary 2p", [0, 2 * P] * 6),
                 ("c0 2p, c1 0", [2 * P] * 6 + [0] * 6), ("c0 0, c1 2p", [0] * 6 + [2 * P] * 6)]:
        recs.append(_tower_krec("gtw_mul(V, V, V) %s" % n, "edge", v, _sqr_ref(v), BOUND_2P))
    return recs + _fp12_one_fixed_recs("gtw_mul(V, V, V)", 14802, _sqr_ref, BOUND_2P)


def gen_gtw_mul_sparse():
    return [_of(r, _edge_cls(r.name), bound=BOUND_2P) for r in tv.records("fp12_mul_by_014")]


def gen_gtw_miller():
    """P and Q from the curve pools (small orders, subgroup, outside), every coordinate canonical, + p or mixed"""
    rng = random.Random(15701)
    g1, g2 = cv.pool("g1"), cv.pool("g2")
    picks = [(0, 0), (2, 1), (-1, -1), (-2, 4), (9, 5), (len(g1) // 2, -2), (5, 2), (12, 3), (1, 6), (-3, 0)]
    recs = []
    for i, (a, b) in enumerate(picks):
        pp, qq = g1[a], g2[b]
        mode = cv.MODES[i % 3]
        raw = cv.aff_raw(cv.G1, pp.aff, mode, rng) + cv.aff_raw(cv.G2, qq.aff, cv.MODES[(i + 1) % 3], rng)
        recs.append(_tower_krec("gtw_miller_loop(%s, %s) %s" % (pp.name, qq.name, mode),
                                "subgroup" if pp.in_subgroup and qq.in_subgroup else "other", raw,
                                _mont(bls.miller_loop(pp.aff, qq.aff)), BOUND_2P))
    return recs


# ------------------------------------------------------------------------------------------------ the op table
def _unary12(tv_name, bound):
    return _gen_fp12_from(tv_name, None, 0, None, bound)


OPS = [
    Op("lacc_fin", 108, "lane", 2, 1, gen_lacc_fin, host=True),
    Op("fp2x_mul", 109, "pair", 4, 2, gen_fp2x_mul),
    Op("fp2x_sqr", 110, "pair", 2, 2, gen_fp2x_sqr),
    Op("fp2x_mul_xi", 111, "pair", 2, 2, gen_fp2x_mul_xi),
    Op("fp2x_norm", 112, "pair", 2, 2, gen_fp2x_norm),
    Op("fp2x_is_zero", 113, "pair", 2, 0, gen_f_is_zero),
    Op("lc_xi<1; 1>", 114, "pair", 4, 2, _gen_lc_xi("lc_xi<1; 1>", 1, (1,))),
    Op("lc_xi<1; 1,-1,-1>", 115, "pair", 8, 2, _gen_lc_xi("lc_xi<1; 1,-1,-1>", 1, (1, -1, -1))),
    Op("lc_xi<-1; 1,-1>", 116, "pair", 6, 2, _gen_lc_xi("lc_xi<-1; 1,-1>", -1, (1, -1))),
    Op("lc_xi<1; 1,-1>", 117, "pair", 6, 2, _gen_lc_xi("lc_xi<1; 1,-1>", 1, (1, -1))),
    Op("lc_xi<3; 4,-5>", 118, "pair", 6, 2, _gen_lc_xi("lc_xi<3; 4,-5>", 3, (4, -5))),  # total weight 15
    Op("fp6x_mul", 119, "pair", 12, 6, gen_fp6x_mul),
    Op("fp12x_sqr", 120, "pair", 12, 12, gen_fp12x_sqr),
    Op("fp12x_mul_by_014", 121, "pair", 18, 12, gen_fp12x_mul_by_014),
    Op("miller_dbl_line", 122, "pair", 6, 12, gen_miller_dbl_line),
    Op("miller_add_line", 123, "pair", 10, 12, gen_miller_add_line),
    Op("g2x_jac_dbl", 124, "pair", 6, 6, _gen_pair_point("g2_jac_dbl")),
    Op("g2x_jac_add", 125, "pair", 12, 6, _gen_pair_point("g2_jac_add")),
    Op("g2x_jac_add_aff", 126, "pair", 10, 6, _gen_pair_point("g2_jac_add_aff")),
    Op("g2x_jac_neg", 127, "pair", 6, 6, _gen_pair_point("g2_jac_neg")),
    Op("g2x_jac_is_inf", 128, "pair", 6, 0, _gen_pair_point("g2_jac_is_inf")),
    Op("g2x_psi", 129, "pair", 6, 6, _gen_pair_point("g2_psi")),
    Op("g2x_psi2", 130, "pair", 6, 6, _gen_pair_point("g2_psi2")),
    Op("g2x_jac_mul_zabs", 131, "pair", 6, 6, _gen_pair_point("g2_jac_mul_zabs")),
    Op("g6_mul", 132, "g6", 24, 12, gen_fp12_mul_pairs("g6_mul", 13201, BOUND_LC)),
    Op("g6_sqr", 133, "g6", 12, 12, _gen_fp12_from("fp12_sqr", "g6_sqr", 13301, _sqr_ref, BOUND_LC)),
    Op("g6_cyc_sqr", 134, "g6", 12, 12, _gen_cyc_sqr(BOUND_LC)),
    Op("g6_frob1", 135, "g6", 12, 12, _unary12("fp12_frob1", BOUND_DOT)),
    Op("g6_frob2", 136, "g6", 12, 12, _unary12("fp12_frob2", BOUND_DOT)),
    Op("g6_conj", 137, "g6", 12, 12, _unary12("fp12_conj", BOUND_2P)),
    Op("g6_line_mul", 138, "g6", 20, 12, gen_g6_line_mul),
    Op("g6_is_one", 139, "g6", 12, 0, gen_g6_is_one),
    Op("g6_pow_z", 140, "g6", 12, 12, _gen_pow_z(BOUND_2P)),
    Op("g6_final_exp", 141, "g6", 12, 12, _gen_final_exp("g6_final_exp", BOUND_LC)),
    Op("g2c_dbl", 142, "g2c", 13, 6, _gen_g2c("g2_jac_dbl", "g2c_dbl", False), host=True),
    Op("g2c_add", 143, "g2c", 13, 6, _gen_g2c("g2_jac_add", "g2c_add", True), host=True),
    Op("g2c_mul_zabs", 144, "g2c", 13, 6, _gen_g2c("g2_jac_mul_zabs", "g2c_mul_zabs", False), host=True),
    Op("gtw_mul", 145, "gtw", 24, 12, gen_fp12_mul_pairs("gtw_mul", 14501, BOUND_2P), host=True),
    Op("gtw_mul C=A", 146, "gtw", 24, 12, gen_fp12_mul_pairs("gtw_mul C=A", 14601, BOUND_2P), host=True),
    Op("gtw_mul C=B", 147, "gtw", 24, 12, gen_fp12_mul_pairs("gtw_mul C=B", 14701, BOUND_2P), host=True),
    Op("gtw_mul A=B=C", 148, "gtw", 12, 12, gen_gtw_sqr_alias, host=True),
    Op("gtw_mul sparse", 149, "gtw", 18, 12, gen_gtw_mul_sparse, host=True),
    Op("gtw_cyc_sqr D=A", 150, "gtw", 12, 12, _gen_cyc_sqr(BOUND_2P)),
    Op("gtw_cyc_sqr", 151, "gtw", 12, 12, _gen_cyc_sqr(BOUND_2P)),
    Op("gtw_conj", 152, "gtw", 12, 12, _unary12("fp12_conj", BOUND_2P)),
    Op("gtw_frob1", 153, "gtw", 12, 12, _unary12("fp12_frob1", BOUND_2P)),
    Op("gtw_frob2", 154, "gtw", 12, 12, _unary12("fp12_frob2", BOUND_2P)),
    Op("gtw_pow_z", 155, "gtw", 12, 12, _gen_pow_z(BOUND_2P)),
    Op("gtw_final_exp", 156, "gtw", 12, 12, _gen_final_exp("gtw_final_exp", BOUND_2P)),
    Op("gtw_miller_loop", 157, "gtw", 6, 12, gen_gtw_miller, host=True),
]
OP_NAMES = [o.name for o in OPS]
HOST_OP_NAMES = [o.name for o in OPS if o.host]
BY_NAME = {o.name: o for o in OPS}
assert [o.code for o in OPS] == list(range(108, 158))
# the whole chains: about ten records each (no second block); everything else fills more than one block
CHAIN_OPS = ("g6_final_exp", "gtw_final_exp", "gtw_miller_loop")
# every user of lacc_fin the host build can run (the audit of tests/test_coop_contracts.py)
LACC_USERS = ("g2c_dbl", "g2c_add", "g2c_mul_zabs", "gtw_mul", "gtw_mul C=A", "gtw_mul C=B", "gtw_mul A=B=C",
              "gtw_mul sparse", "gtw_miller_loop")


@functools.lru_cache(maxsize=None)
def records(name):
    """the op's records (computed once per process; shared, not to be modified): distinct operands, more than one
    block of the engine's kernel and a partly filled last one"""
    op = BY_NAME[name]
    seen, recs = set(), []
    for r in op.gen():
        key = tuple(tuple(l) for l in r.ins)
        if key not in seen:
            seen.add(key)
            recs.append(r)
    blk = BLOCK[op.engine]
    if blk > 1 and name not in CHAIN_OPS:
        while len(recs) % blk == 0:
            recs.pop()
        assert len(recs) > blk, name
    for r in recs:
        assert len(r.ins) == op.n_in and len(r.want) == len(r.bound) == op.n_out, r.name
    return recs


def check(name, outs, statuses, recs=None):
    """tower_vectors.check on this module's records (`recs`: a subset of them, in the order of `outs`)"""
    return tv.check(name, outs, statuses, op=BY_NAME[name], recs=records(name) if recs is None else recs)


def format_failures(name, bad, limit=12):
    return tv.format_failures(name, bad, limit, total=len(records(name)))


def _arrange(items, start, slot, blk):
    """`items` in an order close to the given one for the positions start, start + 1, ... such that none sits at the
    position within its block that `slot` gives it; None where the items alone cannot be arranged so"""
    rest, out = list(items), []
    for j in range(start, start + len(items)):
        k = next((k for k, r in enumerate(rest) if slot[r] != j % blk), None)
        if k is not None:
            out.append(rest.pop(k))
            continue
        r = rest.pop(0)  # only records of this very slot are left: trade places with one placed earlier
        m = next((m for m, q in enumerate(out) if slot[q] != j % blk and slot[r] != (start + m) % blk), None)
        if m is None:
            return None
        out.append(out[m])
        out[m] = r
    return out


def launch_orders(name):
    """Two orders of the op's records, as index lists.  `interleaved`: every branch class spread evenly over the launch,
    so neighbouring pairs / groups hold different data on different branches.  `grouped`: first, class by class (the
    largest first), as many whole waves of every class as it fills, each starting at a wave boundary -- so a class of
    at least a wave's elements has a wave in which every lane takes its branch; then what is left of the classes.  No
    record keeps the position within its block that it has in the interleaved order."""
    recs = records(name)
    eng = BY_NAME[name].engine
    blk, wave = BLOCK[eng], WAVE[eng]
    by_cls = {}
    for i, r in enumerate(recs):
        by_cls.setdefault(r.cls, []).append(i)
    groups = sorted(by_cls.values(), key=len, reverse=True)
    keyed = sorted(((k + 0.5) / len(g), gi, i) for gi, g in enumerate(groups) for k, i in enumerate(g))
    inter = [i for _, _, i in keyed]
    if blk == 1:
        return inter, [i for g in groups for i in g]
    slot = {r: j % blk for j, r in enumerate(inter)}
    grouped, left = [], []
    for g in groups:
        whole = len(g) // wave * wave
        for c in range(0, whole, wave):
            placed = _arrange(g[c:c + wave], len(grouped), slot, blk)
            if placed is None:
                left += g[c:c + wave]
            else:
                grouped += placed
        left += g[whole:]
    grouped += _arrange(left, len(grouped), slot, blk)
    assert sorted(grouped) == list(range(len(recs))) and all(slot[r] != j % blk for j, r in enumerate(grouped)), name
    return inter, grouped


def wave_classes(name, order):
    """the set of branch classes in each 64-lane wave of a launch in `order`"""
    recs = records(name)
    n = WAVE[BY_NAME[name].engine]
    return [{recs[i].cls for i in order[w:w + n]} for w in range(0, len(order), n)]
