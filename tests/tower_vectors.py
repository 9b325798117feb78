"""Test vectors for the field tower (lodestar_amd/csrc/fp.hpp, tower.hpp, pairing.hpp fp12_pow_zabs) at the edges of
its operand contracts, shared by the host test (tests/test_tower_contracts.py, through tests/native/emu.cpp) and the
device test (tests/test_gpu_tower_contracts.py, blsgpu_debug_op ops 32..68).  Plain Python, fixed seeds; the only
reference is the oracle (oracle/bls12_381.py) and Python integers -- nothing here calls the code under test.

Values are raw: 14 limbs of 28 bits per Fp value, exactly as the code holds them.  The code works in Montgomery form
with R = 2^392, which the vectors never enter or leave: an operation on raw integers is expected to return
R * op(x / R, ...) mod p -- a product of raw a, b gives a b / R, an inverse of raw a gives R^2 / a, additive operations
carry no factor, and the Montgomery one is R mod p.

Operand domains follow the header comments:
  stored values        normalized limbs (limbs 0..12 < 2^28), value in [0, 2p]: every representative of a residue
  fp_mul, fp2_mul_fp   limbs < 2^30, values < 16p (fp_add_nr of four stored values, fp_sub_k8's a + 8p - b)
  fp_sqr               limbs < 2^29, values <= 4p
  fp2_mul              limbs < 2^29, values <= 8p, 8p itself included (fp6_mul's un-normalized 4p + 4p)
  fp2_sqr, fp6_mul, fp6_mul_by_01, fp6_mul_by_12   normalized, values <= 4p (fp_add_norm of two stored values)
Every record carries, per output, the expected residue and an inclusive upper bound of the value: the header's stated
bound (fp_lc outputs < 1.003 p, fp_half <= 1.5 p, fp_canon in [0, p), fp2_mul < 1.1 p, fp2_sqr and fp_inv < 1.05 p),
the derived bound out < p + (product of the operands) / 2^392 for the plain Montgomery products, and otherwise the
stored-value invariant <= 2p.  check() also requires limbs 0..12 of every output below 2^28."""
import functools
import random

from oracle import bls12_381 as bls

P = bls.P
NL = 14
LB = 28
MASK = (1 << LB) - 1
R = 1 << (NL * LB)
RM = R % P  # the Montgomery one
RINV = pow(R, -1, P)
Z_ABS = bls.BLS_X_ABS
BOUND_2P = 2 * P


def lt_frac(num, den):
    """largest integer v with v < (num / den) p"""
    return (num * P - 1) // den


BOUND_LC = lt_frac(1003, 1000)


def limbs(v):
    """normalized limbs: 0..12 in [0, 2^28), the top limb holds the rest"""
    return [(v >> (LB * i)) & MASK for i in range(NL - 1)] + [v >> (LB * (NL - 1))]


def val(l):
    return sum(int(x) << (LB * i) for i, x in enumerate(l))


def borrowed(v, rng, bits, full=False):
    """_limbs_of's borrow pattern (tests/test_emu_logic.py): units of limb i + 1 moved down into limb i as 2^28 each,
    as many as keep every limb below 2^bits (one for 2^29, three for 2^30); `full` borrows the most everywhere."""
    l = limbs(v)
    most = (1 << (bits - LB)) - 1
    for i in range(NL - 1):
        k = min(most, l[i + 1])
        if not full:
            k = rng.randint(0, k)
        l[i + 1] -= k
        l[i] += k << LB
    assert val(l) == v and all(0 <= x < (1 << bits) for x in l)
    return l


def saturated(bits, vmax):
    """every limb below the top at 2^bits - 1, the top limb the largest that keeps the value <= vmax"""
    l = [(1 << bits) - 1] * (NL - 1)
    l.append((vmax - val(l)) >> (LB * (NL - 1)))
    assert 0 <= l[-1] and val(l) <= vmax
    return l


def add_nr(*ls):
    """fp_add_nr: the limb-wise sum, no carries"""
    return [sum(x) for x in zip(*ls)]


def _fp_8p_k():
    """fp.hpp FP_8P_K: 8p with every limb but the top borrowed up into [2^28 - 1, 2^29)"""
    l = limbs(8 * P)
    l[0] += 1 << LB
    for i in range(1, NL - 1):
        l[i] += (1 << LB) - 1
    l[NL - 1] -= 1
    assert val(l) == 8 * P
    return l


FP_8P_K = _fp_8p_k()


def sub_k8(la, lb):
    """fp_sub_k8: a + FP_8P_K - b limb by limb"""
    l = [a + k - b for a, k, b in zip(la, FP_8P_K, lb)]
    assert all(0 <= x < (1 << 30) for x in l)
    return l


def edge_values(K, closed=True):
    """{0, 1, p - 1, p, p + 1, 2p - 1, 2p, ..., Kp - 1, Kp}; without Kp for a contract that says `<`"""
    out = [0, 1]
    for j in range(1, K + 1):
        out += [j * P - 1, j * P, j * P + 1]
    out.pop()
    if not closed:
        out.pop()
    return out


E2 = edge_values(2)
E4 = edge_values(4)
E8 = edge_values(8)
E16 = edge_values(16, closed=False)
# stored values whose limbs are at their extremes (all ones, a single bit at a limb boundary)
LIMB_EDGES = [MASK, 1 << LB, (1 << (LB * 13)) - 1, 1 << (LB * 13), (1 << 381) - 1, 2 * P - (1 << LB), 2 * P - MASK]


class Rec:
    """One test vector: `ins` = the operands' limb lists; per output the expected residue (`want`, None = any), the
    inclusive bound of the value (`bound`) and, where the value itself is fixed, `exact`; `status` = the status word;
    `post` = an extra check on the output values (fp2_sqrt's root)."""
    __slots__ = ("name", "ins", "want", "bound", "exact", "status", "post")

    def __init__(self, name, ins, want, bound, exact=None, status=0, post=None):
        self.name, self.ins, self.want, self.bound, self.exact, self.status, self.post = (
            name, ins, want, bound, exact, status, post)


class Op:
    def __init__(self, name, code, n_in, n_out, gen):
        self.name, self.code, self.n_in, self.n_out, self.gen = name, code, n_in, n_out, gen


def _finish(recs):
    """distinct operands in every record (no two lanes of a launch hold the same data); a count that leaves the last
    128-lane workgroup partly filled"""
    seen, out = set(), []
    for r in recs:
        key = tuple(tuple(l) for l in r.ins)
        if key not in seen:
            seen.add(key)
            out.append(r)
    if len(out) % 128 == 0:
        out.pop()  # (the generators end with their random records)
    assert len(out) > 128
    return out


# ------------------------------------------------------------------------------------------------ operand shapes
def stored(rng):
    """a stored value: an edge of [0, 2p], a limb-pattern edge, or random"""
    x = rng.random()
    if x < 0.3:
        return rng.choice(E2)
    if x < 0.4:
        return rng.choice(LIMB_EDGES)
    return rng.randrange(2 * P + 1)


def upto(rng, edges, vmax):
    return rng.choice(edges) if rng.random() < 0.4 else rng.randrange(vmax + 1)


def mul_operand(rng):
    """an fp_mul operand (limbs < 2^30, value < 16p) -> (limbs, label)"""
    shape = rng.choice(["norm", "borrow", "full", "add4", "add4", "subk8", "subk8", "sat"])
    if shape in ("norm", "borrow", "full"):
        v = upto(rng, E16, 16 * P - 1)
        l = limbs(v) if shape == "norm" else borrowed(v, rng, 30, full=shape == "full")
        return l, "%s(%s)" % (shape, _vname(v))
    if shape == "add4":
        t = [stored(rng) for _ in range(rng.choice([2, 3, 4, 4]))]
        return add_nr(*[limbs(x) for x in t]), "add_nr(%s)" % ",".join(_vname(x) for x in t)
    if shape == "subk8":
        a, b = upto(rng, E4, 4 * P), upto(rng, E4, 4 * P)
        if rng.random() < 0.5:  # a as one fp_add_nr level
            a0, a1 = stored(rng), stored(rng)
            return sub_k8(add_nr(limbs(a0), limbs(a1)), limbs(b)), "sub_k8(add_nr(%s,%s),%s)" % (
                _vname(a0), _vname(a1), _vname(b))
        return sub_k8(limbs(a), limbs(b)), "sub_k8(%s,%s)" % (_vname(a), _vname(b))
    return saturated(30, 16 * P - 1), "saturated30"


def sqr_operand(rng, edges, vmax, half_edges, bits=29):
    """limbs < 2^bits, value <= vmax: normalized, borrowed, or one fp_add_nr level of two values <= vmax / 2
    -> (limbs, label)"""
    shape = rng.choice(["norm", "borrow", "full", "add2", "add2"])
    if shape == "add2":
        a = upto(rng, half_edges, vmax // 2)
        b = rng.choice([a, upto(rng, half_edges, vmax // 2)])
        return add_nr(limbs(a), limbs(b)), "add_nr(%s,%s)" % (_vname(a), _vname(b))
    v = upto(rng, edges, vmax)
    l = limbs(v) if shape == "norm" else borrowed(v, rng, bits, full=shape == "full")
    return l, "%s(%s)" % (shape, _vname(v))


def _vname(v):
    """a short readable name of a value: k p + d for small d, else its size in units of p"""
    k, d = divmod(v, P)
    if d > P // 2:
        k, d = k + 1, d - P
    if abs(d) < 1000:
        kp = "%dp" % k if k > 1 else "p"
        return (kp + ("%+d" % d if d else "")) if k else str(d)
    return "~%.3fp" % (v / P)


def s_(x):
    return x * RINV % P


def m_(x):
    return x * RM % P


def _mont_bound(*ops):
    """out < p + prod / 2^392"""
    prod = 1
    for x in ops:
        prod *= x
    return (P * R + prod - 1) // R


# ------------------------------------------------------------------------------------------------ Fp, Fp2 products
def gen_fp_mul():
    rng = random.Random(3201)
    recs = []

    def rec(name, la, lb):
        a, b = val(la), val(lb)
        recs.append(Rec(name, [la, lb], [a * b * RINV % P], [_mont_bound(a, b)]))

    for a in E16:
        for b in E16:
            rec("fp_mul edges %s * %s" % (_vname(a), _vname(b)), limbs(a), limbs(b))
    sat = saturated(30, 16 * P - 1)
    rec("fp_mul saturated30^2", sat, sat)
    for a in (0, 16 * P - 1, 8 * P):
        rec("fp_mul saturated30 * %s" % _vname(a), sat, limbs(a))
        rec("fp_mul full-borrow(16p-1) * %s" % _vname(a), borrowed(16 * P - 1, rng, 30, True),
            borrowed(a, rng, 30, True))
    for i in range(1000):
        (la, na), (lb, nb) = mul_operand(rng), mul_operand(rng)
        rec("fp_mul #%d %s * %s" % (i, na, nb), la, lb)
    return recs


def gen_fp_sqr():
    rng = random.Random(3301)
    recs = []

    def rec(name, la):
        a = val(la)
        recs.append(Rec(name, [la], [a * a * RINV % P], [_mont_bound(a, a)]))

    for a in E4 + [x for x in LIMB_EDGES]:
        rec("fp_sqr %s" % _vname(a), limbs(a))
        rec("fp_sqr full-borrow %s" % _vname(a), borrowed(a, rng, 29, True))
    for a in E2:
        for b in E2:
            rec("fp_sqr add_nr(%s,%s)" % (_vname(a), _vname(b)), add_nr(limbs(a), limbs(b)))
    rec("fp_sqr saturated29", saturated(29, 4 * P))
    for i in range(1000):
        la, na = sqr_operand(rng, E4, 4 * P, E2)
        rec("fp_sqr #%d %s" % (i, na), la)
    return recs


def _fp2_mul_rec(name, ls):
    a0, a1, b0, b1 = (val(l) for l in ls)
    return Rec(name, list(ls), [(a0 * b0 - a1 * b1) * RINV % P, (a0 * b1 + a1 * b0) * RINV % P],
               [lt_frac(11, 10)] * 2)


def gen_fp2_mul():
    rng = random.Random(3401)
    recs = []
    p4 = limbs(4 * P)
    forms = {"4p+4p": add_nr(p4, p4), "8p": limbs(8 * P), "full-borrow(8p)": borrowed(8 * P, rng, 29, True)}
    for n, l8 in forms.items():
        recs.append(_fp2_mul_rec("fp2_mul all four at %s" % n, [l8] * 4))
    z = limbs(0)
    for mask in range(16):  # every corner of {0, 8p}^4, 8p as the un-normalized 4p + 4p
        ls = [forms["4p+4p"] if (mask >> k) & 1 else z for k in range(4)]
        recs.append(_fp2_mul_rec("fp2_mul corner %s" % format(mask, "04b"), ls))
    for a in E8[-5:]:  # the top of the range against itself, normalized
        for b in E8[-5:]:
            recs.append(_fp2_mul_rec("fp2_mul top %s,%s" % (_vname(a), _vname(b)),
                                     [limbs(a), limbs(b), limbs(b), limbs(a)]))
    sat = saturated(29, 8 * P)
    recs.append(_fp2_mul_rec("fp2_mul saturated29 x4", [sat] * 4))
    for i in range(1500):
        ops = [sqr_operand(rng, E8, 8 * P, E4) for _ in range(4)]
        recs.append(_fp2_mul_rec("fp2_mul #%d %s" % (i, " ".join(n for _, n in ops)), [l for l, _ in ops]))
    return recs


def gen_fp2_sqr():
    rng = random.Random(3501)
    recs = []

    def rec(name, a0, a1):
        recs.append(Rec(name, [limbs(a0), limbs(a1)], [(a0 * a0 - a1 * a1) * RINV % P, 2 * a0 * a1 * RINV % P],
                        [lt_frac(105, 100)] * 2))

    for a0 in E4:
        for a1 in E4:
            rec("fp2_sqr edges %s,%s" % (_vname(a0), _vname(a1)), a0, a1)
    for i in range(150):  # a1 - a0 > 2p
        rec("fp2_sqr underflow-shape #%d" % i, rng.randrange(P // 8), rng.randrange(3 * P, 4 * P + 1))
    for i in range(1000):
        a0 = stored(rng) + stored(rng) if rng.random() < 0.5 else upto(rng, E4, 4 * P)
        a1 = stored(rng) + stored(rng) if rng.random() < 0.5 else upto(rng, E4, 4 * P)
        rec("fp2_sqr #%d %s,%s" % (i, _vname(a0), _vname(a1)), a0, a1)
    return recs


def gen_fp2_mul_fp():
    rng = random.Random(3601)
    recs = []

    def rec(name, l0, l1, ls):
        a0, a1, s = val(l0), val(l1), val(ls)
        recs.append(Rec(name, [l0, l1, ls], [a0 * s * RINV % P, a1 * s * RINV % P],
                        [_mont_bound(a0, s), _mont_bound(a1, s)]))

    top = [0, 1, P, 2 * P, 16 * P - 1]
    for a0 in top:
        for a1 in top:
            for s in top:
                rec("fp2_mul_fp edges (%s,%s) * %s" % (_vname(a0), _vname(a1), _vname(s)), limbs(a0), limbs(a1),
                    limbs(s))
    sat = saturated(30, 16 * P - 1)
    rec("fp2_mul_fp saturated30 x3", sat, sat, sat)
    for i in range(400):
        a0, a1, s = stored(rng), stored(rng), stored(rng)
        rec("fp2_mul_fp stored #%d" % i, limbs(a0), limbs(a1), limbs(s))
    for i in range(600):
        ops = [mul_operand(rng) for _ in range(3)]
        rec("fp2_mul_fp #%d %s" % (i, " ".join(n for _, n in ops)), *[l for l, _ in ops])
    return recs


# ------------------------------------------------------------------------------------------------ additive glue
def _unary_values(rng, n):
    return E2 + LIMB_EDGES + [rng.randrange(2 * P + 1) for _ in range(n)]


def _gen_unary(name, seed, f, bound=BOUND_2P, exact=False, n=800):
    def gen():
        rng = random.Random(seed)
        recs = []
        for a in _unary_values(rng, n):
            w = f(a)
            recs.append(Rec("%s(%s)" % (name, _vname(a)), [limbs(a)], [w % P], [bound], exact=[w] if exact else None))
        return recs
    return gen


def _gen_binary(name, seed, f, bound=BOUND_2P, exact=False, n=1000):
    def gen():
        rng = random.Random(seed)
        recs = []
        ed = E2 + LIMB_EDGES
        pairs = [(a, b) for a in ed for b in ed] + [(stored(rng), stored(rng)) for _ in range(n)]
        for a, b in pairs:
            w = f(a, b)
            recs.append(Rec("%s(%s, %s)" % (name, _vname(a), _vname(b)), [limbs(a), limbs(b)], [w % P],
                            [4 * P if exact else bound], exact=[w] if exact else None))
        return recs
    return gen


def gen_fp2_mul_xi():
    rng = random.Random(4701)
    ed = E2 + LIMB_EDGES
    pairs = [(a, b) for a in ed for b in ed] + [(stored(rng), stored(rng)) for _ in range(1000)]
    return [Rec("fp2_mul_xi(%s, %s)" % (_vname(a), _vname(b)), [limbs(a), limbs(b)], [(a - b) % P, (a + b) % P],
                [BOUND_2P] * 2) for a, b in pairs]


# ------------------------------------------------------------------------------------------------ predicates
def gen_fp_is_zero():
    rng = random.Random(4801)
    recs = [Rec("fp_is_zero(%s)" % _vname(a), [limbs(a)], [], [], status=int(a in (0, P, 2 * P)))
            for a in _unary_values(rng, 300)]
    assert sum(r.status for r in recs) == 3
    return recs


def gen_fp_eq():
    rng = random.Random(4901)
    ed = E2 + LIMB_EDGES
    pairs = [(a, b) for a in ed for b in ed]
    for _ in range(150):
        r = rng.randrange(P)
        d = rng.choice([-1, 1])
        r1 = (r + d) % P
        pairs += [(r, r + P), (r + P, r), (r, r1), (r + P, r1), (r, r1 + P), (r + P, r1 + P)]
    pairs += [(stored(rng), stored(rng)) for _ in range(200)]
    pairs = [(a, b) for a, b in pairs if a <= 2 * P and b <= 2 * P]
    return [Rec("fp_eq(%s, %s)" % (_vname(a), _vname(b)), [limbs(a), limbs(b)], [], [], status=int((a - b) % P == 0))
            for a, b in pairs]


def gen_fp12_is_one():
    rng = random.Random(5001)
    recs = []

    def rec(name, vals, want):
        assert all(0 <= v <= 2 * P for v in vals)
        recs.append(Rec(name, [limbs(v) for v in vals], [], [], status=want))

    def one():
        return [rng.choice([RM, RM + P])] + [rng.choice([0, P, 2 * P]) for _ in range(11)]

    for z in (0, P, 2 * P):
        for o in (RM, RM + P):
            rec("fp12_is_one: %s, zeros all %s" % (_vname(o), _vname(z)), [o] + [z] * 11, 1)
    for i in range(150):
        rec("fp12_is_one: one #%d" % i, one(), 1)
    for i in range(240):  # near misses: one coefficient off by one
        v = one()
        k = i % 12
        v[k] += rng.choice([-1, 1]) if v[k] not in (0, 2 * P) else (1 if v[k] == 0 else -1)
        rec("fp12_is_one: coefficient %d off by one #%d" % (k, i), v, 0)
    for k in range(1, 12):  # the one in the wrong place
        v = [0] * 12
        v[k] = RM
        rec("fp12_is_one: one at coefficient %d" % k, v, 0)
    rec("fp12_is_one: zero", [2 * P] * 12, 0)
    rec("fp12_is_one: plain 1 (not the Montgomery one)", [1] + [0] * 11, 0)
    for i in range(40):
        rec("fp12_is_one: random #%d" % i, [stored(rng) for _ in range(12)], 0)
    return recs


# ------------------------------------------------------------------------------------------------ inversion, roots
def _inv_values():
    """the divsteps list of tests/test_emu_logic.py test_fp_inv_divsteps_edges_and_random: its edges and the first
    half of its random stream (every value is used twice here, as v and as v + p)"""
    fib = [1, 1]
    while fib[-1] < P:
        fib.append(fib[-1] + fib[-2])
    vals = [0, 1, 2, 3, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, 2**380 % P, 2**28, 2**364 % P, (2**381 - 1) % P,
            int("0fffffff" * 12, 16) % P, fib[-2] % P, fib[-3] % P, (P * fib[-4]) // fib[-3]]
    vals += [2**k % P for k in range(0, 381, 17)]
    r2 = random.Random(2024)
    vals += [r2.randrange(P) for _ in range(750)]
    return vals


def gen_fp_inv():
    recs = []
    for i, v in enumerate(_inv_values()):
        for a in (v, v + P) + ((2 * P,) if v == 0 else ()):
            want = RM * RM * pow(a, P - 2, P) % P
            recs.append(Rec("fp_inv divsteps[%d]%s = %s" % (i, " + p" * (a // P), _vname(a)), [limbs(a)], [want],
                            [lt_frac(105, 100)]))
    return recs


def gen_fp_pow_p34():
    rng = random.Random(5201)
    return [Rec("fp_pow_p34(%s)" % _vname(a), [limbs(a)], [m_(pow(s_(a), (P - 3) // 4, P))], [BOUND_2P])
            for a in _unary_values(rng, 200)]


def _reps(rng, res, mode=None):
    """representatives of canonical residues: all canonical, all + p, or mixed (zero also as 2p)"""
    mode = mode or rng.choice(["canon", "+p", "mixed"])
    out = []
    for r in res:
        if mode == "canon":
            out.append(r)
        elif mode == "+p":
            out.append(r + P)
        else:
            out.append(rng.choice([r, r + P] + ([2 * P] if r == 0 else [])))
    return out


def _flat(t):
    """a tower tuple -> its Fp coefficients in tower order"""
    if isinstance(t, int):
        return [t]
    return [x for c in t for x in _flat(c)]


def _f2(v):
    return (v[0], v[1])


def _f6(v):
    return (_f2(v[0:2]), _f2(v[2:4]), _f2(v[4:6]))


def _f12(v):
    return (_f6(v[0:6]), _f6(v[6:12]))


def _std(v):
    return [s_(x) for x in v]


def _mont(t):
    return [m_(x) for x in _flat(t)]


def _tower_rec(name, vals, want, bound):
    assert all(0 <= v for v in vals)
    return Rec(name, [limbs(v) for v in vals], want, [bound] * len(want))


def _stored_patterns(rng, n_coef, n_random):
    """stored-value coefficient lists: uniform edges, random edges, limb edges, random"""
    pats = [("all %s" % _vname(e), [e] * n_coef) for e in E2]
    for i in range(n_random):
        k = i % 3
        if k == 0:
            pats.append(("edges #%d" % i, [rng.choice(E2) for _ in range(n_coef)]))
        elif k == 1:
            pats.append(("stored #%d" % i, [stored(rng) for _ in range(n_coef)]))
        else:
            pats.append(("random #%d" % i, [rng.randrange(2 * P + 1) for _ in range(n_coef)]))
    return pats


def gen_fp2_inv():
    rng = random.Random(5301)
    return [_tower_rec("fp2_inv %s" % n, v, _mont(bls.f2inv(_f2(_std(v)))), BOUND_2P)
            for n, v in _stored_patterns(rng, 2, 200)]


def gen_fp6_inv():
    rng = random.Random(5401)
    return [_tower_rec("fp6_inv %s" % n, v, _mont(bls.f6inv(_f6(_std(v)))), BOUND_2P)
            for n, v in _stored_patterns(rng, 6, 150)]


def gen_fp12_inv():
    rng = random.Random(5501)
    return [_tower_rec("fp12_inv %s" % n, v, _mont(bls.f12inv(_f12(_std(v)))), BOUND_2P)
            for n, v in _fp12_patterns(rng, 140)]


def sqrt_takes_alt(A):
    """whether fp2_sqrt's t = (a0 + sqrt(norm)) / 2 is zero for the element A (residues), so it selects t_alt"""
    n = (A[0] * A[0] + A[1] * A[1]) % P
    s = pow(n, (P + 1) // 4, P)
    return (A[0] + s) % P == 0


def gen_fp2_sqrt():
    rng = random.Random(5601)
    recs = []

    def rec(name, A, mode=None):
        sq = bls.f2_is_square(A)
        raw = _reps(rng, [m_(A[0]), m_(A[1])], mode)

        def post(out, A=A, sq=sq):
            return not sq or bls.f2sqr((s_(out[0]), s_(out[1]))) == A

        recs.append(Rec("fp2_sqrt %s%s" % (name, " [t == 0]" if sqrt_takes_alt(A) else ""), [limbs(v) for v in raw],
                        [None, None], [BOUND_2P] * 2, status=int(sq), post=post))

    for z0 in (0, P, 2 * P):
        for z1 in (0, P, 2 * P):
            recs.append(Rec("fp2_sqrt zero (%s, %s) [t == 0]" % (_vname(z0), _vname(z1)), [limbs(z0), limbs(z1)],
                            [0, 0], [BOUND_2P] * 2, status=1))
    n_res = n_non = 0
    i = 0
    while n_res < 30 or n_non < 30:  # real elements: squares k^2, and non-residues of Fp (roots purely imaginary)
        c = rng.randrange(1, P)
        i += 1
        if bls.f_is_square(c) and n_res < 30:
            n_res += 1
            rec("real square #%d" % i, (c, 0))
        elif not bls.f_is_square(c) and n_non < 30:
            n_non += 1
            rec("real non-residue #%d" % i, (c, 0))
    for k in (1, 2, 3, 4):
        rec("real %d" % k, (k, 0), "canon")
        rec("real -%d" % k, (P - k, 0), "canon")
    for i in range(30):
        rec("imaginary #%d" % i, (0, rng.randrange(1, P)))
    n_sq = n_ns = 0
    while n_sq < 50 or n_ns < 50:
        A = (rng.randrange(P), rng.randrange(P))
        if bls.f2_is_square(A) and n_sq < 50:
            n_sq += 1
            rec("random square #%d" % n_sq, A)
        elif not bls.f2_is_square(A) and n_ns < 50:
            n_ns += 1
            rec("random non-square #%d" % n_ns, A)
    return recs


# ------------------------------------------------------------------------------------------------ Fp6 / Fp12
def _le4(rng):
    """a normalized operand-side sum: value <= 4p"""
    x = rng.random()
    if x < 0.35:
        return rng.choice(E4)
    if x < 0.7:
        return stored(rng) + stored(rng)
    return rng.randrange(4 * P + 1)


def _le4_patterns(rng, n_coef, n_random):
    pats = [("all %s" % _vname(e), [e] * n_coef) for e in E4]
    pats.append(("first half 4p, second 0", [4 * P] * (n_coef // 2) + [0] * (n_coef - n_coef // 2)))
    pats.append(("first half 0, second 4p", [0] * (n_coef // 2) + [4 * P] * (n_coef - n_coef // 2)))
    pats.append(("alternating 4p, 0", [4 * P * ((k + 1) % 2) for k in range(n_coef)]))
    pats.append(("alternating 0, 4p", [4 * P * (k % 2) for k in range(n_coef)]))
    for i in range(n_random):
        pats.append(("<=4p #%d" % i, [_le4(rng) for _ in range(n_coef)]))
    return pats


def gen_fp6_mul():
    rng = random.Random(5701)
    return [_tower_rec("fp6_mul %s" % n, v, _mont(bls.f6mul(_f6(_std(v[:6])), _f6(_std(v[6:])))), BOUND_LC)
            for n, v in _le4_patterns(rng, 12, 280)]


def gen_fp6_mul_by_01():
    rng = random.Random(5801)
    recs = []
    for n, v in _le4_patterns(rng, 10, 240):
        s = _std(v)
        want = bls.f6mul(_f6(s[:6]), (_f2(s[6:8]), _f2(s[8:10]), bls.F2_ZERO))
        recs.append(_tower_rec("fp6_mul_by_01 %s" % n, v, _mont(want), BOUND_LC))
    return recs


def gen_fp6_mul_by_12():
    rng = random.Random(5901)
    recs = []
    for n, v in _le4_patterns(rng, 10, 240):
        s = _std(v)
        want = bls.f6mul(_f6(s[:6]), (bls.F2_ZERO, _f2(s[6:8]), _f2(s[8:10])))
        recs.append(_tower_rec("fp6_mul_by_12 %s" % n, v, _mont(want), BOUND_LC))
    return recs


def _fp12_patterns(rng, n_random):
    """stored Fp12 elements: all twelve coefficients at 2p, c1 entirely 2p (a conjugated real element), sparse
    elements with their zeros drawn from {0, p, 2p}, uniform and random edges, random"""
    pats = _stored_patterns(rng, 12, 0)
    for i in range(8):
        pats.append(("c1 all 2p, c0 stored #%d" % i, [stored(rng) for _ in range(6)] + [2 * P] * 6))
    for e in E2:
        pats.append(("c1 all 2p, c0 all %s" % _vname(e), [e] * 6 + [2 * P] * 6))
    for i in range(24):
        v = [rng.choice([0, P, 2 * P]) for _ in range(12)]
        for k in rng.sample(range(12), 1 + i % 4):
            v[k] = stored(rng)
        pats.append(("sparse #%d" % i, v))
    return pats + _stored_patterns(rng, 12, n_random)[len(E2):]


def gen_fp12_mul():
    rng = random.Random(6001)
    pa, pb = _fp12_patterns(rng, 100), _fp12_patterns(rng, 100)
    pairs = [(a, b) for a in pa[:10] for b in pb[:10]] + list(zip(pa[10:], pb[10:]))
    return [_tower_rec("fp12_mul [%s] * [%s]" % (na, nb), a + b,
                       _mont(bls.f12mul(_f12(_std(a)), _f12(_std(b)))), BOUND_LC) for (na, a), (nb, b) in pairs]


def gen_fp12_sqr():
    rng = random.Random(6101)
    return [_tower_rec("fp12_sqr %s" % n, v, _mont(bls.f12sqr(_f12(_std(v)))), BOUND_LC)
            for n, v in _fp12_patterns(rng, 160)]


def _line12(l0, l1, l4):
    """l0 + l1 v + l4 v w in the tower"""
    return ((l0, l1, bls.F2_ZERO), (bls.F2_ZERO, l4, bls.F2_ZERO))


def gen_fp12_mul_by_014():
    rng = random.Random(6201)
    recs = []
    for n, f in _fp12_patterns(rng, 160):
        l = [stored(rng) for _ in range(6)]
        if n.startswith("all "):  # the uniform patterns extend to the line
            l = [f[0]] * 6
        sl = _std(l)
        want = bls.f12mul(_f12(_std(f)), _line12(_f2(sl[0:2]), _f2(sl[2:4]), _f2(sl[4:6])))
        recs.append(_tower_rec("fp12_mul_by_014 %s" % n, f + l, _mont(want), BOUND_LC))
    return recs


def gen_fp12_line2():
    rng = random.Random(6301)
    recs = []
    for n, f in _fp12_patterns(rng, 140):
        l = [stored(rng) for _ in range(12)]
        if n.startswith("all "):
            l = [f[0]] * 12
        sl = _std(l)
        la = _line12(_f2(sl[0:2]), _f2(sl[2:4]), _f2(sl[4:6]))
        lb = _line12(_f2(sl[6:8]), _f2(sl[8:10]), _f2(sl[10:12]))
        # line_pair's product carries one 1/R, the product with f another: R * (f/R * la/R * lb/R)
        want = bls.f12mul(_f12(_std(f)), bls.f12mul(la, lb))
        recs.append(_tower_rec("line_pair + fp12_mul_by_line2 %s" % n, f + l, _mont(want), BOUND_LC))
    return recs


def _gen_fp12_unary(name, seed, f, n=150):
    def gen():
        rng = random.Random(seed)
        return [_tower_rec("%s %s" % (name, pn), v, f(v), BOUND_2P) for pn, v in _fp12_patterns(rng, n)]
    return gen


def _frob(k):
    # the Frobenius constants are stored in Montgomery form, so the raw coefficients map with no factor
    return lambda v: _flat(bls.f12frob(_f12([x % P for x in v]), k))


def _conj(v):
    return [x % P for x in v[:6]] + [-x % P for x in v[6:]]


def _cyclotomic(rng):
    """an element of the cyclotomic subgroup (the easy part of the final exponentiation), as residues"""
    a = _f12([rng.randrange(P) for _ in range(12)])
    c = bls.f12mul(bls.f12conj(a), bls.f12inv(a))
    return bls.f12mul(bls.f12frob(c, 2), c)


def _cyclotomic_inputs(rng, n):
    """cyclotomic elements as canonical, + p and mixed representatives of their Montgomery form; the one (with its
    zeros at 0, p, 2p -- c1 entirely 2p is a conjugated real element) and zero, where x -> x^2 holds as well"""
    out = []
    for z in (0, P, 2 * P):
        out.append(("zero, all %s" % _vname(z), _f12([0] * 12), [z] * 12))
        for o in (RM, RM + P):
            out.append(("one %s, zeros %s" % (_vname(o), _vname(z)), bls.F12_ONE, [o] + [z] * 11))
    for i in range(n):
        c = _cyclotomic(rng)
        mode = ["canon", "+p", "mixed"][i % 3]
        out.append(("cyclotomic #%d %s" % (i, mode), c, _reps(rng, _mont(c), mode)))
    return out


def gen_fp12_cyclotomic_sqr():
    rng = random.Random(6801)
    return [_tower_rec("fp12_cyclotomic_sqr %s" % n, raw, _mont(bls.f12sqr(c)), BOUND_2P)
            for n, c, raw in _cyclotomic_inputs(rng, 150)]


def gen_fp12_pow_zabs():
    # only cyclotomic elements (and 0, 1): the chain squares with fp12_cyclotomic_sqr
    rng = random.Random(6701)
    return [_tower_rec("fp12_pow_zabs %s" % n, raw, _mont(bls.f12pow(c, Z_ABS)), BOUND_2P)
            for n, c, raw in _cyclotomic_inputs(rng, 122)]


INV2 = (P + 1) // 2
OPS = [
    Op("fp_mul", 32, 2, 1, gen_fp_mul),
    Op("fp_sqr", 33, 1, 1, gen_fp_sqr),
    Op("fp2_mul", 34, 4, 2, gen_fp2_mul),
    Op("fp2_sqr", 35, 2, 2, gen_fp2_sqr),
    Op("fp2_mul_fp", 36, 3, 2, gen_fp2_mul_fp),
    Op("fp_add", 37, 2, 1, _gen_binary("fp_add", 3701, lambda a, b: a + b)),
    Op("fp_sub", 38, 2, 1, _gen_binary("fp_sub", 3801, lambda a, b: a - b)),
    Op("fp_neg", 39, 1, 1, _gen_unary("fp_neg", 3901, lambda a: -a)),
    Op("fp_dbl", 40, 1, 1, _gen_unary("fp_dbl", 4001, lambda a: 2 * a)),
    Op("fp_half", 41, 1, 1, _gen_unary("fp_half", 4101, lambda a: a * INV2, bound=3 * P // 2)),
    Op("fp_mul3", 42, 1, 1, _gen_unary("fp_mul3", 4201, lambda a: 3 * a)),
    Op("fp_mul4", 43, 1, 1, _gen_unary("fp_mul4", 4301, lambda a: 4 * a)),
    Op("fp_mul8", 44, 1, 1, _gen_unary("fp_mul8", 4401, lambda a: 8 * a)),
    Op("fp_canon", 45, 1, 1, _gen_unary("fp_canon", 4501, lambda a: a % P, bound=P - 1, exact=True)),
    Op("fp_add_norm", 46, 2, 1, _gen_binary("fp_add_norm", 4601, lambda a, b: a + b, exact=True)),
    Op("fp2_mul_xi", 47, 2, 2, gen_fp2_mul_xi),
    Op("fp_is_zero", 48, 1, 0, gen_fp_is_zero),
    Op("fp_eq", 49, 2, 0, gen_fp_eq),
    Op("fp12_is_one", 50, 12, 0, gen_fp12_is_one),
    Op("fp_inv", 51, 1, 1, gen_fp_inv),
    Op("fp_pow_p34", 52, 1, 1, gen_fp_pow_p34),
    Op("fp2_inv", 53, 2, 2, gen_fp2_inv),
    Op("fp6_inv", 54, 6, 6, gen_fp6_inv),
    Op("fp12_inv", 55, 12, 12, gen_fp12_inv),
    Op("fp2_sqrt", 56, 2, 2, gen_fp2_sqrt),
    Op("fp6_mul", 57, 12, 6, gen_fp6_mul),
    Op("fp6_mul_by_01", 58, 10, 6, gen_fp6_mul_by_01),
    Op("fp6_mul_by_12", 59, 10, 6, gen_fp6_mul_by_12),
    Op("fp12_mul", 60, 24, 12, gen_fp12_mul),
    Op("fp12_sqr", 61, 12, 12, gen_fp12_sqr),
    Op("fp12_mul_by_014", 62, 18, 12, gen_fp12_mul_by_014),
    Op("fp12_line2", 63, 24, 12, gen_fp12_line2),
    Op("fp12_frob1", 64, 12, 12, _gen_fp12_unary("fp12_frob1", 6401, _frob(1))),
    Op("fp12_frob2", 65, 12, 12, _gen_fp12_unary("fp12_frob2", 6501, _frob(2))),
    Op("fp12_conj", 66, 12, 12, _gen_fp12_unary("fp12_conj", 6601, _conj)),
    Op("fp12_pow_zabs", 67, 12, 12, gen_fp12_pow_zabs),
    Op("fp12_cyclotomic_sqr", 68, 12, 12, gen_fp12_cyclotomic_sqr),
]
OP_NAMES = [o.name for o in OPS]
BY_NAME = {o.name: o for o in OPS}


@functools.lru_cache(maxsize=None)
def records(name):
    """the op's records (computed once per process; shared, not to be modified)"""
    recs = _finish(BY_NAME[name].gen())
    op = BY_NAME[name]
    for r in recs:
        assert len(r.ins) == op.n_in and len(r.want) == len(r.bound) == op.n_out, r.name
    return recs


def check(name, outs, statuses, op=None, recs=None):
    """outs[i]: the n_out * 14 output limb words of record i; statuses[i]: its status word.  Every record is checked:
    the status, limbs 0..12 below 2^28, the value within the bound, the residue (or the exact value, where the record
    fixes one for that output) equal to the reference, then the record's `post` check on the output values (False, or
    the text of what failed).  Returns the failures as (record name, what failed).  `op` / `recs`: another module's
    operation and records (tests/curve_vectors.py); by default this module's, by name."""
    if op is None:
        op, recs = BY_NAME[name], records(name)
    assert len(outs) == len(statuses) == len(recs)
    bad = []
    for r, o, st in zip(recs, outs, statuses):
        o = [int(x) for x in o]
        if int(st) != r.status:
            bad.append((r.name, "status %d, expected %d" % (st, r.status)))
            continue
        vals = []
        for j in range(op.n_out):
            l = o[NL * j: NL * j + NL]
            v = val(l)
            vals.append(v)
            if not all(x < (1 << LB) for x in l[:NL - 1]):
                bad.append((r.name, "output %d: a limb at or above 2^28" % j))
            elif v > r.bound[j]:
                bad.append((r.name, "output %d: value %.4f p above its bound %.4f p" % (j, v / P, r.bound[j] / P)))
            elif r.exact is not None and r.exact[j] is not None and v != r.exact[j]:
                bad.append((r.name, "output %d: value differs from the exact expectation" % j))
            elif r.want[j] is not None and v % P != r.want[j]:
                bad.append((r.name, "output %d: wrong residue" % j))
        if r.post is not None:
            ok = r.post(vals)
            if ok is not True:
                bad.append((r.name, ok or "the returned root does not square to the input"))
    return bad


def format_failures(name, bad, limit=12, total=None):
    total = len(records(name)) if total is None else total
    return "%s: %d of %d records failed:\n" % (name, len({n for n, _ in bad}), total) + "\n".join(
        "  %s -- %s" % b for b in bad[:limit])
