"""Signature.aggregate(sigs.map(fromBytes)).toBytes() on the GPU (blsgpu_aggregate_signatures, csrc/k_sigagg.hip)
against the oracle: keys from bls.interop_secret_key, signatures from oracle.cpu.sign, the reference sum a fold of
bls.g2_add over bls.signature_from_bytes, encoded by bls.g2_compress / bls.g2_serialize.

Signing and the Python decompression of every pool signature happen once per module (fixtures `same`, `pool`); the
tests only fold cached points.
"""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import cpu

pytestmark = pytest.mark.gpu

THREADS = 16
INF96 = bytes([0xC0]) + bytes(95)
INF192 = bytes([0x40]) + bytes(191)
NONE = 0xFFFFFFFF
SEG_SIZES = [1, 2, 3, 0, 64, 65, 130]  # test 2's groups (the empty one included)
N_POOL = sum(SEG_SIZES)


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd.native import Context

    c = Context([0])
    yield c
    c.close()


def sk_bytes(i):
    return bls.interop_secret_key(i).to_bytes(32, "big")


def msg(j, tag=b"sigagg"):
    return hashlib.sha256(tag + j.to_bytes(4, "little")).digest()


def negate(sig96):
    """-S of a compressed, finite signature: the sign bit flipped."""
    return bytes([sig96[0] ^ 0x20]) + sig96[1:]


class Points:
    """Decoded signatures by their bytes: each distinct encoding goes through the Python oracle once."""

    def __init__(self):
        self.cache = {INF96: None, INF192: None}

    def get(self, b, validate=True):
        b = bytes(b)
        if b not in self.cache:
            self.cache[b] = bls.signature_from_bytes(b, validate=validate)
        return self.cache[b]

    def put_valid(self, sig96):
        """An oracle-made signature (in G2 by construction): decompress without the subgroup chain; its negation and
        its 192-byte form come for free."""
        p = bls.signature_from_bytes(sig96, validate=False)
        self.cache[bytes(sig96)] = p
        self.cache[negate(sig96)] = bls.g2_neg(p)
        self.cache[bls.g2_serialize(p)] = p
        return p

    def fold(self, sigs, validate=True):
        """Signature.aggregate(sigs.map(fromBytes)): the affine sum (None = identity); raises bls.BlstError."""
        acc = None
        for s in sigs:
            p = self.get(s, validate)
            if p is None:
                continue
            acc = p if acc is None else bls.g2_add(acc, p)
        return acc


@pytest.fixture(scope="module")
def points():
    return Points()


@pytest.fixture(scope="module")
def same():
    """129 interop keys signing ONE message: (secret keys, compressed pubkeys, message, signatures)."""
    k = 129
    sks = [bls.interop_secret_key(i) for i in range(k)]
    m = msg(0, b"same")
    sigs = cpu.sign(b"".join(s.to_bytes(32, "big") for s in sks), m * k, threads=THREADS)
    pk96 = cpu.sk_to_pk(b"".join(s.to_bytes(32, "big") for s in sks), threads=THREADS)
    pk48 = [bls.g1_compress(bls.g1_deserialize(pk96[96 * i: 96 * i + 96])) for i in range(k)]
    return sks, pk48, m, [sigs[96 * i: 96 * i + 96] for i in range(k)]


@pytest.fixture(scope="module")
def pool(points):
    """N_POOL signatures over distinct messages (key i % 64 signs message i), decoded once."""
    sks = b"".join(sk_bytes(i % 64) for i in range(N_POOL))
    sigs = cpu.sign(sks, b"".join(msg(i) for i in range(N_POOL)), threads=THREADS)
    out = [sigs[96 * i: 96 * i + 96] for i in range(N_POOL)]
    for s in out:
        points.put_valid(s)
    return out


def pack(groups, stride=None):
    """(buffer, group_first, sig_len, stride) of a call over lists of signature byte strings."""
    flat = [s for g in groups for s in g]
    if stride is None:
        stride = 192 if any(len(s) > 96 for s in flat) else 96
    first = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint32)
    buf = b"".join(bytes(s)[:stride].ljust(stride, b"\0") for s in flat)
    return buf, first, np.array([len(s) for s in flat], np.uint32), stride


def run(ctx, groups, validate=True, out_len=96, stride=None):
    buf, first, sl, stride = pack(groups, stride)
    return ctx.aggregate_signatures(buf, first, sig_len=sl, sig_stride=stride, validate=validate, out_len=out_len)


def lanes_of(groups):
    from lodestar_amd import native

    return native.sig_agg_lanes(len(groups), sum(len(g) for g in groups))


@pytest.fixture(scope="module")
def seg(pool, points):
    """Test 2's call: group sizes SEG_SIZES over the pool, every third signature as its 192-byte encoding (stride 192),
    and the reference aggregate of each group."""
    groups, k = [], 0
    for n in SEG_SIZES:
        g = []
        for s in pool[k: k + n]:
            g.append(bls.g2_serialize(points.get(s)) if (k + len(g)) % 3 == 1 else s)
        groups.append(g)
        k += n
    want = [bls.g2_compress(points.fold(g)) if g else None for g in groups]
    return groups, want


def check_seg(seg, out, st, fb):
    groups, want = seg
    for g, w in enumerate(want):
        if w is None:
            assert st[g] == 9 and out[g] == bytes(96) and fb[g] == NONE  # EMPTY_AGGREGATE
        else:
            assert st[g] == 0 and fb[g] == NONE, (g, st[g], fb[g])
            assert out[g] == w, f"group {g} ({len(groups[g])} signatures)"


# ---------------------------------------------------------------------------------------------- 1
@pytest.mark.parametrize("out_len", [96, 192])
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 129])
def test_linearity_known_answer(ctx, same, k, out_len):
    """sum_i sk_i H(m) == (sum_i sk_i) H(m): the aggregate of k signatures over one message is byte-equal to the
    signature of the summed key, at the wave-stride and tree boundaries (k = 63, 64, 65: one pass of a wave, every
    lane; 129: three strides), in both output encodings; it verifies as FastAggregateVerify of the k keys."""
    from lodestar_amd import api

    sks, pk48, m, sigs = same
    expected = cpu.sign((sum(sks[:k]) % bls.R).to_bytes(32, "big"), m)
    out, st, fb = run(ctx, [sigs[:k]], out_len=out_len)
    assert st[0] == 0 and fb[0] == NONE
    if out_len == 96:
        assert out[0] == expected
        assert api.fast_aggregate_verify(ctx, pk48[:k], m, out[0])
    else:
        assert out[0] == bls.g2_serialize(bls.signature_from_bytes(expected))


# ---------------------------------------------------------------------------------------------- 2
def test_segmented_mixed_encodings_vs_oracle(ctx, seg):
    """One call, groups of [1, 2, 3, 0, 64, 65, 130] signatures over distinct messages, a third of them 192-byte
    encodings in a 192-byte stride: every group byte-equal to the oracle's fold, the empty one EMPTY_AGGREGATE."""
    groups, _ = seg
    assert lanes_of(groups) == 64
    check_seg(seg, *run(ctx, groups, stride=192))


# ---------------------------------------------------------------------------------------------- 3
def test_addition_edge_cases(ctx, pool, points):
    """The smallest inputs on which the sum can go wrong, in the one-lane, butterfly and wave-tree forms: the same
    signature twice (the doubling branch of jac_add_aff on one lane; of jac_add when the copies sit on different
    lanes), a signature and its negation (identity, status 0), identity signatures inside a group (nothing added), a
    group of identity signatures only (identity, status 0)."""
    a, b, c = pool[0], pool[1], pool[2]
    calls = {
        # mean group size <= 3: one lane per group, everything through jac_add_aff
        1: [[a, a], [a, negate(a)], [INF96, a, INF96], [INF96, INF96], [a, a, negate(a)]],
        # lanes 0..3 hold one signature each: the butterfly adds lane 0 and lane 2 (a + a, a - a) with jac_add
        8: [[a, b, a, b], [a, b, negate(a), negate(b)], [INF96, INF96, INF96, INF96], [a, INF96, b, INF96, c],
            [a, b, negate(a), c]],
        # one signature per lane, lane k + 32 a copy / the negation of lane k: level 32 of the tree doubles / cancels
        64: [pool[:32] + pool[:32], pool[:32] + [negate(s) for s in pool[:32]], [INF96] * 64,
             pool[:32] + [INF96] * 31 + [pool[40]]],
    }
    for form, groups in calls.items():
        assert lanes_of(groups) == form
        for out_len, inf in ((96, INF96), (192, INF192)):
            out, st, fb = run(ctx, groups, out_len=out_len)
            for g, sigs in enumerate(groups):
                p = points.fold(sigs)
                want = inf if p is None else (bls.g2_compress(p) if out_len == 96 else bls.g2_serialize(p))
                assert st[g] == 0 and fb[g] == NONE and out[g] == want, (form, g, out_len)
    # the identity cases really are the identity
    assert points.fold(calls[1][1]) is None and points.fold(calls[8][1]) is None and points.fold(calls[64][1]) is None
    assert points.fold(calls[1][3]) is None and points.fold(calls[64][2]) is None


# ---------------------------------------------------------------------------------------------- 4
def adversarial_sigs():
    """One signature per Signature.fromBytes error class (first candidates of a fixed scan; the scan of
    tests/test_gpu_parity.py) plus a 48-byte length."""
    out = {}
    for t in range(1, 400):
        cand = bytes([0x80]) + bytes(45) + t.to_bytes(2, "big") + bytes(48)
        c = bls.classify_signature(cand)
        if c and c not in out:
            out[c] = cand
        if bls.BLST_POINT_NOT_ON_CURVE in out and bls.BLST_POINT_NOT_IN_GROUP in out:
            break
    out[bls.BLST_BAD_ENCODING] = bytes([0x80 | 0x1F]) + bytes([0xFF]) * 95  # x >= p
    out[bls.BLST_INVALID_SIZE] = bytes([0x80]) + bytes(47)
    return out


@pytest.fixture(scope="module")
def adv():
    a = adversarial_sigs()
    assert sorted(a) == [bls.BLST_BAD_ENCODING, bls.BLST_POINT_NOT_ON_CURVE, bls.BLST_POINT_NOT_IN_GROUP,
                         bls.BLST_INVALID_SIZE]
    return a


def test_error_classes_and_isolation(ctx, pool, points, adv):
    """One adversarial signature per class in the middle of an otherwise valid 5-signature group, valid neighbour
    groups around each: status = the class code, first_bad = its call-wide index, output zeros, neighbours byte-equal
    to the oracle; a group with two bad signatures reports the lower index."""
    groups, expect = [pool[0:3]], [None]
    k = 3
    for code in sorted(adv):
        groups.append(pool[k: k + 2] + [adv[code]] + pool[k + 2: k + 4])
        expect.append((code, sum(len(g) for g in groups[:-1]) + 2))
        groups.append(pool[k + 4: k + 7])
        expect.append(None)
        k += 7
    two = pool[k: k + 1] + [adv[bls.BLST_POINT_NOT_IN_GROUP]] + pool[k + 1: k + 2] + [adv[bls.BLST_BAD_ENCODING]] + \
        pool[k + 2: k + 3]
    groups.append(two)
    expect.append((bls.BLST_POINT_NOT_IN_GROUP, sum(len(g) for g in groups[:-1]) + 1))
    assert lanes_of(groups) == 8  # the two bad signatures sit on different lanes
    out, st, fb = run(ctx, groups)
    for g, e in enumerate(expect):
        if e is None:
            assert st[g] == 0 and fb[g] == NONE and out[g] == bls.g2_compress(points.fold(groups[g])), g
        else:
            assert (st[g], fb[g]) == e and out[g] == bytes(96), (g, st[g], fb[g], e)
            with pytest.raises(bls.BlstError) as ei:
                points.fold(groups[g])
            assert ei.value.code == e[0]


@pytest.mark.parametrize("form,n_before,size,hi,lo", [(1, 3, 3, 2, 1), (8, 3, 12, 9, 3), (16, 4, 28, 17, 5),
                                                      (32, 4, 60, 33, 7), (64, 70, 70, 69, 40)])
def test_first_error_is_lowest_index(ctx, pool, adv, form, n_before, size, hi, lo):
    """Two rejected signatures in one group, the one with the HIGHER index on a lower lane (second stride of lane
    hi % form; the same lane when a lane owns the whole group): every form reports the lower index and its code.  A
    valid neighbour group precedes it, so the index is call-wide."""
    g = list(pool[:size])
    g[hi] = adv[bls.BLST_BAD_ENCODING]
    g[lo] = adv[bls.BLST_POINT_NOT_ON_CURVE]
    groups = [pool[100: 100 + n_before], g]
    assert lanes_of(groups) == form and (form == 1 or hi % form < lo % form)
    out, st, fb = run(ctx, groups)
    assert st[0] == 0 and fb[0] == NONE
    assert st[1] == bls.BLST_POINT_NOT_ON_CURVE and fb[1] == n_before + lo and out[1] == bytes(96)


def test_validate_false_accepts_out_of_group_point(ctx, pool, points, adv):
    """validate=False is Signature.fromBytes(b, validate=false): the curve point outside G2 is summed like any other
    (and still rejected with validate=True); decode errors stay errors."""
    rogue = adv[bls.BLST_POINT_NOT_IN_GROUP]
    groups = [[pool[0], rogue, pool[1]], [pool[2], adv[bls.BLST_POINT_NOT_ON_CURVE]], [rogue]]
    out, st, fb = run(ctx, groups, validate=False)
    pts = Points()
    pts.cache.update(points.cache)
    assert st[0] == 0 and out[0] == bls.g2_compress(pts.fold(groups[0], validate=False))
    assert st[1] == bls.BLST_POINT_NOT_ON_CURVE and fb[1] == 4 and out[1] == bytes(96)
    assert st[2] == 0 and out[2] == bls.g2_compress(bls.signature_from_bytes(rogue, validate=False))
    out, st, fb = run(ctx, groups, validate=True)
    assert list(st) == [bls.BLST_POINT_NOT_IN_GROUP, bls.BLST_POINT_NOT_ON_CURVE, bls.BLST_POINT_NOT_IN_GROUP]
    assert list(fb) == [1, 4, 5]


# ---------------------------------------------------------------------------------------------- 5
# (n_groups, base size, form): sizes cycle base - 1, base, base + 1 over the groups
FORM_SHAPES = [
    (3, 2, 1),        # mean size <= 3: one lane per group (the pool insert)
    (3, 5, 8),        # few groups, mean size 4..8
    (3, 12, 16),      # few groups, mean size 9..16
    (3, 20, 32),      # few groups, mean size 17..32
    (8, 64, 64),      # few groups, mean size > 32: a wave per group
    (1025, 64, 32),   # > 1,024 groups: 32 lanes
    (4097, 17, 16),   # > 4,096 groups: 16 lanes
    (8193, 9, 8),     # > 8,192 groups: 8 lanes
    (16385, 4, 1),    # > 16,384 groups: one lane per group
]


@pytest.mark.parametrize("n_groups,base,form", FORM_SHAPES)
def test_every_launch_form(ctx, pool, points, n_groups, base, form):
    """Every value sig_agg_lanes can return (64, 32, 16, 8, 1), each reached both ways the rule has -- by the mean
    group size with few groups and by the group count -- with groups of base - 1, base, base + 1 signatures:

        3 x ~2 -> 1      3 x ~5 -> 8      3 x ~12 -> 16     3 x ~20 -> 32     8 x ~64 -> 64
        1,025 x ~64 -> 32     4,097 x ~17 -> 16     8,193 x ~9 -> 8     16,385 x ~4 -> 1

    The call tiles at most 64 distinct groups (slices of the signed pool), so the oracle folds each distinct group
    once; every group of the call is compared."""
    from lodestar_amd import native

    d = min(n_groups, 64)
    distinct = []
    for j in range(d):
        size = base - 1 + j % 3
        start = (37 * j) % (N_POOL - size)
        distinct.append(list(range(start, start + size)))
    want = [bls.g2_compress(points.fold([pool[i] for i in idx])) for idx in distinct]
    arr = np.frombuffer(b"".join(pool), np.uint8).reshape(N_POOL, 96)
    sizes = np.array([len(distinct[g % d]) for g in range(n_groups)])
    first = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    idx = np.concatenate([distinct[g % d] for g in range(n_groups)])
    assert native.sig_agg_lanes(n_groups, len(idx)) == form
    out, st, fb = ctx.aggregate_signatures(np.ascontiguousarray(arr[idx]).reshape(-1), first)
    assert not st.any() and (fb == NONE).all()
    bad = [g for g in range(n_groups) if out[g] != want[g % d]]
    assert not bad, f"{len(bad)} of {n_groups} groups differ, first {bad[:5]}"


# ---------------------------------------------------------------------------------------------- 6
def test_beside_the_verifier(ctx, seg):
    """A 2,048-set verification call in flight on the pipeline streams while the aggregation runs on the helper
    stream: both results are right."""
    n = 2048
    sks = b"".join(sk_bytes(i % 64) for i in range(n))
    msgs = b"".join(msg(i, b"beside") for i in range(n))
    sigs = cpu.sign(sks, msgs, threads=THREADS)
    pks = cpu.sk_to_pk(sks, threads=THREADS)
    pending = ctx.submit_raw(np.arange(n + 1), sigs, [96] * n, msgs, pk_bytes=pks, job_flags=np.ones(n),
                             sig_stride=96)
    got = run(ctx, seg[0], stride=192)
    res, _ = pending.wait(120)
    check_seg(seg, *got)
    assert (res == 1).all()


# ---------------------------------------------------------------------------------------------- 7
def test_argument_errors_and_closed_context(pool):
    """Every BLSGPU_ERR_ARGS condition of the header through raw ctypes (refused on the host: the bad pointers and
    counts are never read), n_groups == 0, and BLSGPU_ERR_CLOSED from a context that is being destroyed."""
    from lodestar_amd import native

    lib = native.load()
    c = native.Context([0])
    buf = np.frombuffer(b"".join(pool[:4]), np.uint8).copy()
    gf = np.array([0, 1, 4], np.uint32)
    sl = np.full(4, 96, np.uint32)
    out, st, fb = np.zeros(2 * 192, np.uint8), np.zeros(2, np.int8), np.zeros(2, np.uint32)

    def call(h=None, n=2, gf=gf, buf=buf, stride=96, sl=sl, flags=1, out=out, out_len=96, st=st, fb=fb):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.blsgpu_aggregate_signatures(c.h if h is None else h, n, p(gf), p(buf), stride, p(sl), flags, p(out),
                                               out_len, p(st), p(fb))

    assert call() == native.OK and list(st) == [0, 0]
    assert call(fb=None) == native.OK  # first_bad is optional
    assert call(n=0) == native.OK
    assert call(n=0, gf=np.array([7], np.uint32)) == native.OK
    bad = {
        "null ctx": dict(h=ctypes.c_void_p(None)),
        "null group_first": dict(gf=None),
        "null sigs": dict(buf=None),
        "null sig_len": dict(sl=None),
        "null out": dict(out=None),
        "null status": dict(st=None),
        "out_len": dict(out_len=48),
        "out_len 0": dict(out_len=0),
        "sig_stride < 96": dict(stride=95),
        "unknown flag": dict(flags=3),
        "group_first[0] != 0": dict(gf=np.array([1, 2, 4], np.uint32)),
        "group_first decreasing": dict(gf=np.array([0, 3, 2], np.uint32)),
        "too many signatures": dict(gf=np.array([0, 1, (1 << 20) + 1], np.uint32)),
        "192-byte signature in a 96-byte stride": dict(sl=np.array([96, 96, 192, 96], np.uint32)),
    }
    for name, kw in bad.items():
        assert call(**kw) == native.ERR_ARGS, name

    # closed: hold the context open from a submission's completion callback, let blsgpu_destroy mark it closed, and
    # call until the refusal shows (each earlier call is a valid one-signature aggregation)
    release, entered = threading.Event(), threading.Event()

    def done(user, status):
        entered.set()
        release.wait(60)

    cb = native.DONE_CB(done)
    sk = sk_bytes(0)
    m = msg(0, b"closed")
    b, keep = native.make_batch([0, 1], cpu.sign(sk, m), [96], m, pk_bytes=cpu.sk_to_pk(sk), job_flags=[0],
                                sig_stride=96)
    res, stats = np.zeros(1, np.int8), native.Stats()
    assert lib.blsgpu_submit(c.h, ctypes.byref(b), res.ctypes.data, ctypes.byref(stats), cb, None) == native.OK
    assert entered.wait(60)
    h, c.h = c.h, None
    t = threading.Thread(target=lib.blsgpu_destroy, args=(h,))
    t.start()
    try:
        rc = native.OK
        for _ in range(100000):
            rc = call(h=h, n=1, gf=np.array([0, 1], np.uint32))
            if rc != native.OK:
                break
        assert rc == native.ERR_CLOSED
    finally:
        release.set()
        t.join(60)
    assert res[0] == 1


# ---------------------------------------------------------------------------------------------- api
def test_api_aggregate(ctx, pool, points, adv):
    """lodestar_amd.api: the spec Aggregate and its grouped form, errors as the reference throws them."""
    from lodestar_amd import api

    assert api.aggregate_signatures(ctx, pool[:3]) == bls.g2_compress(points.fold(pool[:3]))
    with pytest.raises(api.BlstError, match="EMPTY_AGGREGATE_ARRAY"):
        api.aggregate_signatures(ctx, [])
    with pytest.raises(api.BlstError, match="BLST_ERROR: BLST_POINT_NOT_IN_GROUP"):
        api.aggregate_signatures(ctx, [pool[0], adv[bls.BLST_POINT_NOT_IN_GROUP]])
    with pytest.raises(api.BlstError, match="BLST_ERROR: BLST_INVALID_SIZE"):
        api.aggregate_signatures(ctx, [pool[0], pool[1][:95]])
    u = bls.g2_serialize(points.get(pool[4]))
    r = api.aggregate_signature_groups(ctx, [pool[:2], [], [pool[3], u], [adv[bls.BLST_BAD_ENCODING]]])
    assert r[0] == bls.g2_compress(points.fold(pool[:2])) and r[2] == bls.g2_compress(points.fold([pool[3], pool[4]]))
    assert isinstance(r[1], api.BlstError) and r[1].code == 9
    assert isinstance(r[3], api.BlstError) and r[3].code == bls.BLST_BAD_ENCODING
    assert api.aggregate_signature_groups(ctx, []) == []
