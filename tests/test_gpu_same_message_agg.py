"""Same-message verification that also returns each group's aggregate signature (blsgpu_verify_same_message_agg,
csrc/k_sigagg.hip k_same_agg*) against the oracle.

Expected values come from the oracle alone: per-set results are oracle.cpu.verify_jobs of the sets as one-set
non-batchable jobs; a group's expected aggregate is bls.g2_add over bls.signature_from_bytes of the sets whose oracle
result is 1 and whose mask byte is set, encoded with bls.g2_compress / bls.g2_serialize; its count is how many those
are.  A group with none gives zero bytes.  Comparisons are exact bytes.

The world is that of test_gpu_same_message_fused.py: 129 interop keys sign three messages, once per module; each
scenario's oracle answers are computed once and shared.
"""
import ctypes
import hashlib
from collections import namedtuple

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import corrupt, cpu

pytestmark = pytest.mark.gpu

THREADS = 16
K = 129
SEED = 0x46555345444D5347
EMPTY = -9

Set = namedtuple("Set", "key sig pk", defaults=(None,))
Scenario = namedtuple("Scenario", "groups msgs want")


def sk32(x):
    return (x % bls.R).to_bytes(32, "big")


def msg(j):
    return hashlib.sha256(b"same-message-fused" + j.to_bytes(4, "little")).digest()


class World:
    def __init__(self):
        self.sks = [bls.interop_secret_key(i) for i in range(K)]
        skb = b"".join(sk32(s) for s in self.sks)
        self.m = [msg(0), msg(1), msg(2)]
        pk = cpu.sk_to_pk(skb, threads=THREADS)
        self.pk96 = [pk[96 * i: 96 * i + 96] for i in range(K)]
        self.sig96 = []
        for m in self.m:
            sg = cpu.sign(skb, m * K, threads=THREADS)
            self.sig96.append([sg[96 * i: 96 * i + 96] for i in range(K)])
        self._points = {}

    def point(self, sig):
        """The oracle's decoding of a signature that the oracle verified (decoded once per distinct encoding)."""
        sig = bytes(sig)
        if sig not in self._points:
            self._points[sig] = bls.signature_from_bytes(sig, validate=False)
        return self._points[sig]

    def wide(self, sig96):
        return bls.g2_serialize(self.point(sig96))

    def valid(self, i, mi, wide=False):
        s = self.sig96[mi][i]
        return Set(i, self.wide(s) if wide else s)


@pytest.fixture(scope="module")
def world():
    return World()


@pytest.fixture(scope="module")
def ctx(world):
    from lodestar_amd.native import Context

    c = Context([0])
    c.upload_pubkeys(0, b"".join(world.pk96))
    yield c
    c.close()


def arrays(world, groups, msgs, table=False):
    flat = [s for g in groups for s in g]
    stride = 192 if any(len(s.sig) > 96 for s in flat) else 96
    first = np.cumsum([0] + [len(g) for g in groups])
    buf = b"".join(s.sig[:stride].ljust(stride, b"\0") for s in flat)
    keys = dict(pk_index=[s.key for s in flat]) if table else \
        dict(pk_bytes=b"".join(s.pk if s.pk is not None else world.pk96[s.key] for s in flat))
    return dict(group_first=first, msgs=b"".join(world.m[i] for i in msgs), sigs=buf,
                sig_len=[len(s.sig) for s in flat], sig_stride=stride, **keys)


def oracle(world, groups, msgs):
    """Every set as a one-set non-batchable job over its group's message: int results 1 / 0 / -code."""
    flat = [s for g in groups for s in g]
    n = len(flat)
    if n == 0:
        return []
    stride = 192 if any(len(s.sig) > 96 for s in flat) else 96
    res, _ = cpu.verify_jobs(threads=THREADS, job_first_set=np.arange(n + 1),
                             sigs=b"".join(s.sig[:stride].ljust(stride, b"\0") for s in flat),
                             sig_len=[len(s.sig) for s in flat],
                             msgs=b"".join(world.m[mi] * len(g) for g, mi in zip(groups, msgs)),
                             pk_bytes=b"".join(s.pk if s.pk is not None else world.pk96[s.key] for s in flat),
                             job_flags=np.zeros(n), sig_stride=stride)
    return [int(r) for r in res]


def scenario(world, groups, msgs):
    return Scenario(groups, msgs, oracle(world, groups, msgs))


def group_rule(groups, want):
    out, k = [], 0
    for g in groups:
        out.append(EMPTY if not g else int(all(r == 1 for r in want[k: k + len(g)])))
        k += len(g)
    return out


def expected_sums(world, sc, mask=None):
    """Per group (the oracle's sum as an affine point or None, the number of sets summed)."""
    out, k = [], 0
    for g in sc.groups:
        acc, cnt = None, 0
        for j, s in enumerate(g):
            if sc.want[k + j] == 1 and (mask is None or mask[k + j]):
                acc = bls.g2_add(acc, world.point(s.sig))
                cnt += 1
        out.append((acc, cnt))
        k += len(g)
    return out


def encode(sums, out_len):
    enc = bls.g2_compress if out_len == 96 else bls.g2_serialize
    return [enc(p) if c else bytes(out_len) for p, c in sums]


def run_agg(ctx, world, sc, table=False, seed=SEED, flags=0, mask=None, out_len=96):
    return ctx.verify_same_message_agg(seed=seed, flags=flags, include=mask, out_sig_len=out_len,
                                       **arrays(world, sc.groups, sc.msgs, table))


def check_parent(ctx, world, sc, got, table=False, seed=SEED, flags=0):
    """Case 2: the answers are those of blsgpu_verify_same_message for the same arrays, seed and flags."""
    res, gres, st = ctx.verify_same_message(seed=seed, flags=flags, **arrays(world, sc.groups, sc.msgs, table))
    assert (np.asarray(got[0]) == res).all() and (np.asarray(got[1]) == gres).all()
    for f in ("groups_accepted", "groups_retried", "retry_sets", "unique_messages", "form"):
        assert getattr(got[2], f) == getattr(st, f), f


def check(ctx, world, sc, sums, mask=None, table=False, seed=SEED, flags=0, out_lens=(96, 192)):
    """One call per output length: results against the oracle, aggregates and counts against `sums`."""
    want_g = group_rule(sc.groups, sc.want)
    got = None
    for out_len in out_lens:
        got = run_agg(ctx, world, sc, table=table, seed=seed, flags=flags, mask=mask, out_len=out_len)
        res, gres, st, out, cnt = got
        assert [int(r) for r in res] == sc.want
        assert [int(x) for x in gres] == want_g
        assert [int(c) for c in cnt] == [c for _, c in sums]
        want_out = encode(sums, out_len)
        bad = [g for g in range(len(sc.groups)) if out[g] != want_out[g]]
        assert not bad, f"out_sig_len {out_len}: aggregates of groups {bad} differ"
    check_parent(ctx, world, sc, got, table=table, seed=seed, flags=flags)
    return got


# ------------------------------------------------------------------------------------------- 1 known groups
KNOWN_SIZES = [1, 2, 3, 0, 63, 64, 65, 129]
KNOWN_MSGS = [0, 1, 0, 2, 1, 0, 1, 0]


@pytest.fixture(scope="module")
def known(world):
    groups, k = [], 0
    for n, mi in zip(KNOWN_SIZES, KNOWN_MSGS):
        groups.append([world.valid((7 * (k + j) + 3) % K, mi, wide=(k + j) % 3 == 1) for j in range(n)])
        k += n
    return scenario(world, groups, KNOWN_MSGS)


@pytest.fixture(scope="module")
def known_sums(world, known):
    return expected_sums(world, known)


@pytest.mark.parametrize("table", [False, True])
def test_known_groups(ctx, world, known, known_sums, table):
    assert all(r == 1 for r in known.want)
    assert [c for _, c in known_sums] == KNOWN_SIZES
    res, gres, st, out, cnt = check(ctx, world, known, known_sums, table=table)
    assert out[3] == bytes(192) and cnt[3] == 0 and gres[3] == EMPTY
    assert list(gres) == [1, 1, 1, EMPTY, 1, 1, 1, 1] and st.retry_sets == 0


# -------------------------------------------------------------------------------------------- 3 launch forms
def form_groups(world, lanes):
    """Group sizes around the form's lane count (several waves of groups for the lane-group forms), every eleventh set
    carrying the next key's signature, so each form also skips sets."""
    if lanes == 1:
        sizes = [(1, 2, 3, 0)[g % 4] for g in range(70)]
    else:
        sizes = [lanes - 1, lanes, lanes + 1] * {64: 1, 32: 1, 16: 2, 8: 3}[lanes]
    groups, msgs, k = [], [], 0
    for g, n in enumerate(sizes):
        mi = g % 3
        grp = []
        for j in range(n):
            i = (5 * (k + j) + 1) % K
            grp.append(Set(i, world.sig96[mi][(i + 1) % K if (k + j) % 11 == 5 else i]))
        groups.append(grp)
        msgs.append(mi)
        k += n
    return groups, msgs


@pytest.mark.parametrize("lanes", [1, 8, 16, 32, 64])
def test_launch_forms(ctx, world, lanes):
    from lodestar_amd import native

    groups, msgs = form_groups(world, lanes)
    n = sum(len(g) for g in groups)
    assert n <= 300
    assert native.same_message_agg_lanes(len(groups), n) == lanes
    sc = scenario(world, groups, msgs)
    assert 0 in sc.want and 1 in sc.want
    check(ctx, world, sc, expected_sums(world, sc), out_lens=(96,))


# ----------------------------------------------------------------------------------- 4 failing sets are left out
def corrupted_sig(world, kind, i, j, mi):
    for s in range(64):
        _, buf, sig_len, applied = corrupt.corrupt_sets([world.sig96[mi][i], world.sig96[mi][j]],
                                                        [world.m[mi], world.m[mi]], np.random.default_rng(s), frac=0,
                                                        min_bad=1, kinds=[kind])
        if list(applied) == [0]:
            return bytes(buf[:min(sig_len[0], 192)])
    raise AssertionError("no seed corrupts the first set")


@pytest.fixture(scope="module")
def failing(world):
    """A 65-set group with a valid signature over another message at its first, a middle and its last position; one
    5-set group per signature error class of oracle.corrupt (an identity signature among them); a group with a
    malformed bytes-mode key; a group in which every set fails."""
    groups, msgs = [], []
    g = [world.valid(j, 1) for j in range(65)]
    for pos in (0, 32, 64):
        g[pos] = Set(pos, world.sig96[2][pos])
    groups.append(g)
    msgs.append(1)
    for t, kind in enumerate(corrupt.KINDS):
        pos, mi = (0, 2, 4)[t % 3], t % 3
        g = [world.valid((13 * t + j) % K, mi) for j in range(5)]
        i = g[pos].key
        g[pos] = Set(i, corrupted_sig(world, kind, i, (i + 1) % K, mi))
        groups.append(g)
        msgs.append(mi)
    g = [world.valid(80 + j, 0) for j in range(5)]
    pk = bytearray(world.pk96[83])
    pk[95] ^= 1
    g[3] = g[3]._replace(pk=bytes(pk))
    groups.append(g)
    msgs.append(0)
    groups.append([Set(90 + j, world.sig96[1][90 + j]) for j in range(3)])  # signatures over m1 in a group signing m2
    msgs.append(2)
    return scenario(world, groups, msgs)


@pytest.fixture(scope="module")
def failing_sums(world, failing):
    return expected_sums(world, failing)


def test_failing_sets_are_left_out(ctx, world, failing, failing_sums):
    k0 = 65
    assert [failing.want[k] for k in (0, 32, 64)] == [0, 0, 0] and failing.want[:65].count(1) == 62
    by_kind = {kind: failing.want[k0 + 5 * t: k0 + 5 * t + 5] for t, kind in enumerate(corrupt.KINDS)}
    assert by_kind["infinity"].count(0) == 1 and by_kind["uncompressed_valid"] == [1] * 5
    assert {-r for r in failing.want if r < 0} >= {bls.BLST_BAD_ENCODING, bls.BLST_POINT_NOT_ON_CURVE,
                                                   bls.BLST_POINT_NOT_IN_GROUP, bls.BLST_INVALID_SIZE}
    assert failing.want[-8:-3].count(1) == 4 and failing.want[-3:] == [0, 0, 0]
    res, gres, st, out, cnt = check(ctx, world, failing, failing_sums)
    assert cnt[0] == 62 and cnt[-1] == 0 and out[-1] == bytes(192)
    assert sum(int(c) for c in cnt) == failing.want.count(1)


def test_failing_sets_table_mode(ctx, world, failing):
    keep = [g for g, grp in enumerate(failing.groups) if all(s.pk is None for s in grp)]
    sub = scenario(world, [failing.groups[g] for g in keep], [failing.msgs[g] for g in keep])
    check(ctx, world, sub, expected_sums(world, sub), table=True, out_lens=(96,))


# ------------------------------------------------------------------------------------------- 5 agg_include
def test_include_mask(ctx, world, known, known_sums, failing, failing_sums):
    n = len(known.want)
    alt = np.arange(n, dtype=np.uint8) % 2
    check(ctx, world, known, expected_sums(world, known, alt), mask=alt)
    none = np.zeros(n, np.uint8)
    res, gres, st, out, cnt = check(ctx, world, known, expected_sums(world, known, none), mask=none, out_lens=(96,))
    assert (res == 1).all() and not cnt.any() and all(o == bytes(96) for o in out)
    check(ctx, world, known, known_sums, mask=np.full(n, 255, np.uint8), out_lens=(96,))
    drop_failed = np.array([1 if r == 1 else 0 for r in failing.want], np.uint8)
    check(ctx, world, failing, failing_sums, mask=drop_failed, out_lens=(96,))


# ------------------------------------------------------------------------------------------ 6 identity sum
def test_identity_sum(ctx, world):
    """(pk, sig) and the pair of the secret key R - sk, (-pk, -sig): both verify, their sum is the identity.  The group
    beside it sums a signature with itself (the doubling branch of the mixed addition)."""
    sk = world.sks[17]
    skb = sk32(sk) + sk32(bls.R - sk)
    pk = cpu.sk_to_pk(skb, threads=THREADS)
    sg = cpu.sign(skb, world.m[1] * 2, threads=THREADS)
    pair = [Set(17, sg[:96], pk[:96]), Set(17, sg[96:], pk[96:])]
    assert world.point(sg[96:]) == bls.g2_neg(world.point(sg[:96]))
    sc = scenario(world, [pair, [world.valid(17, 1), world.valid(17, 1)]], [1, 1])
    assert sc.want == [1, 1, 1, 1]
    sums = expected_sums(world, sc)
    assert sums[0] == (None, 2) and sums[1][0] is not None
    res, gres, st, out, cnt = run_agg(ctx, world, sc, out_len=96)
    assert list(res) == [1, 1, 1, 1] and list(cnt) == [2, 2]
    assert out[0] == bytes([0xC0]) + bytes(95) and out[1] == bls.g2_compress(sums[1][0])
    out192 = run_agg(ctx, world, sc, out_len=192)[3]
    assert out192[0] == bytes([0x40]) + bytes(191) and out192[1] == bls.g2_serialize(sums[1][0])
    check(ctx, world, sc, sums)


# ------------------------------------------------------------------------------------------------- 7 flags
@pytest.mark.parametrize("flags", [1, 4, 5])
def test_flags_change_no_output(ctx, world, known, known_sums, failing, failing_sums, flags):
    from lodestar_amd import native

    assert (native.SAME_LANE_FORMS, native.SAME_BLOCK_CHECK) == (1, 4)
    for sc, sums in ((known, known_sums), (failing, failing_sums)):
        base = run_agg(ctx, world, sc)
        got = check(ctx, world, sc, sums, flags=flags, out_lens=(96,))
        assert (got[0] == base[0]).all() and (got[1] == base[1]).all()
        assert got[3] == base[3] and (got[4] == base[4]).all()


# --------------------------------------------------------------------------------------- 8 seed independence
def test_seed_independence(ctx, world, failing, failing_sums):
    outs = [check(ctx, world, failing, failing_sums, seed=seed, out_lens=(96,)) for seed in (SEED, 0x1234567, 0)]
    assert outs[0][3] == outs[1][3] == outs[2][3]
    assert (outs[0][4] == outs[1][4]).all() and (outs[0][4] == outs[2][4]).all()


# ------------------------------------------------------------------------------------------------ 9 refusals
def test_refusals_leave_the_outputs_untouched(ctx, world):
    from lodestar_amd import native

    lib = native.load()
    buf = np.frombuffer(b"".join(world.sig96[0][:4]), np.uint8).copy()
    pkb = np.frombuffer(b"".join(world.pk96[:4]), np.uint8).copy()
    gf = np.array([0, 1, 4], np.uint32)
    sl = np.full(4, 96, np.uint32)
    m = np.frombuffer(world.m[0] * 2, np.uint8).copy()
    res, gres = np.full(4, 0x55, np.int8), np.full(2, 0x55, np.int8)
    out, cnt = np.full(2 * 192, 0x55, np.uint8), np.full(2, 0x55555555, np.uint32)
    st = native.SameMessageStats()
    st.retry_sets = 0xABAB

    def call(n=2, out=out, out_len=96, cnt=cnt, inc=None):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.blsgpu_verify_same_message_agg(ctx.h, n, gf.ctypes.data, m.ctypes.data, pkb.ctypes.data, None,
                                                  buf.ctypes.data, 96, sl.ctypes.data, 3, 0, res.ctypes.data,
                                                  gres.ctypes.data, ctypes.byref(st), p(inc), p(out), out_len, p(cnt))

    assert call(out=None) == native.ERR_ARGS
    assert call(cnt=None) == native.ERR_ARGS
    assert call(out_len=95) == native.ERR_ARGS
    assert call(out_len=0) == native.ERR_ARGS
    assert (res == 0x55).all() and (gres == 0x55).all() and (out == 0x55).all() and (cnt == 0x55555555).all()
    assert st.retry_sets == 0xABAB
    assert call(n=0, out=None, cnt=None) == native.OK and st.retry_sets == 0
    assert (res == 0x55).all() and (out == 0x55).all()
    assert call(out_len=192) == native.OK
    assert list(res) == [1] * 4 and list(gres) == [1, 1] and list(cnt) == [1, 3]
    want = bls.g2_add(bls.g2_add(world.point(world.sig96[0][1]), world.point(world.sig96[0][2])),
                      world.point(world.sig96[0][3]))
    assert out[:192].tobytes() == world.wide(world.sig96[0][0]) and out[192:].tobytes() == bls.g2_serialize(want)


def test_entropy_failure_writes_nothing(ctx, world, known):
    from lodestar_amd import native

    a = arrays(world, known.groups[:3], known.msgs[:3])
    gf = np.asarray(a["group_first"], np.uint32)
    m = np.frombuffer(a["msgs"], np.uint8).copy()
    buf = np.frombuffer(a["sigs"], np.uint8).copy()
    pkb = np.frombuffer(a["pk_bytes"], np.uint8).copy()
    sl = np.asarray(a["sig_len"], np.uint32)
    res, out, cnt = np.full(6, 0x55, np.int8), np.full(3 * 96, 0x55, np.uint8), np.full(3, 0x55555555, np.uint32)
    native.debug_inject(native.INJECT_ENTROPY, 0, 1)
    try:
        rc = native.load().blsgpu_verify_same_message_agg(
            ctx.h, 3, gf.ctypes.data, m.ctypes.data, pkb.ctypes.data, None, buf.ctypes.data, a["sig_stride"],
            sl.ctypes.data, 0, 0, res.ctypes.data, None, None, None, out.ctypes.data, 96, cnt.ctypes.data)
    finally:
        native.debug_inject(native.INJECT_ENTROPY, 0, 0)
    assert rc == native.ERR_ENTROPY
    assert (res == 0x55).all() and (out == 0x55).all() and (cnt == 0x55555555).all()


# ---------------------------------------------------------------------------------------------- 10 round trip
def test_round_trip_fast_aggregate_verify(ctx, world, known):
    """The aggregate of the 65-set group verifies as a FastAggregateVerify over the counted keys (the oracle, one
    aggregate set), and no longer does once a key is left out."""
    g = KNOWN_SIZES.index(65)
    res, gres, st, out, cnt = run_agg(ctx, world, known)
    assert cnt[g] == 65
    keys = [world.pk96[s.key] for s in known.groups[g]]

    def fav(keys):
        r, _ = cpu.verify_jobs(threads=1, job_first_set=[0, 1], sigs=out[g], sig_len=[96],
                               msgs=world.m[known.msgs[g]], pk_bytes=b"".join(keys), set_pk_first=[0, len(keys)],
                               job_flags=[0], sig_stride=96)
        return int(r[0])

    assert fav(keys) == 1
    assert fav(keys[:-1]) == 0
