"""aggregateWithRandomness on the GPU (blsgpu_aggregate_with_randomness, csrc/k_awr.hip) and the same-message method
built on it (api.verify_signature_sets_same_message) against the oracle.

Expected values come from the oracle alone.  A set is (key i, signature bytes); the oracle knows every signature as
terms [(secret scalar, message)], so with r_k = r_of_word(words[k]) of randomness_words(n, seed) a group's outputs are

    P = sk_to_pk(sum r_k sk_k mod R)        S = sum over messages of sign(sum r_k t_k mod R, message)

computed by oracle.cpu.sk_to_pk / oracle.cpu.sign (one message per group except where a test swaps one in; the sum
over messages is bls.g2_add) and compared byte for byte: the arithmetic is exact.

Keys and signatures are made once per module (129 interop keys signing ONE message).
"""
import ctypes
import functools
import hashlib
import threading
from collections import namedtuple

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import corrupt, cpu
from tests.emu_helpers import r_of_word

pytestmark = pytest.mark.gpu

THREADS = 16
K = 129
NONE = 0xFFFFFFFF
SEED = 0x53414D454D5347
INF96 = bytes([0xC0]) + bytes(95)
INF192 = bytes([0x40]) + bytes(191)
FORMS = (64, 32, 16, 8, 1)

# key: index of the set's key (table entry / world.pk96[key]); sig: its bytes; terms: [(scalar, message)] the oracle
# knows the signature as ([] = the identity); code: the code Signature.fromBytes rejects it with (0 = accepted);
# pk: replacement key bytes (bytes mode only) and pk_code: the code those are rejected with
Set = namedtuple("Set", "key sig terms code pk pk_code", defaults=(0, None, 0))


def sk32(x):
    return (x % bls.R).to_bytes(32, "big")


def msg(j, tag=b"same-message"):
    return hashlib.sha256(tag + j.to_bytes(4, "little")).digest()


class World:
    def __init__(self):
        self.sks = [bls.interop_secret_key(i) for i in range(K)]
        skb = b"".join(sk32(s) for s in self.sks)
        self.m = msg(0)
        pk = cpu.sk_to_pk(skb, threads=THREADS)
        self.pk96 = [pk[96 * i: 96 * i + 96] for i in range(K)]
        sg = cpu.sign(skb, self.m * K, threads=THREADS)
        self.sig96 = [sg[96 * i: 96 * i + 96] for i in range(K)]
        self._sig192 = {}

    def sig192(self, i):
        if i not in self._sig192:
            self._sig192[i] = bls.g2_serialize(bls.signature_from_bytes(self.sig96[i], validate=False))
        return self._sig192[i]

    def valid(self, i, wide=False):
        return Set(i, self.sig192(i) if wide else self.sig96[i], [(self.sks[i], self.m)])


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


def run(ctx, world, groups, table=False, seed=SEED, out_pk_len=96, out_sig_len=192):
    from lodestar_amd import native

    flat = [s for g in groups for s in g]
    stride = 192 if any(len(s.sig) > 96 for s in flat) else 96
    first = np.cumsum([0] + [len(g) for g in groups])
    buf = b"".join(s.sig[:stride].ljust(stride, b"\0") for s in flat)
    keys = dict(pk_index=[s.key for s in flat]) if table else \
        dict(pk_bytes=b"".join(s.pk if s.pk is not None else world.pk96[s.key] for s in flat))
    lanes = native.awr_lanes(len(groups), len(flat))
    return ctx.aggregate_with_randomness(first, buf, sig_len=[len(s.sig) for s in flat], sig_stride=stride, seed=seed,
                                         out_pk_len=out_pk_len, out_sig_len=out_sig_len, **keys), lanes


def expected(world, groups, seed=SEED, want_sig=None):
    """Per group: None for an empty group, (code, call-wide index) for a rejected one, else (P 96 bytes, S) with S the
    96-byte compressed sum (None = the identity; "skipped" where want_sig(g) is false: the P-only groups of the
    largest call).  One oracle.cpu.sk_to_pk and one oracle.cpu.sign call for the whole list."""
    from lodestar_amd import native

    n = sum(len(g) for g in groups)
    words = [int(w) for w in native.randomness_words(n, seed)]
    out, pk_jobs, sig_jobs = [], [], []
    k = 0
    for gi, g in enumerate(groups):
        bad = None
        p_sum, s_sums = 0, {}
        for j, s in enumerate(g):
            code = s.pk_code or s.code  # the key's code when both are rejected
            if code and bad is None:
                bad = (code, k + j)
            r = r_of_word(words[k + j], raw=True)
            p_sum += r * world.sks[s.key]
            for t, m in s.terms:
                s_sums[m] = s_sums.get(m, 0) + r * t
        k += len(g)
        if not g:
            out.append(None)
        elif bad:
            out.append(bad)
        else:
            out.append([len(pk_jobs), None])
            pk_jobs.append(sk32(p_sum))
            if want_sig is None or want_sig(gi):
                out[-1][1] = [len(sig_jobs) + i for i in range(len(s_sums))]
                sig_jobs.extend((sk32(v), m) for m, v in s_sums.items())
            else:
                out[-1][1] = "skipped"
    pks = cpu.sk_to_pk(b"".join(pk_jobs), threads=THREADS) if pk_jobs else b""
    sigs = cpu.sign(b"".join(a for a, _ in sig_jobs), b"".join(m for _, m in sig_jobs), threads=THREADS) \
        if sig_jobs else b""
    for e in out:
        if isinstance(e, list):
            e[0] = pks[96 * e[0]: 96 * e[0] + 96]
            if e[1] == "skipped":
                continue
            parts = [sigs[96 * i: 96 * i + 96] for i in e[1]]
            if len(parts) == 1:
                e[1] = None if parts[0] == INF96 else parts[0]
            else:
                acc = None
                for b in parts:
                    p = None if b == INF96 else bls.signature_from_bytes(b, validate=False)
                    acc = p if acc is None else (acc if p is None else bls.g2_add(acc, p))
                e[1] = None if acc is None else bls.g2_compress(acc)
    return out


def pk_form(p96, out_len):
    return p96 if out_len == 96 else bls.g1_compress(bls.g1_deserialize(p96))


def sig_form(s96, out_len):
    if s96 is None:
        return INF96 if out_len == 96 else INF192
    return s96 if out_len == 96 else bls.g2_serialize(bls.signature_from_bytes(s96, validate=False))


def check(got, want, out_pk_len=96, out_sig_len=192):
    p, s, st, fb = got
    assert len(p) == len(s) == len(st) == len(fb) == len(want)
    bad = []
    for g, e in enumerate(want):
        if e is None:
            ok = st[g] == 9 and fb[g] == NONE and p[g] == bytes(out_pk_len) and s[g] == bytes(out_sig_len)
        elif isinstance(e, tuple):
            ok = (st[g], fb[g]) == e and p[g] == bytes(out_pk_len) and s[g] == bytes(out_sig_len)
        else:
            ok = st[g] == 0 and fb[g] == NONE and p[g] == pk_form(e[0], out_pk_len) and \
                (e[1] == "skipped" or s[g] == sig_form(e[1], out_sig_len))
        if not ok:
            bad.append((g, int(st[g]), int(fb[g])))
    assert not bad, f"{len(bad)} of {len(want)} groups differ, first (group, status, first_bad): {bad[:5]}"


# ---------------------------------------------------------------------------------------------- 1 known answers
KNOWN_SIZES = [1, 2, 3, 0, 63, 64, 65, 129]


@pytest.fixture(scope="module")
def known(world):
    """Groups of 1, 2, 3, 0, 63, 64, 65 and 129 sets, set k with key (7 k + 3) % K, every third signature in its
    192-byte encoding, and the oracle's answers."""
    groups, k = [], 0
    for n in KNOWN_SIZES:
        groups.append([world.valid((7 * (k + j) + 3) % K, wide=(k + j) % 3 == 1) for j in range(n)])
        k += n
    return groups, expected(world, groups)


@pytest.mark.parametrize("out_pk_len,out_sig_len", [(96, 192), (96, 96), (48, 192), (48, 96)])
def test_known_answers(ctx, world, known, out_pk_len, out_sig_len):
    """P = sk_to_pk(sum r_i sk_i) and S = sign(sum r_i sk_i, m) for groups at the wave-stride and tree boundaries (63,
    64, 65: one stride of a wave; 129: three), mixed 96- / 192-byte signatures, every output encoding; table mode and
    bytes mode give the same bytes; each (P, m, S) verifies."""
    from lodestar_amd import api

    groups, want = known
    got_b, lanes = run(ctx, world, groups, table=False, out_pk_len=out_pk_len, out_sig_len=out_sig_len)
    got_t, _ = run(ctx, world, groups, table=True, out_pk_len=out_pk_len, out_sig_len=out_sig_len)
    assert lanes == 64
    check(got_b, want, out_pk_len, out_sig_len)
    assert got_t[0] == got_b[0] and got_t[1] == got_b[1]
    assert (got_t[2] == got_b[2]).all() and (got_t[3] == got_b[3]).all()
    if out_pk_len == 96:
        for g, e in enumerate(want):
            if e is not None:
                assert api.verify_signature_set(ctx, got_b[0][g], world.m, got_b[1][g]), g


def test_fresh_scalars_differ_and_verify(ctx, world):
    """seed 0: two calls give different (P, S), both verifying; a one-set group is randomized too."""
    from lodestar_amd import api

    groups = [[world.valid(5)], [world.valid(i) for i in range(8)]]
    (p1, s1, st1, _), _ = run(ctx, world, groups, seed=0)
    (p2, s2, st2, _), _ = run(ctx, world, groups, seed=0)
    assert not st1.any() and not st2.any()
    for g in range(2):
        assert p1[g] != p2[g] and s1[g] != s2[g] and p1[g] != world.pk96[5]
        assert api.verify_signature_set(ctx, p1[g], world.m, s1[g])
        assert api.verify_signature_set(ctx, p2[g], world.m, s2[g])


# ---------------------------------------------------------------------------------------------- 2 launch forms
@functools.lru_cache(maxsize=None)
def form_shape(lanes):
    """(n_groups, sizes) of the call that exercises form `lanes`: group sizes cycle lanes - 2 .. lanes + 2 (at least
    1: five sizes around the lane count, so lanes with no set, one set and two sets all occur); n_groups is the
    smallest count for which the rule itself returns `lanes` for such groups, then up to four more groups while the
    rule still does (so the sizes vary within the call)."""
    from lodestar_amd import native

    def size(g):
        return max(1, lanes - 2 + g % 5)

    n, total = 0, 0
    while True:
        total += size(n)
        n += 1
        if native.awr_lanes(n, total) == lanes:
            break
        assert n < 1 << 17, f"the rule never returns {lanes} for such groups"
    for _ in range(4):
        if native.awr_lanes(n + 1, total + size(n)) != lanes:
            break
        total += size(n)
        n += 1
    return n, tuple(size(g) for g in range(n))


@pytest.mark.parametrize("lanes", FORMS)
def test_every_launch_form(ctx, world, lanes):
    """Each of the five forms, in table mode, every group against the oracle (status, first_bad, P and S)."""
    from lodestar_amd import native

    n, sizes = form_shape(lanes)
    groups, k = [], 0
    for sz in sizes:
        groups.append([world.valid((5 * (k + j) + 1) % K) for j in range(sz)])
        k += sz
    assert native.awr_lanes(n, k) == lanes
    got, used = run(ctx, world, groups, table=True, out_sig_len=96)
    assert used == lanes
    check(got, expected(world, groups), 96, 96)


def test_one_lane_form_by_group_count(ctx, world):
    """Beyond the forms above: the one-lane form as the group COUNT brings it about (the smallest count of groups of 1
    .. 5 sets for which the rule returns 1, taken from the rule), where a lane sums several sets by itself and the
    last wave is partial.  Every group's status, first_bad and P against the oracle; S for every 16th group and the
    last 64 (the oracle signs at a few ms per group: all of them would take tens of seconds)."""
    from lodestar_amd import native

    n, total = 5, 15  # at least one group of every size: the mean size is above 1
    while native.awr_lanes(n, total) != 1:
        total += 1 + n % 5
        n += 1
    assert n > 1024
    groups, k = [], 0
    for g in range(n):
        groups.append([world.valid((5 * (k + j) + 1) % K) for j in range(1 + g % 5)])
        k += 1 + g % 5
    want = expected(world, groups, want_sig=lambda g: g % 16 == 0 or g >= n - 64)
    got, used = run(ctx, world, groups, table=True, out_sig_len=96)
    assert used == 1
    check(got, want, 96, 96)


def test_forms_covered_are_all_five():
    from lodestar_amd import native

    covered = set()
    for lanes in FORMS:
        n, sizes = form_shape(lanes)
        covered.add(native.awr_lanes(n, sum(sizes)))
    assert covered == {64, 32, 16, 8, 1}


# ------------------------------------------------------------------------------- 3 error classes and isolation
def corrupted(world, kind, i, j):
    """Key i's set with its signature corrupted by oracle.corrupt kind `kind` (j: the key whose signature `swap`
    puts in its place)."""
    for s in range(64):
        msgs, buf, sig_len, applied = corrupt.corrupt_sets([world.sig96[i], world.sig96[j]], [world.m, world.m],
                                                           np.random.default_rng(s), frac=0, min_bad=1, kinds=[kind])
        if list(applied) == [0]:
            break
    else:
        raise AssertionError("no seed corrupts the first set")
    sig = buf[:sig_len[0]] if sig_len[0] <= 192 else buf[:192]
    code = cpu.sig_status(sig)
    if code:
        return Set(i, sig, [], code)
    terms = {"swap": [(world.sks[j], world.m)], "negated": [(-world.sks[i], world.m)], "infinity": [],
             "infinity_192": []}.get(kind, [(world.sks[i], world.m)])
    return Set(i, sig, terms)


def bad_key(world, i, how):
    pk = bytearray(world.pk96[i])
    if how == "compressed_flag":
        pk[0] |= 0x80
    elif how == "off_curve":
        pk[95] ^= 1
    else:
        pk = bytearray([0x40]) + bytearray(95)
    code = cpu.pk_decode(bytes(pk))[0] or bls.BLST_PK_IS_INFINITY
    return Set(i, world.sig96[i], [(world.sks[i], world.m)], 0, bytes(pk), code)


def test_error_classes_and_isolation(ctx, world):
    """One 5-set group per oracle.corrupt kind (the identity signature among them) and per malformed bytes-mode key,
    the touched set first, in the middle or last in its group, after eight clean groups: a rejected group reports its
    class code and the set's call-wide index and writes zeros; a well-formed corruption (another key's signature, the
    negation, the identity, the 192-byte form) is summed as the oracle sums it; the clean groups' bytes equal the same
    call without the other groups.  A group with two rejected sets reports the lower one; a set whose key and signature
    are both rejected reports the key's code."""
    clean = [[world.valid((11 * g + j) % K, wide=j == 2) for j in range(5)] for g in range(8)]
    touched, kinds = [], []
    specials = list(corrupt.KINDS) + ["key:compressed_flag", "key:off_curve", "key:infinity"]
    for t, kind in enumerate(specials):
        pos = (0, 2, 4)[t % 3]
        g = [world.valid((13 * t + j) % K) for j in range(5)]
        i = g[pos].key
        g[pos] = bad_key(world, i, kind[4:]) if kind.startswith("key:") else corrupted(world, kind, i, (i + 1) % K)
        touched.append(g)
        kinds.append((kind, pos))
    two = [world.valid(j) for j in range(5)]
    two[3] = corrupted(world, "not_in_group", 3, 4)
    two[1] = bad_key(world, 1, "off_curve")
    both = [world.valid(j + 20) for j in range(3)]
    both[1] = bad_key(world, 21, "off_curve")._replace(sig=corrupted(world, "x_ge_p", 21, 22).sig, terms=[],
                                                       code=bls.BLST_BAD_ENCODING)
    groups = clean + touched + [two, both]
    want = expected(world, groups)
    # every class occurred, each position held a rejected set
    codes = {e[0] for e in want if isinstance(e, tuple)}
    assert codes == {bls.BLST_BAD_ENCODING, bls.BLST_POINT_NOT_ON_CURVE, bls.BLST_POINT_NOT_IN_GROUP,
                     bls.BLST_INVALID_SIZE, bls.BLST_PK_IS_INFINITY}
    rejected_pos = {pos for (kind, pos), e in zip(kinds, want[8:]) if isinstance(e, tuple)}
    assert rejected_pos == {0, 2, 4}
    assert want[-2] == (bls.BLST_POINT_NOT_ON_CURVE, 5 * (8 + len(touched)) + 1)
    assert want[-1] == (bls.BLST_POINT_NOT_ON_CURVE, 5 * (9 + len(touched)) + 1)
    got, lanes = run(ctx, world, groups)
    assert lanes == 8
    check(got, want)
    alone, _ = run(ctx, world, clean)
    assert got[0][:8] == alone[0] and got[1][:8] == alone[1]
    # the identity signature's group: the other four sets make S, all five keys make P (checked above against the
    # oracle's terms); and the group of table-mode keys with a signature error behaves the same
    got_t, _ = run(ctx, world, clean + touched[:len(corrupt.KINDS)], table=True)
    check(got_t, want[:8 + len(corrupt.KINDS)])


def test_table_index_beyond_the_table_is_an_argument_error(ctx, world):
    from lodestar_amd import native

    g = [world.valid(0), world.valid(1)]
    g[1] = g[1]._replace(key=K)
    with pytest.raises(RuntimeError, match="ERR_ARGS"):
        run(ctx, world, [g], table=True)
    assert native.code_name(native.ERR_ARGS) == "BLSGPU_ERR_ARGS"


# ------------------------------------------------------------------------------------------------ 4 identity
def test_identity_encodings(ctx, world):
    """(pk, sig) and (-pk, -sig) in one group: the scalars differ, so nothing cancels -- the outputs are finite and
    equal the oracle's.  A group whose only signature is the identity: S is the identity encoding, P is finite."""
    a = world.valid(9)
    neg_pk = bls.g1_serialize(bls.g1_neg(bls.g1_deserialize(world.pk96[9])))
    neg_sig = bytes([a.sig[0] ^ 0x20]) + a.sig[1:]
    # the oracle's view of the negated set: key scalar -sk, signature term -sk
    world.sks.append(-world.sks[9] % bls.R)
    try:
        minus = Set(len(world.sks) - 1, neg_sig, [(-world.sks[9], world.m)], 0, neg_pk, 0)
        groups = [[a, minus], [Set(4, INF96, [])], [Set(4, INF192, []), Set(6, INF96, [])]]
        want = expected(world, groups)
    finally:
        world.sks.pop()
    for out_pk_len, out_sig_len in ((96, 192), (48, 96)):
        (p, s, st, fb), _ = run(ctx, world, groups, out_pk_len=out_pk_len, out_sig_len=out_sig_len)
        assert not st.any() and (fb == NONE).all()
        inf_pk = bytes([0xC0 if out_pk_len == 48 else 0x40]) + bytes(out_pk_len - 1)
        inf_sig = INF96 if out_sig_len == 96 else INF192
        assert p[0] != inf_pk and s[0] != inf_sig and p[0] != bytes(out_pk_len) and s[0] != bytes(out_sig_len)
        assert s[1] == inf_sig and s[2] == inf_sig and p[1] != inf_pk and p[2] != inf_pk
        check((p, s, st, fb), want, out_pk_len, out_sig_len)


def test_call_of_empty_groups_only(ctx, world):
    """No set at all: every group EMPTY_AGGREGATE with zero outputs (nothing to decode, nothing to scale)."""
    (p, s, st, fb), lanes = run(ctx, world, [[], [], []])
    assert lanes == 1 and list(st) == [9, 9, 9] and (fb == NONE).all()
    assert p == [bytes(96)] * 3 and s == [bytes(192)] * 3


# ------------------------------------------------------------------------------------------------ 5 soundness
def sets_of(world, sigs, keys):
    return [(world.pk96[k], s) for k, s in zip(keys, sigs)]


def oracle_same_message(world, keys, sigs, message):
    n = len(keys)
    stride = 192 if any(len(s) > 96 for s in sigs) else 96
    res, _ = cpu.verify_jobs(threads=THREADS, job_first_set=np.arange(n + 1),
                             sigs=b"".join(s[:stride].ljust(stride, b"\0") for s in sigs),
                             sig_len=[len(s) for s in sigs], msgs=message * n,
                             pk_bytes=b"".join(world.pk96[k] for k in keys), job_flags=np.ones(n), sig_stride=stride)
    return [int(r) == 1 for r in res]


def test_cancelling_forgery_is_caught(ctx, world):
    """sig_1 + D and sig_2 - D for a valid signature point D: the plain sums still verify (the oracle's
    fast_aggregate_verify of the plain aggregate is true), the randomized sums do not, so the method answers false
    exactly at positions 1 and 2, as the oracle's eight one-set jobs do."""
    from lodestar_amd import api

    keys = list(range(30, 38))
    pts = [bls.signature_from_bytes(world.sig96[k], validate=False) for k in keys]
    d = bls.signature_from_bytes(world.sig96[50], validate=False)
    forged = list(pts)
    forged[1] = bls.g2_add(pts[1], d)
    forged[2] = bls.g2_add(pts[2], bls.g2_neg(d))
    sigs = [bls.g2_compress(p) for p in forged]
    plain = forged[0]
    for p in forged[1:]:
        plain = bls.g2_add(plain, p)
    pk48 = [bls.g1_compress(bls.g1_deserialize(world.pk96[k])) for k in keys]
    assert bls.fast_aggregate_verify(pk48, world.m, bls.g2_compress(plain))
    want = oracle_same_message(world, keys, sigs, world.m)
    assert want == [True, False, False, True, True, True, True, True]
    assert api.verify_signature_sets_same_message(ctx, sets_of(world, sigs, keys), world.m, seed=0) == want


# ------------------------------------------------------------------------------------------- 6 the method
def test_same_message_method_vs_oracle(ctx, world):
    """verify_signature_sets_same_message equals the oracle's one-set jobs: all valid (bytes and table mode), one
    signature over another message, one malformed signature (false there, true elsewhere, no exception), one set
    alone (valid, and invalid)."""
    from lodestar_amd import api

    keys = list(range(60, 72))
    good = [world.sig96[k] for k in keys]
    other = cpu.sign(sk32(world.sks[keys[4]]), msg(1))
    cases = {
        "all valid": good,
        "wrong message": good[:4] + [other] + good[5:],
        "malformed": good[:7] + [corrupted(world, "not_on_curve", keys[7], keys[8]).sig] + good[8:],
        "short": good[:2] + [good[2][:48]] + good[3:],
    }
    for name, sigs in cases.items():
        want = oracle_same_message(world, keys, sigs, world.m)
        assert api.verify_signature_sets_same_message(ctx, sets_of(world, sigs, keys), world.m) == want, name
        assert sum(want) == (len(keys) if name == "all valid" else len(keys) - 1), name
    assert api.verify_signature_sets_same_message(ctx, list(zip(keys, good)), world.m) == [True] * len(keys)
    assert api.verify_signature_sets_same_message(ctx, list(zip(keys, cases["wrong message"])), world.m) == \
        oracle_same_message(world, keys, cases["wrong message"], world.m)
    assert api.verify_signature_sets_same_message(ctx, [(world.pk96[3], world.sig96[3])], world.m) == [True]
    assert api.verify_signature_sets_same_message(ctx, [(world.pk96[3], world.sig96[4])], world.m) == [False]
    with pytest.raises(api.BlstError, match="Empty signature set"):
        api.verify_signature_sets_same_message(ctx, [], world.m)
    p, s = api.aggregate_with_randomness(ctx, sets_of(world, good, keys))
    assert api.verify_signature_set(ctx, p, world.m, s)
    with pytest.raises(api.BlstError, match="BLST_ERROR: BLST_POINT_NOT_ON_CURVE"):
        api.aggregate_with_randomness(ctx, sets_of(world, cases["malformed"], keys))
    with pytest.raises(api.BlstError, match="EMPTY_AGGREGATE_ARRAY"):
        api.aggregate_with_randomness(ctx, [])


# ------------------------------------------------------------------------------- 7 beside a verification call
def test_beside_the_verifier(ctx, world, known):
    """A 2,048-set verification call in flight on the pipeline streams while the aggregation runs on the helper
    stream from this thread: both results are right."""
    n = 2048
    sks = b"".join(sk32(world.sks[i % 64]) for i in range(n))
    msgs = b"".join(msg(i, b"beside") for i in range(n))
    sigs = cpu.sign(sks, msgs, threads=THREADS)
    pks = b"".join(world.pk96[i % 64] for i in range(n))
    box = {}

    def verify():
        box["res"] = ctx.verify_raw(np.arange(n + 1), sigs, [96] * n, msgs, pk_bytes=pks, job_flags=np.ones(n),
                                    sig_stride=96)[0]

    t = threading.Thread(target=verify)
    t.start()
    got, _ = run(ctx, world, known[0])
    t.join(120)
    check(got, known[1])
    assert (box["res"] == 1).all()


# ------------------------------------------------------------------------ 8 argument errors, closed context
def test_argument_errors_and_closed_context(world):
    """Every BLSGPU_ERR_ARGS condition of the header through raw ctypes (refused on the host: the bad pointers and
    counts are never read), n_groups == 0, and BLSGPU_ERR_CLOSED from a context that is being destroyed."""
    from lodestar_amd import native

    lib = native.load()
    c = native.Context([0])
    c.upload_pubkeys(0, b"".join(world.pk96[:4]))
    buf = np.frombuffer(b"".join(world.sig96[:4]), np.uint8).copy()
    pkb = np.frombuffer(b"".join(world.pk96[:4]), np.uint8).copy()
    pki = np.arange(4, dtype=np.uint32)
    gf = np.array([0, 1, 4], np.uint32)
    sl = np.full(4, 96, np.uint32)
    opk, osig = np.zeros(2 * 96, np.uint8), np.zeros(2 * 192, np.uint8)
    st, fb = np.zeros(2, np.int8), np.zeros(2, np.uint32)

    def call(h=None, n=2, gf=gf, pkb=pkb, pki=None, buf=buf, stride=96, sl=sl, seed=3, opk=opk, opl=96, osig=osig,
             osl=192, st=st, fb=fb):
        p = lambda a: None if a is None else a.ctypes.data
        return lib.blsgpu_aggregate_with_randomness(c.h if h is None else h, n, p(gf), p(pkb), p(pki), p(buf), stride,
                                                    p(sl), seed, p(opk), opl, p(osig), osl, p(st), p(fb))

    assert call() == native.OK and list(st) == [0, 0]
    first = (opk.tobytes(), osig.tobytes())
    assert call(pkb=None, pki=pki) == native.OK and (opk.tobytes(), osig.tobytes()) == first
    assert call(fb=None) == native.OK  # first_bad is optional
    assert call(n=0) == native.OK
    assert call(n=0, gf=np.array([7], np.uint32)) == native.OK
    bad = {
        "null ctx": dict(h=ctypes.c_void_p(None)),
        "null group_first": dict(gf=None),
        "no keys": dict(pkb=None),
        "both key modes": dict(pki=pki),
        "null sigs": dict(buf=None),
        "null sig_len": dict(sl=None),
        "null out_pk": dict(opk=None),
        "null out_sig": dict(osig=None),
        "null status": dict(st=None),
        "out_pk_len": dict(opl=192),
        "out_pk_len 0": dict(opl=0),
        "out_sig_len": dict(osl=48),
        "sig_stride < 96": dict(stride=95),
        "group_first[0] != 0": dict(gf=np.array([1, 2, 4], np.uint32)),
        "group_first decreasing": dict(gf=np.array([0, 3, 2], np.uint32)),
        "too many sets": dict(gf=np.array([0, 1, (1 << 20) + 1], np.uint32)),
        "192-byte signature in a 96-byte stride": dict(sl=np.array([96, 96, 192, 96], np.uint32)),
        "index beyond the table": dict(pkb=None, pki=np.array([0, 1, 2, 4], np.uint32)),
    }
    for name, kw in bad.items():
        assert call(**kw) == native.ERR_ARGS, name

    # closed: hold the context open from a submission's completion callback, let blsgpu_destroy mark it closed, and
    # call until the refusal shows (each earlier call is a valid one-set aggregation)
    release, entered = threading.Event(), threading.Event()

    def done(user, status):
        entered.set()
        release.wait(60)

    cb = native.DONE_CB(done)
    b, keep = native.make_batch([0, 1], world.sig96[0], [96], world.m, pk_bytes=world.pk96[0], job_flags=[0],
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


def test_entropy_failure_refuses_the_call(ctx, world):
    """seed 0 with the entropy source failing: BLSGPU_ERR_ENTROPY, nothing written; the next call works."""
    from lodestar_amd import native

    lib = native.load()
    gf, sl = np.array([0, 1], np.uint32), np.full(1, 96, np.uint32)
    buf = np.frombuffer(world.sig96[0], np.uint8).copy()
    pkb = np.frombuffer(world.pk96[0], np.uint8).copy()
    opk, osig = np.full(96, 0xAB, np.uint8), np.full(192, 0xAB, np.uint8)
    st, fb = np.full(1, 0x55, np.int8), np.full(1, 0xABABABAB, np.uint32)

    def call():
        return lib.blsgpu_aggregate_with_randomness(ctx.h, 1, gf.ctypes.data, pkb.ctypes.data, None, buf.ctypes.data,
                                                    96, sl.ctypes.data, 0, opk.ctypes.data, 96, osig.ctypes.data, 192,
                                                    st.ctypes.data, fb.ctypes.data)

    native.debug_inject(native.INJECT_ENTROPY, 0, 1)
    try:
        assert call() == native.ERR_ENTROPY
    finally:
        native.debug_inject(native.INJECT_ENTROPY, 0, 0)
    assert (opk == 0xAB).all() and (osig == 0xAB).all() and st[0] == 0x55 and fb[0] == 0xABABABAB
    assert call() == native.OK and st[0] == 0 and fb[0] == NONE and not (opk == 0xAB).all()
