"""The committee store and blsgpu_aggregate_pubkeys_bits on the GPU.  The table is built on the device
from 600 interop secret keys and five keys that cancel (debug op 8), so the oracle's answer for a set is one scalar
multiplication (tests/committee_bits_helpers.py); every case is also compared, byte for byte, with table-mode
blsgpu_aggregate_pubkeys on the expanded index lists, and run with and without BLSGPU_BITS_NO_COMPLEMENT.  The kernel
strides 32-bit words of a segment's bits over 8 to 64 lanes: the committee sizes 1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65 and
512 put the tail mask, the word boundary and the lane stride on both sides of every edge."""
import numpy as np
import pytest

from oracle import cpu
from tests import committee_bits_helpers as H

pytestmark = pytest.mark.gpu

N_SIZE = len(H.SIZES)


def committees():
    """Ids 0..11: the size committees; then one committee per cancellation case."""
    return list(H.size_committees()) + [c for _, c, _, _ in H.CANCELLATION]


def upload(ctx, first, cms):
    ctx.upload_committees(first, np.cumsum([0] + [len(c) for c in cms]), [i for c in cms for i in c])


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd.native import Context

    c = Context([0])
    pk96, st = c.debug_op(8, H.sks_bytes(), 32, 96)
    assert (st == 0).all() and pk96 == H.table_pk96()
    c.upload_pubkeys(0, pk96)
    upload(c, 0, committees())
    assert c.committees_count == len(committees())
    yield c
    c.close()


@pytest.fixture()
def fresh():
    """A context of its own for the tests that change the table or the store."""
    from lodestar_amd.native import Context

    c = Context([0])
    c.upload_pubkeys(0, H.table_pk96())
    yield c
    c.close()


def check(ctx, sets, out_len=96, oracle=True, lanes=None):
    """Runs `sets` as shipped and under the flag, compares both with table-mode blsgpu_aggregate_pubkeys on the expanded
    lists and (oracle) with the oracle; returns the two stats."""
    cms = committees()
    lists = H.expand(cms, sets)
    arrays = H.call_arrays(sets)
    spf = np.cumsum([0] + [len(x) for x in lists])
    idx = np.array([i for x in lists for i in x] or [0], np.uint32)
    ref, ref_st = ctx.aggregate_pubkeys(set_pk_first=spf, pk_index=idx, out_len=out_len)
    if oracle:
        want = H.oracle_sums(lists, out_len)
        assert ref == [w for w, _ in want] and list(ref_st) == [s for _, s in want]
    stats = []
    for flags in (0, H.NO_COMPLEMENT):
        got, st, stat = ctx.aggregate_pubkeys_bits(*arrays, flags=flags, out_len=out_len)
        assert list(st) == list(ref_st), flags
        assert got == ref, (flags, [k for k in range(len(ref)) if got[k] != ref[k]][:8])
        want_plan = H.plan(cms, sets, no_complement=bool(flags))
        assert {k: getattr(stat, k) for k in want_plan if k != "n_items"} == \
            {k: v for k, v in want_plan.items() if k != "n_items"}
        assert stat.lanes == H.lanes_rule(len(sets), want_plan["n_items"]) and stat.device_ms > 0
        stats.append(stat)
    assert stats[1].segments_complemented == 0 and stats[1].keys_subtracted == 0
    if lanes is not None:
        assert stats[0].lanes == lanes
    return stats


@pytest.mark.parametrize("out_len", [48, 96])
def test_every_size_and_participation(ctx, out_len):
    """Per committee size: no bit, one bit (first, last), one clear (first, last), all, the three counts around the
    tie of the complement rule, a seeded random half -- 120 one-segment sets in one call."""
    rng = np.random.default_rng(77)
    sets, names = [], []
    for c, n in enumerate(H.SIZES):
        for name, bits in H.participations(n, rng).items():
            sets.append([(c, bits)])
            names.append((n, name))
    assert len(sets) == 10 * N_SIZE
    default, flagged = check(ctx, sets, out_len)
    assert default.segments_complemented > 0 and default.keys_subtracted > 0 and default.keys_added > 0
    assert flagged.keys_added == flagged.keys_present == default.keys_present


def test_multi_segment_sets(ctx):
    """Sets of 1, 2 and 64 segments mixing direct and complement segments, a committee used twice in one set, a set
    whose segments are all empty of bits, a set with no segment."""
    rng = np.random.default_rng(78)

    def seg(c, frac):
        return (c, rng.random(H.SIZES[c]) < frac)

    sets = [
        [seg(11, 0.95)],
        [seg(10, 0.97), seg(5, 0.2)],
        [seg(int(k % N_SIZE), (0.1, 0.96, 1.0, 0.5)[k % 4]) for k in range(64)],
        [seg(9, 0.9), seg(9, 0.9)],          # the same committee twice, both by complement
        [seg(8, 1.0), seg(8, 0.1)],          # twice: once by complement, once directly
        [seg(3, 0.0), seg(11, 0.0), seg(0, 0.0)],
        [],
        [seg(0, 1.0)],
    ]
    default, _ = check(ctx, sets)
    assert 0 < default.segments_complemented < default.segments == 1 + 2 + 64 + 2 + 2 + 3 + 1
    check(ctx, sets, out_len=48)


@pytest.mark.parametrize("out_len", [48, 96])
def test_cancellation(ctx, out_len):
    """Sums equal to the identity, an absent key equal to the stored sum, equal and opposite points within a lane and
    across lanes: as shipped and under the flag, equal to each other, to the table-mode call and to the oracle."""
    sets = [[(N_SIZE + k, np.array(bits, bool))] for k, (_, _, bits, _) in enumerate(H.CANCELLATION)]
    default, _ = check(ctx, sets, out_len)
    assert default.segments_complemented == sum(1 for *_, comp in H.CANCELLATION if comp)
    got, st, _ = ctx.aggregate_pubkeys_bits(*H.call_arrays(sets), out_len=out_len)
    by_name = {name: got[k] for k, (name, *_) in enumerate(H.CANCELLATION)}
    for name in ("sum_is_identity", "q_absent", "q_absent_complement", "absent_equals_sum",
                 "absent_equals_sum_complement", "opposite_across_lanes"):
        assert by_name[name] == H.identity(out_len), name
    assert not st.any()
    # all of them in one set: every segment's part cancels or adds up as the oracle says
    check(ctx, [[s[0] for s in sets]], out_len)


def few_bits(c, present, rng):
    b = np.zeros(H.SIZES[c], bool)
    b[rng.permutation(H.SIZES[c])[:present]] = True
    return (c, b)


@pytest.mark.parametrize("lanes,n_sets,committee,present", [
    (64, 3, 11, 200), (32, 3, 9, 24), (16, 3, 5, 12), (8, 3, 3, 3),  # by the mean items of a set
    (32, 1025, 11, 40), (16, 4097, 11, 40), (8, 8193, 11, 40),       # by the set count (40 items: 64 by the mean)
])
def test_lane_forms(ctx, lanes, n_sets, committee, present):
    """Every lane form the rule can choose; stats.lanes proves which one ran.  The many-set calls are compared with the
    table-mode call on every set and with the oracle on their first sets."""
    rng = np.random.default_rng(lanes * 1000 + n_sets)
    sets = [[few_bits(committee, present, rng)] for _ in range(n_sets)]
    if n_sets > 8:
        sets[5], sets[n_sets - 1] = [], [few_bits(committee, 0, rng)]  # an empty set inside a wave and at the end
    check(ctx, sets, oracle=n_sets <= 8, lanes=lanes)
    if n_sets > 8:
        check(ctx, sets[:16])  # (with the oracle)


def test_stats_of_a_mixed_call(ctx):
    """stats equals the plan the rule gives (checked inside check()); here the C4 shape of one set: a 512-member
    committee with 26 absent gathers 26 rows and one stored sum instead of 486 rows."""
    rng = np.random.default_rng(80)
    bits = np.ones(512, bool)
    bits[rng.permutation(512)[:26]] = False
    default, flagged = check(ctx, [[(11, bits)]])
    assert (default.segments_complemented, default.keys_subtracted, default.keys_added) == (1, 26, 0)
    assert (flagged.keys_added, flagged.keys_subtracted, flagged.keys_present) == (486, 0, 486)
    assert default.lanes == 32 and flagged.lanes == 64


def test_refusals_with_a_context(ctx):
    from lodestar_amd import native

    lib = native.load()
    sets = [[(2, np.ones(7, bool))], [(3, np.ones(8, bool)), (4, np.zeros(9, bool))]]
    ssf, seg, sbf, bits = H.call_arrays(sets)
    out, st = np.full(192, 0x5A, np.uint8), np.full(2, 77, np.int8)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731

    def call(n=2, ssf=ssf, seg=seg, sbf=sbf, bits=bits, flags=0, out=out, out_len=96, st=st):
        return lib.blsgpu_aggregate_pubkeys_bits(ctx.h, n, p(ssf), p(seg), p(sbf), p(bits), flags, p(out), out_len,
                                                 p(st), None)

    for kw in [dict(ssf=None), dict(seg=None), dict(sbf=None), dict(bits=None), dict(out=None), dict(st=None),
               dict(out_len=0), dict(out_len=97), dict(flags=2), dict(flags=0x80000001),
               dict(ssf=np.array([1, 1, 3], np.uint32)), dict(ssf=np.array([0, 2, 1], np.uint32)),
               dict(sbf=np.array([0, 2, 1], np.uint32)), dict(seg=np.array([2, 3, len(committees())], np.uint32)),
               dict(sbf=np.array([0, 1, 3], np.uint32)), dict(sbf=np.array([0, 1, 5], np.uint32)),
               dict(bits=np.array([0xFF, 0xFF, 0x00, 0x00], np.uint8)),  # bit 7 of the 7-bit string
               dict(bits=np.array([0x7F, 0xFF, 0x00, 0x02], np.uint8)),  # bit 17 of the 17-bit string
               dict(n=(1 << 20) + 1)]:
        assert call(**kw) == native.ERR_ARGS, kw
    assert (out == 0x5A).all() and (st == 77).all()  # a refused call writes nothing
    assert call(n=0) == native.OK and (out == 0x5A).all()
    assert call() == native.OK and st.tolist() == [0, 0]


def test_store_semantics(fresh):
    from lodestar_amd import native

    c = fresh
    cms = list(H.size_committees())
    one = [(0, np.ones(1, bool))]

    def answers(sets):
        return c.aggregate_pubkeys_bits(*H.call_arrays(sets))[0]

    def want(cm_list, sets):
        return [w for w, _ in H.oracle_sums(H.expand(cm_list, sets), 96)]

    assert c.committees_count == 0
    with pytest.raises(ValueError):
        answers([one])  # no committee stored: id 0 is refused
    upload(c, 0, cms[:4])
    assert c.committees_count == 4
    upload(c, 4, cms[4:6])  # append
    assert c.committees_count == 6
    sets = [[(k, np.ones(H.SIZES[k], bool))] for k in range(6)]
    assert answers(sets) == want(cms, sets)
    # truncate and append: committees 2.. are dropped, 2 and 3 become other committees
    other = [cms[7], cms[9]]
    upload(c, 2, other)
    assert c.committees_count == 4
    now = cms[:2] + other
    sets = [[(k, np.ones(len(now[k]), bool))] for k in range(4)]
    assert answers(sets) == want(now, sets)
    with pytest.raises(ValueError):
        answers([[(4, np.ones(9, bool))]])  # a dropped id
    # n == 0 only truncates
    upload(c, 1, [])
    assert c.committees_count == 1 and answers([one]) == want(cms, [one])
    with pytest.raises(ValueError):
        answers([[(1, np.ones(2, bool))]])
    # refused uploads store nothing and drop nothing
    for first, cm_list in [(2, [cms[1]]), (1, [()]), (1, [cms[1], ()]), (1, [(0, H.Q + 1)])]:
        with pytest.raises(ValueError):
            upload(c, first, cm_list)
        assert c.committees_count == 1 and answers([one]) == want(cms, [one])
    lib = native.load()
    cf, mem = np.array([0, 1], np.uint32), np.array([0], np.uint32)
    assert lib.blsgpu_committees_upload(c.h, 1, 1, None, mem.ctypes.data) == native.ERR_ARGS
    assert lib.blsgpu_committees_upload(c.h, 1, 1, cf.ctypes.data, None) == native.ERR_ARGS
    big = np.zeros((1 << 20) + 1, np.uint32)
    cf_big = np.array([0, (1 << 20) + 1], np.uint32)
    assert lib.blsgpu_committees_upload(c.h, 1, 1, cf_big.ctypes.data, big.ctypes.data) == native.ERR_ARGS
    assert c.committees_count == 1
    # appending table rows keeps the store; overwriting a row empties it (both uploads)
    upload(c, 1, cms[1:3])
    n = c.pubkeys_count
    c.upload_pubkeys(n, H.table_pk96()[:96 * 3])
    assert c.pubkeys_count == n + 3 and c.committees_count == 3 and answers([one]) == want(cms, [one])
    c.upload_pubkeys(n + 2, H.table_pk96()[:96])  # overwrites the last row (with the key it holds)
    assert c.committees_count == 0
    with pytest.raises(ValueError):
        answers([one])
    upload(c, 0, cms[:2])
    from oracle import bls12_381 as bls

    pk48 = bls.g1_compress(bls.g1_deserialize(H.table_pk96()[:96]))
    st, fb = c.upload_pubkeys_compressed(c.pubkeys_count, pk48)  # appends
    assert fb == 0xFFFFFFFF and c.committees_count == 2
    st, fb = c.upload_pubkeys_compressed(0, pk48)  # overwrites row 0
    assert fb == 0xFFFFFFFF and c.committees_count == 0
    # a committee may name the rows appended since
    upload(c, 0, [(c.pubkeys_count - 1, 0)])
    assert answers([[(0, np.ones(2, bool))]]) == want([(0, 0)], [[(0, np.ones(2, bool))]])


def test_store_grows_across_uploads(fresh):
    """Appends that outgrow the store's buffers keep what was stored: 40 uploads of 3 committees each."""
    c = fresh
    rng = np.random.default_rng(81)
    cms = []
    for k in range(40):
        new = [tuple(int(x) for x in rng.integers(0, H.N_INTEROP, int(rng.integers(1, 40)))) for _ in range(3)]
        upload(c, len(cms), new)
        cms += new
    assert c.committees_count == 120
    sets = [[(k, rng.random(len(cms[k])) < 0.9)] for k in range(120)]
    got, st, stat = c.aggregate_pubkeys_bits(*H.call_arrays(sets))
    assert got == [w for w, _ in H.oracle_sums(H.expand(cms, sets), 96)] and stat.segments_complemented > 0


def test_aggregate_then_verify_in_bytes_mode(ctx):
    """A few sets aggregated from bits and verified in bytes mode against signatures under the summed secret keys
    answer 1; with one participation bit flipped the key is another one and they answer 0."""
    rng = np.random.default_rng(82)
    cms = committees()
    sets = [[(11, rng.random(512) < 0.95)], [(10, rng.random(65) < 0.9), (6, rng.random(32) < 0.3)],
            [(4, np.ones(9, bool))], [(9, rng.random(64) < 0.5)]]
    lists = H.expand(cms, sets)
    sks = b"".join((sum(H.SKS[i] for i in x) % H.R_ORDER).to_bytes(32, "big") for x in lists)
    msgs = b"".join(bytes([0x40 + k]) * 32 for k in range(len(sets)))
    sigs = cpu.sign(sks, msgs)
    n = len(sets)

    def verify(the_sets):
        keys, st, _ = ctx.aggregate_pubkeys_bits(*H.call_arrays(the_sets), out_len=96)
        assert not st.any()
        res, _ = ctx.verify_raw(np.arange(n + 1), sigs, [96] * n, msgs, pk_bytes=b"".join(keys),
                                job_flags=np.ones(n), sig_stride=96)
        return list(res)

    assert verify(sets) == [1] * n
    flipped = [[(c, b.copy()) for c, b in s] for s in sets]
    for s in flipped:
        s[0][1][3] ^= True
    assert verify(flipped) == [0] * n


def test_api_functions(fresh):
    from lodestar_amd import api

    c = fresh
    cms = list(H.size_committees())
    api.upload_committees(c, 0, cms[:5])
    api.upload_committees(c, 5, cms[5:])
    assert c.committees_count == N_SIZE
    rng = np.random.default_rng(83)
    sets = [[(11, rng.random(512) < 0.95)], [(2, np.zeros(7, bool))], [(3, [1, 0, 1, 1, 1, 1, 1, 1]), (0, [True])], []]
    norm = [[(k, np.asarray(b, bool)) for k, b in s] for s in sets]
    want = [None if st else w for w, st in H.oracle_sums(H.expand(cms, norm), 96)]
    assert api.aggregate_pubkeys_from_bits(c, sets) == want
    assert api.aggregate_pubkeys_from_bits(c, sets, no_complement=True) == want
    want48 = [None if st else w for w, st in H.oracle_sums(H.expand(cms, norm), 48)]
    assert api.aggregate_pubkeys_from_bits(c, sets, compressed=True) == want48
    assert api.aggregate_pubkeys_from_bits(c, []) == []
    with pytest.raises(ValueError):
        api.upload_committees(c, 0, [[0, 1], []])
    with pytest.raises(ValueError):
        api.aggregate_pubkeys_from_bits(c, [[(2, np.ones(9, bool))]])  # nine bits for a committee of seven
