"""Batched AggregateVerify on the GPU (blsgpu_aggregate_verify, csrc/k_aggverify.hip) against the oracle.

Expected values come from the oracle alone (tests/aggverify_helpers.py: keys through key_validate or g1_deserialize,
the signature through signature_from_bytes, then final_exp over the product of the pairs' Miller values and
miller_loop(-g1, sig)); every comparison is exact.  Each scenario runs with the keys as bytes and as table entries,
and in both kernel forms (the default -- cooperative at these sizes -- and AV_LANE_FORMS).
"""
import ctypes

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import corrupt
from tests.aggverify_helpers import INF96, INF192, INF_PK48, NONE, Job, K, M, call, expected_all, get_world

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 130]  # the empty job, the edges of the 8-item chunk and of the 64-lane product
MODES = [pytest.param(False, id="bytes"), pytest.param(True, id="table")]
FORMS = [pytest.param(False, id="default"), pytest.param(True, id="lane")]


@pytest.fixture(scope="module")
def world():
    return get_world()


@pytest.fixture(scope="module")
def ctx(world):
    from lodestar_amd.native import Context

    c = Context([0])
    c.upload_pubkeys(0, b"".join(world.pk96))
    yield c
    c.close()


def flags_of(lane, validate=False):
    from lodestar_amd import native

    return (native.AV_LANE_FORMS if lane else 0) | (native.AV_VALIDATE_KEYS if validate else 0)


def check(ctx, world, jobs, table, lane, validate=False, pk_len=96):
    res, fb, st = call(ctx, world, jobs, table, flags_of(lane, validate), pk_len)
    want, want_fb = expected_all(world, jobs, validate, pk_len)
    assert res == want
    assert fb == want_fb
    return res, st


def plan_counts(jobs, res, lane):
    """(items, chunks, checked jobs) the plan predicts: every job that reached the check (result 0 or 1 with a finite
    signature) is its pairs plus one signature item, cut into chunks of 1 (cooperative) or 8 (lane form) items."""
    k = 8 if lane else 1
    items = chunks = checked = 0
    for j, r in zip(jobs, res):
        if r in (0, 1) and j.pairs and j.sig not in (INF96, INF192):
            items += len(j.pairs) + 1
            chunks += -(-(len(j.pairs) + 1) // k)
            checked += 1
    return items, chunks, checked


# ---------------------------------------------------------------------------------------------------------- sizes
@pytest.fixture(scope="module")
def size_jobs(world):
    """One call with jobs of every size in SIZES, all valid but the empty one; pair q of the call is (key q % 16,
    message (q // 16 + q) % 16), so all 256 (key, message) combinations occur and messages repeat within jobs."""
    jobs, q = [], 0
    for n in SIZES:
        pairs = [((q + t) % K, ((q + t) // K + q + t) % M) for t in range(n)]
        q += n
        jobs.append(world.job(pairs) if pairs else Job([], INF96))
    return jobs


@pytest.mark.parametrize("lane", FORMS)
@pytest.mark.parametrize("table", MODES)
def test_sizes(ctx, world, size_jobs, table, lane):
    from lodestar_amd import native

    res, st = check(ctx, world, size_jobs, table, lane)
    assert res == [-9] + [1] * (len(SIZES) - 1)
    n_pairs = sum(SIZES)
    planned = n_pairs + len(SIZES) - 1  # the pairs of the non-empty jobs and a signature item each
    assert planned == 393 and planned <= 512
    items, chunks, checked = plan_counts(size_jobs, res, lane)
    assert items == planned and checked == len(SIZES) - 1
    assert chunks == (planned if not lane else sum(-(-(n + 1) // 8) for n in SIZES if n))
    assert (st.pairs, st.miller_items, st.miller_chunks, st.jobs_checked) == (n_pairs, items, chunks, checked)
    assert st.unique_messages == len({m for j in size_jobs for _, m in j.pairs}) == M
    assert st.form == (1 if lane else 0) == native.aggregate_verify_form(planned, flags_of(lane))


@pytest.mark.parametrize("table", MODES)
@pytest.mark.parametrize("shape", ["large_jobs", "small_jobs"])
def test_automatic_lane_form(ctx, world, shape, table):
    """Above 512 Miller items a call takes the lane forms on its own, with one item per accumulator while a lane per
    item fits the chip: jobs of many chunks (a wave multiplies a job's chunk values) and many jobs of few chunks (a lane
    does).  One job of each call is invalid, one is rejected, one is empty."""
    from lodestar_amd import native

    adv = corrupt.adversarial_sigs()
    if shape == "large_jobs":
        sizes = [200, 150, 170]
        jobs, q = [], 0
        for n in sizes:
            jobs.append(world.job([((q + t) % K, ((q + t) // K + q + t) % M) for t in range(n)]))
            q += n
        jobs += [Job(jobs[1].pairs, jobs[0].sig), Job([], INF96)]
    else:
        kinds = [world.job([(0, 0), (1, 1), (2, 2)]), world.job([(3, 3), (4, 3), (5, 6)]), world.job([(7, 7), (8, 9)])]
        jobs = [kinds[i % 3] for i in range(150)]
        jobs[40] = Job(kinds[0].pairs, kinds[1].sig)
        jobs[41] = Job(kinds[1].pairs, adv[bls.BLST_POINT_NOT_IN_GROUP])
        jobs[42] = Job([], INF96)
    planned = sum(len(j.pairs) + 1 for j in jobs if j.pairs)
    assert planned > 512 and native.aggregate_verify_form(planned) == 1
    res, fb, st = call(ctx, world, jobs, table, 0)
    want, want_fb = expected_all(world, jobs)
    assert (res, fb) == (want, want_fb)
    assert sorted(set(res)) == ([-9, 0, 1] if shape == "large_jobs" else [-9, -3, 0, 1])
    items, chunks, checked = plan_counts(jobs, res, lane=False)  # one item per chunk, as in the cooperative form
    assert st.form == 1
    assert (st.miller_items, st.miller_chunks, st.jobs_checked) == (items, chunks, checked) and items == chunks


# --------------------------------------------------------------------------------------- wrong answers that must be 0
@pytest.mark.parametrize("lane", FORMS)
@pytest.mark.parametrize("table", MODES)
def test_wrong_answers_are_zero(ctx, world, table, lane):
    a = [(0, 0), (1, 1), (2, 2)]
    b = [(3, 3), (4, 4), (5, 5)]
    d = world.sig_point(6, 6)
    plus = bls.g2_compress(bls.g2_add(world.sum_point(a), d))
    minus = bls.g2_compress(bls.g2_add(world.sum_point(b), bls.g2_neg(d)))
    jobs = [
        world.job(a),                                     # the valid job itself
        Job([(0, 0), (1, 7), (2, 2)], world.sign(a)),     # one message replaced
        Job([(0, 1), (1, 0), (2, 2)], world.sign(a)),     # two messages swapped between keys
        Job(a, world.sign(b)),                            # the signature of another job
        Job(a, world.sign(a[:2])),                        # summed over one pair too few
        Job(a, world.sign(a + [(3, 3)])),                 # and one too many
        Job(a, plus), Job(b, minus),                      # S_a + D and S_b - D: jobs are never batched together
        world.job(b),
    ]
    res, st = check(ctx, world, jobs, table, lane)
    assert res == [1, 0, 0, 0, 0, 0, 0, 0, 1]
    assert st.jobs_checked == len(jobs)


# ------------------------------------------------------------------------------------------------------ still valid
@pytest.mark.parametrize("lane", FORMS)
@pytest.mark.parametrize("table", MODES)
def test_still_valid(ctx, world, table, lane):
    a = [(0, 0), (1, 1), (2, 2), (3, 3)]
    jobs = [
        Job([a[2], a[0], a[3], a[1]], world.sign(a)),     # the pairs permuted
        world.job([(4, 5), (6, 5), (7, 8)]),              # a message repeated within a job: two keys sign it
        world.job([(8, 5), (9, 0)]),                      # the same messages across jobs
        world.job([(4, 5), (4, 5)]),                      # the same pair twice
    ]
    res, st = check(ctx, world, jobs, table, lane)
    assert res == [1, 1, 1, 1]
    assert st.unique_messages == len({m for j in jobs for _, m in j.pairs}) == 6


# ---------------------------------------------------------------------------------------------------- error classes
def signature_classes(world, pairs):
    """{kind: signature bytes} over every decode class of oracle.corrupt, from the job's valid signature."""
    s = world.sign(pairs)
    u = world.sign(pairs, wide=True)
    adv = corrupt.adversarial_sigs()
    bad192 = bytearray(u)
    bad192[191] ^= 1
    return {
        "negated": bytes([s[0] ^ 0x20]) + s[1:],
        "infinity": INF96,
        "infinity_192": INF192,
        "size_48": s[:48],
        "size_0": b"",
        "bad_flag_96": bytes([s[0] & 0x7F]) + s[1:],
        "x_ge_p": bytes([0x80 | 0x1F]) + bytes([0xFF]) * 95,
        "flag_on_192": bytes([u[0] | 0x80]) + u[1:],
        "not_on_curve": adv[bls.BLST_POINT_NOT_ON_CURVE],
        "not_on_curve_192": bytes(bad192),
        "not_in_group": adv[bls.BLST_POINT_NOT_IN_GROUP],
        "uncompressed_valid": u,
    }


@pytest.mark.parametrize("lane", FORMS)
@pytest.mark.parametrize("table", MODES)
def test_signature_classes(ctx, world, table, lane):
    pairs = [(0, 0), (1, 1), (2, 2)]
    classes = signature_classes(world, pairs)
    jobs = [Job(pairs, sig) for sig in classes.values()]
    res, _ = check(ctx, world, jobs, table, lane)
    got = dict(zip(classes, res))
    assert got == {"negated": 0, "infinity": 0, "infinity_192": 0, "size_48": -8, "size_0": -8, "bad_flag_96": -1,
                   "x_ge_p": -1, "flag_on_192": -1, "not_on_curve": -2, "not_on_curve_192": -2, "not_in_group": -3,
                   "uncompressed_valid": 1}


@pytest.mark.parametrize("lane", FORMS)
@pytest.mark.parametrize("table", MODES)
def test_rejected_job_between_valid_ones(ctx, world, table, lane):
    """Isolation: a rejected job, an identity signature and an empty job between valid ones change no other answer,
    and only the checked jobs are counted."""
    adv = corrupt.adversarial_sigs()
    a, b = [(0, 0), (1, 1)], [(2, 2), (3, 3), (4, 4)]
    jobs = [world.job(a), Job(b, adv[bls.BLST_POINT_NOT_IN_GROUP]), world.job(b), Job([], world.sign(a)), Job(a, INF96),
            world.job(a, wide=True)]
    res, st = check(ctx, world, jobs, table, lane)
    assert res == [1, -3, 1, -9, 0, 1]
    items, chunks, checked = plan_counts(jobs, res, lane)
    assert (st.miller_items, st.miller_chunks, st.jobs_checked) == (items, chunks, checked) and checked == 3


def off_curve_x():
    """The least x >= 1 with x^3 + 4 a non-residue: no curve point has it."""
    x = 1
    while pow((x * x * x + 4) % bls.P, (bls.P - 1) // 2, bls.P) == 1:
        x += 1
    return x


def point_outside_g1():
    """A curve point outside the subgroup: the first x >= 1 with a y (a random curve point lies in G1 with probability
    1 / cofactor), checked."""
    x = 1
    while True:
        rhs = (x * x * x + 4) % bls.P
        y = pow(rhs, (bls.P + 1) // 4, bls.P)
        if y * y % bls.P == rhs and bls.g1_mul((x, y), bls.R) is not None:
            return (x, y)
        x += 1


@pytest.mark.parametrize("lane", FORMS)
def test_trusted_key_errors(ctx, world, lane):
    """Bytes mode, trusted keys: BAD_ENCODING, POINT_NOT_ON_CURVE and PK_IS_INFINITY; the middle pair's key sets
    first_bad; a key error and a bad signature in one job give the key's code; a key outside G1 is not checked."""
    pairs = [(0, 0), (1, 1), (2, 2)]
    good = world.sign(pairs)
    x = off_curve_x()
    not_on_curve = x.to_bytes(48, "big") + (1).to_bytes(48, "big")
    bad_enc = bytes([0x80]) + world.pk96[1][1:]
    inf96 = bytes([0x40]) + bytes(95)
    outside = bls.g1_serialize(point_outside_g1())
    adv = corrupt.adversarial_sigs()
    jobs = [
        world.job(pairs),
        Job(pairs, good, {1: not_on_curve}),
        Job(pairs, good, {1: bad_enc}),
        Job(pairs, good, {2: inf96}),
        Job(pairs, adv[bls.BLST_POINT_NOT_IN_GROUP], {1: inf96}),    # a key error and a bad signature
        Job(pairs, good, {0: bad_enc, 2: not_on_curve}),            # the lowest-index key's code
        Job(pairs, good, {1: outside}),                              # trusted: no subgroup check, the check fails
        world.job(pairs),
    ]
    res, fb, st = call(ctx, world, jobs, False, flags_of(lane))
    want, want_fb = expected_all(world, jobs)
    assert (res, fb) == (want, want_fb)
    assert res == [1, -2, -1, -6, -6, -1, 0, 1]
    assert fb == [NONE, 4, 7, 11, 13, 15, NONE, NONE]
    assert st.jobs_checked == 3


@pytest.mark.parametrize("lane", FORMS)
@pytest.mark.parametrize("pk_len", [48, 96])
def test_validated_key_errors(ctx, world, pk_len, lane):
    """AV_VALIDATE_KEYS with 48- and 96-byte keys: a key outside the subgroup (-3), an identity key (-6), an off-curve
    x (-2), and valid keys of both lengths."""
    pairs = [(0, 0), (1, 1), (2, 2)]
    good = world.sign(pairs)
    x = off_curve_x()
    out_pt = point_outside_g1()
    if pk_len == 48:
        outside, inf, off = bls.g1_compress(out_pt), INF_PK48, bytes([0x80]) + x.to_bytes(48, "big")[1:]
    else:
        outside, inf = bls.g1_serialize(out_pt), bytes([0x40]) + bytes(95)
        off = x.to_bytes(48, "big") + (1).to_bytes(48, "big")
    jobs = [world.job(pairs), Job(pairs, good, {1: outside}), Job(pairs, good, {2: inf}), Job(pairs, good, {0: off}),
            Job(pairs, world.sign(pairs[:2])), world.job(pairs[::-1])]
    res, _ = check(ctx, world, jobs, False, lane, validate=True, pk_len=pk_len)
    assert res == [1, -3, -6, -2, 0, 1]


# ------------------------------------------------------------------------------------------------ argument refusals
def test_argument_refusals(ctx, world):
    """Every refusal of the contract returns ERR_ARGS with job_result untouched; n_jobs == 0 returns OK with zeroed
    stats."""
    from lodestar_amd import native

    lib = ctx._lib
    jobs = [world.job([(0, 0), (1, 1)]), world.job([(2, 2)])]
    n, J = 3, 2
    jf = np.array([0, 2, 3], np.uint32)
    msgs = np.frombuffer(b"".join(world.msgs[m] for j in jobs for _, m in j.pairs), np.uint8).copy()
    pkb = np.frombuffer(b"".join(world.pk96[i] for j in jobs for i, _ in j.pairs), np.uint8).copy()
    pk48 = np.frombuffer(b"".join(world.pk48[i] for j in jobs for i, _ in j.pairs), np.uint8).copy()
    pki = np.array([i for j in jobs for i, _ in j.pairs], np.uint32)
    sigs = np.frombuffer(b"".join(j.sig for j in jobs), np.uint8).copy()
    slen = np.array([96, 96], np.uint32)

    def run(**kw):
        a = dict(ctx=ctx.h, n_jobs=J, jf=jf, msgs=msgs, pkb=pkb, pk_len=96, pki=None, sigs=sigs, stride=96, slen=slen,
                 flags=0, res="own", fb=None, st=None)
        a.update(kw)
        res = np.full(J, 77, np.int8)
        ptr = lambda x: None if x is None else x.ctypes.data  # noqa: E731
        st = native.AggregateVerifyStats()
        st.pairs = 99
        rc = lib.blsgpu_aggregate_verify(a["ctx"], a["n_jobs"], ptr(a["jf"]), ptr(a["msgs"]), ptr(a["pkb"]), a["pk_len"],
                                         ptr(a["pki"]), ptr(a["sigs"]), a["stride"], ptr(a["slen"]), a["flags"],
                                         res.ctypes.data if a["res"] == "own" else None, None, ctypes.byref(st))
        return rc, res, st

    rc, res, st = run()
    assert rc == native.OK and list(res) == [1, 1] and st.pairs == 3
    refusals = {
        "null ctx": dict(ctx=None), "null job_first": dict(jf=None), "null msgs": dict(msgs=None),
        "null sigs": dict(sigs=None), "null sig_len": dict(slen=None), "null job_result": dict(res=None),
        "both key pointers": dict(pki=pki), "neither key pointer": dict(pkb=None),
        "pk_len 48 without the flag": dict(pkb=pk48, pk_len=48), "pk_len 95": dict(pk_len=95),
        "pk_len 0 with the flag": dict(pk_len=0, flags=native.AV_VALIDATE_KEYS),
        "the flag with pk_index": dict(pkb=None, pki=pki, flags=native.AV_VALIDATE_KEYS),
        "sig_stride < 96": dict(stride=95),
        "a 192-byte signature under a narrower stride": dict(slen=np.array([96, 192], np.uint32)),
        "an unknown flag": dict(flags=4),
        "job_first not from 0": dict(jf=np.array([1, 2, 3], np.uint32)),
        "job_first decreasing": dict(jf=np.array([0, 3, 2], np.uint32)),
        "job_first above 1 << 20 pairs": dict(jf=np.array([0, 2, (1 << 20) + 1], np.uint32)),
        "a table index beyond the table": dict(pkb=None, pki=np.array([0, 1, ctx.pubkeys_count], np.uint32)),
    }
    for name, kw in refusals.items():
        rc, res, st = run(**kw)
        assert rc == native.ERR_ARGS, name
        assert list(res) == [77, 77], name
        assert st.pairs == 99, name
    rc, res, st = run(n_jobs=0)
    assert rc == native.OK and list(res) == [77, 77]
    assert (st.pairs, st.unique_messages, st.miller_items, st.miller_chunks, st.form, st.jobs_checked) == (0,) * 6
    assert st.device_ms == 0
    # the table mode of the same call, and the wrapper's own layout checks
    rc, res, _ = run(pkb=None, pki=pki)
    assert rc == native.OK and list(res) == [1, 1]
    with pytest.raises(ValueError, match="exactly one of"):
        ctx.aggregate_verify([0, 1], bytes(32), bytes(96))
    with pytest.raises(ValueError, match="message bytes"):
        ctx.aggregate_verify([0, 2], bytes(32), bytes(96), pk_bytes=bytes(192))
