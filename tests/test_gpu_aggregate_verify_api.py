"""The Python entry points of AggregateVerify (lodestar_amd/api.py) on the GPU: api.aggregate_verify on the spec
runner's cases (beacon-node/test/spec/general/bls.ts `aggregate_verify`, restated from the handler's rule: untrusted
keys, any error -> False), api.verify against process_deposit_signature, and api.aggregate_verify_jobs over table
entries.  Expected values come from the oracle (tests/aggverify_helpers.py)."""
import pytest

from oracle import bls12_381 as bls
from tests.aggverify_helpers import INF96, INF_PK48, Job, expected_all, get_world

pytestmark = pytest.mark.gpu


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


def test_aggregate_verify_runner_cases(ctx, world):
    from lodestar_amd import api

    pairs = [(0, 0), (1, 1), (2, 2)]
    pks = [world.pk48[i] for i, _ in pairs]
    msgs = [world.msgs[j] for _, j in pairs]
    sig = world.sign(pairs)
    assert world.expected(Job(pairs, sig), 0, validate=True, pk_len=48)[0] == 1
    assert api.aggregate_verify(ctx, pks, msgs, sig) is True
    # tampered signature: the last four bytes replaced, as the runner's case does
    tampered = sig[:-4] + b"\xff\xff\xff\xff"
    assert world.expected(Job(pairs, tampered), 0, validate=True, pk_len=48)[0] != 1
    assert api.aggregate_verify(ctx, pks, msgs, tampered) is False
    # a well-formed signature over other pairs
    assert api.aggregate_verify(ctx, pks, msgs, world.sign(pairs[:2])) is False
    # an infinity pubkey among the keys: KeyValidate rejects it
    assert api.aggregate_verify(ctx, pks + [INF_PK48], msgs + [world.msgs[3]], sig) is False
    # no pubkeys, with an infinity signature and with a zero signature
    assert api.aggregate_verify(ctx, [], [], INF96) is False
    assert api.aggregate_verify(ctx, [], [], bytes(96)) is False
    # mismatched lengths
    assert api.aggregate_verify(ctx, pks, msgs[:2], sig) is False
    assert api.aggregate_verify(ctx, pks[:2], msgs, sig) is False
    # a malformed key length is an error of the handler -> False
    assert api.aggregate_verify(ctx, [pks[0][:47]] + pks[1:], msgs, sig) is False


def test_verify_is_the_runners_verify(ctx, world):
    from lodestar_amd import api

    sig = world.sign([(3, 4)])
    cases = [(world.pk48[3], world.msgs[4], sig), (world.pk48[3], world.msgs[5], sig), (world.pk48[2], world.msgs[4], sig),
             (INF_PK48, world.msgs[4], sig), (world.pk48[3], world.msgs[4], INF96), (world.pk48[3], world.msgs[4], sig[:95])]
    got = [api.verify(ctx, *c) for c in cases]
    assert got == [api.process_deposit_signature(ctx, *c) for c in cases]
    assert got == [True, False, False, False, False, False]
    # the one-pair AggregateVerify answers the same
    assert [api.aggregate_verify(ctx, [pk], [m], s) for pk, m, s in cases] == got


def test_aggregate_verify_jobs_table_mode(ctx, world):
    from lodestar_amd import api

    a, b = [(0, 0), (1, 1), (2, 2)], [(5, 9), (6, 9)]
    jobs = [world.job(a), Job(b, world.sign(a)), world.job(b, wide=True), Job([], INF96), Job(a, INF96)]
    want, _ = expected_all(world, jobs)
    assert want == [1, 0, 1, -9, 0]
    as_api = lambda keys: [(keys(j), [world.msgs[m] for _, m in j.pairs], j.sig) for j in jobs]  # noqa: E731
    assert api.aggregate_verify_jobs(ctx, as_api(lambda j: [i for i, _ in j.pairs])) == want
    assert api.aggregate_verify_jobs(ctx, as_api(lambda j: [world.pk96[i] for i, _ in j.pairs]), lane_forms=True) == want
    assert api.aggregate_verify_jobs(ctx, as_api(lambda j: [world.pk48[i] for i, _ in j.pairs]), validate_keys=True) == want
    assert api.aggregate_verify_jobs(ctx, []) == []
    with pytest.raises(ValueError, match="mix"):
        api.aggregate_verify_jobs(ctx, [([0, world.pk96[1]], [world.msgs[0]] * 2, INF96)])
    with pytest.raises(ValueError, match="48-byte"):
        api.aggregate_verify_jobs(ctx, [([world.pk48[0]], [world.msgs[0]], INF96)])
