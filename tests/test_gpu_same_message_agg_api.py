"""lodestar_amd.api.verify_and_aggregate_same_message(_groups) on the GPU against the oracle: per-set booleans from
oracle.cpu.verify_jobs (one-set non-batchable jobs), aggregates from bls.g2_add over the signatures the oracle
verified, exact bytes.  Scenario 1 is the known groups of tests/test_gpu_same_message_agg.py (1, 2, 3, 0, 63, 64, 65,
129 sets over three messages); the bad-set scenario has a set signing another message, a malformed signature, a short
one, and a group in which nothing verifies."""
import hashlib

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import cpu

pytestmark = pytest.mark.gpu

THREADS = 16
K = 129
SIZES = [1, 2, 3, 0, 63, 64, 65, 129]
MSGS = [0, 1, 0, 2, 1, 0, 1, 0]


class World:
    def __init__(self):
        skb = b"".join(bls.interop_secret_key(i).to_bytes(32, "big") for i in range(K))
        self.m = [hashlib.sha256(b"same-message-fused" + j.to_bytes(4, "little")).digest() for j in range(3)]
        pk = cpu.sk_to_pk(skb, threads=THREADS)
        self.pk96 = [pk[96 * i: 96 * i + 96] for i in range(K)]
        self.sig96 = []
        for m in self.m:
            sg = cpu.sign(skb, m * K, threads=THREADS)
            self.sig96.append([sg[96 * i: 96 * i + 96] for i in range(K)])


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


def expected(world, groups, msgs, include=None):
    """[(bools, aggregate96 or None, count)] from the oracle; groups of (key index, signature bytes)."""
    flat = [(k, s, mi) for g, mi in zip(groups, msgs) for k, s in g]
    n = len(flat)
    stride = 192 if any(len(s) > 96 for _, s, _ in flat) else 96
    res, _ = cpu.verify_jobs(threads=THREADS, job_first_set=np.arange(n + 1),
                             sigs=b"".join(s[:stride].ljust(stride, b"\0") for _, s, _ in flat),
                             sig_len=[len(s) for _, s, _ in flat], msgs=b"".join(world.m[mi] for _, _, mi in flat),
                             pk_bytes=b"".join(world.pk96[k] for k, _, _ in flat), job_flags=np.zeros(n),
                             sig_stride=stride)
    out, at = [], 0
    for gi, g in enumerate(groups):
        acc, cnt = None, 0
        for j, (_, s) in enumerate(g):
            if int(res[at + j]) == 1 and (include is None or include[gi] is None or include[gi][j]):
                acc = bls.g2_add(acc, bls.signature_from_bytes(s, validate=False))
                cnt += 1
        out.append(([int(r) == 1 for r in res[at: at + len(g)]], bls.g2_compress(acc) if cnt else None, cnt))
        at += len(g)
    return out


@pytest.fixture(scope="module")
def known(world):
    groups, k = [], 0
    for n, mi in zip(SIZES, MSGS):
        groups.append([((7 * (k + j) + 3) % K, world.sig96[mi][(7 * (k + j) + 3) % K]) for j in range(n)])
        k += n
    return groups


@pytest.fixture(scope="module")
def bad(world):
    g0 = [(k, world.sig96[0][k]) for k in range(60, 72)]
    g0[4] = (64, world.sig96[1][64])  # another message
    g1 = [(k, world.sig96[1][k]) for k in range(20, 29)]
    g1[0] = (20, bytes([0x9F]) + bytes([0xFF]) * 95)  # x >= p
    g1[8] = (28, world.sig96[1][28][:48])  # short
    g2 = [(k, world.sig96[0][k]) for k in range(3)]  # signatures over m0 in a group that signs m2
    return [g0, g1, g2], [0, 1, 2]


def with_bytes(world, groups):
    return [[(world.pk96[k], s) for k, s in g] for g in groups]


@pytest.mark.parametrize("table", [False, True])
def test_groups_known(ctx, world, known, table):
    from lodestar_amd import api

    want = expected(world, known, MSGS)
    assert [c for _, _, c in want] == SIZES and want[3] == ([], None, 0)
    groups = known if table else with_bytes(world, known)
    got = api.verify_and_aggregate_same_message_groups(ctx, groups, [world.m[i] for i in MSGS])
    assert got == want
    m = [world.m[i] for i in MSGS]
    assert api.verify_and_aggregate_same_message_groups(ctx, groups, m, block_check=True) == want


def test_groups_bad_sets_and_include(ctx, world, bad):
    from lodestar_amd import api

    groups, msgs = bad
    want = expected(world, groups, msgs)
    assert [c for _, _, c in want] == [11, 7, 0] and want[2] == ([False] * 3, None, 0)
    m = [world.m[i] for i in msgs]
    assert api.verify_and_aggregate_same_message_groups(ctx, with_bytes(world, groups), m) == want
    assert api.verify_and_aggregate_same_message_groups(ctx, groups, m, seed=5) == want
    include = [[j % 2 == 0 for j in range(12)], None, [True, False, True]]
    want_inc = expected(world, groups, msgs, include)
    assert [c for _, _, c in want_inc] == [5, 7, 0]
    assert api.verify_and_aggregate_same_message_groups(ctx, groups, m, include=include) == want_inc
    assert api.verify_and_aggregate_same_message_groups(ctx, [], []) == []
    with pytest.raises(ValueError):
        api.verify_and_aggregate_same_message_groups(ctx, groups, m, include=[None, None])
    with pytest.raises(ValueError):
        api.verify_and_aggregate_same_message_groups(ctx, groups, m, include=[[True], None, None])


def test_single_group(ctx, world, known, bad):
    from lodestar_amd import api

    g = known[SIZES.index(65)]
    want = expected(world, [g], [1])[0]
    assert api.verify_and_aggregate_same_message(ctx, with_bytes(world, [g])[0], world.m[1]) == want[:2]
    assert api.verify_and_aggregate_same_message(ctx, g, world.m[1]) == want[:2]
    groups, msgs = bad
    for grp, mi in zip(groups, msgs):
        bools, agg = api.verify_and_aggregate_same_message(ctx, grp, world.m[mi])
        assert (bools, agg) == expected(world, [grp], [mi])[0][:2]
        assert bools == api.verify_signature_sets_same_message(ctx, grp, world.m[mi])
    # nothing verified: no aggregate
    assert api.verify_and_aggregate_same_message(ctx, groups[2], world.m[2]) == ([False] * 3, None)
    with pytest.raises(api.BlstError):
        api.verify_and_aggregate_same_message(ctx, [], world.m[0])
