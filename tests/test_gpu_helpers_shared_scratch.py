"""Every synchronous helper call in ONE context, one after another (csrc/helpers.cpp).

The helper calls share device 0's helper buffers (Device::helper), and each of their own suites exercises one call per
context.  Here one context runs aggregate_signatures, verify_same_message (with a retried group), aggregate_with_
randomness on the same sets and seed, key_validate, aggregate_pubkeys and signing_roots in a row, twice; the second
round is larger, so every shared buffer grows once between two calls that use it differently.  Every answer is checked
against the CPU oracle with the helpers of the calls' own suites, and the one-call same-message answers against the
two-step method's.  All inputs are valid encodings; the only invalid item is a well-formed signature over another
message."""
import numpy as np
import pytest

import tests.test_gpu_same_message as awr
import tests.test_gpu_same_message_fused as fused
import tests.test_gpu_sig_aggregate as agg
from oracle import bls12_381 as bls
from oracle import cpu, ssz_min

pytestmark = pytest.mark.gpu

THREADS = 16
K = 8
SEED = 0x5348415245445343
# (group sizes, message of each group, (group, position) of the set signed over the other message)
ROUNDS = [([2, 1, 2], [0, 1, 0], (0, 1)), ([3, 1, 2, 2], [0, 1, 0, 1], (2, 0))]
AGG_SIZES = [[1, 2], [3, 1, 2, 2]]  # aggregate_signatures: G = 2, n = 3, then G = 4, n = 8


class World:
    def __init__(self):
        self.sks = [bls.interop_secret_key(i) for i in range(K)]
        skb = b"".join(fused.sk32(s) for s in self.sks)
        self.m = [fused.msg(0), fused.msg(1)]
        pk = cpu.sk_to_pk(skb, threads=THREADS)
        self.pk96 = [pk[96 * i: 96 * i + 96] for i in range(K)]
        self.pk48 = [bls.g1_compress(bls.g1_deserialize(p)) for p in self.pk96]
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


def one_round(ctx, world, points, r):
    from lodestar_amd import api
    from lodestar_amd.native import ROOT_OBJECT

    sizes, msgs, wrong = ROUNDS[r]
    # the sets: key k signs its group's message, but for the one set signed over the other message
    signed, k = [], 0
    for g, size in enumerate(sizes):
        signed.append([(k + j, 1 - msgs[g] if (g, j) == wrong else msgs[g]) for j in range(size)])
        k += size
    n = k

    # 1 aggregate_signatures
    flat = [world.sig96[0][i] for i in range(sum(AGG_SIZES[r]))]
    for s in flat:
        points.put_valid(s)
    groups = [flat[sum(AGG_SIZES[r][:g]): sum(AGG_SIZES[r][:g + 1])] for g in range(len(AGG_SIZES[r]))]
    out, st, fb = agg.run(ctx, groups)
    agg.check_seg((groups, [bls.g2_compress(points.fold(g)) for g in groups]), out, st, fb)

    # 2 verify_same_message: the group of the wrong-message set goes through the retry phase
    fgroups = [[fused.Set(i, world.sig96[mi][i]) for i, mi in g] for g in signed]
    sc = fused.Scenario(fgroups, msgs, fused.oracle(world, fgroups, msgs), {})
    assert sc.want.count(1) == n - 1 and sc.want.count(0) == 1
    got = fused.run(ctx, world, fgroups, msgs, table=bool(r), seed=SEED)
    fused.check(got, sc, lane_forms=0)
    assert got[2].groups_retried == 1 and got[2].retry_sets == sizes[wrong[0]]

    # 3 aggregate_with_randomness, same sets and seed
    agroups = [[awr.Set(i, world.sig96[mi][i], [(world.sks[i], world.m[mi])]) for i, mi in g] for g in signed]
    res, _ = awr.run(ctx, world, agroups, table=bool(r), seed=SEED)
    awr.check(res, awr.expected(world, agroups, seed=SEED))

    # ... and the two-step method (that aggregation, one verification, set by set when it fails) answers as the one call
    for g, mi, first in zip(signed, msgs, np.cumsum([0] + sizes)):
        sets = [(world.pk96[i], world.sig96[smi][i]) for i, smi in g]
        two_step = api.verify_signature_sets_same_message(ctx, sets, world.m[mi], seed=SEED)
        assert two_step == [int(x) == 1 for x in got[0][first: first + len(g)]]

    # 4 key_validate
    nk = 4 * (r + 1)
    pk96, st = ctx.key_validate(b"".join(world.pk48[:nk]), 48)
    assert list(st) == [cpu.key_validate(p) for p in world.pk48[:nk]] == [0] * nk
    assert pk96 == b"".join(world.pk96[:nk])

    # 5 aggregate_pubkeys: sets of 1-2 keys, as bytes and as table indices
    spf = np.cumsum([0] + [1, 2, 1, 2, 2][: 3 + 2 * r])
    idx = [(3 * i) % K for i in range(spf[-1])]
    kb = b"".join(world.pk96[i] for i in idx)
    for out_len in (96, 48):
        want, wst = cpu.aggregate_pubkeys(out_len=out_len, job_first_set=[0, len(spf) - 1],
                                          sigs=bytes(96 * (len(spf) - 1)), sig_len=[96] * (len(spf) - 1),
                                          msgs=bytes(32 * (len(spf) - 1)), pk_bytes=kb, set_pk_first=spf)
        for keys in (dict(pk_bytes=kb), dict(pk_index=idx)):
            out, st = ctx.aggregate_pubkeys(set_pk_first=spf, out_len=out_len, **keys)
            assert list(st) == list(wst) == [0] * (len(spf) - 1) and out == want

    # 6 signing_roots
    domain = ssz_min.compute_domain(ssz_min.DOMAIN_DEPOSIT, bytes.fromhex("00000001"))
    objs = [fused.msg(100 + 10 * r + i) for i in range(2 * (r + 1))]
    assert ctx.signing_roots(ROOT_OBJECT, b"".join(objs), domain) == \
        [ssz_min.compute_signing_root(o, domain) for o in objs]


def test_helpers_share_one_contexts_buffers(ctx, world):
    points = agg.Points()
    for r in range(len(ROUNDS)):
        one_round(ctx, world, points, r)
