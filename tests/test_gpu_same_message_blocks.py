"""blsgpu_verify_same_message with BLSGPU_SAME_BLOCK_CHECK (one pairing check per block of 1024 groups, the per-group
descent of a block that fails, then the per-set retry; csrc/k_same.hip) against the oracle.

Expected values come from the oracle alone, exactly as in tests/test_gpu_same_message_fused.py, whose world (129 interop
keys over three messages), scenarios and helpers this file reuses: set_result is compared, code for code, with
oracle.cpu.verify_jobs of the same sets as one-set non-batchable jobs, group_result with its group rule.  The flag must
never change an answer, so the flagged call is also compared element-wise with the flag-0 call; stats.form says which
phases ran and in which kernel forms: 1 group-phase Miller values in the lane form, 2 retry phase in the lane forms,
4 block phase ran, 8 descent ran, 16 descent in the lane forms."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import cpu
from tests.test_gpu_same_message_fused import (EMPTY, K, SEED, THREADS, Scenario, Set, arrays, check,  # noqa: F401
                                               corrupted_sig, ctx, group_rule, known, mixed, no_key_corruption,
                                               oracle, run, sk32, world)

pytestmark = pytest.mark.gpu

BLOCK = 4  # native.SAME_BLOCK_CHECK
LANE = 1  # native.SAME_LANE_FORMS


def same_answers(a, b):
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all()
    for f in ("groups_accepted", "groups_retried", "retry_sets", "unique_messages"):
        assert getattr(a[2], f) == getattr(b[2], f), f


def test_flag_value():
    from lodestar_amd import native

    assert native.SAME_BLOCK_CHECK == BLOCK and native.SAME_LANE_FORMS == LANE


# ---------------------------------------------------------------------------------------------- 1 all valid
@pytest.mark.parametrize("table", [False, True])
def test_all_valid_known_shapes(ctx, world, known, table):
    assert all(r == 1 for r in known.want)
    res, gres, st = run(ctx, world, known.groups, known.msgs, table=table, flags=BLOCK)
    check((res, gres, st), known, lane_forms=4)
    assert (res == 1).all() and list(gres) == [1, 1, 1, EMPTY, 1, 1, 1, 1]
    assert st.retry_sets == 0 and st.unique_messages == 3 and st.form == 4


# ---------------------------------------------------------------------------- 2 error classes and soundness
@pytest.mark.parametrize("flags,form", [(BLOCK, 12), (BLOCK | LANE, 31)])
def test_error_classes_and_soundness(ctx, world, mixed, flags, form):
    want_g = group_rule(mixed.groups, mixed.want)
    assert want_g[:8] == [1] * 8 and want_g.count(0) >= 6
    plain = run(ctx, world, mixed.groups, mixed.msgs)
    got = run(ctx, world, mixed.groups, mixed.msgs, flags=flags)
    check(got, mixed, lane_forms=form)
    same_answers(got, plain)
    sub = no_key_corruption(mixed)
    got = run(ctx, world, sub.groups, sub.msgs, table=True, flags=flags)
    check(got, sub, lane_forms=form)
    same_answers(got, run(ctx, world, sub.groups, sub.msgs, table=True))


# ------------------------------------------------------------------------------- 3 forgeries across groups
def test_forgeries_across_groups(ctx, world):
    """What one check per block could be fooled by if the groups' sums were added without their scalars: (a) sig + D in
    group A and sig - D in group B, (b) a set of C and a set of D carrying each other's valid signatures -- in both the
    plain sum over the two groups verifies and neither group does.  Every set has its own scalar, so the block fails,
    the descent fails the four groups and the retry finds the four sets."""
    from lodestar_amd import native

    mi = 1
    groups = [[world.valid(10 * g + j, mi) for j in range(5)] for g in range(10)]
    msgs = [mi] * 10
    A, B, C, D = 3, 4, 5, 6
    ka, kb, kd = groups[A][1].key, groups[B][3].key, 120
    pa, pb, d = (bls.signature_from_bytes(world.sig96[mi][k], validate=False) for k in (ka, kb, kd))
    groups[A][1] = Set(ka, bls.g2_compress(bls.g2_add(pa, d)))
    groups[B][3] = Set(kb, bls.g2_compress(bls.g2_add(pb, bls.g2_neg(d))))
    sc, sd = groups[C][0], groups[D][4]
    groups[C][0], groups[D][4] = Set(sc.key, sd.sig), Set(sd.key, sc.sig)
    touched = {5 * A + 1, 5 * B + 3, 5 * C + 0, 5 * D + 4}
    sc = Scenario(groups, msgs, oracle(world, groups, msgs), {})
    assert sc.want == [0 if k in touched else 1 for k in range(50)]
    words = native.randomness_words(50, SEED)
    assert int(words[5 * A + 1]) != int(words[5 * B + 3]) and int(words[5 * C]) != int(words[5 * D + 4])
    got = run(ctx, world, groups, msgs, flags=BLOCK)
    check(got, sc, lane_forms=12)
    assert [int(x) for x in got[1]] == [0 if g in (A, B, C, D) else 1 for g in range(10)]
    assert [k for k in range(50) if got[0][k] != 1] == sorted(touched)
    same_answers(got, run(ctx, world, groups, msgs))


# ------------------------------------------------------------------------------------------ 4 several blocks
N_MANY = 2050  # blocks of 1024, 1024 and 2 groups: a full, a second full and a partial block


def many(world, bad=()):
    """2,050 one-set groups, key g % 129, messages alternating over two roots; group g in `bad` carries the next key's
    signature."""
    groups = [[Set(g % K, world.sig96[g % 2][(g + 1) % K if g in bad else g % K])] for g in range(N_MANY)]
    msgs = [g % 2 for g in range(N_MANY)]
    return Scenario(groups, msgs, oracle(world, groups, msgs), {})


@pytest.mark.parametrize("bad,form", [((), 5), ((1500,), 29), ((2049,), 13), ((3, 2049), 29)])
def test_several_blocks(ctx, world, bad, form):
    """form: 1 (2,050 Miller values in the lane form) + 4; a failed full block descends over 1,024 groups in the lane
    forms (8 + 16), the failed two-group block cooperatively (8); the retry of one or two sets stays cooperative."""
    sc = many(world, bad)
    assert sc.want == [0 if g in bad else 1 for g in range(N_MANY)]
    got = run(ctx, world, sc.groups, sc.msgs, table=True, flags=BLOCK)
    check(got, sc, lane_forms=form)
    assert [g for g in range(N_MANY) if got[0][g] != 1] == list(bad)
    assert got[2].groups_retried == len(bad) and got[2].retry_sets == len(bad)
    assert got[2].groups_accepted == N_MANY - len(bad)


# ---------------------------------------------------------------------------------------- 5 degenerate blocks
def test_degenerate_blocks(ctx, world):
    res, gres, st = run(ctx, world, [[], [], []], [0, 1, 2], flags=BLOCK)
    assert len(res) == 0 and list(gres) == [EMPTY] * 3
    assert st.groups_accepted == 0 and st.groups_retried == 0 and st.retry_sets == 0
    # every group holds a malformed signature: the aggregation rejects all, no block has an included group
    groups = []
    for g in range(5):
        grp = [world.valid(20 * g + j, g % 3) for j in range(4)]
        i = grp[g % 4].key
        grp[g % 4] = Set(i, corrupted_sig(world, "not_on_curve", i, (i + 1) % K, g % 3))
        groups.append(grp)
    sc = Scenario(groups, [g % 3 for g in range(5)], None, {})
    sc = sc._replace(want=oracle(world, sc.groups, sc.msgs))
    assert group_rule(sc.groups, sc.want) == [0] * 5 and sum(1 for r in sc.want if r < 0) == 5
    got = run(ctx, world, sc.groups, sc.msgs, flags=BLOCK)
    check(got, sc, lane_forms=4)
    assert got[2].groups_retried == 5 and got[2].retry_sets == 20
    # one group that fails: its block's verdict is its own, no descent; the set answers come from the retry
    one = [world.valid(7, 2), Set(8, world.sig96[1][8]), world.valid(9, 2)]
    sc = Scenario([one], [2], oracle(world, [one], [2]), {})
    assert sc.want == [1, 0, 1]
    check(run(ctx, world, sc.groups, sc.msgs, flags=BLOCK), sc, lane_forms=4)
    # one group that passes
    ok = [world.valid(7, 2), world.valid(8, 2)]
    sc = Scenario([ok], [2], oracle(world, [ok], [2]), {})
    assert sc.want == [1, 1]
    check(run(ctx, world, sc.groups, sc.msgs, flags=BLOCK), sc, lane_forms=4)


# --------------------------------------------------------------------------- 6 buffer growth between calls
def test_buffers_grow_between_calls(world, known):
    from lodestar_amd.native import Context

    n = 1025
    groups = [[Set(g % K, world.sig96[g % 2][(g + 1) % K if g == 600 else g % K])] for g in range(n)]
    big = Scenario(groups, [g % 2 for g in range(n)], None, {})
    big = big._replace(want=oracle(world, big.groups, big.msgs))
    assert big.want == [0 if g == 600 else 1 for g in range(n)]
    one = Scenario([[world.valid(5, 1)]], [1], [1], {})
    assert oracle(world, one.groups, one.msgs) == [1]
    c = Context([0])
    try:
        c.upload_pubkeys(0, b"".join(world.pk96))
        for flags in (BLOCK, 0, BLOCK):
            check(run(c, world, one.groups, one.msgs, flags=flags), one)
            check(run(c, world, known.groups, known.msgs, flags=flags ^ BLOCK), known)
            check(run(c, world, known.groups, known.msgs, flags=flags), known)
            check(run(c, world, big.groups, big.msgs, table=True, flags=flags), big, lane_forms=29 if flags else 1)
            check(run(c, world, one.groups, one.msgs, flags=flags ^ BLOCK), one)
    finally:
        c.close()


# ------------------------------------------------------------------------------ 7 beside a verification call
def test_beside_the_verifier(ctx, world, mixed):
    n = 2048
    sks = b"".join(sk32(world.sks[i % 64]) for i in range(n))
    msgs = b"".join(hashlib.sha256(b"beside-blocks" + i.to_bytes(4, "little")).digest() for i in range(n))
    sigs = cpu.sign(sks, msgs, threads=THREADS)
    pks = b"".join(world.pk96[i % 64] for i in range(n))
    box = {}

    def verify():
        box["res"] = ctx.verify_raw(np.arange(n + 1), sigs, [96] * n, msgs, pk_bytes=pks, job_flags=np.ones(n),
                                    sig_stride=96)[0]

    t = threading.Thread(target=verify)
    t.start()
    got = run(ctx, world, mixed.groups, mixed.msgs, flags=BLOCK)
    t.join(120)
    check(got, mixed, lane_forms=12)
    assert (box["res"] == 1).all()


# ------------------------------------------------------------------------------------ 8 seed 0 and entropy
def test_seed_zero_and_entropy_failure(ctx, world, mixed):
    from lodestar_amd import native

    sub = Scenario(mixed.groups[6:12], mixed.msgs[6:12], None, {})
    sub = sub._replace(want=oracle(world, sub.groups, sub.msgs))
    assert 0 in group_rule(sub.groups, sub.want) and 1 in group_rule(sub.groups, sub.want)
    for _ in range(2):
        check(run(ctx, world, sub.groups, sub.msgs, seed=0, flags=BLOCK), sub)
    a = arrays(world, sub.groups, sub.msgs)
    n, ng = int(a["group_first"][-1]), len(sub.groups)
    gf = np.asarray(a["group_first"], np.uint32)
    m = np.frombuffer(a["msgs"], np.uint8).copy()
    buf = np.frombuffer(a["sigs"], np.uint8).copy()
    pkb = np.frombuffer(a["pk_bytes"], np.uint8).copy()
    sl = np.asarray(a["sig_len"], np.uint32)
    res, gres = np.full(n, 0x55, np.int8), np.full(ng, 0x55, np.int8)
    st = native.SameMessageStats()
    st.retry_sets = 0xABAB
    st.form = 0xCDCD

    def call():
        return native.load().blsgpu_verify_same_message(
            ctx.h, ng, gf.ctypes.data, m.ctypes.data, pkb.ctypes.data, None, buf.ctypes.data, a["sig_stride"],
            sl.ctypes.data, 0, BLOCK, res.ctypes.data, gres.ctypes.data, ctypes.byref(st))

    native.debug_inject(native.INJECT_ENTROPY, 0, 1)
    try:
        assert call() == native.ERR_ENTROPY
    finally:
        native.debug_inject(native.INJECT_ENTROPY, 0, 0)
    assert (res == 0x55).all() and (gres == 0x55).all() and st.retry_sets == 0xABAB and st.form == 0xCDCD
    assert call() == native.OK
    check((res, gres, st), sub)
    assert st.form & 4


# ------------------------------------------------------------------------------------------- 9 Python API
def test_python_api(ctx, world):
    from lodestar_amd import api

    keys = list(range(60, 72))
    good = [world.sig96[0][k] for k in keys]
    cases = {
        "all valid": good,
        "wrong message": good[:4] + [world.sig96[1][keys[4]]] + good[5:],
        "malformed": good[:7] + [corrupted_sig(world, "not_on_curve", keys[7], keys[8], 0)] + good[8:],
        "short": good[:2] + [good[2][:48]] + good[3:],
    }
    groups = [[(world.pk96[k], s) for k, s in zip(keys, sigs)] for sigs in cases.values()]
    messages = [world.m[0]] * len(groups)
    got = api.verify_same_message_groups(ctx, groups, messages, block_check=True)
    assert got == api.verify_same_message_groups(ctx, groups, messages)
    for name, g, r in zip(cases, groups, got):
        assert r == api.verify_signature_sets_same_message(ctx, g, world.m[0]), name
        assert sum(r) == (len(keys) if name == "all valid" else len(keys) - 1), name
    table = [list(zip(keys, sigs)) for sigs in cases.values()]
    assert api.verify_same_message_groups(ctx, table, messages, block_check=True) == got
    assert api.verify_same_message_groups(ctx, [], [], block_check=True) == []
    assert api.verify_same_message_groups(ctx, [[], groups[0]], [world.m[1], world.m[0]], block_check=True) == [[], got[0]]
