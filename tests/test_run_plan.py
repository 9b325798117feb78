"""The host plan of one pipeline run (lodestar_amd/csrc/run_plan.hpp), CPU only.

pipeline.cpp's run_shard takes its batch groups, message index, same-message units, forms, Miller chunks, MSM slices,
F product tree, arena offsets, verdict sorting, fallback lists and pool groups from that header.
tests/native/run_plan_probe.cpp exposes them; here they are checked for what they mean (partitions, covers, a
simulated product tree) and against the chained expressions run_shard held before the plan had names, restated in
Python."""
import os
import subprocess

import numpy as np
import pytest

from tests import run_plan_probe as rp
from tests.test_pool_policy import reference_rule

W_FP = 14
W_G1A, W_G1J, W_G2A, W_G2J, W_FP12 = 2 * W_FP, 3 * W_FP, 4 * W_FP, 6 * W_FP, 12 * W_FP
MSM_SLICE, MSM_BUCKET_WORDS, MSM_WINDOW_WORDS = 256, 128 * W_G2J, 16 * W_G2J
MILLER_LINE_WORDS = 68 * 3 * 2 * W_FP

COUNTS = [2, 0, 1, 3, 1, 2, 1]  # seven jobs, ten sets
FLAGS = [1, 1, 0, 1, 1, 1, 1]
# repeats inside a group and across groups (group_sets 4: groups {0}, {2}, {3, 4}, {5, 6})
MSGS = [5, 5, 6, 7, 5, 7, 7, 5, 8, 8]


def al256(x):
    return (x + 255) & ~255


def job_sets(counts):
    first = np.concatenate([[0], np.cumsum(counts)]).tolist()
    return [(first[j], first[j + 1]) for j in range(len(counts))]


def pairs(v):
    return [(v[2 * i], v[2 * i + 1]) for i in range(len(v) // 2)]


def test_header_is_hip_free():
    src = open(rp.HDR).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == sorted(["<stddef.h>", "<stdint.h>", "<string.h>", "<algorithm>", "<cmath>", "<utility>",
                                       "<vector>", '"../../include/blsgpu.h"', '"helper_layout.hpp"',
                                       '"miller_plan.hpp"', '"options.hpp"'])
    # and the four project headers it includes bring in none
    for dep in (os.path.join(rp.CSRC, "helper_layout.hpp"), os.path.join(rp.CSRC, "miller_plan.hpp"),
                os.path.join(rp.CSRC, "options.hpp"), os.path.join(os.path.dirname(rp.HERE), "include", "blsgpu.h")):
        assert all("hip" not in ln and '"' not in ln for ln in open(dep).read().splitlines() if ln.startswith("#include"))


# ---- groups ------------------------------------------------------------------------------------------------------
def groups_rule(counts, flags, gs):
    """run_shard's packing restated: contiguous job ranges; an empty job closes the open group and joins none, a
    non-batchable job is alone, a batchable group closes once it holds >= gs sets."""
    out, cur, is_open = [], 0, False
    for j, c in enumerate(counts):
        if c == 0:
            is_open = False
            continue
        if not flags[j] & 1:
            out.append([j, j + 1])
            is_open = False
            continue
        if not is_open or cur >= gs:
            out.append([j, j])
            cur, is_open = 0, True
        out[-1][1] = j + 1
        cur += c
    return [tuple(g) for g in out]


@pytest.mark.parametrize("gs", [1, 4, 1024])
def test_groups(gs):
    p = rp.plan(COUNTS, FLAGS, MSGS, opts=rp.Opts(group_sets=gs, group_adapt=0))
    groups = pairs(p.vec("group_jobs"))
    assert groups == groups_rule(COUNTS, FLAGS, gs) and p["ng0"] == len(groups)
    member = [j for a, e in groups for j in range(a, e)]
    nonempty = [j for j, c in enumerate(COUNTS) if c]
    assert [j for j in member if COUNTS[j]] == nonempty  # each non-empty job once, in order
    for a, e in groups:
        assert COUNTS[a] and COUNTS[e - 1]  # a group begins and ends on a non-empty job
        assert all(COUNTS[j] == 0 or FLAGS[j] & 1 for j in range(a, e)) or e - a == 1
    assert (2, 3) in groups  # the non-batchable job is alone
    for g, (a, e) in enumerate(groups):
        if (a, e) == (2, 3):
            continue
        # a batchable group closes only once it has >= gs sets: if the next job continues the batchable stretch (no
        # empty or non-batchable job between), this group reached gs; and it was below gs before its last job
        nxt = groups[g + 1][0] if g + 1 < len(groups) else None
        if nxt == e and FLAGS[nxt] & 1:
            assert sum(COUNTS[a:e]) >= gs
        assert sum(COUNTS[a:e - 1]) < gs or e - a == 1
    if gs == 1:
        assert groups == [(j, j + 1) for j in nonempty]
    if gs == 1024:
        assert groups == [(0, 1), (2, 3), (3, 7)]  # the empty job and the non-batchable one cut the stretch


def test_groups_from_a_pool_policy_list():
    pool = [(0, 1, 1), (1, 2, 1), (2, 3, 0), (3, 7, 1)]  # (1, 2): only an empty job -> dropped
    p = rp.plan(COUNTS, FLAGS, MSGS, pool=pool)
    assert pairs(p.vec("group_jobs")) == [(0, 1), (2, 3), (3, 7)] and p.vec("group_batchable") == [1, 0, 1]


def test_group_adapt_rule():
    """adapt_group_sets: group_sets while no set was invalid, the model's 32 at the pool's 1% invalid gossip."""
    L = rp.lib()
    import ctypes
    f = lambda rate, gs, spj: L.rp_adapt_group_sets(ctypes.c_double(rate), ctypes.c_int64(gs), ctypes.c_double(spj))
    assert f(0.0, 1024, 2.0) == 1024 and f(0.01, 8, 2.0) == 8 and f(0.01, 1024, 2.0) == 32
    p = rp.plan([1] * 200, [1] * 200, range(200), opts=rp.Opts(group_adapt=1), fail_rate=0.01)
    assert all(e - a == f(0.01, 1024, 1.0) for a, e in pairs(p.vec("group_jobs"))[:-1])


# ---- dedupe and units --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gs", [1, 4, 1024])
def test_units(gs):
    p = rp.plan(COUNTS, FLAGS, MSGS, opts=rp.Opts(group_sets=gs, group_adapt=0))
    n = len(MSGS)
    msg_idx, uniq = p.vec("msg_idx"), p.vec("uniq")
    assert [MSGS[uniq[m]] for m in msg_idx] == MSGS and len(set(MSGS)) == len(uniq) == p["n_umsg"]
    assert uniq == sorted(uniq) and all(MSGS.index(MSGS[u]) == u for u in uniq)  # first occurrences
    sets = job_sets(COUNTS)
    group_of = {}
    for g, (a, e) in enumerate(pairs(p.vec("group_jobs"))):
        for i in range(sets[a][0], sets[e - 1][1]):
            group_of[i] = g
    assert sorted(group_of) == list(range(n))
    unit = p.vec("unit_of_set")
    for i in range(n):
        for k in range(n):
            same = group_of[i] == group_of[k] and MSGS[i] == MSGS[k]
            assert (unit[i] == unit[k]) == same, (i, k)
    n_units_seen = len(set(unit))
    assert p["merged"] == (n_units_seen < n)
    if p["merged"]:
        assert p["n_units"] == n_units_seen and p["n_items"] == n_units_seen
        first, usets, umsg = p.vec("unit_first"), p.vec("unit_sets"), p.vec("unit_msg")
        assert first[0] == 0 and first[-1] == n and sorted(usets) == list(range(n))
        for u in range(n_units_seen):
            mine = usets[first[u]:first[u + 1]]
            assert mine == sorted(mine) and mine and all(unit[i] == u and msg_idx[i] == umsg[u] for i in mine)
        gf = p.vec("g_unit_first")
        for g in range(p["ng0"]):  # a group's units are consecutive
            assert {unit[i] for i in group_of if group_of[i] == g} == set(range(gf[g], gf[g + 1]))
    else:
        assert p["n_units"] == 0 and p["n_items"] == n


def test_no_units_without_repeats_or_dedupe():
    for msgs, dedupe in [(list(range(10)), 1), (MSGS, 0)]:
        p = rp.plan(COUNTS, FLAGS, msgs, opts=rp.Opts(group_sets=4, dedupe=dedupe, group_adapt=0))
        assert not p["merged"] and p["n_units"] == 0 and p["n_items"] == 10 and p["n_umsg"] == 10
        assert p.vec("unit_first") == [] and p.vec("unit_sets") == []
        assert p.vec("msg_idx") == list(range(10))


def test_merged_at_group_sets_4():
    p = rp.plan(COUNTS, FLAGS, MSGS, opts=rp.Opts(group_sets=4, group_adapt=0))
    # groups {sets 0-1}, {2}, {3-6}, {7-9}: units (5), (6), (7, 5), (5, 8) -> 6 units of 10 sets
    assert p["merged"] and p["n_units"] == 6 and p["n_umsg"] == 4


# ---- chunks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("miller_k", [0, 1, 2, 4])
@pytest.mark.parametrize("segments", [0, 2])
@pytest.mark.parametrize("msgs,dedupe,keep_opt", [(MSGS, 1, 1), (MSGS, 0, 1), (list(range(10)), 1, 0)])
def test_chunks(miller_k, segments, msgs, dedupe, keep_opt):
    p = rp.plan(COUNTS, FLAGS, msgs, opts=rp.Opts(group_sets=4, dedupe=dedupe, miller_k=miller_k, keep_f=keep_opt,
                                                  miller_segments=segments, group_adapt=0))
    first, items, gc = p.vec("chunk_first"), p.vec("chunk_items"), pairs(p.vec("g_chunks"))
    mk, n_chunks = p["mk"], p["n_chunks"]
    coop = miller_k <= 1  # ten items: a cooperative run unless miller_k asks for chunks
    assert p["coop"] == coop and mk == (1 if coop else miller_k) == p["mk_whole"]
    assert len(first) == n_chunks + 1 and first[0] == 0 and first[-1] == len(items) == p["n_items"]
    merged = bool(p["merged"])
    sets = job_sets(COUNTS)
    gf = p.vec("g_unit_first")
    at = 0
    for g, (a, e) in enumerate(pairs(p.vec("group_jobs"))):
        want = list(range(gf[g], gf[g + 1])) if merged else list(range(sets[a][0], sets[e - 1][1]))
        c0, c1 = gc[g]
        assert c0 == at and c1 > c0
        got = [items[k] for c in range(c0, c1) for k in range(first[c], first[c + 1])]
        assert sorted(got) == want  # the group's items exactly once
        assert all(1 <= first[c + 1] - first[c] <= mk for c in range(c0, c1))
        assert c1 - c0 == -(-len(want) // mk)
        at = c1
    assert at == n_chunks
    # step segments: only the one-lane chunk form takes them (here the chunks of 2 and 4), at most mk, and only while
    # the segments' slots fit the n slots of f_chunk
    want_segs = min(segments, mk) if segments and not coop else 1
    assert p["segs"] == min(want_segs, max(1, 10 // max(n_chunks, 1))) and p["interleave"] == (want_segs > 1)
    seg_first = p.vec("seg_first")
    assert len(seg_first) == p["segs"] + 1 and seg_first[0] == 0 and seg_first[-1] == 68
    # keep_f: the option, no units, one item per chunk and one chunk per set
    assert p["keep_f"] == bool(keep_opt and not merged and mk == 1 and n_chunks == 10)
    assert p["fkeep_words"] == 10 * W_FP12 and p["fseg_words"] == W_FP12 * p["n_franges"]
    assert p["n_franges"] == p["ng0"] * p["segs"]


def test_miller_k_auto_and_large_run_forms():
    L = rp.lib()
    assert [L.rp_miller_k_auto(n) for n in (1, 131071, 131072, 262143, 262144, 1 << 22)] == [1, 1, 2, 2, 4, 4]
    n = 70000  # >= 65,536 items: the step-segment plan takes chunks of 8 (miller_plan.hpp); it gives up keep_f
    p = rp.plan([n], [1], range(n), opts=rp.Opts(group_adapt=0))
    assert not p["coop"] and p["seg_plan"] and p["mk"] == 8 and p["mk_whole"] == 1 and not p["keep_f"]
    assert p["n_chunks"] * p["segs"] >= 65536 and p["n_chunks"] == -(-n // 8) and p["interleave"]
    assert not p["small"] and not p["coop_g2"] and p["slice_len"] == MSM_SLICE
    p = rp.plan([n], [1], range(n), opts=rp.Opts(group_adapt=0), fail_rate=0.01)  # many failing groups: held
    assert not p["seg_plan"] and p["mk"] == 1 and p["keep_f"]


@pytest.mark.parametrize("alone", [0, 1])
@pytest.mark.parametrize("urgent", [0, 1])
def test_forms_of_a_small_run(alone, urgent):
    p = rp.plan(COUNTS, FLAGS, MSGS, alone=alone, urgent=urgent, opts=rp.Opts(group_adapt=0))
    assert p["coop"] and p["coop_g2"] and p["small"] and not p["lane_tail"]
    assert p["excl"] == (not urgent) and p["spec"] == alone and p["rsig_spec"] == alone
    q = rp.plan(COUNTS, FLAGS, MSGS, alone=alone, urgent=urgent,
                opts=rp.Opts(small_max=5, spec_large=0, urgent_excl=1, lane_tail_min=10, coop_g2_max=9, group_adapt=0))
    assert not q["small"] and not q["spec"] and not q["rsig_spec"] and q["excl"] and q["lane_tail"] and not q["coop_g2"]
    r = rp.plan(COUNTS, FLAGS, MSGS, alone=alone, opts=rp.Opts(small_max=5, serial=0, group_adapt=0))
    assert r["spec"] == alone and not r["rsig_spec"]  # spec_large: the MSM alone
    s = rp.plan(COUNTS, FLAGS, MSGS, alone=alone, opts=rp.Opts(serial=1, group_adapt=0))
    assert not s["spec"]


# ---- F tree by simulation ----------------------------------------------------------------------------------------
def simulate_tree(t, ranges_len, segs):
    gc, at = [], 0
    for ln in ranges_len:
        gc.append((at, at + ln))
        at += ln
    n_chunks = at
    f_rng = pairs(t.vec("f_rng"))
    assert f_rng == [(j * n_chunks + a, j * n_chunks + e) for j in range(segs) for a, e in gc]
    tree, n_fruns, levels = pairs(t.vec("ftree")), t["n_fruns"], t.vec("f_level_end")
    slot = [{i} for i in range(n_chunks * segs)]
    consumed = set()
    touched = set()
    for a, e in tree[:n_fruns]:  # one launch: slot a becomes the product of [a, e)
        assert 1 < e - a <= t["f_k"]
        rng = set(range(a, e))
        assert not (rng & touched)
        touched |= rng
        for i in range(a + 1, e):
            slot[a] |= slot[i]
            consumed.add(i)
    assert levels == sorted(levels) and (not levels or levels[-1] == len(tree) - n_fruns)
    lo = 0
    for hi in levels:  # each level one launch of k_f_pairs, in place: no slot twice
        seen = set()
        for dst, src in tree[n_fruns + lo:n_fruns + hi]:
            assert dst not in seen and src not in seen and dst not in consumed and src not in consumed
            seen |= {dst, src}
        for dst, src in tree[n_fruns + lo:n_fruns + hi]:
            slot[dst] |= slot[src]
            consumed.add(src)
        lo = hi
    for a, e in f_rng:
        if e > a:
            assert slot[a] == set(range(a, e)) and a not in consumed


@pytest.mark.parametrize("seed", range(6))
def test_f_tree_small_random(seed):
    rng = np.random.default_rng(seed)
    lens = rng.choice([0, 1, 2, 3, 5, 8, 17, 33], size=int(rng.integers(1, 9))).tolist()
    for segs in (1, 2, 3):
        t, _, _ = rp.ftree(lens, segs, 16)
        assert t["f_k"] == 1 and t["n_fruns"] == 0
        simulate_tree(t, lens, segs)


@pytest.mark.parametrize("f_run_max,segs,f_k", [(16, 1, 4), (32, 1, 32), (16, 2, 8)])
def test_f_tree_past_the_run_threshold(f_run_max, segs, f_k):
    lens = [9000, 1, 0, 7001, 37, 400]  # 16,439 slots: more than 16,384, so lane-serial runs come first
    t, _, n_chunks = rp.ftree(lens, segs, f_run_max)
    assert n_chunks == 16439 and t["f_k"] == f_k and t["n_fruns"] > 0
    simulate_tree(t, lens, segs)


def test_f_tree_of_a_plan_is_the_function():
    p = rp.plan(COUNTS, FLAGS, MSGS, opts=rp.Opts(group_sets=4, miller_k=4, miller_segments=2, coop_max=0, group_adapt=0))
    lens = [e - a for a, e in pairs(p.vec("g_chunks"))]
    t, _, _ = rp.ftree(lens, p["segs"], 16)
    assert p["segs"] == 2 and all(p.vec(k) == t.vec(k) for k in ("f_rng", "ftree", "f_level_end"))
    simulate_tree(p, lens, p["segs"])


# ---- MSM slices --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,slice_len", [(1024, 32), (1025, 48), (32768, 48), (32769, MSM_SLICE)])
def test_msm_slices(n, slice_len):
    counts = [n - 2 * (n // 3), n // 3, n // 3]  # about equal ranges: the slice tree stays on
    p = rp.plan(counts, [1, 0, 0], range(n), opts=rp.Opts(msm_slice_mid=48, group_sets=64, group_adapt=0))
    assert p["slice_len"] == slice_len
    sl, rs, sets = pairs(p.vec("slices")), p.vec("range_slices"), job_sets(counts)
    assert rs[0] == 0 and rs[-1] == len(sl) == p["n_slices"] and len(rs) == p["ng0"] + 1 == 4
    most = 0
    for g, (a, e) in enumerate(pairs(p.vec("group_jobs"))):
        mine = sl[rs[g]:rs[g + 1]]
        assert mine[0][0] == sets[a][0] and mine[-1][1] == sets[e - 1][1]
        assert all(x[1] == y[0] for x, y in zip(mine, mine[1:])) and all(0 < y - x <= slice_len for x, y in mine)
        most = max(most, len(mine))
    assert p["msm_tree"] == (most if n <= 32768 else 0)  # the ranges are about equal; no tree above 32k sets
    assert p["msmB_words"] == MSM_BUCKET_WORDS * len(sl)


def test_msm_tree_off_for_unequal_ranges():
    counts = [2000] + [1] * 50  # one 2,000-set job beside 50 single-set groups
    p = rp.plan(counts, [0] * 51, range(2050), opts=rp.Opts(group_adapt=0))
    rs = p.vec("range_slices")
    most = max(b - a for a, b in zip(rs, rs[1:]))
    assert p["ng0"] == 51 and most == -(-2000 // 32) and 51 * most > 2 * p["n_slices"] and p["msm_tree"] == 0
    q = rp.plan(counts, [0] * 51, range(2050), opts=rp.Opts(msm_tree=0, group_adapt=0))
    assert q["msm_tree"] == 0


# ---- arenas ------------------------------------------------------------------------------------------------------
IN_FIELDS = ["scal", "jobs", "sigs", "siglen", "umsg", "midx", "ranges", "franges", "ufirst", "usets", "umsgi", "cfirst",
             "citems", "agg", "slices", "rslices", "ftree"]
ARENA_SHAPES = [(COUNTS, FLAGS, MSGS), ([1], [1], [3]), ([0, 0, 0], [1, 0, 1], []), ([3, 2], [1, 1], [1, 1, 1, 1, 1])]


@pytest.mark.parametrize("shape", range(len(ARENA_SHAPES)))
@pytest.mark.parametrize("pk_mode", [0, 1, 2])
@pytest.mark.parametrize("sig_w", [96, 192])
@pytest.mark.parametrize("dedupe", [0, 1])
def test_arenas(shape, pk_mode, sig_w, dedupe):
    counts, flags, msgs = ARENA_SHAPES[shape]
    n, nj = sum(counts), len(counts)
    keys = [1 + (i % 3) for i in range(n)] if pk_mode != 1 else [1] * n
    sig_len = [96] * n
    if sig_w == 192 and n:
        sig_len[-1] = 192
    p = rp.plan(counts, flags, msgs, keys_per_set=keys, pk_mode=pk_mode, sig_len=sig_len,
                opts=rp.Opts(group_sets=4, dedupe=dedupe, group_adapt=0))
    assert p["sig_w"] == (sig_w if n else 96)
    sig_w = p["sig_w"]
    stride, ng0, n_umsg, nm, n_units = max(n, 1), p["ng0"], p["n_umsg"], p["nm"], p["n_units"]
    merged = bool(p["merged"])
    assert p["stride"] == stride and nm == max(n_umsg, 1) and p["n"] == n and p["nj"] == nj
    npk = sum(keys) if pk_mode != 1 else 0
    assert p["npk"] == npk
    assert p.vec("agg_sets") == ([i for i in range(n) if keys[i] >= 2] if pk_mode != 1 else [])
    n_franges, n_chunks = p["n_franges"], p["n_chunks"]
    sizes = [n * 8, (nj + 1) * 4, n * sig_w, n * 4, n_umsg * 32, n * 4, max(ng0, 1) * 8, max(n_franges, 1) * 8,
             (n_units + 1) * 4, len(p.vec("unit_sets")) * 4, n_units * 4, (n_chunks + 1) * 4,
             len(p.vec("chunk_items")) * 4, len(p.vec("agg_sets")) * 4, len(p.vec("slices")) * 4,
             len(p.vec("range_slices")) * 4, len(p.vec("ftree")) * 4]
    # the chained expression run_shard held: o_next = al256(o + size)
    at = 0
    for f, size in zip(IN_FIELDS, sizes):
        assert p["in." + f] == at and at % 256 == 0, f
        at = al256(at + size)
    o_pk = at
    assert p["in.pk_first"] == o_pk
    o_pk2 = al256(o_pk + (n + 1) * 4)
    if pk_mode == 0:
        assert p["in.pk_keys"] == o_pk2 and p["in.bytes"] == o_pk2 + npk * 4
    elif pk_mode == 2:
        assert p["in.pk_keys"] == o_pk2 and p["in.bytes"] == o_pk2 + npk * 96
    else:
        assert p["in.pk_keys"] == o_pk and p["in.bytes"] == o_pk + n * 96
    # byte arena and results
    ob = [0, al256(n)]
    ob.append(al256(ob[1] + nm))
    ob.append(al256(ob[2] + n))
    ob.append(al256(ob[3] + 3 * stride))
    ob.append(al256(ob[4] + stride))
    assert [p["by." + f] for f in ("flags", "mflags", "unit_ok", "status", "include", "spec")] == ob
    assert p["by.total"] == al256(ob[5] + stride)
    max_ranges = max(ng0, nj, 1)
    assert p["res.job_err"] == 0 and p["res.ok"] == al256(nj) and p["res.bytes"] == al256(nj) + max_ranges
    assert p["res.max_ranges"] == max_ranges
    # d_work: the total run_shard passed to ensure, and its pointer walk
    per_set = W_G2A + W_G1J + W_G1A + W_FP12 + 8 * W_G1J + 2 * W_FP + (W_G1A if merged else 0)
    assert p["work.words"] == stride * per_set + nm * (W_G2A + W_G2J + W_FP + 14 * W_FP + 2 * W_G2J)
    w = 0
    walk = [("sig_aff", stride * W_G2A), ("pk_jac", stride * W_G1J), ("pk_aff", stride * W_G1A),
            ("f_chunk", stride * W_FP12), ("scal_tab", stride * 8 * W_G1J)]
    if merged:
        walk.append(("unit_p", stride * W_G1A))
    walk += [("inv_buf", stride * W_FP), ("inv_buf_pk", stride * W_FP), ("h_aff", nm * W_G2A), ("h_jac", nm * W_G2J),
             ("h_norm", nm * W_FP), ("h_prep", nm * 14 * W_FP), ("h_q", nm * 2 * W_G2J)]
    for f, words in walk:
        assert p["work." + f] == w, f
        w += words
    assert w == p["work.words"]  # h_q, the last field, ends where the total does
    # the other buffers of the batch pass
    assert p["S_words"] == W_G2J * max_ranges and p["F_words"] == W_FP12 * max_ranges
    assert p["G_words"] == W_FP12 * max(ng0, 1) and p["msmW_words"] == MSM_WINDOW_WORDS * max_ranges
    assert p["msmB_words"] == MSM_BUCKET_WORDS * max(p["n_slices"], 1) and p["lines_words"] == nm * MILLER_LINE_WORDS
    assert p["fb_words"] == stride * 9 * W_G2J


def test_shard_relative_plan():
    """Jobs [2, 6) of the batch as a shard: sets 2 .. 8, everything relative to the shard's first job and set."""
    p = rp.plan(COUNTS, FLAGS, MSGS, job_begin=2, job_end=6, opts=rp.Opts(group_sets=4, group_adapt=0))
    assert p["n"] == 7 and p["nj"] == 4 and pairs(p.vec("group_jobs")) == [(0, 1), (1, 3), (3, 4)]
    assert [MSGS[2 + u] for u in p.vec("uniq")] == [6, 7, 5, 8] and p.vec("msg_idx") == [0, 1, 2, 1, 1, 2, 3]
    assert pairs(p.vec("slices")) == [(0, 1), (1, 5), (5, 7)]


# ---- classify_groups ---------------------------------------------------------------------------------------------
# three groups at group_sets 4 over jobs of [2, 1, 1, 3, 1] sets: {0, 1, 2}, {3}, {4}
C_COUNTS, C_FLAGS = [2, 1, 1, 3, 1], [1, 1, 1, 1, 0]
C_POOL = {"batchable": [(0, 3, 1), (3, 4, 1), (4, 5, 0)], "not": [(0, 3, 0), (3, 4, 0), (4, 5, 0)]}
E = 3  # an error code

# (job_err, group_ok, spec) -> jr, retry, failed_g, (retries, sigs) without a list, with a batchable, a non-batchable
CLASSIFY_TABLE = [
    # every group passes: the multi-job group's sets count as batch successes; single-job groups never do
    ([0, 0, 0, 0, 0], [1, 1, 1], 0, [1, 1, 1, 1, 1], [], [], (0, 4), (0, 7), (0, 0)),
    # the three-clean-job group fails: all three retried, one batch retry
    ([0, 0, 0, 0, 0], [0, 1, 1], 0, [2, 2, 2, 1, 1], [0, 1, 2], [0], (1, 0), (1, 3), (0, 0)),
    # a failing group with one clean job: retried, no batch retry without a list (a list's batchable chunk counts)
    ([0, 0, 0, 0, 0], [1, 0, 0], 0, [1, 1, 1, 2, 2], [3, 4], [1, 2], (0, 4), (1, 4), (0, 0)),
    # one errored job, spec on: the clean jobs are retried whatever ok says, the group is not a failed group
    ([0, E, 0, 0, 0], [1, 1, 1], 1, [2, -E, 2, 1, 1], [0, 2], [], (1, 0), (1, 3), (0, 0)),
    ([0, E, 0, 0, 0], [0, 1, 1], 1, [2, -E, 2, 1, 1], [0, 2], [], (1, 0), (1, 3), (0, 0)),
    # the same with spec off: ok is read; a passing group's clean jobs are valid (a list counts the chunk as a retry:
    # one of its jobs threw)
    ([0, E, 0, 0, 0], [1, 1, 1], 0, [1, -E, 1, 1, 1], [], [], (0, 3), (1, 3), (0, 0)),
    ([0, E, 0, 0, 0], [0, 1, 1], 0, [2, -E, 2, 1, 1], [0, 2], [0], (1, 0), (1, 3), (0, 0)),
    # a group of only errored jobs: nothing to retry, spec or not
    ([E, E, E, 0, 0], [0, 1, 1], 1, [-E, -E, -E, 1, 1], [], [], (0, 0), (1, 3), (0, 0)),
    ([E, E, E, 0, 0], [0, 1, 1], 0, [-E, -E, -E, 1, 1], [], [], (0, 0), (1, 3), (0, 0)),
    # spec with one clean job beside a dropped one: retried, no batch retry without a list
    ([0, E, E, 0, 0], [1, 1, 1], 1, [2, -E, -E, 1, 1], [0], [], (0, 0), (1, 3), (0, 0)),
]


@pytest.mark.parametrize("case", range(len(CLASSIFY_TABLE)))
@pytest.mark.parametrize("grouping", ["packed", "batchable", "not"])
def test_classify_groups(case, grouping):
    job_err, ok, spec, jr, retry, failed_g, packed, batchable, non = CLASSIFY_TABLE[case]
    p = rp.plan(C_COUNTS, C_FLAGS, range(8), opts=rp.Opts(group_sets=4, group_adapt=0), pool=C_POOL.get(grouping))
    assert pairs(p.vec("group_jobs")) == [(0, 3), (3, 4), (4, 5)]
    c, got_jr = rp.classify(p, job_err, ok, spec)
    assert got_jr == jr and c.vec("retry") == retry and c.vec("failed_g") == failed_g
    want = {"packed": packed, "batchable": batchable, "not": non}[grouping]
    assert (c["batch_retries"], c["batch_sigs_success"]) == want


def test_fail_rate_estimate():
    p = rp.plan(C_COUNTS, C_FLAGS, range(8), opts=rp.Opts(group_sets=4, group_adapt=0))
    n, ng = 8, 3
    for jr, failed in [([1, 1, 1, 1, 1], 0), ([1, 0, 1, 1, 1], 1), ([0, 0, 0, 1, -E], 2), ([0, 1, 1, 0, 0], 3)]:
        pf = min(failed, ng - 0.5) / ng
        f = 1.0 - (1.0 - pf) ** (ng / n)
        assert rp.next_fail_rate(p, jr, 0.25) == pytest.approx(0.5 * 0.25 + 0.5 * f, rel=1e-12)


# ---- plan_fallback -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nr,nsub", [(31, 0), (32, 2), (33, 3)])
def test_fallback_sub_groups(nr, nsub):
    o = rp.Opts(small_max=0, group_sets=64, group_adapt=0)  # not small, idle device: no direct rule
    p = rp.plan([1] * nr, [1] * nr, range(nr), opts=o, alone=True)
    f = rp.fallback(p, list(range(nr)), o, alone=True)
    assert (f["kFbSub"], f["kFbLaneMin"], f["kFbDirectMax"]) == (16, 128, 640)
    assert not f["direct"] and not f["busy"] and f["nsub"] == nsub and f["small_jobs"]
    sub = pairs(f.vec("subr"))
    assert sub == [(16 * t, min(nr, 16 * t + 16)) for t in range(nsub)]
    if nr == 33:
        assert sub[-1] == (32, 33)  # the last sub-group holds one job
    assert f["nc"] == 0 and f.vec("rf") == f.vec("rr") and f.vec("ritems") == []  # keep_f: chunk = set
    # d_list: rr | rf | rfirst | ritems | rsl | rrs | rset | subr | sel
    o_rsl = 4 * nr + 1 + 0
    o_rrs = o_rsl + 2 * nr
    o_rset = o_rrs + nr + 1
    o_sub = o_rset + nr
    o_sel = o_sub + 2 * nsub
    assert (f["o_rf"], f["o_rfirst"], f["o_ritems"]) == (2 * nr, 4 * nr, 4 * nr + 1)
    assert (f["o_rsl"], f["o_rrs"], f["o_rset"], f["o_sub"], f["o_sel"], f["words"]) == (
        o_rsl, o_rrs, o_rset, o_sub, o_sel, o_sel + nr)


@pytest.mark.parametrize("nr,direct", [(640, 1), (641, 0)])
def test_fallback_direct_checks_of_a_small_run(nr, direct):
    o = rp.Opts(group_adapt=0)
    p = rp.plan([1] * nr, [1] * nr, range(nr), opts=o)
    assert p["small"]
    f = rp.fallback(p, list(range(nr)), o, alone=False)
    assert f["direct"] == direct and f["nsub"] == (0 if direct else 41) and not f["busy"]


def test_fallback_busy_forms():
    o = rp.Opts(small_max=0, fb_direct_min=40, fb_lane_min=40, group_adapt=0)
    p = rp.plan([1] * 48, [1] * 48, range(48), opts=o)
    f = rp.fallback(p, list(range(48)), o, alone=False)
    assert f["busy"] and f["direct"] and f["nsub"] == 0 and f["lane_checks_nr"]
    f = rp.fallback(p, list(range(39)), o, alone=False)
    assert f["busy"] and not f["direct"] and f["nsub"] == 3 and not f["lane_checks_nr"]
    f = rp.fallback(p, list(range(48)), o, alone=True)
    assert not f["busy"] and not f["direct"] and f["nsub"] == 3
    o2 = rp.Opts(small_max=0, fb_direct_min=40, fb_force_busy=1, group_adapt=0)
    assert rp.fallback(p, list(range(48)), o2, alone=True)["busy"]


@pytest.mark.parametrize("keep_f", [0, 1])
def test_fallback_lists(keep_f):
    counts = [3, 70, 1, 300, 2]
    n = sum(counts)
    o = rp.Opts(keep_f=keep_f, miller_k=2, coop_max=0, group_adapt=0) if not keep_f else rp.Opts(group_adapt=0)
    p = rp.plan(counts, [1] * 5, range(n), opts=o)
    assert p["keep_f"] == keep_f and p["mk_whole"] == (1 if keep_f else 2)
    retry = [0, 1, 3, 4]
    f = rp.fallback(p, retry, o, alone=True)
    sets = job_sets(counts)
    rr, rf = pairs(f.vec("rr")), pairs(f.vec("rf"))
    assert rr == [sets[j] for j in retry]
    assert f.vec("rset") == [i for j in retry for i in range(*sets[j])]
    rsl, rrs = pairs(f.vec("rsl")), f.vec("rrs")
    assert rrs[0] == 0 and len(rrs) == 5 and f["nrs"] == len(rsl) == rrs[-1]
    for q, (a, e) in enumerate(rr):  # full-length slices
        mine = rsl[rrs[q]:rrs[q + 1]]
        assert mine == [(x, min(e, x + MSM_SLICE)) for x in range(a, e, MSM_SLICE)]
    if keep_f:
        assert rf == rr and f["nc"] == 0 and f.vec("rfirst") == [0]
    else:
        first, items = f.vec("rfirst"), f.vec("ritems")
        assert f["nc"] == len(first) - 1 and items == f.vec("rset")
        at = 0
        for q, (a, e) in enumerate(rr):
            assert rf[q] == (at, at + -(-(e - a) // 2))
            for c in range(*rf[q]):
                assert first[c + 1] - first[c] <= 2
            assert [items[k] for k in range(first[rf[q][0]], first[rf[q][1]])] == list(range(a, e))
            at = rf[q][1]
    # small_jobs: fewer than 32 sets per retried job on average
    assert not f["small_jobs"] and len(f.vec("rset")) == 375 >= 32 * 4
    g = rp.fallback(p, [0, 1, 2, 4], o, alone=True)  # 76 sets in 4 jobs
    assert g["small_jobs"] and len(g.vec("rset")) == 76 < 32 * 4
    words = 4 * 4 + len(f.vec("rfirst")) + len(f.vec("ritems")) + len(f.vec("rsl")) + 5 + 375
    assert f["o_sel"] == words and f["words"] == words + 4


# ---- plan_pool_groups --------------------------------------------------------------------------------------------
def pool_rule(counts, flags):
    """run_pool_policy's grouping restated with the reference's chunking rule."""
    sets = job_sets(counts)
    subs = []
    for j, (a, e) in enumerate(sets):
        bt = flags[j] & 1
        if a == e:
            subs.append((j, a, a, bt))
            continue
        for ch in reference_rule(e - a, 128):
            subs.append((j, a + ch[0], a + ch[-1] + 1, bt))
    order, groups, q = [], [], 0
    while q < len(subs):
        q1, total = q, 0
        while q1 < len(subs) and total < 128:
            total += subs[q1][2] - subs[q1][1]
            q1 += 1
        bat = [x for x in range(q, q1) if subs[x][3] and subs[x][2] > subs[x][1]]
        rest = [x for x in range(q, q1) if x not in bat]
        if bat:
            for ch in reference_rule(len(bat), 16):
                groups.append((len(order), len(order) + len(ch), 1))
                order += [bat[k] for k in ch]
        for x in rest:
            groups.append((len(order), len(order) + 1, 0))
            order.append(x)
        q = q1
    return subs, order, groups


@pytest.mark.parametrize("counts,flags", [
    ([0, 1, 127, 128, 129, 300], [1, 1, 0, 1, 1, 0]),
    ([0, 1, 127, 128, 129, 300], [0, 0, 1, 0, 1, 1]),
    ([1] * 200 + [0, 300] + [2] * 40, [1] * 100 + [0] * 50 + [1] * 92),
])
def test_pool_groups(counts, flags):
    r = rp.pool_groups(counts, flags)
    subs, order, groups = pool_rule(counts, flags)
    v = r.vec("subs")
    assert [tuple(v[4 * i:4 * i + 4]) for i in range(len(v) // 4)] == subs
    g = r.vec("groups")
    assert r.vec("order") == order and [tuple(g[3 * i:3 * i + 3]) for i in range(len(g) // 3)] == groups
    assert sorted(order) == list(range(len(subs)))  # every sub-job in exactly one group
    assert all(e - a < 256 for _, a, e, _ in subs)  # below two minimum chunks
    L = rp.lib()
    assert all(L.rp_chunk_size(n, m) == len(reference_rule(n, m)[0]) for n in (1, 127, 128, 129, 300, 4097) for m in (16, 128))


# ---- sanitized stand-alone run -----------------------------------------------------------------------------------
def test_probe_program_under_sanitizers(tmp_path):
    """The probe's own main (the shapes above and more) as a stand-alone program under ASan + UBSan: a child process,
    never loaded into Python."""
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "one"), str(one)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "one")], capture_output=True).returncode != 0:
        pytest.skip("no sanitized host build here")
    exe = tmp_path / "run_plan_probe"
    subprocess.check_call(["g++", *flags, "-DRUN_PLAN_PROBE_MAIN", "-o", str(exe), rp.SRC])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "plans, checksum" in r.stdout
