"""The host decisions of the same-message calls (lodestar_amd/csrc/same_plan.hpp), CPU only: the form and block rules,
the descent list, the retry list and the message dedupe the helper calls take from run_plan.hpp.
tests/native/same_plan_probe.cpp exposes them; each is compared with a direct model of its rule written here."""
import ctypes
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
SRC = os.path.join(HERE, "native", "same_plan_probe.cpp")
LIB = os.path.join(HERE, "native", "libsame_plan_probe.so")
HDRS = [os.path.join(CSRC, h) for h in ("same_plan.hpp", "run_plan.hpp", "aggverify_plan.hpp", "miller_plan.hpp",
                                        "helper_layout.hpp", "options.hpp")]
U8P, I8P, U32P = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_int8), ctypes.POINTER(ctypes.c_uint32)
LANE_FORMS, BLOCK_CHECK = 1, 4  # include/blsgpu.h BLSGPU_SAME_LANE_FORMS, BLSGPU_SAME_BLOCK_CHECK
BLOCK = 1024


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    for f in ("probe_form", "probe_blocks", "probe_descent_list", "probe_retry_list", "probe_dedupe"):
        getattr(lib, f).restype = ctypes.c_uint32
    lib.probe_form.argtypes = lib.probe_blocks.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.probe_msg_key.restype = ctypes.c_uint64
    lib.probe_msg_key.argtypes = [ctypes.c_int, ctypes.c_uint64]
    lib.probe_descent_list.argtypes = [ctypes.c_uint32, ctypes.c_uint32, U8P, U8P, U8P, U32P]
    lib.probe_retry_list.argtypes = [U32P, ctypes.c_uint32, I8P, U32P, U32P, U32P, U32P]
    lib.probe_dedupe.argtypes = [U8P, ctypes.c_uint32, ctypes.c_uint64, U32P, U32P, U8P]
    return lib


def test_header_is_hip_free():
    src = open(HDRS[0]).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ['"../../include/blsgpu.h"', "<stdint.h>", "<vector>"]


# ------------------------------------------------------------------------------------------- form and block rules
def test_constants(probe):
    out = (ctypes.c_uint32 * 8)()
    probe.probe_constants(out)
    assert list(out) == [512, BLOCK, 1, 2, 4, 8, 16, 512]  # thresholds, the stats.form bits, AggregateVerify's threshold


@pytest.mark.parametrize("flags", [0, LANE_FORMS, BLOCK_CHECK, LANE_FORMS | BLOCK_CHECK])
def test_form_and_block_rules(probe, flags):
    for n in (0, 512, 513):
        assert probe.probe_form(n, flags) == (1 if flags & LANE_FORMS or n > 512 else 0), n
    for G, nb in ((0, 0), (1, 1), (1024, 1), (1025, 2), (2048, 2), (2049, 3)):
        assert probe.probe_blocks(G, flags) == (nb if flags & BLOCK_CHECK else 0), G
        assert nb == -(-G // BLOCK)


# ----------------------------------------------------------------------------------------------------- descent list
def model_descent(G, NB, any_, ok, include):
    """The included groups of every failed block (it has an included group and its check did not hold), ascending; a
    failed block with exactly one included group lists nothing."""
    out = []
    for b in range(NB):
        if not any_[b] or ok[b]:
            continue
        groups = [g for g in range(BLOCK * b, min(G, BLOCK * (b + 1))) if include[g]]
        if len(groups) != 1:
            out += groups
    return out


def descent(probe, G, any_, ok, include):
    NB = -(-G // BLOCK)
    a, o, i = (np.ascontiguousarray(x, np.uint8) for x in (any_, ok, include))
    assert len(a) == len(o) == NB and len(i) == G
    listed = np.full(G, 0xFFFFFFFF, np.uint32)
    k = probe.probe_descent_list(G, NB, a.ctypes.data_as(U8P), o.ctypes.data_as(U8P), i.ctypes.data_as(U8P),
                                 listed.ctypes.data_as(U32P))
    got = listed[:k].tolist()
    assert got == model_descent(G, NB, a, o, i)
    return got


def test_descent_list_three_blocks(probe):
    G = 2050  # blocks [0, 1024), [1024, 2048), [2048, 2050)
    ones, zeros = np.ones(G, np.uint8), np.zeros(G, np.uint8)
    assert descent(probe, G, [1, 1, 1], [1, 1, 1], ones) == []                          # no block failed
    assert descent(probe, G, [1, 1, 1], [0, 1, 1], ones) == list(range(1024))          # block 0, all included
    assert descent(probe, G, [1, 1, 1], [1, 1, 0], ones) == [2048, 2049]               # block 2, both included
    one = ones.copy()
    one[2049] = 0
    assert descent(probe, G, [1, 1, 1], [1, 1, 0], one) == []                          # block 2, one group: listed nothing
    one = ones.copy()
    one[2048] = 0
    assert descent(probe, G, [1, 1, 1], [1, 1, 0], one) == []
    empty = ones.copy()
    empty[1024:2048] = 0
    assert descent(probe, G, [1, 0, 1], [1, 0, 1], empty) == []                        # a failed block with any == 0
    assert descent(probe, G, [1, 0, 1], [1, 0, 1], ones) == []                         # (`any` decides, not `include`)
    ends = zeros.copy()
    ends[[1024, 2047]] = 1
    assert descent(probe, G, [1, 1, 1], [1, 0, 1], ends) == [1024, 2047]               # only its first and its last
    assert descent(probe, G, [1, 1, 1], [0, 0, 0], zeros) == []                        # include all zero
    # several failed blocks: ascending, each block by its own count
    mixed = zeros.copy()
    mixed[[3, 1000, 1023, 1500, 2048, 2049]] = 1
    assert descent(probe, G, [1, 1, 1], [0, 0, 0], mixed) == [3, 1000, 1023, 2048, 2049]
    assert descent(probe, G, [1, 1, 1], [0, 1, 0], ones) == list(range(1024)) + [2048, 2049]


@pytest.mark.parametrize("G", [1, 1024])
def test_descent_list_one_block(probe, G):
    ones, zeros = np.ones(G, np.uint8), np.zeros(G, np.uint8)
    assert descent(probe, G, [1], [1], ones) == []                                     # not failed
    assert descent(probe, G, [1], [0], ones) == ([] if G == 1 else list(range(G)))     # failed, all included
    assert descent(probe, G, [0], [0], ones) == []                                     # any == 0
    assert descent(probe, G, [0], [0], zeros) == []
    assert descent(probe, G, [1], [0], zeros) == []                                    # include all zero
    one = zeros.copy()
    one[G - 1] = 1
    assert descent(probe, G, [1], [0], one) == []                                      # exactly one included group
    if G > 1:
        one[0] = 1
        assert descent(probe, G, [1], [0], one) == [0, G - 1]                          # its first and its last


# ------------------------------------------------------------------------------------------------------- retry list
def model_retry(sizes, results, gmsg):
    """Every set of each non-empty group whose result is not 1, with the group's message index; empty groups count as
    neither accepted nor retried."""
    sets, msg, accepted, retried, at = [], [], 0, 0, 0
    for size, res, m in zip(sizes, results, gmsg):
        if size and res == 1:
            accepted += 1
        elif size:
            retried += 1
            sets += range(at, at + size)
            msg += [m] * size
        at += size
    return sets, msg, [accepted, retried]


def retry(probe, sizes, results, gmsg):
    G, n = len(sizes), sum(sizes)
    gf = np.cumsum([0] + list(sizes)).astype(np.uint32)
    res, gm = np.asarray(results, np.int8), np.asarray(gmsg, np.uint32)
    sets, msg = np.full(n + 1, 0xFFFFFFFF, np.uint32), np.full(n + 1, 0xFFFFFFFF, np.uint32)
    counts = np.zeros(2, np.uint32)
    k = probe.probe_retry_list(gf.ctypes.data_as(U32P), G, res.ctypes.data_as(I8P), gm.ctypes.data_as(U32P),
                               sets.ctypes.data_as(U32P), msg.ctypes.data_as(U32P), counts.ctypes.data_as(U32P))
    assert k <= n and sets[k] == msg[k] == 0xFFFFFFFF
    got = (sets[:k].tolist(), msg[:k].tolist(), counts.tolist())
    assert got == model_retry(sizes, results, gmsg)
    return got


def test_retry_list(probe):
    sizes, gmsg = [0, 3, 1, 0, 2], [7, 1, 0, 2, 1]  # groups 1 and 4 sign the same message: rmsg is not the group number
    for r1, r2, r4 in itertools.product((1, 0, -5), repeat=3):
        for empty in (1, 0, -5):  # an empty group's result changes nothing
            sets, msg, counts = retry(probe, sizes, [empty, r1, r2, empty, r4], gmsg)
            assert counts[0] + counts[1] == 3
            assert msg == [gmsg[g] for g, size in enumerate(sizes) for _ in range(size)
                           if [None, r1, r2, None, r4][g] != 1]
    assert retry(probe, sizes, [1, 0, 1, 1, -5], gmsg) == ([0, 1, 2, 4, 5], [1, 1, 1, 1, 1], [1, 2])
    assert retry(probe, sizes, [0, 1, 0, 0, 1], gmsg) == ([3], [0], [2, 1])


def test_retry_list_edges(probe):
    for results in ([1, 1, 1], [0, 0, 0], [-5, 1, 0]):  # a call of empty groups only
        assert retry(probe, [0, 0, 0], results, [0, 1, 2]) == ([], [], [0, 0])
    assert retry(probe, [1], [1], [0]) == ([], [], [1, 0])  # one group of one set
    assert retry(probe, [1], [0], [0]) == ([0], [0], [0, 1])
    assert retry(probe, [1], [-3], [0]) == ([0], [0], [0, 1])


# ----------------------------------------------------------------------------------------------------------- dedupe
def test_message_keys(probe):
    for hash_key in (0, 1, 0x0123456789ABCDEF, 0xFFFFFFFFFFFFFFFF):
        assert probe.probe_msg_key(0, hash_key) == hash_key ^ 0x6A09E667F3BCC908  # the same-message calls
        assert probe.probe_msg_key(1, hash_key) == 0xBB67AE8584CAA73B            # blsgpu_aggregate_verify


@pytest.mark.parametrize("which", [0, 1])
def test_dedupe_is_first_occurrence_order(probe, which):
    rng = random.Random(20 + which)
    pool = [rng.randbytes(32) for _ in range(12)]
    pool += [pool[0][:31] + b"\x00", pool[0][:31] + b"\x01", b"\x00" * 32]  # near-equal messages, the zero message
    for n in (0, 1, 2, 16, 17, 40, 41):  # (the index hashes 16 messages ahead)
        msgs = [rng.choice(pool) for _ in range(n)]
        first, want_idx, want_uniq = {}, [], []
        for i, m in enumerate(msgs):
            if m not in first:
                first[m] = len(want_uniq)
                want_uniq.append(i)
            want_idx.append(first[m])
        if n >= 40:
            assert len(want_uniq) < n, "the shape has repeats"
        buf = np.frombuffer(b"".join(msgs) + b"\x00", np.uint8).copy()
        idx, uniq = np.full(n + 1, 0xFFFFFFFF, np.uint32), np.full(n + 1, 0xFFFFFFFF, np.uint32)
        key = probe.probe_msg_key(which, rng.getrandbits(64))
        packed = np.full(32 * n + 1, 0xEE, np.uint8)
        U = probe.probe_dedupe(buf.ctypes.data_as(U8P), n, key, idx.ctypes.data_as(U32P), uniq.ctypes.data_as(U32P),
                               packed.ctypes.data_as(U8P))
        assert U == len(want_uniq) and uniq[:U].tolist() == want_uniq and idx[:n].tolist() == want_idx
        assert packed[: 32 * U].tobytes() == b"".join(msgs[i] for i in want_uniq) and packed[32 * U] == 0xEE
        assert idx[n] == 0xFFFFFFFF and uniq[U] == 0xFFFFFFFF
