"""The host plan of the Miller accumulation's step segments (lodestar_amd/csrc/miller_plan.hpp), CPU only.

tests/native/miller_plan_probe.cpp compiles the header alone with g++.  Checked here: the segment boundaries for
J = 1..8, the automatic (k, J) rule over regular, ragged and tiny groups, and the interleaved item assignment."""
import ctypes
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "miller_plan_probe.cpp")
LIB = os.path.join(HERE, "native", "libmiller_plan_probe.so")
HDR = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc", "miller_plan.hpp")

Z_ABS = 0xD201000000010000
FILL = 65536


def schedule():
    """The 68 steps of the device loop: True = doubling step."""
    out = []
    for bit in range(62, -1, -1):
        out.append(True)
        if (Z_ABS >> bit) & 1:
            out.append(False)
    return out


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.probe_count_chunks.restype = ctypes.c_uint64
    lib.probe_count_chunks.argtypes = [ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, ctypes.c_uint32]
    lib.probe_fit.restype = ctypes.c_uint32
    lib.probe_fit.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint64]
    lib.probe_allowed.argtypes = [ctypes.c_uint64, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]
    lib.probe_plan.restype = None
    lib.probe_plan.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint64, ctypes.c_uint64,
                               ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_uint32)]
    lib.probe_chunks.restype = ctypes.c_uint32
    return lib


def test_header_is_hip_free():
    src = open(HDR).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert all(i.startswith("<") and "hip" not in i for i in includes), includes


def test_schedule_matches_the_device_loop(probe):
    sched = schedule()
    assert len(sched) == 68 and sum(sched) == 63
    assert [bool(probe.probe_is_doubling(s)) for s in range(68)] == sched


def segments(probe, J):
    first = (ctypes.c_uint32 * 9)()
    dbl = (ctypes.c_uint32 * 8)()
    n = probe.probe_segments(J, first, dbl)
    return list(first[: n + 1]), list(dbl[:n])


@pytest.mark.parametrize("J", range(1, 9))
def test_boundaries(probe, J):
    sched = schedule()
    first, dbl = segments(probe, J)
    assert len(dbl) == J and first[0] == 0 and first[-1] == 68
    assert all(a < b for a, b in zip(first, first[1:]))  # the steps 0..67, each in exactly one segment
    assert all(sched[s] for s in first[:-1])  # every segment starts at a doubling step
    assert dbl == [sum(sched[a:b]) for a, b in zip(first, first[1:])] and sum(dbl) == 63
    # as equal as the doubling-step rule allows: the ideal boundary 68 j / J rounded to a step (<= 0.5 off), moved at
    # most one step down to reach a doubling step
    assert all(-1.5 <= first[j] - 68 * j / J <= 0.5 for j in range(J + 1))


def plan(probe, glen, capacity=None, explicit=False, k_today=1):
    n = sum(glen)
    arr = (ctypes.c_uint32 * max(len(glen), 1))(*glen)
    out = (ctypes.c_uint32 * 2)()
    probe.probe_plan(n, arr, len(glen), n if capacity is None else capacity, int(explicit), k_today, out)
    return out[0], out[1]


def chunks_of(glen, k):
    return sum((g + k - 1) // k for g in glen)


def allowed_pairs(glen, capacity):
    """(k, J) the rule may return: J <= k, J <= 8, slots within capacity, chunks at least half full on average."""
    n = sum(glen)
    out = []
    for k in (8, 4):
        nc = chunks_of(glen, k)
        for J in range(1, min(k, 8) + 1):
            if nc * J <= capacity and 2 * n >= nc * k:
                out.append((k, J, nc))
    return out


def regular(n, g):
    return [g] * (n // g) + ([n % g] if n % g else [])


GROUPINGS = [
    regular(131072, 1024),
    regular(126 * 1024, 1024),
    regular(65536, 1024),
    regular(65535, 1024),
    regular(70001, 1023),  # ragged last chunks in every group
    regular(100003, 37),
    regular(90000, 5),
    regular(80000, 1),  # one item per group: no chunk ever fills
    regular(300000, 1024),
    regular(600000, 2048),
    [70000],
    [3] * 1000 + [1021] * 80,
]


@pytest.mark.parametrize("gi", range(len(GROUPINGS)))
def test_auto_rule(probe, gi):
    glen = GROUPINGS[gi]
    n = sum(glen)
    arr = (ctypes.c_uint32 * len(glen))(*glen)
    for k in (1, 2, 4, 8):
        assert probe.probe_count_chunks(arr, len(glen), k) == chunks_of(glen, k)
    for k_today in (1, 2):
        assert plan(probe, glen, explicit=True, k_today=k_today) == (k_today, 1)
        for capacity in (n, n + 7 * len(glen), n // 2, 70000):
            k, J = plan(probe, glen, capacity=capacity, k_today=k_today)
            if n < FILL:
                assert (k, J) == (k_today, 1)
                continue
            ok = allowed_pairs(glen, capacity)
            full = [(kk, JJ) for kk, JJ, nc in ok if nc * JJ >= FILL]
            if (k, J) == (k_today, 1) and (k, J) not in full:
                assert not full  # today's form only when no allowed pair fills the chip
                continue
            nc = chunks_of(glen, k)
            assert k in (4, 8) and 1 <= J <= k and J <= 8
            assert nc * J <= capacity and nc * J >= FILL
            assert probe.probe_allowed(n, nc, k, J, capacity) == 1
            # the largest k that can fill the chip, and its smallest J
            assert k == max(kk for kk, _ in full)
            assert J == min(JJ for kk, JJ in full if kk == k)


def test_auto_rule_flagship_shapes(probe):
    assert plan(probe, regular(131072, 1024), k_today=2) == (8, 4)  # 16,384 chunks x 4 = 65,536 lanes
    assert plan(probe, regular(126 * 1024, 1024), k_today=1) == (8, 5)
    assert plan(probe, regular(65536, 1024), k_today=1) == (8, 8)
    assert plan(probe, regular(65535, 1024), k_today=1) == (1, 1)
    assert plan(probe, regular(80000, 1), k_today=1) == (1, 1)


def test_hold_kept_values(probe):
    """Runs that keep their per-set Miller values stay as they are once a fifth of the groups would fail."""
    probe.probe_hold.argtypes = [ctypes.c_double, ctypes.c_double]
    for f in (0.0, 1e-6, 1e-4, 2e-4, 3e-4, 1e-3, 0.01, 0.5, 1.0):
        for g in (1, 16, 128, 1024, 4096):
            assert probe.probe_hold(f, g) == int(f > 0 and 1 - (1 - f) ** g >= 0.2), (f, g)
    assert probe.probe_hold(0.01, 1024) == 1 and probe.probe_hold(0.0, 1024) == 0 and probe.probe_hold(1e-5, 1024) == 0


def test_fit_segments(probe):
    assert probe.probe_fit(16384, 4, 131072) == 4
    assert probe.probe_fit(1000, 8, 7999) == 7
    assert probe.probe_fit(1000, 8, 1000) == 1
    assert probe.probe_fit(1000, 8, 10) == 1  # a chunk always has its own slot
    assert probe.probe_fit(5, 0, 100) == 1 and probe.probe_fit(5, 99, 100) == 8


@pytest.mark.parametrize("k", [1, 2, 3, 4, 8])
@pytest.mark.parametrize("interleave", [0, 1])
def test_item_assignment(probe, k, interleave):
    rng = random.Random(1000 * k + interleave)
    for a, e in [(0, 1), (0, 8), (5, 5), (7, 7 + 2085), (3, 3 + 1024), (10, 10 + 9)] + [
            (rng.randrange(50), 50 + rng.randrange(300)) for _ in range(10)]:
        n = e - a
        first = (ctypes.c_uint32 * (n + 2))()
        items = (ctypes.c_uint32 * (n + 1))()
        nc = probe.probe_chunks(a, e, k, interleave, first, items)
        assert nc == (n + k - 1) // k
        assert first[0] == 0 and first[nc] == n
        assert sorted(items[:n]) == list(range(a, e))  # a permutation of the group's items
        sizes = [first[c + 1] - first[c] for c in range(nc)]
        assert all(1 <= s <= k for s in sizes)
        if interleave:  # chunk c holds a + c, a + c + nc, ...: consecutive chunks read consecutive columns
            for c in range(nc):
                assert list(items[first[c]:first[c + 1]]) == list(range(a + c, e, nc))
        else:
            assert list(items[:n]) == list(range(a, e))
