"""The cut of large same-message groups into parts (lodestar_amd/csrc/awr_parts.hpp, C-ABI blsgpu_awr_parts), CPU
only: the exported rule and the header's own plan against an independent model written here, the lane rule it builds
on, the refusals, the layout of the buffer a split call adds (hl::AwrParts) and hl::Awr / hl::Same at the parts' lanes.
tests/native/awr_parts_probe.cpp exposes the HIP-free headers."""
import ctypes
import os
import random
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "lodestar_amd", "csrc")
SRC = os.path.join(HERE, "native", "awr_parts_probe.cpp")
LIB = os.path.join(HERE, "native", "libawr_parts_probe.so")
HDRS = [os.path.join(CSRC, h) for h in ("awr_parts.hpp", "helper_layout.hpp")]
U32P, U64P = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)

CAP = 65536
MAX_SETS = 1 << 20
W_FP = 14
W_G1J, W_G2A, W_G2J = 3 * W_FP, 4 * W_FP, 6 * W_FP
AWR_TAB_WORDS = 9 * W_G2J


# ------------------------------------------------------------------------------------------------- the model
def model_lanes(G, n):
    """blsgpu_awr_lanes as include/blsgpu.h and DESIGN.md 4.2 state it."""
    if G == 0:
        return 1
    by_count = next((L for L in (64, 32, 16, 8) if G * L <= CAP), 1)
    mean = -(-n // G)
    by_size = 1 if mean <= 1 else next(L for L in (8, 16, 32, 64) if mean <= L or L == 64)
    return min(by_count, by_size)


def model_fold_lanes(G, max_parts):
    """Lanes per group of the fold: by the largest group's parts (one lane up to three), capped by the group count as
    blsgpu_sig_agg_lanes caps its lanes."""
    by_count = 64 if G * 64 <= CAP else next((L for L in (32, 16, 8) if G * L <= 2 * CAP), 1)
    by_size = 1 if max_parts <= 3 else next(L for L in (8, 16, 32, 64) if max_parts <= L or L == 64)
    return min(by_count, by_size)


def model_total(sizes, L, t):
    return sum(max(1, -(-s // (L * t))) for s in sizes) * L


def model_plan(sizes):
    """(L, t or None, part_first): t by a walk from 1 (the header bisects), parts by slicing each group."""
    G, n = len(sizes), sum(sizes)
    L = model_lanes(G, n)
    first = np.cumsum([0] + list(sizes)).tolist()
    if G == 0 or G * L > CAP:
        return L, None, first
    t = 1
    while model_total(sizes, L, t) > CAP:
        t += 1
    if max(sizes) <= L * t:
        return L, None, first
    parts = []
    for g, s in enumerate(sizes):
        parts += [first[g] + j for j in range(0, max(s, 1), L * t)]
    return L, t, parts + [n]


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.probe_awr_lanes.restype = lib.probe_chip_lanes.restype = lib.probe_fold_lanes.restype = ctypes.c_uint32
    lib.probe_awr_lanes.argtypes = lib.probe_fold_lanes.argtypes = [ctypes.c_uint32, ctypes.c_uint32]
    lib.probe_plan.argtypes = [ctypes.c_uint32, U32P, U32P, U32P, U32P]
    lib.probe_parts_layout.argtypes = [ctypes.c_uint64, ctypes.c_uint64, U64P]
    lib.probe_awr_work.argtypes = [ctypes.c_uint64] * 3 + [U64P]
    lib.probe_same_work.argtypes = [ctypes.c_uint64] * 4 + [U64P]
    lib.probe_awr_work.restype = lib.probe_same_work.restype = None
    return lib


def header_plan(probe, sizes):
    """(L, part_sets, part_first, group_part) of awr_parts::plan; the last two None when not split."""
    G = len(sizes)
    gf = np.cumsum([0] + list(sizes)).astype(np.uint32)
    out = np.zeros(4, np.uint32)
    pf, gp = np.full(max(G, CAP) + 2, 0xFFFFFFFF, np.uint32), np.full(G + 2, 0xFFFFFFFF, np.uint32)
    split = probe.probe_plan(G, gf.ctypes.data_as(U32P), out.ctypes.data_as(U32P), pf.ctypes.data_as(U32P),
                             gp.ctypes.data_as(U32P))
    assert split in (0, 1)
    L, part_sets, n_parts, L_fold = (int(x) for x in out)
    if not split:
        assert part_sets == 0 and n_parts == G and pf[0] == gp[0] == 0xFFFFFFFF and L_fold == 1
        return L, 0, None, None
    assert pf[n_parts + 1] == 0xFFFFFFFF and gp[G + 1] == 0xFFFFFFFF
    most = int(max(np.diff(gp[:G + 1])))  # the largest group's parts
    assert L_fold == model_fold_lanes(G, most) == probe.probe_fold_lanes(G, most)
    return L, part_sets, pf[:n_parts + 1].tolist(), gp[:G + 1].tolist()


def check_shape(probe, sizes):
    """Both implementations (the library's export, the header's plan) against the model, and the rule's properties."""
    from lodestar_amd import native

    sizes = list(sizes)
    G, n = len(sizes), sum(sizes)
    first = np.cumsum([0] + sizes).tolist()
    L, t, want = model_plan(sizes)
    part_sets, got = native.awr_parts(first)
    hL, h_sets, h_first, h_gp = header_plan(probe, sizes)
    assert native.awr_lanes(G, n) == hL == L
    assert part_sets == h_sets == (L * t if t else 0)
    assert got.tolist() == want
    n_parts = len(want) - 1
    assert (t is None) == (n_parts == G)  # not split <=> as many parts as groups
    if t is None:
        assert h_first is None and want == first
        return L, None, n_parts
    assert h_first == want
    assert n_parts * L <= CAP                                    # the parts fit the chip
    assert max(np.diff(want)) <= L * t                           # no lane above t sets
    assert t == 1 or model_total(sizes, L, t - 1) > CAP          # t is minimal
    assert set(first) <= set(want) and want == sorted(want)      # a refinement of group_first
    assert h_gp[0] == 0 and h_gp[-1] == n_parts
    for g in range(G):                                           # group g's parts start at its first set
        assert want[h_gp[g]] == first[g] and h_gp[g + 1] - h_gp[g] == max(1, -(-sizes[g] // (L * t)))
    return L, t, n_parts


# ------------------------------------------------------------------------------------------------- the rule
TABLE = [  # sizes, L, t (None: not split), parts
    ([65], 64, 1, 2),
    ([64], 64, None, 1),
    ([65, 1, 0, 130], 64, 1, 7),
    ([2] * 40 + [100], 8, 1, 53),
    ([24] * 10 + [100], 32, 1, 14),
    ([1] * 8193 + [5], 1, 1, 8198),
    ([128] * 128, 64, 1, 256),
    ([64] * 128, 64, None, 128),
    ([1] * 16384, 1, None, 16384),
    ([16384], 64, 1, 256),
    ([1 << 20], 64, 16, 1024),
    ([65] * 1024, 64, None, 1024),          # the cap binds: t = 2 and no group above 128 sets
    ([1] * 70000 + [9], 1, None, 70001),    # G L > cap
]


@pytest.mark.parametrize("case", range(len(TABLE)))
def test_table(probe, case):
    sizes, L, t, parts = TABLE[case]
    assert check_shape(probe, sizes) == (L, t, parts)
    if sizes == [128] * 128:
        assert parts * L == 16384
    if sizes == [1 << 20]:
        assert parts * L == CAP


def test_shapes_of_the_gpu_tests(probe):
    assert check_shape(probe, [10] * 20 + [100])[:2] == (16, 1)
    assert check_shape(probe, [1] * 4096 + [4096]) == (8, 1, 4096 + 512)
    assert check_shape(probe, [1024] * 16) == (64, 1, 256)
    assert check_shape(probe, [1] * 300)[1] is None


def test_random_shapes(probe):
    rng = random.Random(4242)
    n_split = n_t_above_1 = 0
    for trial in range(300):
        kind = trial % 6
        if kind == 0:    # a few groups, some large, some empty
            sizes = [rng.choice([0, 0, 1, 2, 63, 64, 65, 129, 1000, 5000]) for _ in range(rng.randint(1, 12))]
        elif kind == 1:  # many small groups and one or two large ones
            sizes = [rng.randint(0, 3) for _ in range(rng.randint(1, 3000))] + [rng.randint(50, 20000)]
            rng.shuffle(sizes)
        elif kind == 2:  # G L just below, at and above the cap
            L = rng.choice([8, 16, 32, 64])
            G = CAP // L + rng.choice([-1, 0, 1])
            sizes = [rng.randint(max(1, L // 2), L) for _ in range(G)]
            sizes[rng.randrange(G)] = rng.choice([L, L + 1, 3 * L, 10 * L])
        elif kind == 3:  # the cap binds: t > 1
            sizes = [rng.randint(100000, 400000) for _ in range(rng.randint(1, 2))] + \
                    [rng.randint(0, 200) for _ in range(rng.randint(0, 50))]
        elif kind == 4:  # sizes exactly L t and L t + 1 for the shape's own L and t
            base = [rng.randint(1, 300) for _ in range(rng.randint(1, 40))] + [rng.randint(1000, 50000)]
            L, t, _ = model_plan(base)
            sizes = base + [L * (t or 1), L * (t or 1) + 1]
        else:            # uniform groups
            sizes = [rng.choice([1, 2, 8, 9, 64, 65, 128, 1000])] * rng.randint(1, 1200)
        if sum(sizes) > MAX_SETS:
            continue
        _, t, _ = check_shape(probe, sizes)
        n_split += t is not None
        n_t_above_1 += (t or 0) > 1
    assert n_split > 100 and n_t_above_1 > 20


def test_no_groups_and_empty_groups(probe):
    from lodestar_amd import native

    assert check_shape(probe, []) == (1, None, 0)
    assert check_shape(probe, [0]) == (1, None, 1)
    assert check_shape(probe, [0, 0, 0]) == (1, None, 3)
    assert check_shape(probe, [0, 200, 0])[1:] == (1, 6)  # an empty group is one empty part
    sets, first = native.awr_parts([0])
    assert sets == 0 and first.tolist() == [0]


def test_refusals():
    from lodestar_amd import native

    lib = native.load()
    ps, npart = ctypes.c_uint32(7), ctypes.c_uint32(7)
    out = np.full(CAP + 1, 0xABABABAB, np.uint32)

    def call(G, gf, ps=ps, npart=npart, out=out):
        g = None if gf is None else np.asarray(gf, np.uint32)
        return lib.blsgpu_awr_parts(G, None if g is None else g.ctypes.data, None if ps is None else ctypes.addressof(ps),
                                    None if npart is None else ctypes.addressof(npart),
                                    None if out is None else out.ctypes.data)

    assert call(1, None) == native.ERR_ARGS                            # null group_first with groups
    assert call(2, [0, 1, 4], ps=None) == native.ERR_ARGS              # null part_sets
    assert call(2, [0, 1, 4], npart=None) == native.ERR_ARGS           # null n_parts
    assert call(2, [1, 2, 4]) == native.ERR_ARGS                       # not from 0
    assert call(2, [0, 3, 2]) == native.ERR_ARGS                       # decreasing
    assert call(2, [0, 1, MAX_SETS + 1]) == native.ERR_ARGS            # too many sets
    assert (ps.value, npart.value) == (7, 7) and (out == 0xABABABAB).all()  # nothing written
    assert call(1, [0, MAX_SETS]) == native.OK and (ps.value, npart.value) == (64 * 16, 1024)
    assert call(2, [0, 1, 4], out=None) == native.OK and (ps.value, npart.value) == (0, 2)  # part_first is optional
    assert call(0, None) == native.OK and (ps.value, npart.value) == (0, 0) and out[0] == 0
    assert call(0, [7]) == native.OK  # no groups: accepted before group_first is read, as the calls described accept it
    with pytest.raises(ValueError, match="ERR_ARGS"):
        native.awr_parts([0, 3, 2])
    with pytest.raises(ValueError):
        native.awr_parts([])


# -------------------------------------------------------------------------------------- the lane rule it builds on
def test_awr_lanes_unchanged(probe):
    from lodestar_amd import native

    assert probe.probe_chip_lanes() == CAP
    counts = [0, 1, 2, 3, 7, 8, 64, 1023, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385, 65536, 1 << 20]
    sets = [0, 1, 2, 3, 4, 8, 9, 16, 17, 32, 33, 63, 64, 65, 129, 1000, 16384, 16385, 65536, 1 << 20]
    for G in counts:
        for n in sets:
            assert native.awr_lanes(G, n) == probe.probe_awr_lanes(G, n) == model_lanes(G, n), (G, n)
    spot = {(1, 1): 1, (1, 2): 8, (128, 16384): 64, (128, 8192): 64, (1024, 65536): 64, (1025, 65536): 32,
            (2048, 65536): 32, (2049, 1 << 20): 16, (8192, 1 << 20): 8, (8193, 1 << 20): 1, (16384, 16384): 1,
            (41, 180): 8, (21, 300): 16, (11, 340): 32}
    for (G, n), L in spot.items():
        assert native.awr_lanes(G, n) == L, (G, n)


def test_fold_lanes(probe):
    """The fold's lanes: for one group, or equal groups, what blsgpu_sig_agg_lanes gives that many parts per group; in a
    skewed call the largest group decides, up to the cap by group count."""
    from lodestar_amd import native

    for parts in (1, 2, 3, 4, 8, 9, 10, 16, 17, 18, 32, 33, 65, 256, 1024):
        assert probe.probe_fold_lanes(1, parts) == native.sig_agg_lanes(1, parts) == model_fold_lanes(1, parts)
        for G in (2, 16, 128, 1024, 1025, 4096, 4097, 8192, 8193, 16384, 16385, 65536):
            assert probe.probe_fold_lanes(G, parts) == model_fold_lanes(G, parts), (G, parts)
            if G * parts <= CAP:
                assert probe.probe_fold_lanes(G, parts) == native.sig_agg_lanes(G, G * parts), (G, parts)
    want = {(1, 10): 16, (1, 18): 32, (1, 65): 64, (1, 1024): 64, (16, 16): 16, (128, 2): 1, (4097, 512): 16,
            (41, 13): 16, (8194, 5): 8, (20000, 100): 1}
    for (G, parts), L in want.items():
        assert probe.probe_fold_lanes(G, parts) == L, (G, parts)


# ------------------------------------------------------------------------------------------------------ layouts
PARTS_FIELDS = ["sum_pk", "sum_sig", "ek", "pf", "gp", "ec", "total", "total_words"]


def al256(x):
    return (x + 255) & ~255


def launch_lanes(n_parts, L):
    return -(-n_parts * L // 64) * 64


def test_headers_are_hip_free():
    want = {HDRS[0]: ["<stddef.h>", "<stdint.h>", "<vector>"], HDRS[1]: ["<stddef.h>", "<stdint.h>"]}
    for path, incs in want.items():
        src = open(path).read()
        assert sorted(ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")) == incs


def test_parts_layout(probe):
    """Byte regions in the documented order, each on a 256-byte boundary, none overlapping the next, all inside the
    total, which is a whole number of words (the buffer is a word buffer)."""
    rng = np.random.default_rng(7)
    shapes = [(1, 2), (1, 256), (4, 7), (128, 256), (4097, 4608), (1, 1024), (8194, 8198), (65535, 65536)]
    shapes += [(G, G + int(rng.integers(1, CAP - G + 1))) for G in (int(g) for g in rng.integers(1, 60000, 100))]
    out = (ctypes.c_uint64 * 16)()
    for G, P in shapes:
        assert probe.probe_parts_layout(G, P, out) == len(PARTS_FIELDS)
        got = dict(zip(PARTS_FIELDS, out[:len(PARTS_FIELDS)]))
        at = 0
        for f, size in zip(PARTS_FIELDS[:6], [P * W_G1J * 4, P * W_G2J * 4, 2 * P * 4, (P + 1) * 4, (G + 1) * 4, 2 * P]):
            off = got[f]
            assert off % 256 == 0 and at <= off < at + 256, (G, P, f)
            at = off + size
        assert got["sum_pk"] == 0
        assert at <= got["total"] == al256(at) and got["total_words"] * 4 == got["total"]


@pytest.mark.parametrize("sizes", [[65], [65, 1, 0, 130], [2] * 40 + [100], [128] * 128, [16384], [1] * 4096 + [4096]])
def test_call_layouts_at_the_parts_lanes(probe, sizes):
    """hl::Awr and hl::Same of a split call: the call's own G and n, and window scratch for the parts' launched lanes,
    by the formulas tests/test_helper_layout.py holds for any lane count."""
    G, n = len(sizes), sum(sizes)
    L, t, n_parts = check_shape(probe, sizes)
    assert t is not None
    lanes = launch_lanes(n_parts, L)
    assert lanes % 64 == 0 and n_parts * L <= lanes < n_parts * L + 64 and lanes > launch_lanes(G, L) - 64
    out = (ctypes.c_uint64 * 8)()
    probe.probe_awr_work(G, n, lanes, out)
    tab = n * W_G2A
    assert list(out[:4]) == [tab, tab + lanes * AWR_TAB_WORDS, tab + lanes * AWR_TAB_WORDS + G * W_G1J,
                             tab + lanes * AWR_TAB_WORDS + G * (W_G1J + W_G2J)]
    probe.probe_same_work(G, n, G, lanes, out)
    assert list(out[:4]) == [tab, tab + lanes * AWR_TAB_WORDS, tab + 2 * lanes * AWR_TAB_WORDS,
                             tab + 2 * lanes * AWR_TAB_WORDS + G * W_G1J]
    assert out[4] > out[3] + G * W_G2J


# -------------------------------------------------------------------------------------------- symbol and header
def test_symbols_and_header():
    from lodestar_amd import native

    lib = ctypes.CDLL(native.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    assert "blsgpu_awr_parts" in native.EXPORTED_SYMBOLS and lib.blsgpu_awr_parts is not None
    assert ("int blsgpu_awr_parts(uint32_t n_groups, const uint32_t* group_first, uint32_t* part_sets, "
            "uint32_t* n_parts,") in src
    assert "uint32_t blsgpu_awr_lanes(uint32_t n_groups, uint32_t n_sets);" in src
    assert "#define BLSGPU_ABI_VERSION 8" in src
    head = src[src.index("Entry points added since 8"): src.index("#define BLSGPU_ABI_VERSION")]
    assert "blsgpu_awr_parts" in head
    assert src.count("see blsgpu_awr_parts; never changes an answer") == 2
