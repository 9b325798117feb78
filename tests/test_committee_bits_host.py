"""Host side of the committee store and blsgpu_aggregate_pubkeys_bits, no GPU needed: the host plan
(lodestar_amd/csrc/committee_plan.hpp through tests/native/committee_plan_probe.cpp) -- the mode rule, popcounts, item
counts, the lane rule, every refusal --, the arena layout hl::AggPubkeysBits, the per-set core the kernel runs per lane
(committee_bits.hpp, compiled for the host by tests/native/committee_bits_probe.cpp) against the oracle, the exported
symbols and the header, the refusals the library decides before any device is needed, and one run of the core's probe
as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from tests import committee_bits_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "lodestar_amd", "csrc")
PLAN_SRC = os.path.join(HERE, "native", "committee_plan_probe.cpp")
PLAN_LIB = os.path.join(HERE, "native", "libcommittee_plan_probe.so")
CORE_SRC = os.path.join(HERE, "native", "committee_bits_probe.cpp")
CORE_LIB = os.path.join(HERE, "native", "libcommittee_bits_probe.so")
ERR_ARGS, COMPLEMENT = 100, 0x80000000
vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64


def built(src, out):
    deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", out, src])
    return ctypes.CDLL(out)


@pytest.fixture(scope="module")
def planlib():
    lib = built(PLAN_SRC, PLAN_LIB)
    lib.probe_mode.argtypes = [u32, u32, u32]
    lib.probe_mode.restype = u32
    lib.probe_lanes.argtypes = [u32, u64]
    lib.probe_lanes.restype = u32
    lib.probe_popcount.argtypes = [vp, u64, u64, u32]
    lib.probe_popcount.restype = u32
    lib.probe_check_upload.argtypes = [u32, u32, vp, vp, u32, u32]
    lib.probe_check_call.argtypes = [u32, vp, vp, vp, vp, u32, vp, u32, vp]
    lib.probe_plan.argtypes = [u32, vp, vp, vp, vp, u32, vp, u32, vp, vp, vp]
    lib.probe_agg_pubkeys_bits.argtypes = [u64, u64, u64, u64, vp]
    return lib


@pytest.fixture(scope="module")
def corelib():
    lib = built(CORE_SRC, CORE_LIB)
    lib.probe_committee_bits.argtypes = [vp, u32, u32, vp, vp, u32, vp, vp, u32, u32, u32, u32, vp, vp]
    return lib


def ptr(a):
    return None if a is None else a.ctypes.data


def run_plan(lib, committees, sets, flags=0, arrays=None):
    """(code, counts dict, seg_desc, present_first) of the host plan for `sets` over `committees`."""
    ssf, seg, sbf, bits = arrays if arrays is not None else H.call_arrays(sets)
    cf = np.cumsum([0] + [len(c) for c in committees]).astype(np.uint32)
    n = len(ssf) - 1
    counts = np.zeros(8, np.uint64)
    desc, present = np.zeros(max(len(seg), 1), np.uint32), np.zeros(n + 1, np.uint32)
    pad = lambda a, t: a if len(a) else np.zeros(1, t)  # noqa: E731
    rc = lib.probe_plan(n, ptr(ssf), ptr(pad(seg, np.uint32)), ptr(sbf), ptr(pad(bits, np.uint8)), flags, ptr(cf),
                        len(committees), ptr(counts), ptr(desc), ptr(present))
    names = ["segments", "segments_complemented", "keys_present", "keys_added", "keys_subtracted", "lanes", "n_items",
             "bits_bytes"]
    return rc, dict(zip(names, (int(x) for x in counts))), desc[: len(seg)], present


def test_mode_rule(planlib):
    """Complement iff absent + 1 < present, at every (size, present) for sizes <= 65 and at 512; never under the flag."""
    for size in list(range(0, 66)) + [512]:
        for present in range(size + 1):
            want = 1 if (size - present) + 1 < present else 0
            assert planlib.probe_mode(size, present, 0) == want, (size, present)
            assert planlib.probe_mode(size, present, H.NO_COMPLEMENT) == 0
    assert planlib.probe_mode(512, 486, 0) == 1 and planlib.probe_mode(512, 257, 0) == 1
    assert planlib.probe_mode(512, 256, 0) == 0 and planlib.probe_mode(3, 2, 0) == 0 and planlib.probe_mode(2, 2, 0) == 1
    assert planlib.probe_mode(4, 5, 0) == 0  # more participants than members: not a segment, never complemented


def test_popcounts_with_tails_and_padding(planlib):
    rng = np.random.default_rng(11)
    bits = rng.random(1203) < 0.6
    buf = np.frombuffer(H.pack(bits), np.uint8)
    for pos, count in [(0, 0), (0, 1), (0, 7), (0, 8), (0, 9), (3, 29), (3, 32), (3, 33), (5, 64), (7, 65), (31, 512),
                       (1, 1202), (0, 1203), (1200, 3), (1202, 1)] + [tuple(int(x) for x in rng.integers(0, 600, 2))
                                                                      for _ in range(40)]:
        assert planlib.probe_popcount(ptr(buf), len(buf), pos, count) == int(bits[pos: pos + count].sum()), (pos, count)
    # bits past the string's end read as zero
    assert planlib.probe_popcount(ptr(buf), len(buf), 1200, 64) == int(bits[1200:].sum())


def mixed_call(rng):
    """Sets of 0, 1, 2, 3 and 64 segments over the size committees, direct and complement segments mixed."""
    cm = H.size_committees()
    sets = [[]]
    for n_seg in (1, 2, 3, 64, 1, 2):
        s = []
        for k in range(n_seg):
            c = int(rng.integers(0, len(cm)))
            frac = (0.0, 0.3, 0.95, 1.0)[(k + n_seg) % 4]
            s.append((c, rng.random(len(cm[c])) < frac))
        sets.append(s)
    return cm, sets


def test_item_counts_and_descriptors(planlib):
    rng = np.random.default_rng(5)
    cm, sets = mixed_call(rng)
    for flags in (0, H.NO_COMPLEMENT):
        rc, got, desc, present = run_plan(planlib, cm, sets, flags)
        want = H.plan(cm, sets, no_complement=bool(flags))
        assert rc == 0
        assert {k: got[k] for k in want} == want
        assert got["lanes"] == H.lanes_rule(len(sets), want["n_items"])
        assert got["bits_bytes"] == sum((sum(len(b) for _, b in s) + 7) // 8 for s in sets)
        k = 0
        for i, s in enumerate(sets):
            assert present[i + 1] - present[i] == sum(int(np.count_nonzero(b)) for _, b in s)
            for c, b in s:
                comp = not flags and len(b) - int(b.sum()) + 1 < int(b.sum())
                assert desc[k] == (c | (COMPLEMENT if comp else 0))
                k += 1
        if flags:
            assert got["segments_complemented"] == 0 and got["keys_subtracted"] == 0
        else:
            assert got["segments_complemented"] > 0 and got["keys_subtracted"] > 0 and got["keys_added"] > 0


def test_lane_rule(planlib):
    for n_items in (0, 1, 8, 9, 1000, 32768 * 27, 32768 * 486, 1 << 31):
        prev = 64
        for n_sets in [1, 2, 3, 7, 64, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 32768,
                       1 << 20]:
            L = planlib.probe_lanes(n_sets, n_items)
            assert L == H.lanes_rule(n_sets, n_items) and L in (8, 16, 32, 64)
            assert L <= prev, (n_sets, n_items)  # non-increasing in n_sets
            prev = L
    # every form is reachable, by the mean items of a set and by the set count
    assert [planlib.probe_lanes(4, 4 * m) for m in (8, 16, 32, 33)] == [8, 16, 32, 64]
    assert [planlib.probe_lanes(n, n * 500) for n in (1024, 4096, 8192, 8193)] == [64, 32, 16, 8]
    assert planlib.probe_lanes(32768, 32768 * 27) == 8  # C4 as shipped


def test_call_refusals(planlib):
    cm = H.size_committees()
    rng = np.random.default_rng(9)
    sets = [[(2, rng.random(7) < 0.5)], [(3, np.ones(8, bool)), (4, rng.random(9) < 0.5)]]
    ssf, seg, sbf, bits = H.call_arrays(sets)
    assert run_plan(planlib, cm, sets)[0] == 0
    out, st = np.zeros(192, np.uint8), np.zeros(2, np.int8)
    ok = [2, ptr(ssf), ptr(seg), ptr(sbf), ptr(bits), 0, ptr(out), 96, ptr(st)]
    assert planlib.probe_check_call(*ok) == 0
    for pos in (1, 2, 3, 4, 6, 8):  # every pointer
        bad = list(ok)
        bad[pos] = None
        assert planlib.probe_check_call(*bad) == ERR_ARGS, pos
    for out_len in (0, 47, 49, 95, 97, 192):
        assert planlib.probe_check_call(*ok[:7], out_len, ok[8]) == ERR_ARGS
    for flags in (2, 3, 0x80000000):
        assert planlib.probe_check_call(*ok[:5], flags, *ok[6:]) == ERR_ARGS
    assert planlib.probe_check_call((1 << 20) + 1, *ok[1:]) == ERR_ARGS and planlib.probe_check_call(1 << 20, *ok[1:]) == 0

    def refused(ssf=ssf, seg=seg, sbf=sbf, bits=bits, n_committees=len(cm)):
        return run_plan(planlib, cm[:n_committees], None, 0, (ssf, seg, sbf, bits))[0] == ERR_ARGS

    assert refused(ssf=np.array([1, 1, 3], np.uint32))  # offsets do not start at 0
    assert refused(ssf=np.array([0, 2, 1], np.uint32))  # decreasing
    assert refused(sbf=np.array([1, 1, 4], np.uint32)) and refused(sbf=np.array([0, 2, 1], np.uint32))
    assert refused(seg=np.array([2, 3, len(cm)], np.uint32))  # a committee id >= the count
    assert refused(n_committees=4)                             # (an id the store has dropped)
    assert refused(sbf=np.array([0, 1, 5], np.uint32), bits=np.concatenate([bits, [0]]).astype(np.uint8))  # too long
    assert refused(sbf=np.array([0, 1, 3], np.uint32))  # too short
    assert refused(sbf=np.array([0, 2, 5], np.uint32), bits=np.concatenate([bits[:1], [0], bits[1:]]).astype(np.uint8))
    pad = bits.copy()
    pad[0] |= 0x80  # bit 7 of a 7-bit string
    assert refused(bits=pad)
    pad = bits.copy()
    pad[3] |= 0x02  # bit 17 of a 17-bit string
    assert refused(bits=pad)
    assert not refused()


def test_upload_refusals(planlib):
    cf, mem = np.array([0, 2, 3], np.uint32), np.array([4, 4, 9], np.uint32)
    ok = dict(first=3, n=2, cf=cf, mem=mem, count=3, table_n=10)

    def check(**kw):
        a = {**ok, **kw}
        return planlib.probe_check_upload(a["first"], a["n"], ptr(a["cf"]), ptr(a["mem"]), a["count"], a["table_n"])

    assert check() == 0 and check(first=0) == 0  # append, replace; members may repeat
    assert check(first=4) == ERR_ARGS  # beyond the count: a gap
    assert check(cf=None) == ERR_ARGS and check(mem=None) == ERR_ARGS
    assert check(n=0, cf=None, mem=None) == 0 and check(n=0, cf=None, mem=None, first=4) == ERR_ARGS
    assert check(cf=np.array([0, 2, 2], np.uint32)) == ERR_ARGS  # an empty committee
    assert check(cf=np.array([0, 0, 3], np.uint32)) == ERR_ARGS
    assert check(cf=np.array([1, 2, 3], np.uint32)) == ERR_ARGS  # not from 0
    assert check(cf=np.array([0, 3, 2], np.uint32)) == ERR_ARGS  # decreasing
    assert check(table_n=9) == ERR_ARGS and check(table_n=0) == ERR_ARGS  # a member >= the table's size
    big = np.zeros((1 << 20) + 1, np.uint32)
    assert check(n=1, cf=np.array([0, (1 << 20) + 1], np.uint32), mem=big) == ERR_ARGS
    assert check(n=1, cf=np.array([0, 1 << 20], np.uint32), mem=big) == 0


def test_layout(planlib):
    """hl::AggPubkeysBits: d_in fields in order, each on a 256-byte boundary and non-overlapping, status last (three
    bytes per set: k_pk_serialize's status | unused | the aggregation's); d_work a Jacobian sum per set."""
    fields = ["ssf", "seg", "sbf", "bits", "present", "out", "st", "total", "work_words"]
    rng = np.random.default_rng(3)
    shapes = [(1, 0, 0), (1, 1, 1), (3, 5, 7), (64, 64, 4096), (32768, 32768, 32768 * 64), (1 << 20, 1 << 22, 1 << 28)]
    shapes += [tuple(int(x) for x in rng.integers(1, 1 << 16, 3)) for _ in range(30)]
    for n, n_segs, nbytes in shapes:
        for out_len in (48, 96):
            buf = (ctypes.c_uint64 * 16)()
            k = planlib.probe_agg_pubkeys_bits(n, n_segs, nbytes, out_len, buf)
            assert k == len(fields)
            got = dict(zip(fields, buf[:k]))
            sizes = [("ssf", (n + 1) * 4), ("seg", n_segs * 4), ("sbf", (n + 1) * 4), ("bits", nbytes),
                     ("present", (n + 1) * 4), ("out", n * out_len), ("st", 3 * n)]
            at = 0
            for name, size in sizes:
                assert got[name] == at and at % 256 == 0, name
                end = at + size
                at = (end + 255) // 256 * 256
            assert got["total"] == end and got["work_words"] == n * 42


def core(lib, pk96, committees, segs, bits, flags, L, out_len):
    cf = np.cumsum([0] + [len(c) for c in committees]).astype(np.uint32)
    mem = np.array([i for c in committees for i in c], np.uint32)
    seg = np.array(segs, np.uint32)
    buf = np.frombuffer(H.pack(bits), np.uint8).copy()
    keys = np.frombuffer(pk96, np.uint8)
    out = np.full(out_len, 0x5A, np.uint8)
    comp = ctypes.c_uint32(99)
    st = lib.probe_committee_bits(ptr(keys), len(keys) // 96, len(committees), ptr(cf), ptr(mem), len(seg), ptr(seg),
                                  ptr(buf if len(buf) else np.zeros(1, np.uint8)), len(buf), flags, L, out_len,
                                  ptr(out), ctypes.byref(comp))
    return st, out.tobytes(), comp.value


@pytest.mark.parametrize("out_len", [48, 96])
def test_core_cancellation_against_the_oracle(corelib, out_len):
    """The kernel's per-lane text on the host, on 8 and on 64 lanes, with and without the flag: equal to each other and
    to the oracle on every cancellation case."""
    pk96 = H.table_pk96()
    for name, committee, bits, complemented in H.CANCELLATION:
        want, want_st = H.oracle_sums([[committee[i] for i in np.flatnonzero(bits)]], out_len)[0]
        for L in (8, 64):
            st, out, comp = core(corelib, pk96, [committee], [0], bits, 0, L, out_len)
            assert (st, out) == (want_st, want), (name, L)
            assert comp == (1 if complemented else 0), name
            st, out, comp = core(corelib, pk96, [committee], [0], bits, H.NO_COMPLEMENT, L, out_len)
            assert (st, out, comp) == (want_st, want, 0), (name, L, "flag")
    ident = H.identity(out_len)
    got = {name: H.oracle_sums([[c[i] for i in np.flatnonzero(b)]], out_len)[0][0] for name, c, b, _ in H.CANCELLATION}
    for name in ("sum_is_identity", "q_absent", "q_absent_complement", "absent_equals_sum",
                 "absent_equals_sum_complement", "opposite_across_lanes"):
        assert got[name] == ident, name
    assert got["double_direct"] == got["double_all"] == got["equal_across_lanes"] != ident


def test_core_sizes_against_the_oracle(corelib):
    """Committees of 7, 33 and 65 members and a two-segment set that uses one committee twice, around the tie."""
    pk96 = H.table_pk96()
    cm = H.size_committees()
    rng = np.random.default_rng(21)
    for ci in (2, 7, 10):
        c = cm[ci]
        for name, bits in H.participations(len(c), rng).items():
            want = H.oracle_sums([[c[i] for i in np.flatnonzero(bits)]], 96)[0]
            for flags in (0, H.NO_COMPLEMENT):
                st, out, _ = core(corelib, pk96, [c], [0], bits, flags, 8, 96)
                assert (out, st) == want, (len(c), name, flags)
    a, b = rng.random(33) < 0.9, rng.random(33) < 0.2
    want = H.oracle_sums([[cm[7][i] for i in np.flatnonzero(a)] + [cm[7][i] for i in np.flatnonzero(b)]], 48)[0]
    for flags, comp_want in ((0, 1), (H.NO_COMPLEMENT, 0)):
        st, out, comp = core(corelib, pk96, [cm[7]], [0, 0], np.concatenate([a, b]), flags, 16, 48)
        assert (out, st) == want and comp == comp_want


def test_symbols_and_header():
    from lodestar_amd import native

    lib = ctypes.CDLL(native.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    names = ("blsgpu_committees_upload", "blsgpu_committees_count", "blsgpu_aggregate_pubkeys_bits",
             "blsgpu_committee_bits_mode", "blsgpu_committee_bits_lanes")
    head = src[src.index("Entry points added since 8"): src.index("#define BLSGPU_ABI_VERSION")]
    for name in names:
        assert name in native.EXPORTED_SYMBOLS and getattr(lib, name) is not None and name in head
    assert "int blsgpu_committees_upload(blsgpu_ctx* ctx, uint32_t first_committee, uint32_t n," in src
    assert "uint32_t blsgpu_committees_count(const blsgpu_ctx* ctx);" in src
    assert "int blsgpu_aggregate_pubkeys_bits(blsgpu_ctx* ctx, uint32_t n_sets, const uint32_t* set_seg_first" in src
    assert "#define BLSGPU_BITS_NO_COMPLEMENT 1u" in src and native.BITS_NO_COMPLEMENT == 1
    assert "#define BLSGPU_ABI_VERSION 8" in src
    for ref in ("getAttestingIndices", "getSyncCommitteeSignatureSet", "chain/bls/utils.ts:5-16"):
        assert ref in src
    # the struct as the header declares it
    assert [f for f, _ in native.CommitteeBitsStats._fields_] == ["segments", "segments_complemented", "keys_present",
                                                                  "keys_added", "keys_subtracted", "lanes", "device_ms"]
    assert ctypes.sizeof(native.CommitteeBitsStats) == 32


def test_pure_host_entry_points(planlib):
    from lodestar_amd import native

    for size, present in [(512, 486), (512, 256), (512, 257), (3, 2), (2, 2), (1, 1), (1, 0), (65, 33), (65, 34)]:
        for flags in (0, 1):
            assert native.committee_bits_mode(size, present, flags) == planlib.probe_mode(size, present, flags)
    for n_sets, n_items in [(1, 0), (4, 100), (4, 140), (1024, 1 << 20), (8193, 1 << 22), (32768, 32768 * 27)]:
        assert native.committee_bits_lanes(n_sets, n_items) == planlib.probe_lanes(n_sets, n_items)


def test_refusals_before_any_device_is_needed():
    """A null context is refused with BLSGPU_ERR_ARGS whatever else is passed, and nothing is written.  The checks that
    need a context (offsets, ids, bit strings, the store's own) run on the GPU: tests/test_gpu_committee_bits.py."""
    from lodestar_amd import native

    lib = native.load()
    ssf, seg, sbf = np.array([0, 1], np.uint32), np.array([0], np.uint32), np.array([0, 1], np.uint32)
    bits = np.array([1], np.uint8)
    out, st = np.full(96, 0x5A, np.uint8), np.full(1, 77, np.int8)
    stats = native.CommitteeBitsStats()
    stats.lanes = 1234
    for n, flags, out_len in [(1, 0, 96), (1, 0, 48), (1, 2, 96), (1, 0, 95), (0, 0, 96)]:
        rc = lib.blsgpu_aggregate_pubkeys_bits(None, n, ptr(ssf), ptr(seg), ptr(sbf), ptr(bits), flags, ptr(out),
                                               out_len, ptr(st), ctypes.byref(stats))
        assert rc == native.ERR_ARGS, (n, flags, out_len)
    assert (out == 0x5A).all() and st[0] == 77 and stats.lanes == 1234
    cf, mem = np.array([0, 1], np.uint32), np.array([0], np.uint32)
    assert lib.blsgpu_committees_upload(None, 0, 1, ptr(cf), ptr(mem)) == native.ERR_ARGS
    assert lib.blsgpu_committees_upload(None, 0, 0, None, None) == native.ERR_ARGS
    assert lib.blsgpu_committees_count(None) == 0


def test_probe_program_under_sanitizers(tmp_path):
    """The core's probe built stand-alone (its own main) with -fsanitize=address,undefined and run over the oracle's
    keys: host code only -- no device code and nothing loaded into Python is covered."""
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "one"), str(one)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "one")], capture_output=True).returncode != 0:
        pytest.skip("no sanitized host build here")  # (as tests/test_run_plan.py: not even an empty program runs)
    exe = tmp_path / "committee_bits_probe"
    subprocess.check_call(["g++", *flags, "-DCOMMITTEE_BITS_PROBE_MAIN", "-o", str(exe), CORE_SRC])
    path = tmp_path / "keys96.bin"
    path.write_bytes(H.table_pk96()[: 96 * 80])
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    # 7 committees (1, 2, 7, 8, 9, 33, 65 members) x 4 patterns.  Complemented under absent + 1 < present: all bits set,
    # sizes >= 2: 6; first bit clear, sizes >= 4: 5; every other bit: 0; every fifth bit clear over the sets (c, c + 1)
    # and the last committee alone: the 2 of (1, 2), both segments of the five other pairs, the last one: 1 + 10 + 1
    assert r.stdout.splitlines() == ["28 sets, 23 segments complemented, 28 equal under the flag"]
