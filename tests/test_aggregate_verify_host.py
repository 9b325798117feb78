"""Host side of batched AggregateVerify, no GPU needed: the exported symbols, header lines, flags and stats struct,
the form rule blsgpu_aggregate_verify_form, the null-context refusal, the addon's export, and -- through
tests/native/aggverify_probe.cpp, which compiles the two HIP-free headers alone -- hl::AggVerify (fields disjoint and
aligned) and the Miller plan of csrc/aggverify_plan.hpp (chunks never span jobs, a planned job's last item is its
signature item, chunk counts for the sizes the GPU test uses with 1 and 8 items per chunk)."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "lodestar_amd", "csrc")
SRC = os.path.join(HERE, "native", "aggverify_probe.cpp")
LIB = os.path.join(HERE, "native", "libaggverify_probe.so")
HDRS = [os.path.join(CSRC, h) for h in ("aggverify_plan.hpp", "miller_plan.hpp", "helper_layout.hpp")]
SIZES = [0, 1, 2, 7, 8, 9, 16, 17, 63, 64, 65, 130]
U32P = ctypes.POINTER(ctypes.c_uint32)


# ------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_header_flags_and_stats():
    from lodestar_amd import native

    lib = ctypes.CDLL(native.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    for name in ("blsgpu_aggregate_verify", "blsgpu_aggregate_verify_form"):
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
        assert f" {name}(" in src
    assert "#define BLSGPU_AV_VALIDATE_KEYS 1u" in src and native.AV_VALIDATE_KEYS == 1
    assert "#define BLSGPU_AV_LANE_FORMS 2u" in src and native.AV_LANE_FORMS == 2
    assert "#define BLSGPU_ABI_VERSION 8" in src
    assert "} blsgpu_aggregate_verify_stats;" in src
    # the additions since ABI 8 are named in the comment above the version
    head = src[: src.index("#define BLSGPU_ABI_VERSION")]
    assert "blsgpu_aggregate_verify," in head and "blsgpu_aggregate_verify_form" in head
    # six uint32 and a double: 32 bytes, device_ms at 24
    st = native.AggregateVerifyStats
    assert ctypes.sizeof(st) == 32 and st.device_ms.offset == 24
    assert [f for f, _ in st._fields_] == ["pairs", "unique_messages", "miller_items", "miller_chunks", "form",
                                           "jobs_checked", "device_ms"]


def test_form_rule():
    from lodestar_amd import native

    f = native.aggregate_verify_form
    assert [f(n) for n in (0, 1, 393, 511, 512)] == [0] * 5
    assert [f(n) for n in (513, 4096, 1 << 20)] == [1] * 3
    assert [f(n, native.AV_LANE_FORMS) for n in (0, 1, 512, 513)] == [1] * 4
    assert f(512, native.AV_VALIDATE_KEYS) == 0 and f(513, native.AV_VALIDATE_KEYS) == 1
    # the same rule as the same-message call's
    for n in (0, 1, 511, 512, 513, 70000):
        assert f(n) == native.same_message_form(n)
        assert f(n, native.AV_LANE_FORMS) == native.same_message_form(n, native.SAME_LANE_FORMS)


def test_null_context_is_refused_before_anything_is_read():
    from lodestar_amd import native

    lib = native.load()
    res = np.full(2, 77, np.int8)
    a = np.zeros(64, np.uint32)
    b = np.zeros(512, np.uint8)
    rc = lib.blsgpu_aggregate_verify(None, 1, a.ctypes.data, b.ctypes.data, b.ctypes.data, 96, None, b.ctypes.data, 96,
                                     a.ctypes.data, 0, res.ctypes.data, None, None)
    assert rc == native.ERR_ARGS and list(res) == [77, 77]


def test_wrapper_refuses_malformed_layouts():
    from lodestar_amd import native

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called ({name}) for a malformed layout")

    c = native.Context.__new__(native.Context)
    c._lib, c.h = NoLibrary(), None
    ok = dict(job_first=[0, 2], msgs=bytes(64), sigs=bytes(96), pk_bytes=bytes(192))
    for kw, match in [
        (dict(job_first=[]), "job_first"), (dict(job_first=[1, 2]), "start at 0"),
        (dict(job_first=[0, 2, 1]), "never decrease"), (dict(job_first=[0, (1 << 20) + 1]), "at most"),
        (dict(msgs=bytes(32)), "message bytes"), (dict(pk_bytes=None), "exactly one of"),
        (dict(pk_index=[0, 1]), "exactly one of"), (dict(pk_bytes=bytes(96)), "pubkey bytes"),
        (dict(pk_bytes=bytes(96), pk_len=48), "pk_len"),
        (dict(pk_bytes=None, pk_index=[0, 1], flags=native.AV_VALIDATE_KEYS), "AV_VALIDATE_KEYS"),
        (dict(pk_bytes=None, pk_index=[0]), "one entry per pair"), (dict(sig_stride=95), "sig_stride"),
        (dict(sig_len=[192]), "192-byte signature"), (dict(sig_len=[96, 96]), "one entry per signature"),
    ]:
        with pytest.raises(ValueError, match=match):
            c.aggregate_verify(**{**ok, **kw})


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_node_addon_exports_aggregate_verify():
    script = (
        "const m = require(process.argv[1]);"
        "if (typeof m.addon.aggregateVerify !== 'function') throw new Error('missing addon.aggregateVerify');"
        "if (typeof m.aggregateVerify !== 'function') throw new Error('missing aggregateVerify');"
        "if (typeof m.BlsGpuVerifier.prototype.aggregateVerifyJobs !== 'function') throw new Error('missing aggregateVerifyJobs');"
        "if (m.AV_VALIDATE_KEYS !== 1 || m.AV_LANE_FORMS !== 2) throw new Error('flags');"
        "console.log('ok');"
    )
    out = subprocess.run([NODE, "-e", script, os.path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    esm = ("import('" + os.path.join(ROOT, "lodestar_amd", "node", "index.js") + "').then((m) => {"
           "if (typeof m.aggregateVerify !== 'function' || m.AV_LANE_FORMS !== 2) throw new Error('esm export');"
           "console.log('ok'); }).catch((e) => { console.error(e); process.exit(1); });")
    out = subprocess.run([NODE, "-e", esm], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr


# --------------------------------------------------------------------------------- the HIP-free layout and plan
@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    lib.probe_form.restype = ctypes.c_uint32
    lib.probe_chunk_items.restype = ctypes.c_uint32
    lib.probe_plan.restype = ctypes.c_uint32
    lib.probe_layout.restype = ctypes.c_uint32
    lib.probe_layout.argtypes = [ctypes.c_uint64] * 5 + [ctypes.c_int, ctypes.c_uint64, ctypes.c_int,
                                                        ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]
    return lib


def test_headers_are_hip_free():
    for h in HDRS:
        includes = [ln.split()[1] for ln in open(h).read().splitlines() if ln.startswith("#include")]
        assert all("hip" not in i for i in includes), (h, includes)
        assert all(i.startswith("<") or i == '"miller_plan.hpp"' for i in includes), (h, includes)


def plan(probe, sizes, k, planned=None):
    jf = np.cumsum([0] + list(sizes)).astype(np.uint32)
    n, J = int(jf[-1]), len(sizes)
    cf = np.zeros(n + J + 1, np.uint32)
    ci = np.zeros(n + J, np.uint32)
    fr = np.zeros(2 * J, np.uint32)
    ni = ctypes.c_uint32(0)
    pl = None if planned is None else np.asarray(planned, np.uint8)
    nc = probe.probe_plan(jf.ctypes.data_as(U32P), J, None if pl is None else pl.ctypes.data_as(ctypes.c_void_p),
                          k, cf.ctypes.data_as(U32P), ci.ctypes.data_as(U32P), fr.ctypes.data_as(U32P), ctypes.byref(ni))
    cnt = np.zeros(3, np.uint32)
    probe.probe_count(jf.ctypes.data_as(U32P), J, None if pl is None else pl.ctypes.data_as(ctypes.c_void_p), k,
                      cnt.ctypes.data_as(U32P))
    return jf, cf[: nc + 1].tolist(), ci[: ni.value].tolist(), fr.reshape(J, 2).tolist(), [int(x) for x in cnt]


def check_plan(sizes, k, jf, cf, ci, fr, cnt, planned=None):
    n, J = int(jf[-1]), len(sizes)
    is_planned = [(s > 0) if planned is None else bool(planned[j]) for j, s in enumerate(sizes)]
    assert cf[0] == 0 and cf[-1] == len(ci) and all(a < b for a, b in zip(cf, cf[1:]))
    want_items, c = [], 0
    for j in range(J):
        a, e = fr[j]
        assert a == c, "the jobs' chunk ranges follow each other"
        if not is_planned[j]:
            assert a == e
            continue
        items = list(range(int(jf[j]), int(jf[j + 1]))) + [n + j]
        assert e - a == -(-len(items) // k)
        got = ci[cf[a]: cf[e]]
        assert got == items, "the job's pairs in order, then its signature item"
        assert got[-1] == n + j
        for q in range(a, e):  # a chunk never spans two jobs and holds at most k items
            assert 1 <= cf[q + 1] - cf[q] <= k
            assert cf[a] <= cf[q] and cf[q + 1] <= cf[e]
        want_items += items
        c = e
    assert ci == want_items and len(cf) - 1 == c
    assert cnt == [sum(is_planned), len(want_items), c]


@pytest.mark.parametrize("k", [1, 8])
def test_plan_for_the_gpu_tests_sizes(probe, k):
    jf, cf, ci, fr, cnt = plan(probe, SIZES, k)
    check_plan(SIZES, k, jf, cf, ci, fr, cnt)
    assert cnt[0] == 11 and cnt[1] == 393
    per_job = [0 if s == 0 else -(-(s + 1) // k) for s in SIZES]
    assert [e - a for a, e in fr] == per_job
    assert cnt[2] == (393 if k == 1 else sum([1, 1, 1, 2, 2, 3, 3, 8, 9, 9, 17])) == sum(per_job)


@pytest.mark.parametrize("k", [1, 2, 8])
def test_plan_shapes_and_masks(probe, k):
    for sizes in ([], [0], [0, 0, 0], [1], [7], [8], [3, 0, 5, 0], [1] * 70, [256] * 3, [15, 16, 17, 23, 24, 25]):
        check_plan(sizes, k, *plan(probe, sizes, k))
    sizes = [3, 0, 5, 9, 1]
    for mask in ([1, 0, 1, 1, 1], [0, 0, 1, 0, 1], [0] * 5, [1, 0, 0, 0, 0]):
        jf, cf, ci, fr, cnt = plan(probe, sizes, k, mask)
        check_plan(sizes, k, jf, cf, ci, fr, cnt, mask)


def test_form_and_chunk_size(probe):
    assert [probe.probe_form(n, 0) for n in (0, 512, 513)] == [0, 0, 1]
    assert [probe.probe_form(n, 1) for n in (0, 512)] == [1, 1]
    probe.probe_chunk_items.restype = ctypes.c_uint32

    def chunk_items(sizes, form, lane_flag):
        jf = np.cumsum([0] + list(sizes)).astype(np.uint32)
        return probe.probe_chunk_items(jf.ctypes.data_as(U32P), len(sizes), form, lane_flag)

    # cooperative: one item per accumulator; the flag: the largest calls' 8; otherwise the fewest items per accumulator
    # (of 1, 2, 4, 8) whose chunks still fit one lane each on the chip (65,536 lanes)
    assert chunk_items(SIZES, 0, 0) == 1
    assert chunk_items(SIZES, 1, 1) == 8 and chunk_items([1] * 16384, 1, 1) == 8
    assert chunk_items(SIZES, 1, 0) == 1
    assert chunk_items([1] * 16384, 1, 0) == chunk_items([4] * 4096, 1, 0) == chunk_items([256] * 64, 1, 0) == 1
    assert chunk_items([1] * 32768, 1, 0) == 1          # 65,536 items
    assert chunk_items([1] * 32769, 1, 0) == 2          # 65,538 items: pairs of items, 32,769 chunks
    assert chunk_items([255] * 256 + [1], 1, 0) == 2    # 65,538 items in 256 jobs of 256 and one of 2
    assert chunk_items([1023] * 128, 1, 0) == 2         # 131,072 items, 65,536 chunks of 2
    assert chunk_items([1023] * 129, 1, 0) == 4
    assert chunk_items([1023] * 256, 1, 0) == 4         # 262,144 items
    assert chunk_items([1023] * 257, 1, 0) == 8
    assert chunk_items([1] * (1 << 19), 1, 0) == 8      # every job two items: 524,288 chunks whatever k >= 2
    assert probe.probe_lane_reduce_max() == 8


@pytest.mark.parametrize("J,n,U,C,stride,bytes_,pk_len,validate", [
    (12, 382, 16, 393, 96, 1, 96, 0), (12, 382, 16, 56, 192, 0, 96, 0), (3, 9, 9, 12, 96, 1, 48, 1),
    (1, 0, 0, 0, 96, 1, 96, 0), (16384, 16384, 16384, 16384, 96, 1, 96, 1), (64, 16384, 300, 2112, 192, 0, 96, 0),
    (5, 7, 1, 12, 100, 1, 96, 1),
])
def test_layout_fields_are_disjoint_and_aligned(probe, J, n, U, C, stride, bytes_, pk_len, validate):
    out = (ctypes.c_uint64 * 120)()
    tot = (ctypes.c_uint64 * 6)()
    nf = probe.probe_layout(J, n, U, C, stride, bytes_, pk_len, validate, out, tot)
    fields = [(int(out[3 * i]), int(out[3 * i + 1]), int(out[3 * i + 2])) for i in range(nf)]
    assert nf == 32 and tot[4] == n + J and tot[5] == U + J
    assert tot[3] == (U + J) * 68 * 3 * 2 * 14
    for arena, total in ((0, tot[0]), (1, tot[1]), (2, tot[2])):
        fs = [(o, s) for a, o, s in fields if a == arena]
        assert fs[0][0] == 0
        end = 0
        for o, s in fs:  # fields in arena order: each starts at or after the end of the one before
            assert o >= end, (arena, o, end)
            if arena != 2:
                assert o % 256 == 0, "byte arenas: every field on a 256-byte boundary"
            end = o + s
        assert end <= total
    # the sizes that depend on the key mode
    keys = [s for a, o, s in fields if a == 0][3]
    assert keys == n * (pk_len if bytes_ else 4)
    kv96 = [s for a, o, s in fields if a == 0][9]
    assert kv96 == (n * 96 if validate else 0)
