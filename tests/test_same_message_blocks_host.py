"""Host side of BLSGPU_SAME_BLOCK_CHECK (the block check of blsgpu_verify_same_message), no GPU needed:
the exported symbol and the header, the block rule blsgpu_same_message_blocks, the refusal of a null context under the
new flag, the addon's export and the layout of the buffers the block phase and the descent add (hl::SameBlocks,
through tests/native/same_blocks_probe.cpp)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "same_blocks_probe.cpp")
LIB = os.path.join(HERE, "native", "libsame_blocks_probe.so")
HDR = os.path.join(ROOT, "lodestar_amd", "csrc", "helper_layout.hpp")

W_FP = 14
W_G2J, W_FP12 = 6 * W_FP, 12 * W_FP


def test_symbol_and_header():
    from lodestar_amd import native

    lib = ctypes.CDLL(native.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    assert "blsgpu_same_message_blocks" in native.EXPORTED_SYMBOLS
    assert lib.blsgpu_same_message_blocks is not None
    assert "uint32_t blsgpu_same_message_blocks(uint32_t n_groups, uint32_t flags);" in src
    assert "#define BLSGPU_SAME_BLOCK_CHECK 4u" in src
    assert "#define BLSGPU_SAME_LANE_FORMS 1u" in src
    assert "#define BLSGPU_ABI_VERSION 8" in src
    assert native.SAME_BLOCK_CHECK == 4


def test_stats_struct_is_unchanged():
    from lodestar_amd import native

    assert [f[0] for f in native.SameMessageStats._fields_] == ["groups_accepted", "groups_retried", "retry_sets",
                                                                 "unique_messages", "form", "device_ms"]
    assert ctypes.sizeof(native.SameMessageStats) == 32


def test_block_rule():
    """No block without the flag; with it ceil(n_groups / 1024), non-decreasing, whatever the other flag says."""
    from lodestar_amd import native

    blocks, flag = native.same_message_blocks, native.SAME_BLOCK_CHECK
    sizes = list(range(0, 2200)) + [4096, 16384, 1 << 20, 0xFFFFFFFF]
    for n in sizes:
        assert blocks(n) == 0 and blocks(n, 0) == 0 and blocks(n, native.SAME_LANE_FORMS) == 0
    want = {0: 0, 1: 1, 1024: 1, 1025: 2, 2048: 2, 2049: 3, 1 << 20: 1024}
    for n, b in want.items():
        assert blocks(n, flag) == b, n
    prev = 0
    for n in sizes:
        b = blocks(n, flag)
        assert b == (n + 1023) // 1024 and b >= prev
        assert blocks(n, flag | native.SAME_LANE_FORMS) == b
        prev = b


def test_null_context_is_an_argument_error_under_the_flag():
    """Refused on the host before anything is read, with the new flag alone and with both flags."""
    from lodestar_amd import native

    lib = native.load()
    for flags in (4, 5):
        rc = lib.blsgpu_verify_same_message(None, 1, None, None, None, None, None, 96, None, 0, flags, None, None, None)
        assert rc == native.ERR_ARGS


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_node_addon_exports_the_flag():
    script = (
        "const m = require(process.argv[1]);"
        "if (m.SAME_BLOCK_CHECK !== 4) throw new Error('missing SAME_BLOCK_CHECK');"
        "if (m.SAME_LANE_FORMS !== 1) throw new Error('SAME_LANE_FORMS changed');"
    )
    out = subprocess.run([NODE, "-e", script, os.path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr


# ------------------------------------------------------------------------------------------- hl::SameBlocks
FIELDS = ["w_F", "w_S", "w_G", "w_T0", "w_T1", "work_words", "b_any", "b_ok", "bytes_total", "d_list", "d_F", "d_S",
          "d_G", "descent_words", "d_ok_bytes"]


def al256(x):
    return (x + 255) & ~255


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)

    def call(nb, width, nl):
        out = (ctypes.c_uint64 * 64)()
        k = lib.probe_same_blocks(ctypes.c_uint64(nb), ctypes.c_uint64(width), ctypes.c_uint64(nl), out)
        assert k == len(FIELDS)
        return dict(zip(FIELDS, out[:k]))

    return call


def check_regions(got, fields, sizes, total, unit):
    """Regions of `unit`-byte elements in the documented order: each on a 256-byte boundary (the alignment of hl::Same's
    regions in d_in and d_bytes), none overlapping the next, no more than the padding between them, and the total the
    rounded-up sum."""
    at = 0
    for f, size in zip(fields, sizes):
        off = got[f] * unit
        assert off % 256 == 0 and at <= off < at + 256, (f, off, at)
        at = off + size * unit
    assert got[total] * unit == al256(at)
    assert got[total] * unit == sum(al256(s * unit) for s in sizes)


@pytest.mark.parametrize("nb,width", [(1, 1), (1, 2), (1, 64), (1, 512), (2, 512), (3, 512), (16, 512), (1024, 512)])
@pytest.mark.parametrize("nl", [0, 2, 3, 512, 513, 1024, 2048, 1 << 20])
def test_same_blocks_layout(probe, nb, width, nl):
    """width: the products per block of the first level of the F_b tree (1 .. 512, a power of two; 512 for every call
    of more than one block); the levels alternate between T0 and T1, half as large."""
    got = probe(nb, width, nl)
    check_regions(got, ["w_F", "w_S", "w_G", "w_T0", "w_T1"],
                  [nb * W_FP12, nb * W_G2J, nb * W_FP12, nb * width * W_FP12, nb * (width // 2) * W_FP12], "work_words", 4)
    check_regions(got, ["b_any", "b_ok"], [nb, nb], "bytes_total", 1)
    check_regions(got, ["d_list", "d_F", "d_S", "d_G"], [nl, nl * W_FP12, nl * W_G2J, nl * W_FP12], "descent_words", 4)
    assert got["w_F"] == 0 and got["b_any"] == 0 and got["d_list"] == 0 and got["d_ok_bytes"] == nl
    # the block phase's regions do not depend on the descent's size: they are carved before it is known
    assert {k: got[k] for k in FIELDS[:9]} == {k: probe(nb, width, 0)[k] for k in FIELDS[:9]}
