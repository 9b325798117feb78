"""Host side of blsgpu_verify_same_message_agg, no GPU needed: the exported symbols and the header,
the lane rule blsgpu_same_message_agg_lanes, the refusals that are decided before a context is looked at, and the
layout of the buffer the aggregate phase adds (hl::SameAgg, through tests/native/same_agg_probe.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "same_agg_probe.cpp")
LIB = os.path.join(HERE, "native", "libsame_agg_probe.so")
HDR = os.path.join(ROOT, "lodestar_amd", "csrc", "helper_layout.hpp")

W_G2J = 6 * 14


def test_symbols_and_header():
    from lodestar_amd import native

    lib = ctypes.CDLL(native.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    for name in ("blsgpu_verify_same_message_agg", "blsgpu_same_message_agg_lanes"):
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "int blsgpu_verify_same_message_agg(blsgpu_ctx* ctx, uint32_t n_groups, const uint32_t* group_first," in src
    assert "uint32_t blsgpu_same_message_agg_lanes(uint32_t n_groups, uint32_t n_sets);" in src
    assert "#define BLSGPU_ABI_VERSION 8" in src
    head = src[src.index("Entry points added since 8"): src.index("#define BLSGPU_ABI_VERSION")]
    assert "blsgpu_verify_same_message_agg" in head and "blsgpu_same_message_agg_lanes" in head


def test_lane_rule_is_that_of_the_signature_aggregation():
    from lodestar_amd import native

    counts = [0, 1, 2, 3, 7, 8, 64, 1023, 1024, 1025, 2048, 4096, 4097, 8192, 8193, 16384, 16385, 65536, 1 << 20]
    sets = [0, 1, 2, 3, 4, 8, 9, 63, 64, 65, 129, 1000, 16384, 16385, 65536, 1 << 20]
    for n in sets:
        prev = 64
        for g in counts:
            lanes = native.same_message_agg_lanes(g, n)
            assert lanes == native.sig_agg_lanes(g, n), (g, n)
            assert lanes in (1, 8, 16, 32, 64)
            if g:
                assert lanes <= prev, (g, n)  # non-increasing in n_groups
                prev = lanes
    assert native.same_message_agg_lanes(128, 16384) == 64
    assert native.same_message_agg_lanes(16384, 16384) == 1


def test_refusals_before_the_context_is_read():
    """A null context, and the new argument errors with a null context: BLSGPU_ERR_ARGS on the host either way."""
    from lodestar_amd import native

    lib = native.load()
    out, cnt = np.zeros(192, np.uint8), np.zeros(1, np.uint32)
    for out_len in (96, 192, 95, 0):
        rc = lib.blsgpu_verify_same_message_agg(None, 1, None, None, None, None, None, 96, None, 0, 0, None, None,
                                                None, None, out.ctypes.data, out_len, cnt.ctypes.data)
        assert rc == native.ERR_ARGS
    assert not out.any() and not cnt.any()


# --------------------------------------------------------------------------------------------- hl::SameAgg
FIELDS = ["inc", "sums", "count", "out", "total", "total_words"]


def al256(x):
    return (x + 255) & ~255


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)

    def call(G, n, out_len):
        out = (ctypes.c_uint64 * 16)()
        k = lib.probe_same_agg(ctypes.c_uint64(G), ctypes.c_uint64(n), ctypes.c_uint64(out_len), out)
        assert k == len(FIELDS)
        return dict(zip(FIELDS, out[:k]))

    return call


def test_same_agg_layout(probe):
    """Byte regions in the documented order -- include | sums | counts | out -- each on a 256-byte boundary (the
    alignment of hl::Same's and hl::SameBlocks' regions), none overlapping the next, all inside the total, which is a
    whole number of words: the buffer is a word buffer."""
    rng = np.random.default_rng(20)
    shapes = [(0, 0), (1, 0), (1, 1), (2, 255), (3, 256), (3, 257), (1024, 16384), (16384, 16384), (1 << 20, 1 << 20)]
    shapes += [(int(rng.integers(1, 1 << 14)), int(rng.integers(0, 1 << 17))) for _ in range(200)]
    for G, n in shapes:
        for out_len in (96, 192):
            got = probe(G, n, out_len)
            at = 0
            for f, size in zip(FIELDS[:4], [n, G * W_G2J * 4, G * 4, G * out_len]):
                off = got[f]
                assert off % 256 == 0 and at <= off < at + 256, (G, n, out_len, f)
                at = off + size
            assert got["inc"] == 0
            assert at <= got["total"] == al256(at) and got["total_words"] * 4 == got["total"]
