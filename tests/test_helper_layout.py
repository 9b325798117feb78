"""The device-arena layouts of the synchronous helper calls (lodestar_amd/csrc/helper_layout.hpp), CPU only.

helpers.cpp takes every offset, every total it passes to DevBuf::ensure and every d_work word count from the structs
of that header.  tests/native/layout_probe.cpp exposes them; here each one is compared with the chained al256
expressions the calls held before the layouts had names, restated in Python, and every arena is checked to have its
fields on 256-byte boundaries, in the documented order, without overlap.  Totals that end unaligned stay so (o_fl + n
in the two aggregate calls, o_st + 3n in blsgpu_aggregate_pubkeys)."""
import ctypes
import itertools
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "layout_probe.cpp")
LIB = os.path.join(HERE, "native", "liblayout_probe.so")
HDR = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc", "helper_layout.hpp")

W_FP = 14
W_G1A, W_G1J, W_G2A, W_G2J, W_FP12 = 2 * W_FP, 3 * W_FP, 4 * W_FP, 6 * W_FP, 12 * W_FP
AWR_TAB_WORDS = 9 * W_G2J
MILLER_LINE_WORDS = 68 * 3 * 2 * W_FP

SHAPES = [(1, 0), (1, 1), (3, 5), (4, 8), (257, 300)]  # (G, n)
STRIDES = [96, 192]
KEY_MODES = [True, False]  # key bytes, table indices


def al256(x):
    return (x + 255) & ~255


@pytest.fixture(scope="module")
def probe():
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(SRC), os.path.getmtime(HDR)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)

    def call(name, fields, *args):
        out = (ctypes.c_uint64 * 64)()
        cargs = [ctypes.c_int(int(a)) if isinstance(a, bool) else ctypes.c_uint64(a) for a in args]
        k = getattr(lib, name)(*cargs, out)
        assert k == len(fields), (name, k, fields)
        return dict(zip(fields, out[:k]))

    return call


def check_arena(got, fields, sizes, total, aligned_total):
    """fields, in the documented order, with their sizes: each on a 256-byte boundary, none overlapping the next, the
    total at the last one's end (rounded up to 256 when the call rounds it)."""
    at = 0
    for f, size in zip(fields, sizes):
        off = got[f]
        assert off % 256 == 0 and off >= at, (f, off, at)
        assert off - at < 256, (f, off, at)  # no more than the padding
        at = off + size
    assert got[total] == (al256(at) if aligned_total else at)


def test_header_is_hip_free():
    src = open(HDR).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == ["<stddef.h>", "<stdint.h>"]


@pytest.mark.parametrize("G,n", SHAPES)
@pytest.mark.parametrize("key_bytes_mode", KEY_MODES)
@pytest.mark.parametrize("out_len", [48, 96])
def test_aggregate_pubkeys(probe, G, n, key_bytes_mode, out_len):
    # here the sets are the shape's first number and the keys its second plus one per set
    n, npk = G, n + G
    got = probe("probe_agg_pubkeys", ["spf", "keys", "out", "st", "total", "key_bytes", "work_words"], n, npk,
                key_bytes_mode, out_len)
    key_bytes = npk * 96 if key_bytes_mode else npk * 4
    o_keys = al256((n + 1) * 4)
    o_out = al256(o_keys + key_bytes)
    o_st = al256(o_out + n * out_len)
    assert got == {"spf": 0, "keys": o_keys, "out": o_out, "st": o_st, "total": o_st + 3 * n, "key_bytes": key_bytes,
                   "work_words": n * W_G1J}
    check_arena(got, ["spf", "keys", "out", "st"], [(n + 1) * 4, key_bytes, n * out_len, 3 * n], "total", False)


@pytest.mark.parametrize("G,n", SHAPES)
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("out_len", [96, 192])
def test_aggregate_signatures(probe, G, n, stride, out_len):
    fields = ["gf", "len", "sigs", "out", "fb", "gst", "st", "fl", "total", "w_agg", "work_words"]
    got = probe("probe_agg_sigs", fields, G, n, stride, out_len)
    o_len = al256((G + 1) * 4)
    o_sigs = al256(o_len + n * 4)
    o_out = al256(o_sigs + n * stride)
    o_fb = al256(o_out + G * out_len)
    o_gst = al256(o_fb + G * 4)
    o_st = al256(o_gst + G)
    o_fl = al256(o_st + n)
    assert got == {"gf": 0, "len": o_len, "sigs": o_sigs, "out": o_out, "fb": o_fb, "gst": o_gst, "st": o_st,
                   "fl": o_fl, "total": o_fl + n, "w_agg": n * W_G2A, "work_words": n * W_G2A + G * W_G2J}
    check_arena(got, fields[:8], [(G + 1) * 4, n * 4, n * stride, G * out_len, G * 4, G, n, n], "total", False)


INPUT = ["words", "gf", "len", "sigs", "keys", "key_bytes"]


def parent_input(G, n, stride, key_bytes_mode):
    key_bytes = n * 96 if key_bytes_mode else n * 4
    o_gf = al256(n * 8)
    o_len = al256(o_gf + (G + 1) * 4)
    o_sigs = al256(o_len + n * 4)
    o_keys = al256(o_sigs + n * stride)
    return {"words": 0, "gf": o_gf, "len": o_len, "sigs": o_sigs, "keys": o_keys, "key_bytes": key_bytes}


@pytest.mark.parametrize("G,n", SHAPES)
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("key_bytes_mode", KEY_MODES)
@pytest.mark.parametrize("out_pk_len,out_sig_len", [(48, 96), (96, 192), (48, 192)])
def test_aggregate_with_randomness(probe, G, n, stride, key_bytes_mode, out_pk_len, out_sig_len):
    fields = INPUT + ["opk", "osig", "fb", "b_ek", "gst", "b_ec", "b_st", "b_fl", "total", "w_tab", "w_sum_pk",
                      "w_sum_sig", "work_words"]
    for lanes in (G, 4 * G + 3):
        got = probe("probe_awr", fields, G, n, stride, key_bytes_mode, out_pk_len, out_sig_len, lanes)
        want = parent_input(G, n, stride, key_bytes_mode)
        o_opk = al256(want["keys"] + want["key_bytes"])
        o_osig = al256(o_opk + G * out_pk_len)
        o_fb = al256(o_osig + G * out_sig_len)
        o_ek = al256(o_fb + G * 4)
        o_gst = al256(o_ek + G * 8)
        o_ec = al256(o_gst + G)
        o_st = al256(o_ec + 2 * G)
        o_fl = al256(o_st + n)
        tab = n * W_G2A
        sum_pk = tab + lanes * AWR_TAB_WORDS
        want.update({"opk": o_opk, "osig": o_osig, "fb": o_fb, "b_ek": o_ek, "gst": o_gst, "b_ec": o_ec, "b_st": o_st,
                     "b_fl": o_fl, "total": o_fl + n, "w_tab": tab, "w_sum_pk": sum_pk, "w_sum_sig": sum_pk + G * W_G1J,
                     "work_words": n * W_G2A + lanes * AWR_TAB_WORDS + G * (W_G1J + W_G2J)})
        assert got == want
        check_arena(got, INPUT[:5] + ["opk", "osig", "fb", "b_ek", "gst", "b_ec", "b_st", "b_fl"],
                    [n * 8, (G + 1) * 4, n * 4, n * stride, want["key_bytes"], G * out_pk_len, G * out_sig_len, G * 4,
                     G * 8, G, 2 * G, n, n], "total", False)


@pytest.mark.parametrize("G,n", SHAPES)
@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("key_bytes_mode", KEY_MODES)
def test_verify_same_message(probe, G, n, stride, key_bytes_mode):
    b_fields = ["b_ek", "b_ec", "b_st", "b_fl", "b_mf", "b_inc", "b_code", "b_ok", "b_gres", "b_sres"]
    w_fields = ["w_tab", "w_tab_pk", "w_sum_pk", "w_sum_sig", "w_pk_aff", "w_inv", "w_F", "w_G", "w_minv", "w_haff",
                "w_hjac", "w_hnorm", "w_hprep", "w_hq"]
    fields = (INPUT + ["umsg", "gmsg", "iota", "in_total"] + b_fields + ["bytes_total"] + w_fields +
              ["work_words", "lines_words"])
    for U, lanes in itertools.product(sorted({1, G}), (G, 4 * G + 3)):
        got = probe("probe_same", fields, G, n, U, stride, key_bytes_mode, lanes)
        want = parent_input(G, n, stride, key_bytes_mode)
        o_umsg = al256(want["keys"] + want["key_bytes"])
        o_gmsg = al256(o_umsg + U * 32)
        o_iota = al256(o_gmsg + G * 4)
        want.update({"umsg": o_umsg, "gmsg": o_gmsg, "iota": o_iota, "in_total": al256(o_iota + (G + 1) * 4)})
        b_ek = 0
        b_ec = al256(b_ek + G * 8)
        b_st = al256(b_ec + 2 * G)
        b_fl = al256(b_st + n)
        b_mf = al256(b_fl + n)
        b_inc = al256(b_mf + U)
        b_code = al256(b_inc + G)
        b_ok = al256(b_code + G)
        b_gres = al256(b_ok + G)
        b_sres = al256(b_gres + G)
        want.update(dict(zip(b_fields, [b_ek, b_ec, b_st, b_fl, b_mf, b_inc, b_code, b_ok, b_gres, b_sres])))
        want["bytes_total"] = al256(b_sres + n)
        # d_work, as the call walked it: w += each field's words
        nm = U
        w = n * W_G2A
        for f, words in zip(w_fields, [lanes * AWR_TAB_WORDS, lanes * AWR_TAB_WORDS, G * W_G1J, G * W_G2J, G * W_G1A,
                                       G * W_FP, G * W_FP12, G * W_FP12, nm * W_FP, nm * W_G2A, nm * W_G2J, nm * W_FP,
                                       nm * 14 * W_FP]):
            want[f] = w
            w += words
        want["w_hq"] = w
        want["work_words"] = (n * W_G2A + 2 * lanes * AWR_TAB_WORDS + G * (W_G1J + W_G2J + W_G1A + W_FP + 2 * W_FP12) +
                              nm * (W_FP + W_G2A + W_G2J + W_FP + 14 * W_FP + 2 * W_G2J))
        assert want["work_words"] == w + nm * 2 * W_G2J  # h_q, the last field, ends where the total does
        want["lines_words"] = nm * MILLER_LINE_WORDS
        assert got == want
        check_arena(got, INPUT[:5] + ["umsg", "gmsg", "iota"],
                    [n * 8, (G + 1) * 4, n * 4, n * stride, want["key_bytes"], U * 32, G * 4, (G + 1) * 4], "in_total",
                    True)
        check_arena(got, b_fields, [G * 8, 2 * G, n, n, U, G, G, G, G, n], "bytes_total", True)


@pytest.mark.parametrize("nr", [1, 5, 8, 64, 65, 300])
def test_same_message_retry(probe, nr):
    fields = ["msg", "iota", "list_words", "code", "ok", "ok_bytes", "fb_words", "S_words", "F_words"]
    got = probe("probe_same_retry", fields, nr)
    r_msg = al256(nr * 4) // 4
    r_iota = r_msg + al256(nr * 4) // 4
    assert got == {"msg": r_msg, "iota": r_iota, "list_words": r_iota + nr + 1, "code": al256(nr), "ok": 2 * al256(nr),
                   "ok_bytes": 3 * al256(nr), "fb_words": nr * W_G1A, "S_words": nr * W_G2J, "F_words": nr * W_FP12}
    assert got["msg"] * 4 % 256 == 0 and got["iota"] * 4 % 256 == 0 and got["code"] % 256 == 0 and got["ok"] % 256 == 0
    assert nr <= got["msg"] and got["msg"] + nr <= got["iota"] and nr <= got["code"] and got["code"] + nr <= got["ok"]


@pytest.mark.parametrize("n", [1, 5, 8, 300])
@pytest.mark.parametrize("stride", [48, 96, 100])
def test_key_validate(probe, n, stride):
    got = probe("probe_key_validate", ["keys", "out", "st", "total"], n, stride)
    o_out = al256(n * stride)
    o_st = al256(o_out + n * 96)
    assert got == {"keys": 0, "out": o_out, "st": o_st, "total": o_st + n}
    check_arena(got, ["keys", "out", "st"], [n * stride, n * 96, n], "total", False)


@pytest.mark.parametrize("n", [1, 5, 8, 300])
@pytest.mark.parametrize("object_stride", [32, 128])
@pytest.mark.parametrize("domain_stride", [0, 32, 40])
def test_signing_roots(probe, n, object_stride, domain_stride):
    got = probe("probe_signing_roots", ["objects", "dom", "out", "total", "dom_bytes"], n, object_stride, domain_stride)
    dom_bytes = (n if domain_stride else 1) * (domain_stride if domain_stride else 32)
    o_dom = al256(n * object_stride)
    o_out = al256(o_dom + dom_bytes)
    assert got == {"objects": 0, "dom": o_dom, "out": o_out, "total": o_out + 32 * n, "dom_bytes": dom_bytes}
    check_arena(got, ["objects", "dom", "out"], [n * object_stride, dom_bytes, 32 * n], "total", False)
