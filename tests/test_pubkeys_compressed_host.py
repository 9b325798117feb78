"""Host side of blsgpu_pubkeys_upload_compressed / blsgpu_pubkeys_read, no GPU needed: the row builder
the kernels run per lane (lodestar_amd/csrc/pk_row.hpp, compiled for the host by tests/native/pk_ingest_probe.cpp)
against the oracle, the exported symbols and the header, the refusals decided before a context is looked at, the
layout of the readback's staging buffer (hl::PubkeysRead), and one run of the probe as a stand-alone program under
AddressSanitizer and UBSan."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as bls
from tests.pubkeys_compressed_helpers import CACHED48, SCAN, SPECIAL, expected, valid_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "pk_ingest_probe.cpp")
LIB = os.path.join(HERE, "native", "libpk_ingest_probe.so")
CSRC = os.path.join(ROOT, "lodestar_amd", "csrc")
W_PKTAB, NL = 32, 14


def inputs():
    return SCAN + CACHED48 + SPECIAL + list(valid_keys(64))


def stale(out):
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    return not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps)


@pytest.fixture(scope="module")
def probe():
    if stale(LIB):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    lib = ctypes.CDLL(LIB)
    vp = ctypes.c_void_p
    lib.probe_pk_ingest.argtypes = [vp, ctypes.c_uint32, ctypes.c_int, vp, vp, vp, vp]
    lib.probe_pubkeys_read.argtypes = [ctypes.c_uint64, ctypes.c_uint64, vp]
    return lib


def ingest(lib, keys, validate):
    n = len(keys)
    src = np.frombuffer(b"".join(keys), np.uint8)
    st, rows = np.full(n, 99, np.int8), np.full(n * W_PKTAB, 0xDEADBEEF, np.uint32)
    o96, o48 = np.zeros(96 * n, np.uint8), np.zeros(48 * n, np.uint8)
    w = lib.probe_pk_ingest(src.ctypes.data, n, int(validate), st.ctypes.data, rows.ctypes.data, o96.ctypes.data,
                            o48.ctypes.data)
    assert w == W_PKTAB
    return st, rows.reshape(n, W_PKTAB), o96.tobytes(), o48.tobytes()


def check_oracle_classes():
    """What the issue states about the inputs, from the oracle alone: of the 199 scanned candidates 100 are not on the
    curve and 99 are on the curve outside G1 -- so the trusted mode accepts 99 of them and the validate mode none."""
    trusted = [expected(c, False)[0] for c in SCAN]
    checked = [expected(c, True)[0] for c in SCAN]
    assert len(SCAN) == 199
    assert trusted.count(bls.BLST_POINT_NOT_ON_CURVE) == 100 and trusted.count(0) == 99
    assert checked.count(bls.BLST_POINT_NOT_ON_CURVE) == 100 and checked.count(bls.BLST_POINT_NOT_IN_GROUP) == 99
    assert [expected(c, False)[0] for c in SPECIAL] == [6, 1, 1, 1]
    assert [expected(c, True)[0] for c in SPECIAL] == [6, 1, 1, 1]
    assert all(expected(c, v)[0] == 0 for c in CACHED48 + list(valid_keys(64)) for v in (False, True))
    assert {k[0] & 0x20 for k in valid_keys(64)} == {0, 0x20}  # both y signs occur among the valid keys


@pytest.mark.parametrize("validate", [False, True])
def test_row_builder_against_the_oracle(probe, validate):
    check_oracle_classes()
    keys = inputs()
    st, rows, o96, o48 = ingest(probe, keys, validate)
    want = [expected(k, validate) for k in keys]
    assert st.tolist() == [c for c, _ in want]
    assert (rows[:, 2 * NL:] == 0).all()  # the pad words
    accepted = 0
    for k, (code, pk96) in enumerate(want):
        if code:
            assert not rows[k].any(), k  # a rejected row is all zero
            continue
        accepted += 1
        assert rows[k, :2 * NL].any() and (rows[k] >> 28 == 0).all()  # 28-bit Montgomery limbs
        assert o96[96 * k: 96 * k + 96] == pk96 == bls.g1_serialize(bls.g1_decompress(keys[k])), k
        assert o48[48 * k: 48 * k + 48] == keys[k], k
    assert accepted == (4 + 64) + (0 if validate else 99)


def test_symbols_and_header():
    from lodestar_amd import native

    lib = ctypes.CDLL(native.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    for name in ("blsgpu_pubkeys_upload_compressed", "blsgpu_pubkeys_read"):
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    assert "int blsgpu_pubkeys_upload_compressed(blsgpu_ctx* ctx, uint32_t first_index, const uint8_t* pk48," in src
    assert "int blsgpu_pubkeys_read(blsgpu_ctx* ctx, uint32_t first_index, uint32_t n, uint8_t* out," in src
    assert "#define BLSGPU_PK_VALIDATE 1u" in src and native.PK_VALIDATE == 1
    assert "#define BLSGPU_ABI_VERSION 8" in src
    head = src[src.index("Entry points added since 8"): src.index("#define BLSGPU_ABI_VERSION")]
    assert "blsgpu_pubkeys_upload_compressed" in head and "blsgpu_pubkeys_read" in head


def test_refusals_before_the_context_is_read():
    """A null context is refused with BLSGPU_ERR_ARGS whatever else is passed, and neither status, first_bad nor out
    is written.  Both entry points look at the context first, so the rows below do not reach the flag, pointer, range
    and out_len checks of their own: tests/test_gpu_pubkeys_compressed.py::test_refusals does, with a context."""
    from lodestar_amd import native

    lib = native.load()
    keys = np.frombuffer(b"".join(valid_keys(2)), np.uint8)
    st, fb = np.full(2, 77, np.int8), np.full(1, 0x12345678, np.uint32)
    for first, src, n, flags in [(0, keys.ctypes.data, 2, 0), (0, keys.ctypes.data, 2, 1), (0, keys.ctypes.data, 2, 2),
                                 (0, keys.ctypes.data, 2, 0x80000001), (0, None, 2, 0), (0xFFFFFFFF, keys.ctypes.data, 2, 0),
                                 (0, None, 0, 0), (0, keys.ctypes.data, 0, 4)]:
        rc = lib.blsgpu_pubkeys_upload_compressed(None, first, src, n, flags, st.ctypes.data, fb.ctypes.data)
        assert rc == native.ERR_ARGS, (first, n, flags)
    assert (st == 77).all() and fb[0] == 0x12345678
    out = np.full(192, 0x5A, np.uint8)
    for first, n, dst, out_len in [(0, 1, out.ctypes.data, 96), (0, 1, out.ctypes.data, 48), (0, 1, out.ctypes.data, 0),
                                   (0, 1, out.ctypes.data, 47), (0, 1, out.ctypes.data, 97), (0, 1, None, 96),
                                   (0, 0, None, 96), (0xFFFFFFFF, 2, out.ctypes.data, 96)]:
        assert lib.blsgpu_pubkeys_read(None, first, n, dst, out_len) == native.ERR_ARGS, (first, n, out_len)
    assert (out == 0x5A).all()
    assert lib.blsgpu_pubkeys_count(None) == 0


def test_pubkeys_read_layout(probe):
    """hl::PubkeysRead: one staging field, `out`, at the start of d_in (16-byte aligned for the kernel's vector stores:
    the arena is), n * out_len bytes, which is the total."""
    fields = ["out", "total"]
    rng = np.random.default_rng(47)
    for n in [0, 1, 63, 64, 65, 130, 1 << 20, (1 << 32) - 1] + [int(x) for x in rng.integers(1, 1 << 22, 50)]:
        for out_len in (48, 96):
            buf = (ctypes.c_uint64 * 8)()
            k = probe.probe_pubkeys_read(n, out_len, buf)
            assert k == len(fields)
            got = dict(zip(fields, buf[:k]))
            assert got["out"] == 0 and got["out"] % 256 == 0
            assert got["out"] + n * out_len <= got["total"] == n * out_len


def test_probe_program_under_sanitizers(tmp_path):
    """The same inputs once through the probe built stand-alone (its own main) with -fsanitize=address,undefined: host
    code only -- no device code and nothing loaded into Python is covered."""
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "one"), str(one)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "one")], capture_output=True).returncode != 0:
        pytest.skip("no sanitized host build here")  # (as tests/test_run_plan.py: not even an empty program runs)
    exe = tmp_path / "pk_ingest_probe"
    subprocess.check_call(["g++", *flags, "-DPK_INGEST_PROBE_MAIN", "-o", str(exe), SRC])
    keys = inputs()
    path = tmp_path / "keys48.bin"
    path.write_bytes(b"".join(keys))
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert r.stdout.splitlines() == [f"validate 0: {68 + 99} of {len(keys)} keys accepted",
                                     f"validate 1: 68 of {len(keys)} keys accepted", "2 layout fields"]
