"""Host side of the same-message path, no GPU needed: blsgpu_randomness_words (the scalar words of a randomized
aggregation, pinned by an independent RFC 8439 ChaCha20 written here), the launch-form rule blsgpu_awr_lanes, the
Python wrapper's layout checks, the exported symbols and the addon's exports."""
import ctypes
import json
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {64, 32, 16, 8, 1}  # the kernels csrc/k_awr.hip implements


# ------------------------------------------------------------------------------------------ randomness words
def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & 0xFFFFFFFF


def chacha20_block(key_words, counter, nonce_words=(0, 0, 0)):
    """RFC 8439 section 2.3: the block function."""
    s = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *key_words, counter, *nonce_words]
    x = list(s)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF
        x[d] = _rotl(x[d] ^ x[a], 16)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF
        x[b] = _rotl(x[b] ^ x[c], 12)
        x[a] = (x[a] + x[b]) & 0xFFFFFFFF
        x[d] = _rotl(x[d] ^ x[a], 8)
        x[c] = (x[c] + x[d]) & 0xFFFFFFFF
        x[b] = _rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return [(x[i] + s[i]) & 0xFFFFFFFF for i in range(16)]


def test_python_chacha20_matches_rfc8439_block_vector():
    key = struct.unpack("<8I", bytes(range(32)))
    nonce = struct.unpack("<3I", bytes.fromhex("000000090000004a00000000"))
    want = bytes.fromhex(
        "10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
        "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    assert struct.pack("<16I", *chacha20_block(key, 1, nonce)) == want


def seed_key(seed):
    # batch_rand.hpp seed_key: the seed under the domain constant "lodestar-amd batch scalar keys"
    return [seed & 0xFFFFFFFF, seed >> 32, 0x65646F6C, 0x72617473, 0x646D612D, 0x61637320, 0x2072616C, 0x7379656B]


def expected_words(n, seed):
    out = []
    for i in range(n):
        blk = chacha20_block(seed_key(seed), i // 8)
        out.append((blk[2 * (i % 8)] | (blk[2 * (i % 8) + 1] << 32)) or 1)
    return out


def test_fixed_seed_words_are_the_chacha20_keystream():
    from lodestar_amd import native

    for seed in (1, 0x4C4F444553544152, 2**64 - 1):
        for n in (0, 1, 7, 8, 9, 70):
            got = native.randomness_words(n, seed)
            assert got.dtype == np.uint64 and [int(x) for x in got] == expected_words(n, seed)
    a, b = native.randomness_words(70, 7), native.randomness_words(70, 7)
    assert (a == b).all() and (a != 0).all()
    assert (native.randomness_words(70, 8) != a).all()


def test_seed_zero_draws_fresh_words():
    from lodestar_amd import native

    a, b = native.randomness_words(4096, 0), native.randomness_words(4096, 0)
    assert (a != 0).all() and (b != 0).all()
    assert len(set(a.tolist())) == 4096 and (a != b).sum() == 4096


def test_randomness_words_argument_errors():
    from lodestar_amd import native

    lib = native.load()
    assert lib.blsgpu_randomness_words(4, 1, None) == native.ERR_ARGS
    assert lib.blsgpu_randomness_words(0, 1, None) == native.OK
    guard = np.full(8, 0xABABABABABABABAB, np.uint64)
    assert lib.blsgpu_randomness_words(3, 1, guard.ctypes.data) == native.OK
    assert (guard[3:] == 0xABABABABABABABAB).all() and (guard[:3] != 0xABABABABABABABAB).all()


def test_randomness_words_entropy_failure_fails_closed():
    """BLSGPU_INJECT_ENTROPY in a child process started with BLSGPU_FAULT_INJECTION=1: the seed-0 draw is refused with
    ERR_ENTROPY and writes nothing, a fixed seed never touches the entropy source, the next seed-0 draw works."""
    code = (
        "import ctypes, numpy as np\n"
        "from lodestar_amd import native\n"
        "lib = native.load()\n"
        "native.debug_inject(native.INJECT_ENTROPY, 0, 1)\n"
        "assert len(native.randomness_words(4, 5)) == 4\n"
        "g = np.full(4, 0xABABABABABABABAB, np.uint64)\n"
        "assert lib.blsgpu_randomness_words(4, 0, g.ctypes.data) == native.ERR_ENTROPY\n"
        "assert (g == 0xABABABABABABABAB).all()\n"
        "assert lib.blsgpu_randomness_words(4, 0, g.ctypes.data) == native.OK\n"
        "assert (g != 0xABABABABABABABAB).all()\n"
        "native.debug_inject(native.INJECT_ENTROPY, 0, 1)\n"
        "try:\n"
        "    native.randomness_words(4, 0)\n"
        "except RuntimeError as e:\n"
        "    assert 'ERR_ENTROPY' in str(e)\n"
        "else:\n"
        "    raise SystemExit(3)\n"
    )
    env = dict(os.environ, BLSGPU_FAULT_INJECTION="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------------------------------------ lane rule
def test_awr_lanes_forms_and_monotone():
    """blsgpu_awr_lanes returns only implemented forms and never more lanes for more groups of the same sets; the
    values DESIGN.md 4.2 states for the measured shapes."""
    from lodestar_amd import native

    f = native.awr_lanes
    counts = sorted({1, 2, 3, 7, 64, 127, 128, 255, 256, 1023, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 8191, 8192,
                     8193, 16383, 16384, 16385, 65536, 1 << 20})
    seen = set()
    for n_sets in (0, 1, 2, 3, 4, 64, 1000, 16384, 65536, 70000, 1 << 20):
        prev = 64
        for g in counts:
            lanes = f(g, n_sets)
            assert lanes in FORMS, (g, n_sets, lanes)
            assert lanes <= prev, f"{n_sets} sets: {g} groups take more lanes ({lanes}) than fewer groups ({prev})"
            prev = lanes
            seen.add(lanes)
    assert seen == FORMS
    assert f(0, 0) == 1
    assert f(128, 128 * 128) == 64 and f(16384, 16384) == 1  # the measured shapes
    assert f(1, 1) == 1 and f(1, 2) == 8 and f(1, 9) == 16 and f(1, 17) == 32 and f(1, 33) == 64
    big = 1 << 20
    assert [f(g, big) for g in (1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)] == [64, 32, 32, 16, 16, 8, 8, 1]


# ------------------------------------------------------------------------------------------- layout checks
class NoLibrary:
    """Stands in for the loaded library: a layout error must be raised before any call reaches it."""

    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) for a malformed layout")


@pytest.fixture()
def wrapper():
    from lodestar_amd import native

    c = native.Context.__new__(native.Context)
    c._lib = NoLibrary()
    c.h = None
    return c


@pytest.mark.parametrize("kw,match", [
    (dict(group_first=[]), "group_first"),
    (dict(group_first=[1, 2]), "start at 0"),
    (dict(group_first=[0, 2, 1]), "never decrease"),
    (dict(group_first=[0, 2], sig_len=[96]), "one entry per signature"),
    (dict(group_first=[0, 2], out_sig_len=48), "out_len"),
    (dict(group_first=[0, 2], out_pk_len=192), "out_pk_len"),
    (dict(group_first=[0, 2], sig_stride=95), "sig_stride"),
    (dict(group_first=[0, 3]), "need 288 bytes"),
    (dict(group_first=[0, 2], sig_len=[96, 192]), "192-byte signature"),
    (dict(group_first=[0, (1 << 20) + 1]), "at most"),
    (dict(group_first=[0, 2], pk_bytes=None), "exactly one of"),
    (dict(group_first=[0, 2], pk_index=[0, 1]), "exactly one of"),
    (dict(group_first=[0, 2], pk_bytes=bytes(96)), "pubkey bytes"),
    (dict(group_first=[0, 2], pk_bytes=None, pk_index=[0]), "one entry per set"),
    (dict(group_first=[0, 2], pk_bytes=None, pk_index=[0, -1]), "table indices"),
])
def test_wrapper_refuses_malformed_layouts(wrapper, kw, match):
    kw.setdefault("sig_stride", 96)
    kw.setdefault("pk_bytes", bytes(192))
    with pytest.raises(ValueError, match=match):
        wrapper.aggregate_with_randomness(sigs=bytes(192), **kw)


def test_layout_defaults():
    from lodestar_amd import native

    gf, buf, sl, stride, pkb, pki = native.awr_layout([0, 1, 3], bytes(3 * 192), pk_index=[5, 6, 7])
    assert stride == 192 and list(sl) == [192] * 3 and list(gf) == [0, 1, 3] and pkb is None
    assert pki.dtype == np.uint32 and list(pki) == [5, 6, 7]
    gf, buf, sl, stride, pkb, pki = native.awr_layout([0, 0, 2], bytes(2 * 96), pk_bytes=bytes(192), sig_len=[96, 7])
    assert stride == 96 and list(sl) == [96, 7] and pki is None and len(pkb) == 192


# ----------------------------------------------------------------------------------------------- exports
def test_symbols_are_exported():
    from lodestar_amd import native

    lib = ctypes.CDLL(native.LIB_PATH)
    for name in ("blsgpu_randomness_words", "blsgpu_aggregate_with_randomness", "blsgpu_awr_lanes"):
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    for name in ("blsgpu_randomness_words", "blsgpu_aggregate_with_randomness", "blsgpu_awr_lanes"):
        assert f" {name}(" in src


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_node_addon_exports_aggregate_with_randomness():
    script = (
        "const m = require(process.argv[1]);"
        "if (typeof m.addon.aggregateWithRandomness !== 'function') throw new Error('missing aggregateWithRandomness');"
        "for (const c of [m.BlsGpuVerifier, m.BlsGpuSingleThreadVerifier])"
        "  for (const f of ['verifySignatureSetsSameMessage', 'canAcceptWork'])"
        "    if (typeof c.prototype[f] !== 'function') throw new Error('missing ' + f);"
        "console.log(JSON.stringify({max: m.MAX_JOBS_CAN_ACCEPT_WORK}));"
    )
    out = subprocess.run([NODE, "-e", script, os.path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout)["max"] == 512
