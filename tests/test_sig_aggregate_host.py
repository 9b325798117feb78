"""Host side of blsgpu_aggregate_signatures, no GPU needed: the Python wrapper's layout checks, the launch-form rule
(blsgpu_sig_agg_lanes, pure host code) and the addon's export."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {64, 32, 16, 8, 1}  # the kernels csrc/k_sigagg.hip implements


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
    (dict(group_first=[0, 2], sig_len=[96, 96, 96]), "one entry per signature"),
    (dict(group_first=[0, 2], out_len=48), "out_len"),
    (dict(group_first=[0, 2], sig_stride=95), "sig_stride"),
    (dict(group_first=[0, 3]), "need 288 bytes"),
    (dict(group_first=[0, 2], sig_len=[96, 192]), "192-byte signature"),
    (dict(group_first=[0, (1 << 20) + 1]), "at most"),
])
def test_wrapper_refuses_malformed_layouts(wrapper, kw, match):
    kw.setdefault("sig_stride", 96)
    with pytest.raises(ValueError, match=match):
        wrapper.aggregate_signatures(bytes(192), **kw)


def test_layout_defaults():
    from lodestar_amd import native

    buf, gf, sl, stride = native.aggregate_layout(bytes(3 * 192), [0, 1, 3])
    assert stride == 192 and list(sl) == [192] * 3 and gf.dtype == np.uint32 and list(gf) == [0, 1, 3]
    buf, gf, sl, stride = native.aggregate_layout(bytes(3 * 96), [0, 0, 3], sig_len=[96, 48, 7])
    assert stride == 96 and list(sl) == [96, 48, 7]  # odd lengths are the device's to reject (INVALID_SIZE)
    assert native.aggregate_layout(b"", [0, 0])[3] == 96


def test_sig_agg_lanes_forms_and_monotone():
    """blsgpu_sig_agg_lanes returns only implemented forms, never more lanes for more groups of the same signatures,
    and the forms the documents state for the measured shapes and the pool insert."""
    from lodestar_amd import native

    f = native.sig_agg_lanes
    counts = sorted({1, 2, 3, 7, 64, 255, 256, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193, 16383, 16384,
                     16385, 65536, 1 << 20})
    seen = set()
    for n_sigs in (0, 1, 3, 4, 64, 1000, 16384, 65536, 70000, 1 << 20):
        prev = 64
        for g in counts:
            lanes = f(g, n_sigs)
            assert lanes in FORMS, (g, n_sigs, lanes)
            assert lanes <= prev, f"{n_sigs} signatures: {g} groups take more lanes ({lanes}) than fewer groups ({prev})"
            prev = lanes
            seen.add(lanes)
    assert seen == FORMS
    assert f(0, 0) == 1
    assert f(1, 1) == 1 and f(1, 3) == 1 and f(1000, 3000) == 1  # pool inserts: one lane per group
    assert f(256, 16384) == 64 and f(16384, 16384) == 1 and f(32, 16384) == 64  # the measured shapes
    assert f(1024, 1 << 20) == 64 and f(1025, 1 << 20) == 32 and f(4096, 1 << 20) == 32 and f(4097, 1 << 20) == 16
    assert f(8192, 1 << 20) == 16 and f(8193, 1 << 20) == 8 and f(16384, 1 << 20) == 8 and f(16385, 1 << 20) == 1
    assert f(1, 4) == 8 and f(1, 8) == 8 and f(1, 9) == 16 and f(1, 17) == 32 and f(1, 33) == 64


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_node_addon_exports_aggregate_signatures():
    script = (
        "const m = require(process.argv[1]);"
        "if (typeof m.addon.aggregateSignatures !== 'function') throw new Error('missing aggregateSignatures');"
        "for (const c of [m.BlsGpuVerifier, m.BlsGpuSingleThreadVerifier])"
        "  if (typeof c.prototype.aggregateSignatures !== 'function') throw new Error('missing method');"
        "console.log(JSON.stringify({abi: m.addon.abiVersion}));"
    )
    out = subprocess.run([NODE, "-e", script, os.path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout)["abi"] == 8
