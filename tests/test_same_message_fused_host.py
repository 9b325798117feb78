"""Host side of the one-call same-message verification, no GPU needed: the exported symbols, the refusal of a null
context, the form rule blsgpu_same_message_form, the Python wrapper's layout checks and the addon's export."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("blsgpu_verify_same_message", "blsgpu_same_message_form")


def test_symbols_are_exported():
    from lodestar_amd import native

    lib = ctypes.CDLL(native.LIB_PATH)
    src = open(os.path.join(ROOT, "include", "blsgpu.h")).read()
    for name in NEW:
        assert name in native.EXPORTED_SYMBOLS
        assert getattr(lib, name) is not None
        assert f" {name}(" in src
    assert "#define BLSGPU_ABI_VERSION 8" in src and "#define BLSGPU_SAME_LANE_FORMS 1u" in src


def test_null_context_is_an_argument_error():
    """Refused on the host before anything is read: every other pointer is null too."""
    from lodestar_amd import native

    lib = native.load()
    rc = lib.blsgpu_verify_same_message(None, 1, None, None, None, None, None, 96, None, 0, 0, None, None, None)
    assert rc == native.ERR_ARGS
    gf = np.array([0, 1], np.uint32)
    rc = lib.blsgpu_verify_same_message(None, 1, gf.ctypes.data, None, None, None, None, 96, None, 7, 0, None, None,
                                        None)
    assert rc == native.ERR_ARGS


def test_form_rule():
    """At most 512 pairings (the default of option "coop_max") are cooperative; the flag forces the lane forms; the
    result never decreases with the item count."""
    from lodestar_amd import native

    assert native.SAME_LANE_FORMS == 1
    assert native.same_message_form(0) == 0 and native.same_message_form(1) == 0
    assert native.same_message_form(512) == 0 and native.same_message_form(513) == 1
    assert native.same_message_form(1 << 20) == 1
    for n in (0, 1, 512, 513):
        assert native.same_message_form(n, native.SAME_LANE_FORMS) == 1
    prev = 0
    for n in list(range(0, 1100)) + [4096, 16384, 1 << 20, 0xFFFFFFFF]:
        f = native.same_message_form(n)
        assert f in (0, 1) and f >= prev
        prev = f


def test_stats_struct_matches_the_header():
    from lodestar_amd import native

    assert [f[0] for f in native.SameMessageStats._fields_] == ["groups_accepted", "groups_retried", "retry_sets",
                                                                 "unique_messages", "form", "device_ms"]
    assert ctypes.sizeof(native.SameMessageStats) == 32


def test_wrapper_refuses_malformed_layouts():
    """ValueError before the library is called: the context handle is never used."""
    from lodestar_amd import native

    c = native.Context.__new__(native.Context)
    c.h, c._lib = None, None
    sig = bytes(96)
    with pytest.raises(ValueError, match="message bytes"):
        c.verify_same_message([0, 1], bytes(31), sig, pk_bytes=bytes(96))
    with pytest.raises(ValueError, match="exactly one"):
        c.verify_same_message([0, 1], bytes(32), sig)
    with pytest.raises(ValueError):
        c.verify_same_message([1, 1], bytes(32), sig, pk_bytes=bytes(96))


NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_node_addon_exports_verify_same_message():
    script = (
        "const m = require(process.argv[1]);"
        "if (typeof m.addon.verifySameMessage !== 'function') throw new Error('missing verifySameMessage');"
        "if (m.SAME_LANE_FORMS !== 1) throw new Error('missing SAME_LANE_FORMS');"
    )
    out = subprocess.run([NODE, "-e", script, os.path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs")],
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
