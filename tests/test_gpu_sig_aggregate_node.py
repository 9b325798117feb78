"""BlsGpuVerifier.aggregateSignatures (the JS drop-in over the N-API addon) on the GPU: this side writes a fixture from
the oracle -- groups of oracle-signed signatures, mixed encodings, one rejected group per error class, an empty
group -- and tests/node/aggregate_gpu.js checks the device's answers, the live event loop and close()."""
import hashlib
import json
import os
import shutil
import subprocess

import pytest

from oracle import bls12_381 as bls
from oracle import cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")


def fold(sigs, validate):
    acc = None
    for s in sigs:
        p = bls.signature_from_bytes(s, validate=validate)
        if p is not None:
            acc = p if acc is None else bls.g2_add(acc, p)
    return acc


def expected(groups, validate, encode):
    out = []
    for g in groups:
        if not g:
            out.append({"error": "EMPTY_AGGREGATE_ARRAY"})
            continue
        try:
            out.append(encode(fold(g, validate)).hex())
        except bls.BlstError as e:
            out.append({"error": f"BLST_ERROR: {bls.ERROR_NAMES[e.code]}"})
    return out


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_js_aggregate_signatures(tmp_path):
    n = 80
    sks = b"".join(bls.interop_secret_key(i % 16).to_bytes(32, "big") for i in range(n))
    msgs = b"".join(hashlib.sha256(b"node-agg" + i.to_bytes(4, "little")).digest() for i in range(n))
    raw = cpu.sign(sks, msgs, threads=16)
    sigs = [raw[96 * i: 96 * i + 96] for i in range(n)]
    rogue = None  # a curve point outside G2 (the scan of tests/test_gpu_parity.py adversarial_sigs)
    for t in range(1, 400):
        cand = bytes([0x80]) + bytes(45) + t.to_bytes(2, "big") + bytes(48)
        if bls.classify_signature(cand) == bls.BLST_POINT_NOT_IN_GROUP:
            rogue = cand
            break
    assert rogue
    unc = bls.g2_serialize(bls.signature_from_bytes(sigs[3], validate=False))
    inf = bytes([0xC0]) + bytes(95)
    groups = [
        sigs[0:1],
        [sigs[1], sigs[2], unc],
        [],
        sigs[4:70],
        [sigs[70], rogue, sigs[71]],
        [sigs[72], sigs[73][:48]],
        [sigs[74], bytes([0x9F]) + bytes([0xFF]) * 95],
        [sigs[75], bytes([sigs[75][0] ^ 0x20]) + sigs[75][1:]],
        [inf, sigs[76], inf],
        sigs[77:80],
    ]
    fx = {
        "groups": [[s.hex() for s in g] for g in groups],
        "expected": expected(groups, True, bls.g2_compress),
        "expected192": expected(groups, True, bls.g2_serialize),
        "expectedNoValidate": expected(groups, False, bls.g2_compress),
    }
    assert fx["expected"][4] == {"error": "BLST_ERROR: BLST_POINT_NOT_IN_GROUP"}
    assert fx["expected"][5] == {"error": "BLST_ERROR: BLST_INVALID_SIZE"}
    assert fx["expected"][6] == {"error": "BLST_ERROR: BLST_BAD_ENCODING"}
    assert fx["expected"][7] == (bytes([0xC0]) + bytes(95)).hex() and isinstance(fx["expectedNoValidate"][4], str)
    path = tmp_path / "aggregate_fixture.json"
    path.write_text(json.dumps(fx))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "aggregate_gpu.js"), str(path)],
                         capture_output=True, text=True, timeout=180)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
