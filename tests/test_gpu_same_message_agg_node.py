"""BlsGpuVerifier.verifyAndAggregateSameMessage and addon.verifySameMessageAggregate (the JS drop-in over the N-API
addon) on the GPU: this side writes the fixture from the oracle -- three same-message calls (all valid, one set signing
another message, one malformed signature) with the oracle's per-set answers and, per call, the aggregate of the
signatures the oracle verified (bls.g2_add, compressed and uncompressed), also under a mask that leaves two valid sets
out -- and tests/node/same_message_agg_gpu.js checks the device's answers byte for byte, the single device call, the
block-check option and close()."""
import hashlib
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import cpu

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")
MASKED = (1, 4)  # sets of every call that say `aggregate: false` in the masked variant


def aggregate(sigs, res, skip=()):
    acc, cnt = None, 0
    for i, (s, r) in enumerate(zip(sigs, res)):
        if int(r) == 1 and i not in skip:
            acc = bls.g2_add(acc, bls.signature_from_bytes(s, validate=False))
            cnt += 1
    return {"sig96": bls.g2_compress(acc).hex() if cnt else None,
            "sig192": bls.g2_serialize(acc).hex() if cnt else None, "count": cnt}


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_js_verify_and_aggregate_same_message(tmp_path):
    n = 12
    sks = b"".join(bls.interop_secret_key(i).to_bytes(32, "big") for i in range(n))
    m = hashlib.sha256(b"node-agg-same-message").digest()
    other = hashlib.sha256(b"node-another-message").digest()
    pk = cpu.sk_to_pk(sks, threads=16)
    raw = cpu.sign(sks, m * n, threads=16)
    pks = [pk[96 * i: 96 * i + 96] for i in range(n)]
    sigs = [raw[96 * i: 96 * i + 96] for i in range(n)]
    wrong = list(sigs)
    wrong[5] = cpu.sign(sks[32 * 5: 32 * 6], other)
    malformed = list(sigs)
    malformed[8] = bytes([0x9F]) + bytes([0xFF]) * 95  # x >= p: BLST_BAD_ENCODING in Signature.fromBytes
    calls = []
    for case in (sigs, wrong, malformed):
        res, _ = cpu.verify_jobs(threads=16, job_first_set=np.arange(n + 1), sigs=b"".join(case), sig_len=[96] * n,
                                 msgs=m * n, pk_bytes=pk, job_flags=np.zeros(n), sig_stride=96)
        calls.append({"sets": [{"pk": pks[i].hex(), "sig": case[i].hex()} for i in range(n)],
                      "expected": [int(r) == 1 for r in res], "agg": aggregate(case, res),
                      "masked": aggregate(case, res, skip=MASKED)})
    assert calls[0]["expected"] == [True] * n and calls[0]["agg"]["count"] == n
    assert calls[1]["expected"] == [i != 5 for i in range(n)] and calls[1]["agg"]["count"] == n - 1
    assert calls[2]["expected"] == [i != 8 for i in range(n)] and calls[2]["masked"]["count"] == n - 3
    path = tmp_path / "same_message_agg_fixture.json"
    path.write_text(json.dumps({"message": m.hex(), "masked": list(MASKED), "calls": calls}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "same_message_agg_gpu.js"), str(path)],
                         capture_output=True, text=True, timeout=180)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
