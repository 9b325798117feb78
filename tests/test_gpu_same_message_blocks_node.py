"""BlsGpuVerifier with fusedSameMessage and sameMessageBlockCheck, and addon.verifySameMessage with SAME_BLOCK_CHECK, on
the GPU: this side writes the fixture of tests/test_gpu_same_message_fused_node.py from the oracle -- three same-message
calls (all valid, one set signing another message, one malformed signature) with the oracle's per-set answers -- and
tests/node/same_message_blocks_gpu.js checks the device's answers, the single device call, the retry statistics, the
addon's results with the flag against its results without, and close()."""
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


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_js_same_message_block_check(tmp_path):
    n = 12
    sks = b"".join(bls.interop_secret_key(i).to_bytes(32, "big") for i in range(n))
    m = hashlib.sha256(b"node-blocks-same-message").digest()
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
                      "expected": [int(r) == 1 for r in res]})
    assert calls[0]["expected"] == [True] * n
    assert calls[1]["expected"] == [i != 5 for i in range(n)]
    assert calls[2]["expected"] == [i != 8 for i in range(n)]
    path = tmp_path / "same_message_fixture.json"
    path.write_text(json.dumps({"message": m.hex(), "calls": calls}))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "same_message_blocks_gpu.js"), str(path)],
                         capture_output=True, text=True, timeout=180)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
