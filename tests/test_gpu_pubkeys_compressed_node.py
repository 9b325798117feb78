"""The compressed pubkey upload and the table readback through the JS drop-in on the GPU: this side writes a fixture
of keys, the oracle's decompression of each, one key per error class and a few signature sets with the oracle's answers
(tests/pubkeys_compressed_helpers.py, oracle/cpu.py), and tests/node/pubkeys_compressed_gpu.js -- a fresh node process
-- checks addon.uploadPubkeysCompressed / readPubkeys, the verifier's methods, a rejected key's error and .index, and
table-mode verifySignatureSets afterwards."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import cpu
from tests.pubkeys_compressed_helpers import class_examples, expected, valid_keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_js_pubkeys_compressed(tmp_path):
    n = 6
    keys = valid_keys(n)  # secret keys 1 .. n
    pk96 = [expected(k, False)[1] for k in keys]
    ex = class_examples()
    off_group = ex[bls.BLST_POINT_NOT_IN_GROUP]
    # sets: two single (one valid, one over another message), two aggregate (keys 2 + 3 valid, keys 4 + 5 with key 4's
    # signature alone); an aggregate's signature is the sum of the secret keys' signature
    msgs = [bytes([0x40 + i]) * 32 for i in range(4)]
    sks = [1, 2, (3 + 4) % bls.R, 5]
    sigs = cpu.sign(b"".join(s.to_bytes(32, "big") for s in sks), b"".join(msgs))
    pks = [[0], [1], [2, 3], [4, 5]]
    msgs[1] = msgs[0]
    spf = np.cumsum([0] + [len(p) for p in pks])
    table = cpu.Table(b"".join(pk96))
    want, _ = cpu.verify_jobs(table=table, job_first_set=np.arange(5), sigs=sigs, sig_len=[96] * 4, msgs=b"".join(msgs),
                              set_pk_first=spf, pk_index=[i for p in pks for i in p], job_flags=np.zeros(4),
                              sig_stride=96)
    table.close()
    assert list(want) == [1, 0, 1, 0]
    fx = {"pk48": [k.hex() for k in keys], "pk96": [p.hex() for p in pk96],
          "bad": {"offCurve": ex[bls.BLST_POINT_NOT_ON_CURVE].hex(), "offGroup": off_group.hex(),
                  "offGroup96": bls.g1_serialize(bls.g1_decompress(off_group)).hex()},
          "sets": [{"pks": pks[i], "msg": msgs[i].hex(), "sig": sigs[96 * i: 96 * i + 96].hex(),
                    "expected": bool(want[i])} for i in range(4)]}
    path = tmp_path / "pubkeys_compressed_fixture.json"
    path.write_text(json.dumps(fx))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "pubkeys_compressed_gpu.js"), str(path)],
                         capture_output=True, text=True, timeout=180)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
