"""The committee store and the aggregation from participation bits through the JS drop-in on the GPU: this side writes
a fixture of the table's keys, committees, sets of (committee, bits) and the oracle's aggregated key of each
(tests/committee_bits_helpers.py), plus signatures under the summed secret keys of some sets, and
tests/node/committee_bits_gpu.js -- a fresh node process -- checks the addon's calls, the verifier's methods, bytes-mode
verification with the keys it got, the store's invalidation and close() with a call outstanding."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import cpu
from tests import committee_bits_helpers as H

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
ADDON = os.path.join(ROOT, "lodestar_amd", "node", "blsgpu_napi.node")


@pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the N-API addon is absent")
def test_js_committee_bits(tmp_path):
    rng = np.random.default_rng(91)
    sizes = H.size_committees()
    cms = [sizes[2], sizes[4], sizes[7], sizes[10], sizes[11], (H.P, H.NEG_P)]  # 7, 9, 33, 65, 512 members; {P, -P}
    sets = [
        [(4, rng.random(512) < 0.95)],
        [(3, rng.random(65) < 0.9), (0, rng.random(7) < 0.4)],
        [(1, np.zeros(9, bool))],                               # no participant
        [(5, np.ones(2, bool))],                                # the identity
        [(2, np.ones(33, bool)), (2, rng.random(33) < 0.5)],    # a committee twice
        [],
        [(1, np.ones(9, bool))],
    ]
    lists = H.expand(cms, sets)
    ssf, seg, sbf, bits = H.call_arrays(sets)
    plan = H.plan(cms, sets)
    assert plan["segments_complemented"] >= 4

    def enc(out_len):
        return [None if st else w.hex() for w, st in H.oracle_sums(lists, out_len)]

    which, others = [0, 1, 4, 6], [1, 0, 6, 4]
    msgs = [bytes([0x50 + k]) * 32 for k in which]
    sks = b"".join((sum(H.SKS[i] for i in lists[k]) % H.R_ORDER).to_bytes(32, "big") for k in which)
    sigs = cpu.sign(sks, b"".join(msgs))
    fx = {"pk96": H.table_pk96().hex(), "committees": [list(c) for c in cms],
          "sets": [[{"committee": c, "bits": H.pack(b).hex(), "bitLen": len(b)} for c, b in s] for s in sets],
          "expected96": enc(96), "expected48": enc(48), "complemented": plan["segments_complemented"],
          "keysPresent": plan["keys_present"],
          "raw": {"setSegFirst": ssf.tolist(), "segCommittee": seg.tolist(), "setBitsFirst": sbf.tolist(),
                  "bits": bits.tobytes().hex()},
          "verify": [{"set": k, "other": others[j], "msg": msgs[j].hex(), "sig": sigs[96 * j: 96 * j + 96].hex()}
                     for j, k in enumerate(which)]}
    assert fx["expected96"][2] is None and fx["expected96"][5] is None and fx["expected96"][3] == H.identity(96).hex()
    path = tmp_path / "committee_bits_fixture.json"
    path.write_text(json.dumps(fx))
    out = subprocess.run([NODE, os.path.join(ROOT, "tests", "node", "committee_bits_gpu.js"), str(path)],
                         capture_output=True, text=True, timeout=180)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "ALL OK" in out.stdout
