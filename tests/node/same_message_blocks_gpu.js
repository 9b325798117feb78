"use strict";
// BlsGpuVerifier with fusedSameMessage and sameMessageBlockCheck (addon.verifySameMessage with SAME_BLOCK_CHECK: the
// groups' aggregates checked a block at a time, then the descent) on the GPU against a fixture the Python side wrote
// from the oracle (tests/test_gpu_same_message_blocks_node.py):
// {message: hex, calls: [{sets: [{pk, sig}], expected: [bool]}]} -- the scenario of same_message_fused_gpu.js:
//   - three concurrent calls (all valid; one set signing another message; one malformed signature) resolve to the
//     oracle's boolean[] each in ONE device call, the two calls with a bad set counted as retried;
//   - sameMessageBlockCheck applies only together with fusedSameMessage;
//   - the addon's own call with SAME_BLOCK_CHECK: stats.form has bit 2 set and setResult / groupResult equal the
//     flag-0 call's; an unknown flag is still a RangeError;
//   - close() works.
// Usage: node tests/node/same_message_blocks_gpu.js <fixture.json>   (exit code 0 = pass)
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..");
const {BlsGpuVerifier, SAME_LANE_FORMS, SAME_BLOCK_CHECK, addon} = require(path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs"));
const fx = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const hex = (h) => Uint8Array.from(Buffer.from(h, "hex"));

async function main() {
  assert.strictEqual(SAME_BLOCK_CHECK, 4);
  const message = hex(fx.message);
  const calls = fx.calls.map((c) => c.sets.map((s) => ({publicKey: hex(s.pk), signature: hex(s.sig)})));
  const alone = new BlsGpuVerifier({sameMessageBlockCheck: true});
  assert.strictEqual(alone.fusedSameMessage, false);
  assert.strictEqual(alone.sameMessageBlockCheck, false, "the option applies only with fusedSameMessage");
  await alone.close();
  const v = new BlsGpuVerifier({fusedSameMessage: true, sameMessageBlockCheck: true});
  assert.strictEqual(v.fusedSameMessage, true);
  assert.strictEqual(v.sameMessageBlockCheck, true);

  const got = await Promise.all(calls.map((sets) => v.verifySignatureSetsSameMessage(sets, message, {batchable: true})));
  got.forEach((r, ci) => {
    assert.ok(Array.isArray(r) && r.every((x) => typeof x === "boolean"), `call ${ci}: boolean[]`);
    assert.deepStrictEqual(r, fx.calls[ci].expected, `call ${ci}`);
  });
  assert.strictEqual(v.stats.sameMessageAggregations, 1, "one device call for the three calls");
  assert.strictEqual(v.stats.submissions, 0, "no verification submission beside it");
  assert.strictEqual(v.stats.sameMessageRetries, 2, "the two calls with a bad set were retried");
  assert.strictEqual(v.stats.sameMessageRetrySets, calls[1].length + calls[2].length);
  console.log("ok three concurrent calls, one device call");

  // the addon's call itself: three groups over one message, with and without the flag
  const n = calls[0].length;
  const groupFirst = Uint32Array.from([0, n, 2 * n, 3 * n]);
  const msgs = new Uint8Array(96);
  const pkBytes = new Uint8Array(96 * 3 * n);
  const sigs = new Uint8Array(96 * 3 * n);
  calls.forEach((c, ci) => {
    msgs.set(message, 32 * ci);
    c.forEach((s, i) => {
      pkBytes.set(s.publicKey, 96 * (ci * n + i));
      sigs.set(s.signature, 96 * (ci * n + i));
    });
  });
  const sigLen = new Uint32Array(3 * n).fill(96);
  const plain = await addon.verifySameMessage(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, 0);
  assert.strictEqual(plain.stats.form, 0);
  for (const flags of [SAME_BLOCK_CHECK, SAME_BLOCK_CHECK | SAME_LANE_FORMS]) {
    const r = await addon.verifySameMessage(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, flags);
    assert.ok(r.stats.form & 4, "the block phase ran");
    // one block of three groups; the aggregation rejects the malformed one, the block of the other two fails: the
    // descent ran over those two, in the form the flags say
    assert.strictEqual(r.stats.form, flags & SAME_LANE_FORMS ? 31 : 12);
    assert.deepStrictEqual(Array.from(r.setResult), Array.from(plain.setResult));
    assert.deepStrictEqual(Array.from(r.groupResult), Array.from(plain.groupResult));
    assert.deepStrictEqual(Array.from(r.groupResult), [1, 0, 0]);
    assert.deepStrictEqual(
      Array.from(r.setResult, (x) => x === 1),
      fx.calls.flatMap((c) => c.expected)
    );
    assert.strictEqual(r.stats.groupsAccepted, 1);
    assert.strictEqual(r.stats.groupsRetried, 2);
    assert.strictEqual(r.stats.retrySets, 2 * n);
  }
  assert.throws(() => addon.verifySameMessage(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, 2), RangeError);
  assert.throws(() => addon.verifySameMessage(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, 8), RangeError);
  console.log("ok addon.verifySameMessage with SAME_BLOCK_CHECK");

  await v.close();
  let after = null;
  try {
    await v.verifySignatureSetsSameMessage(calls[0], message);
  } catch (e) {
    after = e;
  }
  assert.ok(after && after.message === "QUEUE_ERROR_QUEUE_ABORTED", `after close: ${after && after.message}`);
  console.log("ok close");
  console.log("ALL OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
