"use strict";
// BlsGpuVerifier.verifySignatureSetsSameMessage on the GPU against a fixture the Python side wrote from the oracle
// (tests/test_gpu_same_message_node.py): {message: hex, calls: [{sets: [{pk, sig}], expected: [bool]}]}.
//   - three concurrent calls (all valid; one set signing another message; one malformed signature) resolve to the
//     oracle's boolean[] each -- a bad signature is a `false`, never a throw;
//   - they share ONE device aggregation call (stats.sameMessageAggregations), and only the two calls with a bad set
//     are retried set by set (stats.sameMessageRetries / sameMessageRetrySets);
//   - canAcceptWork() is true when idle;
//   - an empty call rejects as verifySignatureSets does; table-mode keys (validator indices) give the same answers;
//   - close() waits for outstanding calls (they settle before it resolves) and later calls reject with
//     QUEUE_ERROR_QUEUE_ABORTED.
// Usage: node tests/node/same_message_gpu.js <fixture.json>   (exit code 0 = pass)
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..");
const {BlsGpuVerifier, MAX_JOBS_CAN_ACCEPT_WORK} = require(path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs"));
const fx = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const hex = (h) => Uint8Array.from(Buffer.from(h, "hex"));

async function main() {
  const message = hex(fx.message);
  const calls = fx.calls.map((c) => c.sets.map((s) => ({publicKey: hex(s.pk), signature: hex(s.sig)})));
  const v = new BlsGpuVerifier();
  assert.strictEqual(MAX_JOBS_CAN_ACCEPT_WORK, 512);
  assert.strictEqual(v.canAcceptWork(), true, "idle verifier accepts work");

  const got = await Promise.all(calls.map((sets) => v.verifySignatureSetsSameMessage(sets, message, {batchable: true})));
  got.forEach((r, ci) => {
    assert.ok(Array.isArray(r) && r.every((x) => typeof x === "boolean"), `call ${ci}: boolean[]`);
    assert.deepStrictEqual(r, fx.calls[ci].expected, `call ${ci}`);
  });
  assert.strictEqual(v.stats.sameMessageAggregations, 1, "one device aggregation call for the three calls");
  assert.strictEqual(v.stats.sameMessageRetries, 2, "the two calls with a bad set were retried");
  assert.strictEqual(v.stats.sameMessageRetrySets, calls[1].length + calls[2].length);
  assert.strictEqual(v.canAcceptWork(), true, "idle again");
  console.log("ok three concurrent calls, one aggregation");

  // table mode: the same keys by validator index
  const keys = fx.calls[0].sets.map((s) => s.pk);
  v.uploadPubkeys(0, hex(keys.join("")));
  for (const ci of [0, 1]) {
    const sets = calls[ci].map((s, i) => ({publicKey: i, signature: s.signature}));
    assert.deepStrictEqual(await v.verifySignatureSetsSameMessage(sets, message), fx.calls[ci].expected, `table call ${ci}`);
  }
  console.log("ok table mode");

  let empty = null;
  try {
    await v.verifySignatureSetsSameMessage([], message, {batchable: true});
  } catch (e) {
    empty = e;
  }
  assert.ok(empty && empty.message === "Empty results array", `empty sets: ${empty && empty.message}`);
  console.log("ok empty sets reject");

  // the existing method is untouched by the new path
  const s0 = calls[0][0];
  assert.strictEqual(
    await v.verifySignatureSets([{type: "single", pubkey: s0.publicKey, signingRoot: message, signature: s0.signature}]),
    true
  );

  // close() waits for outstanding calls, then refuses new ones
  const outstanding = [v.verifySignatureSetsSameMessage(calls[0], message), v.verifySignatureSetsSameMessage(calls[2], message)];
  let settledBeforeClose = 0;
  const watched = outstanding.map((p) =>
    p.then(
      (r) => (settledBeforeClose++, r),
      (e) => (settledBeforeClose++, e)
    )
  );
  await v.close();
  assert.strictEqual(settledBeforeClose, outstanding.length, "outstanding calls settled before close() resolved");
  for (const r of await Promise.all(watched))
    assert.ok(Array.isArray(r) || r.message === "QUEUE_ERROR_QUEUE_ABORTED", `outstanding at close: ${r && r.message}`);
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
