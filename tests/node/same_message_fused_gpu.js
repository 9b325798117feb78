"use strict";
// BlsGpuVerifier.verifySignatureSetsSameMessage with fusedSameMessage: true (one addon.verifySameMessage call per flush)
// on the GPU against a fixture the Python side wrote from the oracle (tests/test_gpu_same_message_fused_node.py):
// {message: hex, calls: [{sets: [{pk, sig}], expected: [bool]}]} -- the scenario of same_message_gpu.js:
//   - three concurrent calls (all valid; one set signing another message; one malformed signature) resolve to the
//     oracle's boolean[] each -- a bad signature is a `false`, never a throw;
//   - they share ONE device call (stats.sameMessageAggregations) and no verification submission follows it
//     (stats.submissions stays 0); only the two calls with a bad set count as retried (stats.sameMessageRetries /
//     sameMessageRetrySets, from groupResult);
//   - the addon's own answer for the three groups: setResult, groupResult and stats;
//   - an empty call rejects as verifySignatureSets does; table-mode keys (validator indices) give the same answers;
//   - the default verifier (fusedSameMessage off) gives the same booleans;
//   - close() waits for an outstanding call (it settles before close() resolves) and later calls reject with
//     QUEUE_ERROR_QUEUE_ABORTED.
// Usage: node tests/node/same_message_fused_gpu.js <fixture.json>   (exit code 0 = pass)
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..");
const {BlsGpuVerifier, SAME_LANE_FORMS, addon} = require(path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs"));
const fx = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const hex = (h) => Uint8Array.from(Buffer.from(h, "hex"));

async function main() {
  const message = hex(fx.message);
  const calls = fx.calls.map((c) => c.sets.map((s) => ({publicKey: hex(s.pk), signature: hex(s.sig)})));
  const v = new BlsGpuVerifier({fusedSameMessage: true});
  assert.strictEqual(v.fusedSameMessage, true);
  assert.strictEqual(v.canAcceptWork(), true, "idle verifier accepts work");

  const got = await Promise.all(calls.map((sets) => v.verifySignatureSetsSameMessage(sets, message, {batchable: true})));
  got.forEach((r, ci) => {
    assert.ok(Array.isArray(r) && r.every((x) => typeof x === "boolean"), `call ${ci}: boolean[]`);
    assert.deepStrictEqual(r, fx.calls[ci].expected, `call ${ci}`);
  });
  assert.strictEqual(v.stats.sameMessageAggregations, 1, "one device call for the three calls");
  assert.strictEqual(v.stats.submissions, 0, "no verification submission beside it");
  assert.strictEqual(v.stats.sameMessageRetries, 2, "the two calls with a bad set were retried");
  assert.strictEqual(v.stats.sameMessageRetrySets, calls[1].length + calls[2].length);
  assert.strictEqual(v.canAcceptWork(), true, "idle again");
  console.log("ok three concurrent calls, one device call");

  // the addon's call itself: three groups over one message
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
  for (const flags of [0, SAME_LANE_FORMS]) {
    const r = await addon.verifySameMessage(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, flags);
    assert.ok(r.setResult instanceof Int8Array && r.groupResult instanceof Int8Array);
    assert.deepStrictEqual(Array.from(r.groupResult), [1, 0, 0]);
    assert.deepStrictEqual(
      Array.from(r.setResult, (x) => x === 1),
      fx.calls.flatMap((c) => c.expected)
    );
    assert.ok(Array.from(r.setResult).some((x) => x < 0), "the malformed signature answers its code");
    assert.strictEqual(r.stats.groupsAccepted, 1);
    assert.strictEqual(r.stats.groupsRetried, 2);
    assert.strictEqual(r.stats.retrySets, 2 * n);
    assert.strictEqual(r.stats.uniqueMessages, 1);
    assert.strictEqual(r.stats.form, flags ? 3 : 0);
    assert.ok(r.stats.deviceMs > 0);
  }
  assert.throws(() => addon.verifySameMessage(v.ctx, groupFirst, msgs.subarray(0, 64), pkBytes, null, sigs, sigLen, 96, 0, 0), RangeError);
  assert.throws(() => addon.verifySameMessage(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, 2), RangeError);
  console.log("ok addon.verifySameMessage");

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

  // the default verifier takes the two-step path and answers the same
  const plain = new BlsGpuVerifier();
  assert.strictEqual(plain.fusedSameMessage, false);
  assert.deepStrictEqual(await plain.verifySignatureSetsSameMessage(calls[1], message), fx.calls[1].expected);
  assert.ok(plain.stats.submissions > 0);
  await plain.close();
  console.log("ok default path unchanged");

  // close() waits for outstanding calls, then refuses new ones
  const outstanding = [v.verifySignatureSetsSameMessage(calls[0], message), v.verifySignatureSetsSameMessage(calls[2], message)];
  await new Promise((resolve) => setTimeout(resolve, 0)); // the flush: the device call is outstanding now
  let settledBeforeClose = 0;
  const watched = outstanding.map((p) =>
    p.then(
      (r) => (settledBeforeClose++, r),
      (e) => (settledBeforeClose++, e)
    )
  );
  await v.close();
  assert.strictEqual(settledBeforeClose, outstanding.length, "outstanding calls settled before close() resolved");
  const settled = await Promise.all(watched);
  assert.deepStrictEqual(settled[0], fx.calls[0].expected, "the outstanding device call completed");
  assert.deepStrictEqual(settled[1], fx.calls[2].expected);
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
