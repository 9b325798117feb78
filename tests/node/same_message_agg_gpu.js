"use strict";
// BlsGpuVerifier.verifyAndAggregateSameMessage and addon.verifySameMessageAggregate on the GPU against a fixture the
// Python side wrote from the oracle (tests/test_gpu_same_message_agg_node.py):
// {message: hex, masked: [set indices], calls: [{sets: [{pk, sig}], expected: [bool], agg: {sig96, sig192, count},
//  masked: {sig96, sig192, count}}]}:
//   - the addon's own call over the three groups: setResult, groupResult and stats as verifySameMessage answers them,
//     outSig byte for byte in both lengths, aggCount, with and without an include mask; bad shapes are a RangeError;
//   - three concurrent verifyAndAggregateSameMessage calls resolve to the oracle's booleans, aggregate and count each,
//     from ONE device call (stats.sameMessageAggregations) with no verification submission beside it, on a verifier
//     that does not set fusedSameMessage; the two calls with a bad set count as retried;
//   - `aggregate: false` leaves a set out of the sum and still verifies it; a call in which nothing is summed resolves
//     to signature null, count 0;
//   - two calls, one with a mask, share one flush; sameMessageBlockCheck: true gives the same answers; table mode too;
//   - an empty call rejects; close() waits for an outstanding call and later calls reject.
// Usage: node tests/node/same_message_agg_gpu.js <fixture.json>   (exit code 0 = pass)
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..");
const {BlsGpuVerifier, SAME_LANE_FORMS, SAME_BLOCK_CHECK, addon} = require(path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs"));
const fx = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const hex = (h) => Uint8Array.from(Buffer.from(h, "hex"));
const toHex = (b) => (b === null ? null : Buffer.from(b).toString("hex"));

function checkCall(r, ci, want, label) {
  assert.deepStrictEqual(r.results, fx.calls[ci].expected, `${label}: results of call ${ci}`);
  assert.strictEqual(r.count, want.count, `${label}: count of call ${ci}`);
  assert.ok(r.signature === null || Buffer.isBuffer(r.signature), `${label}: Buffer or null`);
  assert.strictEqual(toHex(r.signature), want.sig96, `${label}: aggregate of call ${ci}`);
}

async function main() {
  const message = hex(fx.message);
  const calls = fx.calls.map((c) => c.sets.map((s) => ({publicKey: hex(s.pk), signature: hex(s.sig)})));
  const maskedSets = (ci) => calls[ci].map((s, i) => Object.assign({aggregate: !fx.masked.includes(i)}, s));
  const v = new BlsGpuVerifier();
  assert.strictEqual(v.fusedSameMessage, false);
  assert.strictEqual(typeof addon.verifySameMessageAggregate, "function");

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
  const include = new Uint8Array(3 * n).fill(1);
  for (let ci = 0; ci < 3; ci++) for (const i of fx.masked) include[ci * n + i] = 0;
  for (const flags of [0, SAME_LANE_FORMS, SAME_BLOCK_CHECK]) {
    const plain = await addon.verifySameMessage(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 7, flags);
    for (const [inc, key] of [[null, "agg"], [include, "masked"]]) {
      for (const outLen of [96, 192]) {
        const r = await addon.verifySameMessageAggregate(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 7, flags, inc, outLen);
        assert.deepStrictEqual(Array.from(r.setResult), Array.from(plain.setResult));
        assert.deepStrictEqual(Array.from(r.groupResult), [1, 0, 0]);
        for (const f of ["groupsAccepted", "groupsRetried", "retrySets", "uniqueMessages", "form"])
          assert.strictEqual(r.stats[f], plain.stats[f], f);
        assert.ok(r.outSig instanceof Uint8Array && r.outSig.length === 3 * outLen && r.aggCount instanceof Uint32Array);
        assert.deepStrictEqual(Array.from(r.aggCount), fx.calls.map((c) => c[key].count));
        fx.calls.forEach((c, ci) =>
          assert.strictEqual(toHex(r.outSig.subarray(outLen * ci, outLen * (ci + 1))), c[key][outLen === 96 ? "sig96" : "sig192"], `group ${ci}, ${key}, ${outLen}`)
        );
      }
    }
  }
  const bad = (f) => assert.throws(f, RangeError);
  bad(() => addon.verifySameMessageAggregate(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, 0, null, 95));
  bad(() => addon.verifySameMessageAggregate(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, 0, include.subarray(1), 96));
  bad(() => addon.verifySameMessageAggregate(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, 2, null, 96));
  assert.throws(() => addon.verifySameMessageAggregate(v.ctx, groupFirst, msgs, pkBytes, null, sigs, sigLen, 96, 0, 0), TypeError);
  console.log("ok addon.verifySameMessageAggregate");

  // three concurrent calls: one device call, no submission
  const before = v.stats.sameMessageAggregations;
  const got = await Promise.all(calls.map((sets) => v.verifyAndAggregateSameMessage(sets, message, {batchable: true})));
  got.forEach((r, ci) => checkCall(r, ci, fx.calls[ci].agg, "concurrent"));
  assert.strictEqual(v.stats.sameMessageAggregations, before + 1, "one device call for the three calls");
  assert.strictEqual(v.stats.submissions, 0, "no verification submission beside it");
  assert.strictEqual(v.stats.sameMessageRetries, 2, "the two calls with a bad set were retried");
  assert.strictEqual(v.stats.sameMessageRetrySets, calls[1].length + calls[2].length);
  assert.strictEqual(v.canAcceptWork(), true, "idle again");
  console.log("ok three concurrent calls, one device call");

  // aggregate: false, alone and beside an unmasked call in one flush
  const two = await Promise.all([v.verifyAndAggregateSameMessage(maskedSets(2), message), v.verifyAndAggregateSameMessage(calls[0], message)]);
  checkCall(two[0], 2, fx.calls[2].masked, "masked");
  checkCall(two[1], 0, fx.calls[0].agg, "beside a masked call");
  assert.strictEqual(v.stats.sameMessageAggregations, before + 2, "the two calls shared one flush");
  const none = await v.verifyAndAggregateSameMessage(calls[0].map((s) => Object.assign({aggregate: false}, s)), message);
  assert.deepStrictEqual(none, {results: fx.calls[0].expected, signature: null, count: 0});
  console.log("ok aggregate: false");

  // table mode: the same keys by validator index
  v.uploadPubkeys(0, hex(fx.calls[0].sets.map((s) => s.pk).join("")));
  for (const ci of [0, 1]) {
    const sets = calls[ci].map((s, i) => ({publicKey: i, signature: s.signature}));
    checkCall(await v.verifyAndAggregateSameMessage(sets, message), ci, fx.calls[ci].agg, "table");
  }
  console.log("ok table mode");

  const blocks = new BlsGpuVerifier({sameMessageBlockCheck: true});
  const viaBlocks = await Promise.all([0, 1, 2].map((ci) => blocks.verifyAndAggregateSameMessage(ci === 1 ? maskedSets(1) : calls[ci], message)));
  viaBlocks.forEach((r, ci) => checkCall(r, ci, ci === 1 ? fx.calls[1].masked : fx.calls[ci].agg, "block check"));
  assert.strictEqual(blocks.stats.sameMessageAggregations, 1);
  await blocks.close();
  console.log("ok sameMessageBlockCheck");

  let empty = null;
  try {
    await v.verifyAndAggregateSameMessage([], message, {batchable: true});
  } catch (e) {
    empty = e;
  }
  assert.ok(empty && empty.message === "Empty results array", `empty sets: ${empty && empty.message}`);
  console.log("ok empty sets reject");

  // close() waits for outstanding calls, then refuses new ones
  const outstanding = [v.verifyAndAggregateSameMessage(calls[0], message), v.verifyAndAggregateSameMessage(calls[2], message)];
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
  checkCall(settled[0], 0, fx.calls[0].agg, "outstanding");
  checkCall(settled[1], 2, fx.calls[2].agg, "outstanding");
  let after = null;
  try {
    await v.verifyAndAggregateSameMessage(calls[0], message);
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
