"use strict";
// The compressed pubkey upload and the table readback through the JS drop-in on the GPU, against a fixture the Python
// side wrote from the oracle (tests/test_gpu_pubkeys_compressed_node.py): {pk48: [hex], pk96: [hex] (the oracle's
// decompression of each), bad: {offCurve, offGroup, offGroup96}, sets: [{pks: [table index], msg, sig, expected}]}.
//   - addon.uploadPubkeysCompressed / addon.readPubkeys: status, firstBad, both output lengths, a rejected call leaves
//     the table as it was, call-level refusals throw;
//   - verifier.uploadPubkeysCompressed / readPubkeys: a rejected key throws "BLST_ERROR: <NAME>" with
//     .index; a trusted upload stores an on-curve key outside G1, {validate: true} rejects it;
//   - one table-mode verifySignatureSets per set afterwards.
// Usage: node tests/node/pubkeys_compressed_gpu.js <fixture.json>   (exit code 0 = pass)
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..");
const {BlsGpuVerifier, addon} = require(path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs"));
const fx = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const hex = (h) => Uint8Array.from(Buffer.from(h, "hex"));
const NONE = 0xffffffff;

function thrown(fn) {
  try {
    fn();
  } catch (e) {
    return e;
  }
  return null;
}

async function main() {
  const n = fx.pk48.length;
  const all48 = hex(fx.pk48.join(""));
  const all96 = Buffer.from(fx.pk96.join(""), "hex");
  const v = new BlsGpuVerifier({seed: 0x4c4f4445}, {});

  // the addon's calls
  for (const validate of [false, true]) {
    const r = addon.uploadPubkeysCompressed(v.ctx, 0, all48, validate);
    assert.ok(r.status instanceof Int8Array && r.status.length === n && r.status.every((x) => x === 0));
    assert.strictEqual(r.firstBad, NONE);
    assert.strictEqual(addon.pubkeysCount(v.ctx), n);
  }
  const b96 = addon.readPubkeys(v.ctx, 0, n, 96);
  assert.ok(Buffer.isBuffer(b96) && b96.equals(all96));
  assert.ok(addon.readPubkeys(v.ctx, 0, n, 48).equals(Buffer.from(all48)));
  assert.ok(addon.readPubkeys(v.ctx, 3, 2, 96).equals(all96.subarray(3 * 96, 5 * 96)));
  assert.strictEqual(addon.readPubkeys(v.ctx, 0, 0, 96).length, 0);
  const mixed = Uint8Array.from(all48.subarray(0, 48 * 4));
  mixed.set(hex(fx.bad.offGroup), 48);
  mixed.set(hex(fx.bad.offCurve), 48 * 3);
  let r = addon.uploadPubkeysCompressed(v.ctx, 2, mixed, true);
  assert.deepStrictEqual(Array.from(r.status), [0, 3, 0, 2]);
  assert.strictEqual(r.firstBad, 1);
  r = addon.uploadPubkeysCompressed(v.ctx, 2, mixed, false);
  assert.deepStrictEqual(Array.from(r.status), [0, 0, 0, 2]);
  assert.strictEqual(r.firstBad, 3);
  assert.strictEqual(addon.pubkeysCount(v.ctx), n);
  assert.ok(addon.readPubkeys(v.ctx, 0, n, 48).equals(Buffer.from(all48)), "a rejected call writes nothing");
  let e = thrown(() => addon.uploadPubkeysCompressed(v.ctx, n + 1, all48, false));
  assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `upload beyond the table: ${e && e.message}`);
  assert.throws(() => addon.uploadPubkeysCompressed(v.ctx, 0, all48.subarray(0, 47), false), TypeError);
  for (const [first, m] of [[n, 1], [0, n + 1], [0, 0x80000000], [0xffffffff, 2]]) {
    e = thrown(() => addon.readPubkeys(v.ctx, first, m, 96));
    assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `read past the count (${first}, ${m}): ${e && e.message}`);
  }
  assert.throws(() => addon.readPubkeys(v.ctx, 0, 1, 47), RangeError);
  console.log("ok addon.uploadPubkeysCompressed / readPubkeys");

  // the verifier's methods
  const w = new BlsGpuVerifier({seed: 0x4c4f4445}, {});
  assert.strictEqual(addon.pubkeysCount(w.ctx), 0);
  assert.strictEqual(w.uploadPubkeysCompressed(0, all48), undefined);
  assert.strictEqual(addon.pubkeysCount(w.ctx), n);
  assert.ok(w.readPubkeys(0, n).equals(all96));
  assert.ok(w.readPubkeys(1, n - 1, {compressed: true}).equals(Buffer.from(all48.subarray(48))));
  e = thrown(() => w.uploadPubkeysCompressed(2, mixed, {validate: true}));
  assert.ok(e && e.message === "BLST_ERROR: BLST_POINT_NOT_IN_GROUP", `validate: ${e && e.message}`);
  assert.strictEqual(e.index, 3);
  e = thrown(() => w.uploadPubkeysCompressed(2, mixed));
  assert.ok(e && e.message === "BLST_ERROR: BLST_POINT_NOT_ON_CURVE", `trusted: ${e && e.message}`);
  assert.strictEqual(e.index, 5);
  assert.strictEqual(addon.pubkeysCount(w.ctx), n);
  assert.ok(w.readPubkeys(0, n, {compressed: true}).equals(Buffer.from(all48)));
  w.uploadPubkeysCompressed(n, hex(fx.bad.offGroup)); // trusted: stored as the 96-byte upload stores it
  assert.strictEqual(addon.pubkeysCount(w.ctx), n + 1);
  assert.ok(w.readPubkeys(n, 1).equals(Buffer.from(fx.bad.offGroup96, "hex")));
  console.log("ok verifier.uploadPubkeysCompressed / readPubkeys");

  // table-mode verification over the uploaded keys
  for (const [i, s] of fx.sets.entries()) {
    const set = s.pks.length === 1
      ? {type: "single", pubkey: s.pks[0], signingRoot: hex(s.msg), signature: hex(s.sig)}
      : {type: "aggregate", pubkeys: s.pks.slice(), signingRoot: hex(s.msg), signature: hex(s.sig)};
    assert.strictEqual(await w.verifySignatureSets([set]), s.expected, `set ${i}`);
  }
  assert.strictEqual(await w.verifySignatureSets(fx.sets.filter((s) => s.expected).map((s) => (
    {type: "aggregate", pubkeys: s.pks.slice(), signingRoot: hex(s.msg), signature: hex(s.sig)})), {batchable: true}), true);
  console.log("ok verifySignatureSets in table mode");

  await v.close();
  await w.close();
  console.log("ALL OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
