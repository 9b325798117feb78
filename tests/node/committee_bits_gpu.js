"use strict";
// The committee store and the aggregation from participation bits through the JS drop-in on the GPU, against a fixture
// the Python side wrote from the oracle (tests/test_gpu_committee_bits_node.py): {pk96: hex of the table, committees:
// [[table index]], sets: [[{committee, bits: hex, bitLen}]], expected96 / expected48: [hex | null (no participant)],
// raw: {setSegFirst, segCommittee, setBitsFirst, bits: hex} (the same sets as the addon takes them), complemented: n,
// verify: [{set, msg, sig}] (signatures under the summed secret keys of some sets)}.
//   - addon.uploadCommittees / committeesCount / aggregatePubkeysFromBits: bytes, status, stats, the flag, refusals;
//   - verifier.uploadCommittees / committeesCount / aggregatePubkeysFromBits: an empty set is the reference's Error;
//     the keys verify their sets' signatures through verifySignatureSets (bytes mode);
//   - the event loop stays live while the device works; close() waits for an outstanding call, a call after close()
//     rejects with QUEUE_ERROR_QUEUE_ABORTED; an overwriting pubkey upload empties the store.
// Usage: node tests/node/committee_bits_gpu.js <fixture.json>   (exit code 0 = pass)
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..");
const {BlsGpuVerifier, addon} = require(path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs"));
const fx = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const hex = (h) => Uint8Array.from(Buffer.from(h, "hex"));
const hexOf = (b) => Buffer.from(b).toString("hex");

async function rejected(p) {
  try {
    await p;
  } catch (e) {
    return e;
  }
  return null;
}
function thrown(fn) {
  try {
    fn();
  } catch (e) {
    return e;
  }
  return null;
}

async function main() {
  const pk96 = hex(fx.pk96);
  const n = fx.sets.length;
  const raw = {ssf: Uint32Array.from(fx.raw.setSegFirst), seg: Uint32Array.from(fx.raw.segCommittee),
               sbf: Uint32Array.from(fx.raw.setBitsFirst), bits: hex(fx.raw.bits)};
  const cf = Uint32Array.from(fx.committees.reduce((a, c) => a.concat([a[a.length - 1] + c.length]), [0]));
  const members = Uint32Array.from([].concat(...fx.committees));

  // the addon's calls
  const v = new BlsGpuVerifier({seed: 0x4c4f4445}, {});
  v.uploadPubkeys(0, pk96);
  assert.strictEqual(addon.committeesCount(v.ctx), 0);
  assert.strictEqual(addon.uploadCommittees(v.ctx, 0, cf, members), undefined);
  assert.strictEqual(addon.committeesCount(v.ctx), fx.committees.length);
  for (const [outLen, want] of [[96, fx.expected96], [48, fx.expected48]])
    for (const flag of [false, true]) {
      const r = await addon.aggregatePubkeysFromBits(v.ctx, raw.ssf, raw.seg, raw.sbf, raw.bits, flag, outLen);
      assert.ok(r.out instanceof Uint8Array && r.out.length === n * outLen && r.status instanceof Int8Array);
      want.forEach((w, i) => {
        assert.strictEqual(r.status[i], w === null ? 9 : 0, `status of set ${i}`);
        assert.strictEqual(hexOf(r.out.subarray(outLen * i, outLen * (i + 1))), w === null ? "00".repeat(outLen) : w,
                           `set ${i}, outLen ${outLen}, flag ${flag}`);
      });
      assert.strictEqual(r.stats.segments, raw.seg.length);
      assert.strictEqual(r.stats.segmentsComplemented, flag ? 0 : fx.complemented);
      assert.strictEqual(r.stats.keysSubtracted > 0, !flag);
      assert.strictEqual(r.stats.keysPresent, fx.keysPresent);
      assert.ok([8, 16, 32, 64].includes(r.stats.lanes) && r.stats.deviceMs > 0);
    }
  const badSeg = Uint32Array.from(raw.seg);
  badSeg[0] = fx.committees.length;
  let e = await rejected(addon.aggregatePubkeysFromBits(v.ctx, raw.ssf, badSeg, raw.sbf, raw.bits, false, 96));
  assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `a committee id beyond the count: ${e && e.message}`);
  assert.throws(() => addon.aggregatePubkeysFromBits(v.ctx, raw.ssf, raw.seg, raw.sbf, raw.bits, false, 47), RangeError);
  assert.throws(() => addon.aggregatePubkeysFromBits(v.ctx, raw.ssf, raw.seg, raw.sbf, raw.bits.subarray(1), false, 96),
                RangeError);
  assert.throws(() => addon.aggregatePubkeysFromBits(v.ctx, raw.ssf, raw.seg, raw.sbf, Array.from(raw.bits), false, 96),
                TypeError);
  e = thrown(() => addon.uploadCommittees(v.ctx, fx.committees.length + 1, cf, members));
  assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `a gap: ${e && e.message}`);
  e = thrown(() => addon.uploadCommittees(v.ctx, 0, cf, members.subarray(1)));
  assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `members shorter than the offsets: ${e && e.message}`);
  e = thrown(() => addon.uploadCommittees(v.ctx, 0, Uint32Array.from([0, 1]), Uint32Array.from([pk96.length / 96])));
  assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `a member beyond the table: ${e && e.message}`);
  assert.strictEqual(addon.committeesCount(v.ctx), fx.committees.length);
  addon.uploadCommittees(v.ctx, 2, Uint32Array.from([0]), new Uint32Array(0)); // n == 0 truncates
  assert.strictEqual(addon.committeesCount(v.ctx), 2);
  console.log("ok addon.uploadCommittees / aggregatePubkeysFromBits");

  // the verifier's methods
  const w = new BlsGpuVerifier({seed: 0x4c4f4445}, {});
  w.uploadPubkeys(0, pk96);
  w.uploadCommittees(0, fx.committees.slice(0, 3));
  w.uploadCommittees(w.committeesCount, fx.committees.slice(3));
  assert.strictEqual(w.committeesCount, fx.committees.length);
  const sets = fx.sets.map((s) => s.map((g) => ({committee: g.committee, bits: hex(g.bits), bitLen: g.bitLen})));
  const check = (got, want, what) => {
    assert.strictEqual(got.length, want.length);
    want.forEach((x, i) => {
      if (x === null) assert.ok(got[i] instanceof Error && got[i].message === "EMPTY_AGGREGATE_ARRAY", `${what}: set ${i}`);
      else assert.strictEqual(hexOf(got[i]), x, `${what}: set ${i}`);
    });
  };
  let ticked = false;
  setImmediate(() => (ticked = true));
  const first = await w.aggregatePubkeysFromBits(sets);
  assert.ok(ticked, "the event loop ran while the device worked");
  check(first, fx.expected96, "uncompressed");
  check(await w.aggregatePubkeysFromBits(sets, {compressed: true}), fx.expected48, "compressed");
  check(await w.aggregatePubkeysFromBits(sets, {noComplement: true}), fx.expected96, "noComplement");
  assert.deepStrictEqual(await w.aggregatePubkeysFromBits([]), []);
  e = await rejected(w.aggregatePubkeysFromBits([[{committee: 0, bits: Uint8Array.of(0xff), bitLen: 8}]]));
  assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `eight bits for a smaller committee: ${e && e.message}`);
  // the keys from bits verify their sets' signatures (bytes mode), another set's key does not
  for (const c of fx.verify) {
    const set = {type: "single", pubkey: first[c.set], signingRoot: hex(c.msg), signature: hex(c.sig)};
    assert.strictEqual(await w.verifySignatureSets([set]), true, `verify set ${c.set}`);
    const other = {type: "single", pubkey: first[c.other], signingRoot: hex(c.msg), signature: hex(c.sig)};
    assert.strictEqual(await w.verifySignatureSets([other]), false, `verify set ${c.set} under set ${c.other}'s key`);
  }
  console.log("ok verifier.uploadCommittees / aggregatePubkeysFromBits / verifySignatureSets");

  // an overwriting table upload empties the store; appending keeps it
  w.uploadPubkeys(pk96.length / 96, pk96.subarray(0, 96));
  assert.strictEqual(w.committeesCount, fx.committees.length);
  w.uploadPubkeys(0, pk96.subarray(0, 96));
  assert.strictEqual(w.committeesCount, 0);
  e = await rejected(w.aggregatePubkeysFromBits(sets));
  assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `the store was dropped: ${e && e.message}`);
  w.uploadCommittees(0, fx.committees);
  console.log("ok invalidation");

  // close() lets the outstanding call finish, then refuses new ones; the addon refuses to close under a call
  const pending = addon.aggregatePubkeysFromBits(v.ctx, raw.ssf.subarray(0, 1), raw.seg, raw.sbf.subarray(0, 1), raw.bits,
                                                 false, 96);
  e = thrown(() => addon.close(v.ctx));
  assert.ok(e && e.code === "BLSGPU_ERR_ARGS", `addon.close with a call outstanding: ${e && e.message}`);
  await pending;
  const last = w.aggregatePubkeysFromBits(sets);
  await w.close();
  check(await last, fx.expected96, "outstanding at close");
  e = await rejected(w.aggregatePubkeysFromBits(sets));
  assert.ok(e && e.message === "QUEUE_ERROR_QUEUE_ABORTED", `after close: ${e && e.message}`);
  await v.close();
  console.log("ok close");
  console.log("ALL OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
