"use strict";
// BlsGpuVerifier.aggregateSignatures on the GPU against a fixture the Python side wrote from the oracle
// (tests/test_gpu_sig_aggregate_node.py): {groups: [[hex]], expected: [hex | {error}], expected192: [...]}.
//   - every group byte-equal to the oracle's aggregate, compressed and uncompressed;
//   - a rejected group is an Error with the reference's message, and does not affect its neighbours;
//   - the event loop stays live while the device works: a setImmediate fires before the promise settles;
//   - close() waits for an outstanding aggregation; an aggregation after close() rejects with
//     QUEUE_ERROR_QUEUE_ABORTED.
// Usage: node tests/node/aggregate_gpu.js <fixture.json>   (exit code 0 = pass)
const assert = require("assert");
const fs = require("fs");
const path = require("path");

const ROOT = path.join(__dirname, "..", "..");
const {BlsGpuVerifier, BlsGpuSingleThreadVerifier} = require(path.join(ROOT, "lodestar_amd", "node", "BlsGpuVerifier.cjs"));
const fx = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
const hex = (h) => Uint8Array.from(Buffer.from(h, "hex"));
const toHex = (b) => Buffer.from(b).toString("hex");

function check(got, want, label) {
  assert.strictEqual(got.length, want.length, `${label}: one entry per group`);
  want.forEach((w, g) => {
    if (typeof w === "string") {
      assert.ok(got[g] instanceof Uint8Array, `${label} group ${g}: ${got[g]}`);
      assert.strictEqual(toHex(got[g]), w, `${label} group ${g}`);
    } else {
      assert.ok(got[g] instanceof Error, `${label} group ${g}: expected an Error`);
      assert.strictEqual(got[g].message, w.error, `${label} group ${g}`);
    }
  });
}

async function main() {
  const groups = fx.groups.map((g) => g.map(hex));
  const v = new BlsGpuVerifier({seed: 7});

  let immediates = 0;
  let settled = false;
  const tick = () => {
    if (settled) return;
    immediates++;
    setImmediate(tick);
  };
  const p = v.aggregateSignatures(groups).then((r) => {
    settled = true;
    return r;
  });
  setImmediate(tick);
  const got = await p;
  assert.ok(immediates >= 1, "a setImmediate callback ran before the aggregation settled");
  check(got, fx.expected, "compressed");
  console.log(`ok aggregate (${immediates} event-loop turns while in flight)`);

  check(await v.aggregateSignatures(groups, {compressed: false}), fx.expected192, "uncompressed");
  console.log("ok uncompressed");

  check(await v.aggregateSignatures(groups, {validate: false}), fx.expectedNoValidate, "validate=false");
  console.log("ok validate=false");

  assert.deepStrictEqual(await v.aggregateSignatures([]), []);
  console.log("ok no groups");

  // close() lets the outstanding call finish, then refuses new ones
  const last = v.aggregateSignatures(groups);
  await v.close();
  check(await last, fx.expected, "outstanding at close");
  let after = null;
  try {
    await v.aggregateSignatures(groups);
  } catch (e) {
    after = e;
  }
  assert.ok(after && after.message === "QUEUE_ERROR_QUEUE_ABORTED", `after close: ${after && after.message}`);
  console.log("ok close");

  const st = new BlsGpuSingleThreadVerifier({seed: 7});
  check(await st.aggregateSignatures(groups), fx.expected, "single-thread verifier");
  await st.close();
  console.log("ok single-thread verifier");
  console.log("ALL OK");
}

main().catch((e) => {
  console.error(e);
  process.exit(1);
});
