"use strict";
/**
 * BlsGpuVerifier: the IBlsVerifier drop-in (reference packages/beacon-node/src/chain/bls/interface.ts:20-46)
 * over the blsgpu N-API addon.  It replaces BlsMultiThreadWorkerPool (multithread/index.ts) with the same
 * observable behaviour:
 *
 *   - verifySignatureSets(sets, opts) -> Promise<boolean>: true iff every set is valid; false if a
 *     well-formed set fails the pairing equation; rejects with "BLST_ERROR: <CODE>" when a signature
 *     fails to deserialize (maybeBatch.ts:23,36 -> Signature.fromBytes throws; multithread.test.ts:93-100),
 *     with "EMPTY_AGGREGATE_ARRAY" for an aggregate without pubkeys (utils.ts:11), and with the device
 *     status for a device error (never `false`, index.ts:368-375).
 *   - batchable jobs are buffered for up to MAX_BUFFER_WAIT_MS or until more than MAX_BUFFERED_SIGS sets
 *     are waiting, then submitted together; every job keeps its own result (index.ts:41-57, 238-285).
 *     Non-batchable jobs are submitted on the next macrotask, so a synchronous loop of calls coalesces
 *     into one submission (index.ts:276-283).
 *   - verifySignatureSetsSameMessage(sets, message, opts) -> Promise<boolean[]> (interface.ts; multithread/index.ts
 *     verifySignatureSetsSameMessage + jobItem.ts prepareWork / retry): the sets of the calls waiting in one flush are
 *     aggregated with randomness in ONE device call (blst-ts aggregateWithRandomness, which the reference runs on the
 *     main thread or a libuv worker), each call's (P, message, S) is verified as an ordinary job, and a call whose
 *     aggregate is rejected or does not verify is retried set by set; a bad signature is a `false`, never a throw.
 *     With the constructor option fusedSameMessage (default false) the flush is ONE addon.verifySameMessage call per
 *     pubkey mode instead: aggregation, the aggregates' checks and the per-set retry all on the device.
 *   - canAcceptWork(): fewer than MAX_JOBS_CAN_ACCEPT_WORK jobs pending (index.ts:60, 199-205).
 *   - close() rejects buffered and queued jobs with QUEUE_ERROR_QUEUE_ABORTED (index.ts:176-197) and
 *     destroys the device context.
 *
 * Pubkeys.  A set's pubkey (single) or each of its pubkeys (aggregate) is one of:
 *   - a validator index (number) into the device table filled by uploadPubkeys() from index2pubkey
 *     (state-transition/src/cache/pubkeyCache.ts:56-77) -- GPU aggregation, no main-thread
 *     PublicKey.aggregate (utils.ts:5-16);
 *   - an object registered with registerPubkey(obj, index) (a blst PublicKey, mapped by identity);
 *   - any PublicKey-like object with toBytes() (96 uncompressed affine bytes, PointFormat.uncompressed),
 *     or those 96 bytes as a Uint8Array -- what the pool sends its workers today (index.ts:160).  Aggregate
 *     sets of such keys (the gossip attestation call, attestation.ts:131-138) are aggregated on the GPU
 *     from the per-key bytes (bytes-aggregate mode), so no caller needs a registration pass.
 * A job is in table mode when all its keys are indexed, in bytes mode otherwise; a flush that mixes both
 * is split into one submission per mode.
 *
 * Metrics: the pool's blsThreadPool.* / bls.* series (metrics/metrics/lodestar.ts:382-458) are fed with the
 * GPU as the worker (workerId = "gpu"): jobsWorkerTime, timePerSigSet, jobWaitTime, queueLength,
 * totalJobsGroupsStarted, totalJobsStarted, totalSigSetsStarted, latencyToWorker, latencyFromWorker,
 * successJobsSignatureSetsCount, errorJobsSignatureSetsCount, batchRetries, batchSigsSuccess,
 * mainThreadDurationInThreadPool, aggregatedPubkeys.
 *
 * Also exported: BlsGpuSingleThreadVerifier (chain/bls/singleThread.ts:7-40 semantics: every call verified
 * on its own, immediately, with the maybe-batch rule), verifySignatureSet (state-transition
 * signatureSets.ts:24-38: Signature.verify / verifyAggregate), and the spec-conformance entry points
 * fastAggregateVerify / ethFastAggregateVerify (beacon-node/test/spec/general/bls.ts: untrusted keys
 * through KeyValidate, any error -> false).
 */
const path = require("path");

// CommonJS implementation (.cjs, so it stays CommonJS inside the "type": "module" beacon-node package); ESM callers
// import it through index.js, TypeScript through index.d.ts.  The module never writes process.env: the runtime sizes
// its slots to the hardware queues HIP gives the process (include/blsgpu.h blsgpu_init).
const addon = require(path.join(__dirname, "blsgpu_napi.node"));

const MAX_BUFFERED_SIGS = 32; // multithread/index.ts:48
const MAX_BUFFER_WAIT_MS = 100; // multithread/index.ts:57
const MAX_JOBS_CAN_ACCEPT_WORK = 512; // multithread/index.ts:60
const QUEUE_ABORTED = "QUEUE_ERROR_QUEUE_ABORTED"; // util/queue/errors.ts QueueErrorCode.QUEUE_ABORTED
const SIG_STRIDE = 192;

// job flags (include/blsgpu.h BLSGPU_JOB_*)
const JOB_BATCHABLE = 1;
const JOB_URGENT = 2;
const SAME_LANE_FORMS = 1; // BLSGPU_SAME_LANE_FORMS
const SAME_BLOCK_CHECK = 4; // BLSGPU_SAME_BLOCK_CHECK
const AV_VALIDATE_KEYS = 1; // BLSGPU_AV_VALIDATE_KEYS
const AV_LANE_FORMS = 2; // BLSGPU_AV_LANE_FORMS

// job codes (include/blsgpu.h enum blsgpu_code)
const CODE_EMPTY_AGGREGATE = 9;
const CODE_EMPTY_SET = 10;

class QueueError extends Error {
  constructor(type) {
    super(type.code);
    this.type = type;
  }
}

const SignatureSetType = {single: "single", aggregate: "aggregate"}; // signatureSets.ts:5-8

function jobError(code) {
  const name = addon.codeName(code) || `BLSGPU_${code}`;
  if (code === CODE_EMPTY_SET || code === CODE_EMPTY_AGGREGATE) return new Error(name);
  return new Error(`BLST_ERROR: ${name}`);
}

/**
 * The arrays of addon.aggregatePubkeysFromBits: a set's bit string is the concatenation, bit for bit, of its segments'
 * first bitLen bits, in exactly ceil(total / 8) bytes with zero padding.
 */
function packBitSets(sets) {
  const setSegFirst = new Uint32Array(sets.length + 1);
  const setBitsFirst = new Uint32Array(sets.length + 1);
  let nSegs = 0;
  sets.forEach((s, i) => {
    let total = 0;
    for (const seg of s) total += seg.bitLen;
    nSegs += s.length;
    setSegFirst[i + 1] = nSegs;
    setBitsFirst[i + 1] = setBitsFirst[i] + Math.ceil(total / 8);
  });
  const segCommittee = new Uint32Array(nSegs);
  const bits = new Uint8Array(setBitsFirst[sets.length]);
  let k = 0;
  sets.forEach((s, i) => {
    let pos = 8 * setBitsFirst[i];
    for (const seg of s) {
      segCommittee[k++] = seg.committee;
      for (let b = 0; b < seg.bitLen; b++, pos++)
        if ((seg.bits[b >> 3] >> (b & 7)) & 1) bits[pos >> 3] |= 1 << (pos & 7);
    }
  });
  return {setSegFirst, segCommittee, setBitsFirst, bits};
}

class BlsGpuVerifier {
  /**
   * @param {{devices?: number[], groupSets?: number, groupPolicy?: number, seed?: number,
   *          fusedSameMessage?: boolean, sameMessageBlockCheck?: boolean}} opts  fusedSameMessage (default false): a
   *          flush of same-message calls is ONE addon.verifySameMessage call per pubkey mode (aggregation, the
   *          aggregates' checks and the per-set retry on the device) instead of an aggregation call followed by
   *          verification jobs.  sameMessageBlockCheck (default false; only together with fusedSameMessage): that call
   *          checks the aggregates 1024 at a time under one final exponentiation (SAME_BLOCK_CHECK), the same answers
   * @param {{metrics?: object, logger?: object}} modules
   */
  constructor(opts = {}, modules = {}) {
    this.ctx = addon.init(opts.devices || null);
    if (opts.groupSets) addon.setOption(this.ctx, "group_sets", opts.groupSets);
    // 1 = the pool's job / request / chunk structure (batchRetries / batchSigsSuccess in the reference's units)
    if (opts.groupPolicy) addon.setOption(this.ctx, "group_policy", opts.groupPolicy);
    this.seed = opts.seed || 0; // 0 = OS CSPRNG batch scalars; fixed only for comparison runs
    this.fusedSameMessage = !!opts.fusedSameMessage;
    this.sameMessageBlockCheck = this.fusedSameMessage && !!opts.sameMessageBlockCheck;
    this.blockCheckOption = !!opts.sameMessageBlockCheck; // verifyAndAggregateSameMessage is always one device call
    // verifyOnMainThread calls are latency-critical exceptions to the pool (the block proposer signature): they run on
    // the device's urgent lane.  The single-thread verifier sends every call that way and keeps the shared pipeline.
    this.urgentMainThread = true;
    this.metrics = modules.metrics || null;
    this.closed = false;
    this.bufferedJobs = null; // {jobs, sigCount, timeout}
    this.queued = []; // non-batchable jobs waiting for the next macrotask
    this.queuedTimer = null;
    this.inflight = new Set();
    this.pkIndexOf = new WeakMap();
    this.stats = {submissions: 0, jobs: 0, sets: 0, groups: 0, batchRetries: 0, batchSigsSuccess: 0, uniqueMessages: 0};
    // same-message calls (blsThreadPool.sameMessageRetryJobs / sameMessageRetrySets; device aggregation calls)
    this.stats.sameMessageRetries = 0;
    this.stats.sameMessageRetrySets = 0;
    this.stats.sameMessageAggregations = 0;
    this.sameQueued = []; // same-message calls waiting for the next flush
    this.sameTimer = null;
    this.samePending = 0; // same-message calls not yet settled
    this.jobsOnDevice = 0; // jobs of submissions not yet completed
    this.queueLength = 0; // submissions on the device (blsThreadPool.queueLength)
    const m = this.metrics && this.metrics.blsThreadPool;
    if (m && m.queueLength && m.queueLength.addCollect) m.queueLength.addCollect(() => m.queueLength.set(this.queueLength));
  }

  /** index2pubkey sync: entries [firstIndex, firstIndex + n) as 96-byte uncompressed affine encodings. */
  uploadPubkeys(firstIndex, pk96) {
    addon.uploadPubkeys(this.ctx, firstIndex, pk96);
  }

  /**
   * The same sync from what the state holds: entries [firstIndex, firstIndex + n) from 48-byte compressed keys
   * (state.validators[i].pubkey concatenated), decompressed on the device.  The keys are trusted, as pubkeyCache.ts
   * trusts the state's; {validate: true} runs KeyValidate on each.  A rejected key throws "BLST_ERROR: <NAME>" with
   * .index its validator index; nothing is stored then.
   */
  uploadPubkeysCompressed(firstIndex, pk48, opts = {}) {
    const r = addon.uploadPubkeysCompressed(this.ctx, firstIndex, pk48, !!opts.validate);
    if (r.firstBad !== 0xffffffff) {
      const e = jobError(r.status[r.firstBad]);
      e.index = firstIndex + r.firstBad;
      throw e;
    }
  }

  /**
   * Entries [firstIndex, firstIndex + n) of the device table as a Buffer of 96-byte uncompressed encodings (what
   * PublicKey.fromBytes takes without a square root: index2pubkey can be hydrated from it) or, with
   * {compressed: true}, 48-byte compressed ones.
   */
  readPubkeys(firstIndex, n, opts = {}) {
    return addon.readPubkeys(this.ctx, firstIndex, n, opts.compressed ? 48 : 96);
  }

  /**
   * The epoch's shufflings on the device (epochCache getBeaconCommittee, the sync committee's indices): drops the stored
   * committees with id >= firstCommittee, then stores `committees` (arrays of validator indices into the device table)
   * as ids firstCommittee, firstCommittee + 1, ...  0 replaces the store, committeesCount appends the next epoch's.
   * Synchronous, like uploadPubkeys.  An upload that overwrites table rows empties the store.
   * @param {number} firstCommittee
   * @param {Array<ArrayLike<number>>} committees
   */
  uploadCommittees(firstCommittee, committees) {
    const committeeFirst = new Uint32Array(committees.length + 1);
    committees.forEach((c, i) => (committeeFirst[i + 1] = committeeFirst[i] + c.length));
    const members = new Uint32Array(committeeFirst[committees.length]);
    committees.forEach((c, i) => members.set(c, committeeFirst[i]));
    addon.uploadCommittees(this.ctx, firstCommittee, committeeFirst, members);
  }

  get committeesCount() {
    return addon.committeesCount(this.ctx);
  }

  /**
   * getAggregatedPubkey(set).toBytes() (chain/bls/utils.ts:5-16) for aggregate sets given the way they are born, as
   * committees plus participation bits, without expanding the bits on the main thread (getAttestingIndices,
   * getSyncCommitteeSignatureSet): one device call, off the main thread.  A set is an array of {committee: stored id,
   * bits: Uint8Array in SSZ bit order, bitLen: the committee's size} -- the uint8Array and bitLen of an ssz BitArray
   * (a Bitlist without its delimiter bit); bits from bitLen on are ignored.  Resolves to one entry per set: the key's bytes (96 uncompressed -- what verifySignatureSets takes as a
   * pubkey --, or 48 with {compressed: true}), or the Error "EMPTY_AGGREGATE_ARRAY" for a set without a participant.
   * Rejects for malformed input (BLSGPU_ERR_ARGS), a call-level failure or a closed verifier.
   * @param {Array<Array<{committee: number, bits: Uint8Array}>>} sets
   * @param {{compressed?: boolean, noComplement?: boolean}} opts
   * @returns {Promise<Array<Uint8Array | Error>>}
   */
  async aggregatePubkeysFromBits(sets, {compressed = false, noComplement = false} = {}) {
    if (this.closed) throw new QueueError({code: QUEUE_ABORTED});
    const {setSegFirst, segCommittee, setBitsFirst, bits} = packBitSets(sets);
    const outLen = compressed ? 48 : 96;
    const p = addon
      .aggregatePubkeysFromBits(this.ctx, setSegFirst, segCommittee, setBitsFirst, bits, noComplement, outLen)
      .then(
        (r) => sets.map((_, i) => (r.status[i] === 0 ? r.out.slice(outLen * i, outLen * (i + 1)) : jobError(r.status[i]))),
        (err) => {
          throw err.code === QUEUE_ABORTED ? new QueueError({code: QUEUE_ABORTED}) : err;
        }
      );
    this.inflight.add(p);
    p.finally(() => this.inflight.delete(p)).catch(() => {});
    return p;
  }

  registerPubkey(obj, index) {
    this.pkIndexOf.set(obj, index);
  }

  get deviceCount() {
    return addon.deviceCount(this.ctx);
  }

  /** A runtime tunable or property (include/blsgpu.h blsgpu_get_option: "slots", "hw_queues", "group_sets", ...). */
  getOption(key) {
    return addon.getOption(this.ctx, key);
  }

  /**
   * IBlsVerifier.verifySignatureSets (interface.ts:20-43).
   * @param {Array<{type: string, pubkey?: any, pubkeys?: any[], signingRoot: Uint8Array, signature: Uint8Array}>} sets
   * @param {{batchable?: boolean, verifyOnMainThread?: boolean}} opts
   * @returns {Promise<boolean>}
   */
  async verifySignatureSets(sets, opts = {}) {
    if (this.closed) throw new QueueError({code: QUEUE_ABORTED});
    if (this.metrics && this.metrics.bls && this.metrics.bls.aggregatedPubkeys) {
      let n = 0;
      for (const s of sets) if (s.type === SignatureSetType.aggregate) n += s.pubkeys.length;
      this.metrics.bls.aggregatedPubkeys.inc(n);
    }
    // the pool path chunks the call into jobs and ANDs their results: no jobs -> "Empty results array"
    // (multithread/index.ts:169-171); the main-thread path throws "Empty signature set" (maybeBatch.ts:29-31)
    if (sets.length === 0) throw new Error(opts.verifyOnMainThread ? "Empty signature set" : "Empty results array");
    const job = this.encodeJob(sets, opts);
    job.addedTimeMs = Date.now();
    const code = await new Promise((resolve, reject) => {
      job.resolve = resolve;
      job.reject = reject;
      if (opts.batchable && !opts.verifyOnMainThread) {
        if (!this.bufferedJobs) {
          this.bufferedJobs = {jobs: [], sigCount: 0, timeout: setTimeout(() => this.flushBuffered(), MAX_BUFFER_WAIT_MS)};
        }
        this.bufferedJobs.jobs.push(job);
        this.bufferedJobs.sigCount += job.sets.length;
        if (this.bufferedJobs.sigCount > MAX_BUFFERED_SIGS) {
          clearTimeout(this.bufferedJobs.timeout);
          this.flushBuffered();
        }
      } else if (opts.verifyOnMainThread) {
        // latency-critical (block proposal, interface.ts:8-17): no buffering at all, and on the device the urgent
        // lane (BLSGPU_JOB_URGENT)
        job.mainThread = true;
        this.dispatch([job]);
      } else {
        this.queued.push(job);
        if (!this.queuedTimer) {
          this.queuedTimer = setTimeout(() => {
            this.queuedTimer = null;
            const jobs = this.queued.splice(0, this.queued.length);
            this.dispatch(jobs);
          }, 0);
        }
      }
    });
    if (code < 0) throw jobError(-code);
    return code === 1;
  }

  /**
   * Signature.aggregate(group.map((s) => Signature.fromBytes(s, validate))).toBytes() for every group in one device
   * call: what the op pools do per inserted signature (chain/opPools/attestationPool.ts, aggregatedAttestationPool.ts,
   * syncCommitteeMessagePool.ts, syncContributionAndProofPool.ts), off the main thread (the addon runs the call on a
   * libuv worker).  Resolves to one entry per group: the aggregate's bytes (96 compressed, or 192 with
   * {compressed: false}), or -- for a rejected group -- the Error the reference throws for it ("BLST_ERROR: <NAME>"
   * of its first rejected signature, "EMPTY_AGGREGATE_ARRAY" for an empty group).  Rejects only for a call-level
   * failure or a closed verifier (QUEUE_ERROR_QUEUE_ABORTED).
   * @param {Uint8Array[][]} groups
   * @param {{validate?: boolean, compressed?: boolean}} opts
   * @returns {Promise<Array<Uint8Array | Error>>}
   */
  async aggregateSignatures(groups, {validate = true, compressed = true} = {}) {
    if (this.closed) throw new QueueError({code: QUEUE_ABORTED});
    let n = 0;
    let stride = 96;
    for (const g of groups)
      for (const s of g) {
        n++;
        if (s.length > 96) stride = SIG_STRIDE;
      }
    const groupFirst = new Uint32Array(groups.length + 1);
    const sigs = new Uint8Array(stride * n);
    const sigLen = new Uint32Array(n);
    let k = 0;
    groups.forEach((g, gi) => {
      groupFirst[gi] = k;
      for (const s of g) {
        sigLen[k] = s.length; // 96 / 192, anything else -> BLST_INVALID_SIZE for this group
        sigs.set(s.subarray(0, Math.min(s.length, stride)), stride * k);
        k++;
      }
    });
    groupFirst[groups.length] = k;
    const outLen = compressed ? 96 : SIG_STRIDE;
    const p = addon.aggregateSignatures(this.ctx, sigs, sigLen, stride, groupFirst, validate, outLen).then(
      (r) => groups.map((_, gi) => (r.status[gi] === 0 ? r.out.slice(outLen * gi, outLen * (gi + 1)) : jobError(r.status[gi]))),
      (err) => {
        throw err.code === QUEUE_ABORTED ? new QueueError({code: QUEUE_ABORTED}) : err;
      }
    );
    this.inflight.add(p);
    p.finally(() => this.inflight.delete(p)).catch(() => {});
    return p;
  }

  /**
   * IBlsVerifier.verifySignatureSetsSameMessage (interface.ts; multithread/index.ts): every set signs `message`.
   * Resolves to one boolean per set; a malformed or invalid signature is `false` there.  Rejects for no sets (as
   * verifySignatureSets does), a call-level failure or a closed verifier.
   * @param {Array<{publicKey: any, signature: Uint8Array}>} sets
   * @param {Uint8Array} message
   * @param {{batchable?: boolean}} opts
   * @returns {Promise<boolean[]>}
   */
  verifySignatureSetsSameMessage(sets, message, opts = {}) {
    return this.queueSameMessage(sets, message, opts, false);
  }

  /**
   * verifySignatureSetsSameMessage and, from the same device call, what the attestation pool does with the sets that
   * passed (attestationPool.add: Signature.aggregate of the pool's aggregate and each new signature): resolves to
   * {results: one boolean per set, signature: the 96-byte aggregate of the signatures that verified and whose set does
   * not say `aggregate: false` (a set the pool already holds is verified but not added again) or null when there is
   * none, count: how many were summed}.  Always one addon.verifySameMessageAggregate call per pubkey mode over the
   * calls waiting in one flush, whatever fusedSameMessage says; sameMessageBlockCheck is honoured.  Rejects as
   * verifySignatureSetsSameMessage does.
   * @param {Array<{publicKey: any, signature: Uint8Array, aggregate?: boolean}>} sets
   * @param {Uint8Array} message
   * @param {{batchable?: boolean}} opts
   * @returns {Promise<{results: boolean[], signature: Buffer | null, count: number}>}
   */
  verifyAndAggregateSameMessage(sets, message, opts = {}) {
    return this.queueSameMessage(sets, message, opts, true);
  }

  /** Both same-message methods (async: a throw here is a rejection; the wrappers add no promise of their own). */
  async queueSameMessage(sets, message, opts, aggregate) {
    if (this.closed) throw new QueueError({code: QUEUE_ABORTED});
    if (sets.length === 0) throw new Error(opts.verifyOnMainThread ? "Empty signature set" : "Empty results array");
    const refs = sets.map((s) => this.pkRef(s.publicKey));
    const table = refs.every((r) => r.index !== undefined);
    if (!table)
      for (const r of refs)
        if (r.bytes === undefined || r.bytes.length !== 96)
          throw new TypeError("BlsGpuVerifier: pubkeys of a bytes-mode job must serialize to 96 uncompressed bytes");
    const call = {sets, refs, table, message, batchable: !!opts.batchable, aggregate};
    this.samePending++;
    const p = new Promise((resolve, reject) => {
      call.resolve = resolve;
      call.reject = reject;
    });
    this.sameQueued.push(call);
    if (!this.sameTimer) this.sameTimer = setTimeout(() => this.flushSameMessage(), 0);
    this.inflight.add(p);
    p.finally(() => {
      this.samePending--;
      this.inflight.delete(p);
    }).catch(() => {});
    return p;
  }

  /** IBlsVerifier.canAcceptWork: true while fewer than MAX_JOBS_CAN_ACCEPT_WORK jobs are pending. */
  canAcceptWork() {
    const buffered = this.bufferedJobs ? this.bufferedJobs.jobs.length : 0;
    return buffered + this.queued.length + this.jobsOnDevice + this.samePending < MAX_JOBS_CAN_ACCEPT_WORK;
  }

  /** IBlsVerifier.close (interface.ts:45). */
  async close() {
    if (this.closed) return;
    this.closed = true;
    const pending = [];
    if (this.bufferedJobs) {
      clearTimeout(this.bufferedJobs.timeout);
      pending.push(...this.bufferedJobs.jobs);
      this.bufferedJobs = null;
    }
    if (this.queuedTimer) clearTimeout(this.queuedTimer);
    this.queuedTimer = null;
    pending.push(...this.queued.splice(0, this.queued.length));
    for (const job of pending) job.reject(new QueueError({code: QUEUE_ABORTED}));
    if (this.sameTimer) clearTimeout(this.sameTimer);
    this.sameTimer = null;
    for (const call of this.sameQueued.splice(0, this.sameQueued.length)) call.reject(new QueueError({code: QUEUE_ABORTED}));
    // in-flight submissions and aggregation calls complete (the device finishes them) before the context is freed
    await Promise.allSettled(Array.from(this.inflight));
    addon.close(this.ctx);
  }

  /**
   * AggregateVerify (blst-ts aggregateVerify(msgs, pks, sig)) for many jobs in ONE device call
   * (addon.aggregateVerify): jobs = [{pubkeys, messages, signature}], one aggregated signature over the pairs
   * (pubkeys[i], messages[i]), 32-byte messages.  Over the whole call the keys are all 96-byte uncompressed Uint8Arrays
   * (trusted), all 48-byte compressed or all 96-byte ones with {validateKeys: true} (KeyValidate on the device), or all
   * table indices (numbers; trusted).  Resolves to one number per job: 1 valid, 0 invalid, -code (9 for no pairs, else
   * the lowest-index rejected key's blst code, else the signature's).  Rejects for a call-level failure.
   */
  aggregateVerifyJobs(jobs, opts = {}) {
    if (this.closed) return Promise.reject(new QueueError({code: QUEUE_ABORTED}));
    if (jobs.length === 0) return Promise.resolve([]);
    const validate = !!opts.validateKeys;
    let n = 0;
    for (const j of jobs) {
      if (j.pubkeys.length !== j.messages.length) throw new TypeError("BlsGpuVerifier: aggregateVerifyJobs needs one message per key");
      n += j.pubkeys.length;
    }
    const first = jobs.find((j) => j.pubkeys.length > 0);
    const table = first !== undefined && typeof first.pubkeys[0] === "number";
    const pkLen = first === undefined || table ? 96 : first.pubkeys[0].length;
    if (table ? validate : !(pkLen === 96 || (validate && pkLen === 48)))
      throw new TypeError("BlsGpuVerifier: aggregateVerifyJobs keys are 96-byte, 48-byte with validateKeys, or table indices without it");
    const jobFirst = new Uint32Array(jobs.length + 1);
    const msgs = new Uint8Array(32 * n);
    const sigs = new Uint8Array(SIG_STRIDE * jobs.length);
    const sigLen = new Uint32Array(jobs.length);
    const pkIndex = table ? new Uint32Array(n) : null;
    const pkBytes = table ? null : new Uint8Array(pkLen * n);
    let k = 0;
    jobs.forEach((j, ji) => {
      jobFirst[ji] = k;
      sigLen[ji] = j.signature.length; // 96 / 192, anything else -> BLST_INVALID_SIZE
      sigs.set(j.signature.subarray(0, Math.min(j.signature.length, SIG_STRIDE)), SIG_STRIDE * ji);
      j.pubkeys.forEach((p, i) => {
        if (table ? typeof p !== "number" : typeof p === "number" || p.length !== pkLen)
          throw new TypeError("BlsGpuVerifier: aggregateVerifyJobs keys must all be of one kind and length");
        if (j.messages[i].length !== 32) throw new TypeError("BlsGpuVerifier: aggregateVerifyJobs messages are 32 bytes");
        if (table) pkIndex[k] = p;
        else pkBytes.set(p, pkLen * k);
        msgs.set(j.messages[i], 32 * k);
        k++;
      });
    });
    jobFirst[jobs.length] = k;
    const p = addon
      .aggregateVerify(this.ctx, jobFirst, msgs, pkBytes, pkLen, pkIndex, sigs, sigLen, SIG_STRIDE, validate ? AV_VALIDATE_KEYS : 0)
      .then(
        (r) => Array.from(r.jobResult),
        (err) => {
          throw err.code === QUEUE_ABORTED ? new QueueError({code: QUEUE_ABORTED}) : err;
        }
      );
    // close() waits for it: the device finishes the call before the context is freed
    this.inflight.add(p);
    p.finally(() => this.inflight.delete(p)).catch(() => {});
    return p;
  }

  // ------------------------------------------------------------------------------------ internals
  /** One device aggregation call per pubkey mode over the same-message calls that are waiting, one group per call. */
  flushSameMessage() {
    this.sameTimer = null;
    const calls = this.sameQueued.splice(0, this.sameQueued.length);
    for (const mode of [true, false]) {
      const part = calls.filter((c) => c.table === mode && !c.aggregate);
      if (part.length) this.aggregateSameMessage(part, mode);
      const agg = calls.filter((c) => c.table === mode && c.aggregate);
      if (agg.length) this.verifyAndAggregateFlush(agg, mode);
    }
  }

  /** The arrays of one device call over `calls`, one group per call. */
  packSameMessage(calls, tableMode) {
    let n = 0;
    for (const c of calls) n += c.sets.length;
    const groupFirst = new Uint32Array(calls.length + 1);
    const sigs = new Uint8Array(SIG_STRIDE * n);
    const sigLen = new Uint32Array(n);
    const pkIndex = tableMode ? new Uint32Array(n) : null;
    const pkBytes = tableMode ? null : new Uint8Array(96 * n);
    let k = 0;
    calls.forEach((c, ci) => {
      groupFirst[ci] = k;
      c.sets.forEach((s, i) => {
        sigLen[k] = s.signature.length; // 96 / 192, anything else -> BLST_INVALID_SIZE: the call is retried per set
        sigs.set(s.signature.subarray(0, Math.min(s.signature.length, SIG_STRIDE)), SIG_STRIDE * k);
        if (tableMode) pkIndex[k] = c.refs[i].index;
        else pkBytes.set(c.refs[i].bytes, 96 * k);
        k++;
      });
    });
    groupFirst[calls.length] = k;
    return {groupFirst, pkBytes, pkIndex, sigs, sigLen};
  }

  aggregateSameMessage(calls, tableMode) {
    const {groupFirst, pkBytes, pkIndex, sigs, sigLen} = this.packSameMessage(calls, tableMode);
    this.stats.sameMessageAggregations++;
    if (this.fusedSameMessage) return this.verifySameMessageFused(calls, groupFirst, pkBytes, pkIndex, sigs, sigLen);
    addon.aggregateWithRandomness(this.ctx, groupFirst, pkBytes, pkIndex, sigs, sigLen, SIG_STRIDE, this.seed, 96, SIG_STRIDE).then(
      (r) => {
        calls.forEach((c, ci) => {
          const done =
            r.status[ci] === 0
              ? this.verifySameMessageAggregate(c, r.outPk.slice(96 * ci, 96 * ci + 96), r.outSig.slice(SIG_STRIDE * ci, SIG_STRIDE * (ci + 1)))
              : this.retrySameMessage(c);
          done.then(c.resolve, c.reject);
        });
      },
      (err) => {
        // call-level failure (device error, entropy, closed context): reject every call, never resolve false
        for (const c of calls) c.reject(err.code === QUEUE_ABORTED ? new QueueError({code: QUEUE_ABORTED}) : err);
      }
    );
  }

  /**
   * fusedSameMessage: the whole method in one device call.  Call i resolves to one boolean per set (true iff its
   * result is 1: a rejected set is false, as in the per-set retry); a group verified set by set counts as one retry.
   */
  verifySameMessageFused(calls, groupFirst, pkBytes, pkIndex, sigs, sigLen) {
    const msgs = new Uint8Array(32 * calls.length);
    calls.forEach((c, ci) => msgs.set(c.message.subarray(0, 32), 32 * ci));
    const flags = this.sameMessageBlockCheck ? SAME_BLOCK_CHECK : 0;
    addon.verifySameMessage(this.ctx, groupFirst, msgs, pkBytes, pkIndex, sigs, sigLen, SIG_STRIDE, this.seed, flags).then(
      (r) => {
        const m = this.metrics && this.metrics.blsThreadPool;
        calls.forEach((c, ci) => {
          if (r.groupResult[ci] !== 1) {
            this.stats.sameMessageRetries++;
            this.stats.sameMessageRetrySets += c.sets.length;
            if (m && m.sameMessageRetryJobs) m.sameMessageRetryJobs.inc(1);
            if (m && m.sameMessageRetrySets) m.sameMessageRetrySets.inc(c.sets.length);
          }
          c.resolve(Array.from(r.setResult.subarray(groupFirst[ci], groupFirst[ci + 1]), (x) => x === 1));
        });
      },
      (err) => {
        // call-level failure (device error, entropy, closed context): reject every call, never resolve false
        for (const c of calls) c.reject(err.code === QUEUE_ABORTED ? new QueueError({code: QUEUE_ABORTED}) : err);
      }
    );
  }

  /**
   * verifyAndAggregateSameMessage: the waiting calls of one pubkey mode in one addon.verifySameMessageAggregate call.
   * Call i resolves to its sets' booleans and the aggregate of its group; stats and metrics as verifySameMessageFused.
   */
  verifyAndAggregateFlush(calls, tableMode) {
    const {groupFirst, pkBytes, pkIndex, sigs, sigLen} = this.packSameMessage(calls, tableMode);
    const msgs = new Uint8Array(32 * calls.length);
    calls.forEach((c, ci) => msgs.set(c.message.subarray(0, 32), 32 * ci));
    let include = null;
    if (calls.some((c) => c.sets.some((s) => s.aggregate === false))) {
      include = new Uint8Array(groupFirst[calls.length]).fill(1);
      calls.forEach((c, ci) => c.sets.forEach((s, i) => (include[groupFirst[ci] + i] = s.aggregate === false ? 0 : 1)));
    }
    const flags = this.blockCheckOption ? SAME_BLOCK_CHECK : 0;
    this.stats.sameMessageAggregations++;
    addon
      .verifySameMessageAggregate(this.ctx, groupFirst, msgs, pkBytes, pkIndex, sigs, sigLen, SIG_STRIDE, this.seed, flags, include, 96)
      .then(
        (r) => {
          const m = this.metrics && this.metrics.blsThreadPool;
          calls.forEach((c, ci) => {
            if (r.groupResult[ci] !== 1) {
              this.stats.sameMessageRetries++;
              this.stats.sameMessageRetrySets += c.sets.length;
              if (m && m.sameMessageRetryJobs) m.sameMessageRetryJobs.inc(1);
              if (m && m.sameMessageRetrySets) m.sameMessageRetrySets.inc(c.sets.length);
            }
            const count = r.aggCount[ci];
            c.resolve({
              results: Array.from(r.setResult.subarray(groupFirst[ci], groupFirst[ci + 1]), (x) => x === 1),
              signature: count ? Buffer.from(r.outSig.slice(96 * ci, 96 * ci + 96)) : null,
              count,
            });
          });
        },
        (err) => {
          // call-level failure (device error, entropy, closed context): reject every call, never resolve false
          for (const c of calls) c.reject(err.code === QUEUE_ABORTED ? new QueueError({code: QUEUE_ABORTED}) : err);
        }
      );
  }

  /** (P, message, S) as its own ordinary job; anything but `true` retries the call's sets one by one. */
  async verifySameMessageAggregate(call, pk96, sig192) {
    let ok = false;
    try {
      ok = await this.verifySignatureSets(
        [{type: SignatureSetType.single, pubkey: pk96, signingRoot: call.message, signature: sig192}],
        {batchable: call.batchable}
      );
    } catch (e) {
      if (e instanceof QueueError || e.code) throw e; // call-level failure; a job error (BLST_ERROR) retries
    }
    if (ok) return call.sets.map(() => true);
    return this.retrySameMessage(call);
  }

  /** Every set of the call as a one-set job, all in one submission: entry i is true iff its job's result is 1. */
  retrySameMessage(call) {
    if (this.closed) return Promise.reject(new QueueError({code: QUEUE_ABORTED}));
    this.stats.sameMessageRetries++;
    this.stats.sameMessageRetrySets += call.sets.length;
    const m = this.metrics && this.metrics.blsThreadPool;
    if (m && m.sameMessageRetryJobs) m.sameMessageRetryJobs.inc(1);
    if (m && m.sameMessageRetrySets) m.sameMessageRetrySets.inc(call.sets.length);
    const jobs = [];
    const results = call.sets.map(
      (s) =>
        new Promise((resolve, reject) => {
          const job = this.encodeJob(
            [{type: SignatureSetType.single, pubkey: s.publicKey, signingRoot: call.message, signature: s.signature}],
            {batchable: call.batchable}
          );
          job.addedTimeMs = Date.now();
          job.resolve = resolve;
          job.reject = reject;
          jobs.push(job);
        })
    );
    this.dispatch(jobs);
    return Promise.all(results).then((codes) => codes.map((c) => c === 1));
  }

  flushBuffered() {
    const b = this.bufferedJobs;
    this.bufferedJobs = null;
    if (b && b.jobs.length) this.dispatch(b.jobs);
  }

  pkRef(pk) {
    if (typeof pk === "number") return {index: pk};
    if (pk instanceof Uint8Array) return {bytes: pk};
    if (pk && typeof pk === "object") {
      const idx = this.pkIndexOf.get(pk);
      const ref = {};
      if (idx !== undefined) ref.index = idx;
      // keep the bytes too (when the object serializes), so a job mixing registered and plain keys can go
      // in bytes-aggregate mode
      if (typeof pk.toBytes === "function") ref.bytes = pk.toBytes();
      if (ref.index !== undefined || ref.bytes !== undefined) return ref;
    }
    throw new TypeError("BlsGpuVerifier: pubkey must be an index, a registered object, a PublicKey or 96 bytes");
  }

  encodeJob(sets, opts) {
    const enc = [];
    let allIndexed = true;
    for (const s of sets) {
      const refs = s.type === SignatureSetType.aggregate ? s.pubkeys.map((p) => this.pkRef(p)) : [this.pkRef(s.pubkey)];
      for (const r of refs) if (r.index === undefined) allIndexed = false;
      enc.push({refs, msg: s.signingRoot, sig: s.signature, aggregate: s.type === SignatureSetType.aggregate});
    }
    if (!allIndexed) {
      for (const e of enc)
        for (const r of e.refs)
          if (r.bytes === undefined || r.bytes.length !== 96)
            throw new TypeError("BlsGpuVerifier: pubkeys of a bytes-mode job must serialize to 96 uncompressed bytes");
    }
    return {sets: enc, table: allIndexed, batchable: !!opts.batchable};
  }

  dispatch(jobs) {
    const table = jobs.filter((j) => j.table);
    const bytes = jobs.filter((j) => !j.table);
    if (table.length) this.submit(table, true);
    if (bytes.length) this.submit(bytes, false);
  }

  submit(jobs, tableMode) {
    let nSets = 0;
    let nPk = 0;
    for (const j of jobs) {
      nSets += j.sets.length;
      for (const s of j.sets) nPk += s.refs.length;
    }
    const jobFirstSet = new Uint32Array(jobs.length + 1);
    const jobFlags = new Uint8Array(jobs.length);
    const msgs = new Uint8Array(32 * nSets);
    const sigs = new Uint8Array(SIG_STRIDE * nSets);
    const sigLen = new Uint32Array(nSets);
    const setPkFirst = new Uint32Array(nSets + 1);
    const req = {jobFirstSet, jobFlags, msgs, sigs, sigLen, sigStride: SIG_STRIDE, seed: this.seed, setPkFirst};
    let pkIndex, pkBytes;
    if (tableMode) {
      pkIndex = req.pkIndex = new Uint32Array(Math.max(nPk, 1));
    } else {
      pkBytes = req.pkBytes = new Uint8Array(Math.max(96 * nPk, 96));  // bytes-aggregate mode
    }
    let i = 0;
    let k = 0;
    const now = Date.now();
    const m = this.metrics && this.metrics.blsThreadPool;
    jobs.forEach((j, ji) => {
      jobFirstSet[ji] = i;
      // BLSGPU_JOB_BATCHABLE, and BLSGPU_JOB_URGENT for verifyOnMainThread jobs: the runtime runs those on the
      // device's urgent lane, never queued behind or merged with the gossip flood (multithread/index.ts:138-151)
      jobFlags[ji] = (j.batchable ? JOB_BATCHABLE : 0) | (j.mainThread && this.urgentMainThread ? JOB_URGENT : 0);
      if (m && m.jobWaitTime && j.addedTimeMs) m.jobWaitTime.observe((now - j.addedTimeMs) / 1000);
      for (const s of j.sets) {
        msgs.set(s.msg.subarray(0, 32), 32 * i);
        const sl = s.sig.length;
        sigLen[i] = sl; // 96 / 192, anything else -> BLST_INVALID_SIZE for this job
        sigs.set(s.sig.subarray(0, Math.min(sl, SIG_STRIDE)), SIG_STRIDE * i);
        setPkFirst[i] = k;
        for (const r of s.refs) {
          if (tableMode) pkIndex[k] = r.index;
          else pkBytes.set(r.bytes, 96 * k);
          k++;
        }
        i++;
      }
    });
    jobFirstSet[jobs.length] = nSets;
    setPkFirst[nSets] = k;
    if (m) {
      if (m.totalJobsGroupsStarted) m.totalJobsGroupsStarted.inc(1);
      if (m.totalJobsStarted) m.totalJobsStarted.inc(jobs.length);
      if (m.totalSigSetsStarted) m.totalSigSetsStarted.inc(nSets);
    }
    const submitNs = process.hrtime.bigint();
    this.queueLength += 1;
    this.jobsOnDevice += jobs.length;
    const p = addon.submit(this.ctx, req).then(
      (out) => {
        this.queueLength -= 1;
        this.jobsOnDevice -= jobs.length;
        const st = this.stats;
        st.submissions++;
        st.jobs += jobs.length;
        st.sets += nSets;
        st.groups += out.groups;
        st.batchRetries += out.batchRetries;
        st.batchSigsSuccess += out.batchSigsSuccess;
        st.uniqueMessages += out.uniqueMessages;
        if (out.urgentLane) st.urgentCalls = (st.urgentCalls || 0) + 1;
        let okSets = 0;
        let errSets = 0;
        jobs.forEach((j, ji) => (out.results[ji] < 0 ? (errSets += j.sets.length) : (okSets += j.sets.length)));
        if (m) {
          // the device is the worker: its time is the call's device phase; the rest is host <-> device latency
          const totalSec = Number(process.hrtime.bigint() - submitNs) / 1e9;
          const devSec = out.deviceMs / 1000;
          if (m.jobsWorkerTime) m.jobsWorkerTime.inc({workerId: "gpu"}, devSec);
          if (m.timePerSigSet && nSets) m.timePerSigSet.observe(devSec / nSets);
          if (m.latencyToWorker) m.latencyToWorker.observe(Math.max(0, (totalSec - devSec) / 2));
          if (m.latencyFromWorker) m.latencyFromWorker.observe(Math.max(0, (totalSec - devSec) / 2));
          if (m.successJobsSignatureSetsCount) m.successJobsSignatureSetsCount.inc(okSets);
          if (m.errorJobsSignatureSetsCount) m.errorJobsSignatureSetsCount.inc(errSets);
          if (m.batchRetries) m.batchRetries.inc(out.batchRetries);
          if (m.batchSigsSuccess) m.batchSigsSuccess.inc(out.batchSigsSuccess);
          if (m.mainThreadDurationInThreadPool && jobs.some((j) => j.mainThread))
            m.mainThreadDurationInThreadPool.observe(totalSec);
        }
        jobs.forEach((j, ji) => j.resolve(out.results[ji]));
      },
      (err) => {
        this.queueLength -= 1;
        this.jobsOnDevice -= jobs.length;
        // call-level failure (device error, closed context): reject every job, never resolve false
        for (const j of jobs) j.reject(err.code === QUEUE_ABORTED ? new QueueError({code: QUEUE_ABORTED}) : err);
      }
    );
    this.inflight.add(p);
    p.finally(() => this.inflight.delete(p));
  }
}

/**
 * BlsSingleThreadVerifier semantics (chain/bls/singleThread.ts:7-40): every call is verified on its own,
 * immediately (no buffering, no batching with other calls), by verifySignatureSetsMaybeBatch over its sets;
 * errors reject.  Same device path: one non-batchable job per call.
 */
class BlsGpuSingleThreadVerifier extends BlsGpuVerifier {
  constructor(opts = {}, modules = {}) {
    super(opts, modules);
    // every call is "main thread" here, so none is an exception: calls share the device pipeline (no urgent lane, which
    // runs one burst of calls at a time)
    this.urgentMainThread = false;
  }

  async verifySignatureSets(sets) {
    if (sets.length === 0) throw new Error("Empty signature set");
    return super.verifySignatureSets(sets, {verifyOnMainThread: true});
  }
}

/**
 * verifySignatureSet (state-transition/src/util/signatureSets.ts:24-38): single -> Signature.verify,
 * aggregate -> Signature.verifyAggregate (FastAggregateVerify over trusted keys).  Rejects like
 * Signature.fromBytes(validate = true) on a malformed signature.
 */
async function verifySignatureSet(verifier, set) {
  return verifier.verifySignatureSets([set], {verifyOnMainThread: true});
}

const G1_INFINITY_48 = (() => {
  const b = new Uint8Array(48);
  b[0] = 0xc0;
  return b;
})();
const G2_INFINITY_96 = (() => {
  const b = new Uint8Array(96);
  b[0] = 0xc0;
  return b;
})();
const sameBytes = (a, b) => a.length === b.length && a.every((x, i) => x === b[i]);

/**
 * fast_aggregate_verify of the spec runner (beacon-node/test/spec/general/bls.ts): untrusted 48-byte keys
 * through KeyValidate (PublicKey.fromBytes(validate = true)), the signature through Signature.fromBytes
 * (validate = true); any error -> false.
 */
async function fastAggregateVerify(verifier, pubkeys48, message, signature) {
  if (pubkeys48.length === 0) return false; // EMPTY_AGGREGATE_ARRAY -> caught -> false
  const flat = new Uint8Array(48 * pubkeys48.length);
  pubkeys48.forEach((p, i) => flat.set(p.subarray(0, 48), 48 * i));
  if (pubkeys48.some((p) => p.length !== 48)) return false;
  const kv = addon.keyValidate(verifier.ctx, flat, 48);
  if (kv.status.some((s) => s !== 0)) return false;
  const keys = [];
  for (let i = 0; i < pubkeys48.length; i++) keys.push(kv.pk96.subarray(96 * i, 96 * i + 96));
  try {
    return await verifier.verifySignatureSets(
      [{type: SignatureSetType.aggregate, pubkeys: keys, signingRoot: message, signature}],
      {verifyOnMainThread: true}
    );
  } catch (e) {
    return false;
  }
}

/** eth_fast_aggregate_verify (spec runner): no keys + infinity signature -> true; an infinity key -> false. */
async function ethFastAggregateVerify(verifier, pubkeys48, message, signature) {
  if (pubkeys48.length === 0 && sameBytes(signature, G2_INFINITY_96)) return true;
  if (pubkeys48.some((p) => sameBytes(p, G1_INFINITY_48))) return false;
  return fastAggregateVerify(verifier, pubkeys48, message, signature);
}

/**
 * aggregate_verify of the spec runner (beacon-node/test/spec/general/bls.ts): blst-ts aggregateVerify(msgs, pks, sig)
 * over untrusted 48-byte keys, a message per key; any error, a length mismatch or no pairs -> false.
 */
async function aggregateVerify(verifier, pubkeys48, messages, signature) {
  try {
    if (pubkeys48.length === 0 || pubkeys48.length !== messages.length) return false;
    if (pubkeys48.some((p) => p.length !== 48)) return false;
    const r = await verifier.aggregateVerifyJobs([{pubkeys: pubkeys48, messages, signature}], {validateKeys: true});
    return r[0] === 1;
  } catch (e) {
    return false;
  }
}

module.exports = {
  BlsGpuVerifier,
  BlsGpuSingleThreadVerifier,
  verifySignatureSet,
  fastAggregateVerify,
  ethFastAggregateVerify,
  aggregateVerify,
  AV_VALIDATE_KEYS,
  AV_LANE_FORMS,
  QueueError,
  SignatureSetType,
  MAX_BUFFERED_SIGS,
  MAX_BUFFER_WAIT_MS,
  MAX_JOBS_CAN_ACCEPT_WORK,
  JOB_BATCHABLE,
  JOB_URGENT,
  SAME_LANE_FORMS,
  SAME_BLOCK_CHECK,
  addon,
};
