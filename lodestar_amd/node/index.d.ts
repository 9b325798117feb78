// Types of the IBlsVerifier drop-in, for packages/beacon-node/src/chain/bls/gpu/ (next to interface.ts, reference
// packages/beacon-node/src/chain/bls/interface.ts:20-46, and the ISignatureSet union of
// state-transition/src/util/signatureSets.ts:10-22).
import type {ISignatureSet} from "@lodestar/state-transition";
import type {IBlsVerifier, VerifySignatureOpts} from "../interface.js";

/** A set's pubkey as the drop-in takes it: a validator index into the device table (uploadPubkeys), a PublicKey
 * registered with registerPubkey, any object serializing to 96 uncompressed bytes (blst PublicKey.toBytes()), or
 * those bytes. */
export type GpuPubkey = number | Uint8Array | {toBytes(format?: unknown): Uint8Array};

export type BlsGpuVerifierOpts = {
  /** HIP devices to shard calls over (default: every visible device) */
  devices?: number[];
  /** sets per batch group (default 1024) */
  groupSets?: number;
  /** 0 = batch groups of >= groupSets sets (default); 1 = the pool's jobs / requests / >= 16-job chunks, so the
   * batchRetries / batchSigsSuccess metrics count the reference's units */
  groupPolicy?: 0 | 1;
  /** batch-scalar seed for comparison runs; 0 / undefined = OS CSPRNG */
  seed?: number;
  /** true: a flush of same-message calls is one addon.verifySameMessage call per pubkey mode -- the aggregation, every
   * aggregate's pairing check and the per-set retry of the groups that fail, without leaving the device (default
   * false: an aggregation call, then verification jobs) */
  fusedSameMessage?: boolean;
  /** true, together with fusedSameMessage: that call passes SAME_BLOCK_CHECK -- the aggregates are checked 1024 at a
   * time under one final exponentiation, and only the groups of a block that fails one by one; the same answers
   * (default false; ignored without fusedSameMessage, except by verifyAndAggregateSameMessage, which is always one
   * device call) */
  sameMessageBlockCheck?: boolean;
};

/** What addon.verifySameMessageAggregate resolves to (blsgpu_verify_same_message_agg): SameMessageResult and
 * outSig (outSigLen bytes per group, zeros for a group that summed nothing), aggCount (the sets summed per group). */
export type SameMessageAggregateResult = SameMessageResult & {outSig: Uint8Array; aggCount: Uint32Array};
/** What addon.verifySameMessage resolves to (blsgpu_verify_same_message). */
export type SameMessageResult = {
  /** per set: 1 valid, 0 invalid, -code rejected */
  setResult: Int8Array;
  /** per group: 1 accepted as a whole, 0 verified set by set, -9 empty */
  groupResult: Int8Array;
  stats: {
    groupsAccepted: number;
    groupsRetried: number;
    retrySets: number;
    uniqueMessages: number;
    /** bit 0: group phase took the lane forms, bit 1: retry phase did; with SAME_BLOCK_CHECK bit 2: the block phase
     * ran, bit 3: some block failed and the per-group descent ran, bit 4: the descent's checks took the lane forms */
    form: number;
    deviceMs: number;
  };
};

/** One job of BlsGpuVerifier.aggregateVerifyJobs: pubkeys[i] signs messages[i] under the one aggregated signature. */
export type AggregateVerifyJob = {
  pubkeys: Uint8Array[] | number[];
  messages: Uint8Array[];
  signature: Uint8Array;
};

/** What addon.aggregateVerify resolves to (blsgpu_aggregate_verify). */
export type AggregateVerifyResult = {
  /** per job: 1 valid, 0 invalid, -code rejected */
  jobResult: Int8Array;
  /** per job: the call index of its lowest-index rejected key, 0xffffffff when none */
  firstBad: Uint32Array;
  stats: {
    pairs: number;
    uniqueMessages: number;
    millerItems: number;
    millerChunks: number;
    /** 0 cooperative, 1 lane forms */
    form: number;
    jobsChecked: number;
    deviceMs: number;
  };
};

export type BlsGpuVerifierModules = {
  metrics?: unknown | null;
  logger?: unknown;
};

export declare class QueueError extends Error {
  type: {code: string};
}

export declare class BlsGpuVerifier implements IBlsVerifier {
  constructor(opts?: BlsGpuVerifierOpts, modules?: BlsGpuVerifierModules);
  /** IBlsVerifier.verifySignatureSets: true iff every set verifies; rejects with "BLST_ERROR: <CODE>" where the
   * reference's Signature.fromBytes throws, "QUEUE_ERROR_QUEUE_ABORTED" once closed. */
  verifySignatureSets(sets: ISignatureSet[], opts?: VerifySignatureOpts): Promise<boolean>;
  /** IBlsVerifier.verifySignatureSetsSameMessage: one boolean per set, all signing `message`.  The calls waiting in
   * one flush share one device aggregateWithRandomness call; each call's (P, message, S) is verified as an ordinary
   * job, and a call whose aggregate is rejected or does not verify is retried set by set (stats.sameMessageRetries).
   * A malformed or invalid signature is `false`; rejects for no sets, a call-level failure or once closed. */
  verifySignatureSetsSameMessage(
    sets: {publicKey: GpuPubkey; signature: Uint8Array}[],
    message: Uint8Array,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread">
  ): Promise<boolean[]>;
  /** verifySignatureSetsSameMessage and, from the same device call (addon.verifySameMessageAggregate,
   * blsgpu_verify_same_message_agg), the aggregate the attestation pool folds in: `signature` is Signature.toBytes()
   * (96 bytes) of the sum of the signatures that verified and whose set does not say `aggregate: false` (a set the pool
   * already holds: verified, not added again), null when there is none; `count` is how many were summed.  The calls
   * waiting in one flush share one device call per pubkey mode whatever fusedSameMessage says; sameMessageBlockCheck is
   * honoured.  Rejects as verifySignatureSetsSameMessage does. */
  verifyAndAggregateSameMessage(
    sets: {publicKey: GpuPubkey; signature: Uint8Array; aggregate?: boolean}[],
    message: Uint8Array,
    opts?: Omit<VerifySignatureOpts, "verifyOnMainThread">
  ): Promise<{results: boolean[]; signature: Buffer | null; count: number}>;
  /** IBlsVerifier.canAcceptWork: true while fewer than MAX_JOBS_CAN_ACCEPT_WORK (512) jobs are pending. */
  canAcceptWork(): boolean;
  readonly stats: {
    submissions: number;
    jobs: number;
    sets: number;
    groups: number;
    batchRetries: number;
    batchSigsSuccess: number;
    uniqueMessages: number;
    /** same-message calls retried set by set, and their sets (blsThreadPool.sameMessageRetryJobs / ...Sets) */
    sameMessageRetries: number;
    sameMessageRetrySets: number;
    /** device aggregateWithRandomness calls (fusedSameMessage: verifySameMessage calls) */
    sameMessageAggregations: number;
    urgentCalls?: number;
  };
  /** Signature.aggregate(group.map(fromBytes)).toBytes() for every group in one device call, off the main thread (the
   * op pools' fold, chain/opPools/*.ts).  One entry per group: the aggregate (96 bytes compressed, 192 with
   * compressed: false) or, for a rejected group, the Error the reference throws ("BLST_ERROR: <NAME>",
   * "EMPTY_AGGREGATE_ARRAY").  Rejects only for a call-level failure or once closed (QUEUE_ERROR_QUEUE_ABORTED). */
  aggregateSignatures(
    groups: Uint8Array[][],
    opts?: {validate?: boolean; compressed?: boolean}
  ): Promise<Array<Uint8Array | Error>>;
  /** AggregateVerify (blst-ts aggregateVerify(msgs, pks, sig)) for many jobs in one device call, off the main thread:
   * one aggregated signature per job over the pairs (pubkeys[i], messages[i]), 32-byte messages.  Over the whole call
   * the keys are all 96-byte uncompressed (trusted), all 48- or all 96-byte with validateKeys (KeyValidate on the
   * device), or all table indices (numbers; trusted).  One number per job: 1 valid, 0 invalid, -code (9 for no pairs,
   * else the lowest-index rejected key's blst code, else the signature's).  Rejects only for a call-level failure or
   * once closed (QUEUE_ERROR_QUEUE_ABORTED). */
  aggregateVerifyJobs(jobs: AggregateVerifyJob[], opts?: {validateKeys?: boolean}): Promise<number[]>;
  /** IBlsVerifier.close: rejects buffered jobs with QUEUE_ERROR_QUEUE_ABORTED, waits for in-flight submissions and
   * aggregation calls, then frees the devices. */
  close(): Promise<void>;
  /** index2pubkey sync: entries [firstIndex, firstIndex + n) as 96-byte uncompressed encodings. */
  uploadPubkeys(firstIndex: number, pk96: Uint8Array): void;
  /** The same sync from 48-byte compressed keys (state.validators[i].pubkey concatenated), decompressed on the device;
   * trusted unless {validate: true} (KeyValidate each).  A rejected key throws "BLST_ERROR: <NAME>" with .index its
   * validator index; nothing is stored then. */
  uploadPubkeysCompressed(firstIndex: number, pk48: Uint8Array, opts?: {validate?: boolean}): void;
  /** entries [firstIndex, firstIndex + n) of the device table: 96-byte uncompressed encodings, or 48-byte compressed */
  readPubkeys(firstIndex: number, n: number, opts?: {compressed?: boolean}): Buffer;
  /** The epoch's shufflings on the device: drops the stored committees with id >= firstCommittee, then stores
   * `committees` (validator indices into the device table) as ids firstCommittee, firstCommittee + 1, ...; 0 replaces
   * the store, committeesCount appends.  Synchronous.  An upload that overwrites table rows empties the store. */
  uploadCommittees(firstCommittee: number, committees: ArrayLike<number>[]): void;
  readonly committeesCount: number;
  /** getAggregatedPubkey(set).toBytes() for aggregate sets given as committees plus participation bits (the
   * uint8Array and bitLen of an ssz BitArray per stored committee), in one device call, off the main thread.  One entry
   * per set: the key (96 bytes uncompressed, 48 with compressed: true) or the Error "EMPTY_AGGREGATE_ARRAY" for a set
   * without a participant.  Rejects for malformed input, a call-level failure or once closed. */
  aggregatePubkeysFromBits(
    sets: Array<Array<{committee: number; bits: Uint8Array; bitLen: number}>>,
    opts?: {compressed?: boolean; noComplement?: boolean}
  ): Promise<Array<Uint8Array | Error>>;
  /** maps a PublicKey object (by identity) to its validator index in the device table */
  registerPubkey(pk: object, index: number): void;
  readonly deviceCount: number;
  /** a runtime tunable or property: "slots", "hw_queues", "group_sets", "group_policy", "merge_sets", ... */
  getOption(key: string): number;
}

export declare class BlsGpuSingleThreadVerifier extends BlsGpuVerifier {}

export declare function verifySignatureSet(verifier: BlsGpuVerifier, set: ISignatureSet): Promise<boolean>;
export declare function fastAggregateVerify(
  verifier: BlsGpuVerifier,
  pubkeys48: Uint8Array[],
  message: Uint8Array,
  signature: Uint8Array
): Promise<boolean>;
export declare function ethFastAggregateVerify(
  verifier: BlsGpuVerifier,
  pubkeys48: Uint8Array[],
  message: Uint8Array,
  signature: Uint8Array
): Promise<boolean>;

/** aggregate_verify of the spec runner: untrusted 48-byte keys, a message per key; any error, a length mismatch or no
 * pairs resolves to false. */
export declare function aggregateVerify(
  verifier: BlsGpuVerifier,
  pubkeys48: Uint8Array[],
  messages: Uint8Array[],
  signature: Uint8Array
): Promise<boolean>;
/** flags bits of addon.aggregateVerify: KeyValidate every key / the large-call kernel forms whatever the size */
export declare const AV_VALIDATE_KEYS: number;
export declare const AV_LANE_FORMS: number;

export declare const SignatureSetType: {single: "single"; aggregate: "aggregate"};
export declare const MAX_BUFFERED_SIGS: number;
export declare const MAX_BUFFER_WAIT_MS: number;
export declare const MAX_JOBS_CAN_ACCEPT_WORK: number;
/** flags bit of addon.verifySameMessage: the large-call kernel forms whatever the size (diagnostics) */
export declare const SAME_LANE_FORMS: number;
/** flags bit of addon.verifySameMessage: one check per block of 1024 groups, then the descent (blsgpu.h) */
export declare const SAME_BLOCK_CHECK: number;
export declare const addon: Record<string, (...args: unknown[]) => unknown>;
