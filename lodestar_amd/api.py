"""Host-side entry points around the C-ABI for the callers on either side of the verifier path, mirroring the
reference's own functions (same names in snake_case, same argument meaning and error behaviour):

* verify_signature_set           state-transition/src/util/signatureSets.ts:24-38 (single: Signature.verify;
                                 aggregate: Signature.verifyAggregate -- FastAggregateVerify over trusted keys)
* fast_aggregate_verify          beacon-node/test/spec/general/bls.ts:117-127 (untrusted keys: KeyValidate;
                                 any error -> False)
* eth_fast_aggregate_verify      beacon-node/test/spec/general/bls.ts:93-112
* eth_aggregate_pubkeys          beacon-node/test/spec/general/bls.ts:75-83 (an infinity key -> None)
* aggregate_signatures           beacon-node/test/spec/general/bls.ts `aggregate` (the consensus-spec Aggregate) and
                                 the op pools' Signature.aggregate([...]).toBytes() (chain/opPools/*.ts)
* aggregate_with_randomness      blst-ts aggregateWithRandomness(sets): {pk, sig} = (sum r_i pk_i, sum r_i sig_i)
* verify_signature_sets_same_message  IBlsVerifier.verifySignatureSetsSameMessage (chain/bls/interface.ts;
                                 multithread/index.ts + jobItem.ts: aggregate with randomness, verify the one set,
                                 retry every set on its own when that fails)
* verify_and_aggregate_same_message  the same, and the aggregate of the signatures that verified: what
                                 attestationPool.add folds into the pool's aggregate (chain/opPools/attestationPool.ts)
* aggregate_verify               beacon-node/test/spec/general/bls.ts `aggregate_verify` (blst-ts aggregateVerify(msgs,
                                 pks, sig) over untrusted keys, a message per key; any error -> False)
* verify                         beacon-node/test/spec/general/bls.ts `verify` (one untrusted key; any error -> False)
* upload_pubkeys_compressed      state-transition/src/cache/pubkeyCache.ts:56-77 (syncPubkeys: PublicKey.fromBytes of
                                 every state.validators[i].pubkey; here the GPU decompresses into its table)
* read_pubkeys                   index2pubkey[i].toBytes() of the keys the table holds
* upload_committees              the epoch's shufflings (epochCache getBeaconCommittee, the sync committee's indices)
* aggregate_pubkeys_from_bits    getAttestingIndices(committee, aggregationBits) / getSyncCommitteeSignatureSet's bit
                                 walk followed by getAggregatedPubkey(set).toBytes() (chain/bls/utils.ts:5-16)
* process_deposit_signature      state-transition/src/block/processDeposit.ts:54-64 (KeyValidate + verify;
                                 any error -> False: the deposit is skipped, not rejected)

All of them run on the GPU through lodestar_amd.native.Context (there is no CPU path).
"""
import numpy as np

from lodestar_amd.native import AV_LANE_FORMS, AV_VALIDATE_KEYS, SAME_BLOCK_CHECK, Context, code_name

G1_INFINITY_48 = bytes([0xC0]) + bytes(47)
G2_INFINITY_96 = bytes([0xC0]) + bytes(95)


class BlstError(Exception):
    """Mirrors @chainsafe/blst's ErrorBLST: the message carries 'BLST_ERROR: <CODE>'."""

    def __init__(self, code):
        self.code = code
        name = code_name(code)
        super().__init__(name if code in (9, 10) else f"BLST_ERROR: {name}")


def _one_job(ctx: Context, pk96_list, msg: bytes, sig: bytes):
    """One non-batchable job of one set whose pubkeys (96-byte uncompressed) are aggregated on the GPU."""
    sig = bytes(sig)
    sig_buf = sig.ljust(192, b"\0")[:192]
    res, _ = ctx.verify_raw([0, 1], sig_buf, [len(sig)], bytes(msg)[:32].ljust(32, b"\0"),
                            pk_bytes=b"".join(pk96_list) or bytes(96), set_pk_first=[0, len(pk96_list)],
                            job_flags=[0], sig_stride=192)
    return int(res[0])


def verify_signature_set(ctx: Context, pubkeys96, signing_root: bytes, signature: bytes) -> bool:
    """verifySignatureSet: `pubkeys96` is one trusted key (single set) or a list (aggregate set).  Raises
    BlstError where Signature.fromBytes(validate=true) throws."""
    keys = [pubkeys96] if isinstance(pubkeys96, (bytes, bytearray)) else list(pubkeys96)
    r = _one_job(ctx, keys, signing_root, signature)
    if r < 0:
        raise BlstError(-r)
    return r == 1


def key_validate(ctx: Context, pubkeys48):
    """KeyValidate of 48-byte keys: (list of 96-byte uncompressed or None, status array)."""
    if not pubkeys48:
        return [], np.zeros(0, np.int8)
    if any(len(p) != 48 for p in pubkeys48):
        raise ValueError("48-byte compressed pubkeys expected")
    pk96, st = ctx.key_validate(b"".join(bytes(p) for p in pubkeys48), 48)
    return [pk96[96 * i: 96 * i + 96] if st[i] == 0 else None for i in range(len(pubkeys48))], st


def upload_pubkeys_compressed(ctx: Context, first_index: int, pubkeys48, validate=False):
    """Table entries [first_index, first_index + len(pubkeys48)) from 48-byte compressed keys (trusted, as the keys of
    the state are; validate: KeyValidate each).  Raises BlstError(code) of the first rejected key -- its index is the
    error's .index -- and stores nothing then."""
    pubkeys48 = [bytes(p) for p in pubkeys48]
    if any(len(p) != 48 for p in pubkeys48):
        raise ValueError("48-byte compressed pubkeys expected")
    st, first_bad = ctx.upload_pubkeys_compressed(first_index, b"".join(pubkeys48), validate=validate)
    if first_bad != 0xFFFFFFFF:
        err = BlstError(int(st[first_bad]))
        err.index = first_index + first_bad
        raise err


def read_pubkeys(ctx: Context, first_index: int, n: int, compressed=False):
    """The table's entries [first_index, first_index + n): a list of 96-byte uncompressed (or 48-byte compressed)
    encodings."""
    k = 48 if compressed else 96
    out = ctx.read_pubkeys(first_index, n, k)
    return [out[k * i: k * i + k] for i in range(n)]


def upload_committees(ctx: Context, first_committee: int, committees):
    """Stores `committees` (a list of lists of table indices) as committees first_committee, first_committee + 1, ...
    after dropping the stored committees from first_committee on: 0 replaces the store, ctx.committees_count appends
    the next epoch's shuffling.  ValueError for what the library refuses (an empty committee, an index beyond the
    table, a gap)."""
    committees = [np.asarray(c, dtype=np.int64).reshape(-1) for c in committees]
    if any(len(c) and (c.min() < 0 or c.max() > 0xFFFFFFFF) for c in committees):
        raise ValueError("committee members must be table indices")
    first = np.cumsum([0] + [len(c) for c in committees])
    members = np.concatenate(committees) if committees else np.zeros(0, np.int64)
    ctx.upload_committees(first_committee, first, members)


def aggregate_pubkeys_from_bits(ctx: Context, sets, compressed=False, no_complement=False):
    """getAggregatedPubkey(set).toBytes() for aggregate sets given the way they are born: `sets` is a list of sets, a
    set a list of (committee id, participation bits) pairs -- one bit (any truthy value) per member of that stored
    committee, as getAttestingIndices(committee, aggregationBits) reads them.  Returns a list of 96-byte uncompressed
    (or 48-byte compressed) keys, None for a set without a participant (the reference's EMPTY_AGGREGATE_ARRAY)."""
    from lodestar_amd.native import BITS_NO_COMPLEMENT, EMPTY_AGGREGATE

    seg_first, bits_first, seg, packed = [0], [0], [], []
    for s in sets:
        flat = []
        for committee, bits in s:
            seg.append(int(committee))
            flat.append(np.asarray(bits, dtype=bool).reshape(-1))
        seg_first.append(len(seg))
        packed.append(np.packbits(np.concatenate(flat) if flat else np.zeros(0, bool), bitorder="little"))
        bits_first.append(bits_first[-1] + len(packed[-1]))
    buf = np.concatenate(packed) if packed else np.zeros(0, np.uint8)
    out, st, _ = ctx.aggregate_pubkeys_bits(seg_first, seg, bits_first, buf, BITS_NO_COMPLEMENT if no_complement else 0,
                                            48 if compressed else 96)
    return [None if st[i] == EMPTY_AGGREGATE else out[i] for i in range(len(out))]


def fast_aggregate_verify(ctx: Context, pubkeys48, message: bytes, signature: bytes) -> bool:
    keys, st = key_validate(ctx, list(pubkeys48))
    if not keys or (st != 0).any():
        return False  # EMPTY_AGGREGATE_ARRAY / BLST_* -> caught -> false
    return _one_job(ctx, keys, message, signature) == 1


def eth_fast_aggregate_verify(ctx: Context, pubkeys48, message: bytes, signature: bytes) -> bool:
    pubkeys48 = [bytes(p) for p in pubkeys48]
    if not pubkeys48 and bytes(signature) == G2_INFINITY_96:
        return True
    if any(p == G1_INFINITY_48 for p in pubkeys48):
        return False
    return fast_aggregate_verify(ctx, pubkeys48, message, signature)


def eth_aggregate_pubkeys(ctx: Context, pubkeys48):
    """Aggregate of untrusted compressed keys -> 48-byte compressed, None where the spec runner returns null."""
    pubkeys48 = [bytes(p) for p in pubkeys48]
    if not pubkeys48 or any(p == G1_INFINITY_48 for p in pubkeys48):
        return None
    keys, st = key_validate(ctx, pubkeys48)
    if (st != 0).any():
        return None
    out, ast = ctx.aggregate_pubkeys(pk_bytes=b"".join(keys), set_pk_first=[0, len(keys)], out_len=48)
    return out[0] if ast[0] == 0 else None


def process_deposit_signature(ctx: Context, pubkey48: bytes, signing_root: bytes, signature: bytes) -> bool:
    """processDeposit's signature check: PublicKey.fromBytes(validate) + Signature.fromBytes(validate) +
    verify, and `catch { return false }` -- an invalid deposit is skipped, never thrown."""
    keys, st = key_validate(ctx, [pubkey48])
    if st[0] != 0:
        return False
    return _one_job(ctx, keys, signing_root, signature) == 1


def verify(ctx: Context, pubkey48: bytes, message: bytes, signature: bytes) -> bool:
    """The spec runner's `verify`: one untrusted key, any error -> False (process_deposit_signature's rule)."""
    return process_deposit_signature(ctx, pubkey48, message, signature)


def aggregate_verify_jobs(ctx: Context, jobs, validate_keys=False, lane_forms=False):
    """AggregateVerify for many jobs in ONE device call (Context.aggregate_verify): jobs = [(keys, messages,
    signature)], one aggregated signature over the pairs (keys[i], messages[i]).  Over the whole call the keys are all
    96-byte uncompressed, all 48-byte compressed (only with validate_keys) or all table indices (trusted).  A list
    with one int per job: 1 valid, 0 invalid, -code (native.EMPTY_AGGREGATE for no pairs, else the lowest-index
    rejected key's error, else the signature's)."""
    jobs = [(list(k), [bytes(m)[:32].ljust(32, b"\0") for m in ms], bytes(s)) for k, ms, s in jobs]
    if not jobs:
        return []
    if any(len(k) != len(ms) for k, ms, _ in jobs):
        raise ValueError("one message per key")
    keys = [k for ks, _, _ in jobs for k in ks]
    table = [isinstance(k, (int, np.integer)) for k in keys]
    if any(table) and not all(table):
        raise ValueError("jobs mix table indices and pubkey bytes")
    pkb = pki = None
    pk_len = 96
    if keys and table[0]:
        pki = np.array([int(k) for k in keys], np.int64)
    else:
        keys = [bytes(k) for k in keys]
        pk_len = len(keys[0]) if keys else 96
        if pk_len not in ((48, 96) if validate_keys else (96,)) or any(len(k) != pk_len for k in keys):
            raise ValueError("all keys 96-byte uncompressed, or all 48-byte compressed with validate_keys")
        pkb = b"".join(keys)
    sigs = [s for _, _, s in jobs]
    stride = 192 if any(len(s) > 96 for s in sigs) else 96
    # any other length is refused by the device with INVALID_SIZE; its bytes are not read
    buf = b"".join(s[:stride].ljust(stride, b"\0") for s in sigs)
    flags = (AV_VALIDATE_KEYS if validate_keys else 0) | (AV_LANE_FORMS if lane_forms else 0)
    res, _, _ = ctx.aggregate_verify(np.cumsum([0] + [len(k) for k, _, _ in jobs]),
                                     b"".join(m for _, ms, _ in jobs for m in ms), buf, pk_bytes=pkb, pk_len=pk_len,
                                     pk_index=pki, sig_len=[len(s) for s in sigs], sig_stride=stride, flags=flags)
    return [int(r) for r in res]


def aggregate_verify(ctx: Context, pubkeys48, messages, signature: bytes) -> bool:
    """The spec runner's `aggregate_verify`: blst-ts aggregateVerify over untrusted compressed keys, a message per
    key.  Any error (a key KeyValidate rejects, a malformed signature), a length mismatch or no pairs -> False.
    Messages are 32-byte signing roots, as everywhere in this library: another length is a ValueError, not an answer."""
    pubkeys48 = [bytes(p) for p in pubkeys48]
    messages = [bytes(m) for m in messages]
    if not pubkeys48 or len(pubkeys48) != len(messages):
        return False
    if any(len(m) != 32 for m in messages):
        raise ValueError("32-byte messages (signing roots) expected")
    if any(len(p) != 48 for p in pubkeys48):
        return False
    return aggregate_verify_jobs(ctx, [(pubkeys48, messages, signature)], validate_keys=True)[0] == 1


def process_deposit_signatures(ctx: Context, pubkeys48, signing_roots, signatures):
    """process_deposit_signature over many deposits in two GPU calls (KeyValidate of every key, then one
    non-batchable single-set job per deposit with a valid key): list of bools."""
    n = len(pubkeys48)
    if n == 0:
        return []
    keys, st = key_validate(ctx, [bytes(p) for p in pubkeys48])
    ok = [i for i in range(n) if st[i] == 0]
    out = [False] * n
    if not ok:
        return out
    sigs = [bytes(signatures[i]) for i in ok]
    res, _ = ctx.verify_raw(np.arange(len(ok) + 1), b"".join(s.ljust(192, b"\0")[:192] for s in sigs),
                            [len(s) for s in sigs], b"".join(bytes(signing_roots[i])[:32] for i in ok),
                            pk_bytes=b"".join(keys[i] for i in ok), job_flags=np.zeros(len(ok)), sig_stride=192)
    for k, i in enumerate(ok):
        out[i] = int(res[k]) == 1  # errors (malformed signature) and false both skip the deposit
    return out


def aggregate_signature_groups(ctx: Context, groups, validate=True):
    """Signature.aggregate(group.map(s => Signature.fromBytes(s, validate))).toBytes() for every group of 96- or
    192-byte signatures in one GPU call: a list with the 96-byte compressed aggregate of each group, or the BlstError
    the reference throws for it (an empty group: EMPTY_AGGREGATE_ARRAY; else its first rejected signature's)."""
    groups = [[bytes(s) for s in g] for g in groups]
    if not groups:
        return []
    flat = [s for g in groups for s in g]
    stride = 192 if any(len(s) > 96 for s in flat) else 96
    first = np.cumsum([0] + [len(g) for g in groups])
    # any other length is refused by the device with INVALID_SIZE; its bytes are not read
    buf = b"".join(s[:stride].ljust(stride, b"\0") for s in flat)
    out, st, _ = ctx.aggregate_signatures(buf, first, sig_len=[len(s) for s in flat], sig_stride=stride,
                                          validate=validate)
    return [out[g] if st[g] == 0 else BlstError(int(st[g])) for g in range(len(groups))]


def aggregate_signatures(ctx: Context, signatures, validate=True) -> bytes:
    """The consensus-spec Aggregate: the 96-byte compressed sum of the signatures.  Raises BlstError for an empty list
    (EMPTY_AGGREGATE_ARRAY) or a signature Signature.fromBytes rejects."""
    r = aggregate_signature_groups(ctx, [list(signatures)], validate)[0]
    if isinstance(r, BlstError):
        raise r
    return r


def _same_message_arrays(sets):
    """(pk_bytes or None, pk_index or None, sigs buffer, sig_len, stride) of [(pk96 or table index, sig bytes)]."""
    sets = [(k, bytes(s)) for k, s in sets]
    table = [isinstance(k, (int, np.integer)) for k, _ in sets]
    if any(table) and not all(table):
        raise ValueError("sets mix table indices and pubkey bytes")
    stride = 192 if any(len(s) > 96 for _, s in sets) else 96
    # any other length is refused by the device with INVALID_SIZE; its bytes are not read
    buf = b"".join(s[:stride].ljust(stride, b"\0") for _, s in sets)
    sig_len = [len(s) for _, s in sets]
    if sets and table[0]:
        return None, np.array([int(k) for k, _ in sets], np.int64), buf, sig_len, stride
    pks = [bytes(k) for k, _ in sets]
    if any(len(k) != 96 for k in pks):
        raise ValueError("96-byte uncompressed pubkeys expected")
    return b"".join(pks), None, buf, sig_len, stride


def aggregate_with_randomness(ctx: Context, sets, seed=0):
    """blst-ts aggregateWithRandomness(sets) on the GPU, sets = [(pk96 or table index, signature bytes)]: (P, S) =
    (sum r_i pk_i as 96 bytes uncompressed, sum r_i sig_i as 192 bytes uncompressed) under fresh 64-bit scalars
    (seed 0), every signature subgroup-checked.  Raises BlstError for an empty list (EMPTY_AGGREGATE_ARRAY) or the
    first rejected set's error."""
    sets = list(sets)
    pkb, pki, buf, sig_len, stride = _same_message_arrays(sets)
    if not sets:
        raise BlstError(9)
    p, s, st, _ = ctx.aggregate_with_randomness([0, len(sets)], buf, pk_bytes=pkb, pk_index=pki, sig_len=sig_len,
                                                sig_stride=stride, seed=seed)
    if st[0] != 0:
        raise BlstError(int(st[0]))
    return p[0], s[0]


def verify_signature_sets_same_message(ctx: Context, sets, message: bytes, seed=0):
    """IBlsVerifier.verifySignatureSetsSameMessage: sets = [(pk96 or table index, signature bytes)] all signing
    `message`; a list with one bool per set.  One randomized aggregation, one verification of (P, message, S); when
    the aggregation rejects a set or that verification is not true, every set is verified on its own (a malformed
    signature is a False there, not an exception).  Raises BlstError("Empty signature set") for no sets."""
    sets = list(sets)
    n = len(sets)
    if n == 0:
        raise BlstError(10)
    message = bytes(message)[:32].ljust(32, b"\0")
    pkb, pki, buf, sig_len, stride = _same_message_arrays(sets)
    p, s, st, _ = ctx.aggregate_with_randomness([0, n], buf, pk_bytes=pkb, pk_index=pki, sig_len=sig_len,
                                                sig_stride=stride, seed=seed)
    if st[0] == 0:
        res, _ = ctx.verify_raw([0, 1], s[0], [192], message, pk_bytes=p[0], job_flags=[0], sig_stride=192)
        if int(res[0]) == 1:
            return [True] * n
    # retry: every set as its own one-set job
    keys = dict(pk_bytes=pkb) if pkb is not None else dict(set_pk_first=np.arange(n + 1), pk_index=pki)
    res, _ = ctx.verify_raw(np.arange(n + 1), buf, sig_len, message * n, job_flags=np.ones(n), sig_stride=stride,
                            **keys)
    return [int(r) == 1 for r in res]


def verify_same_message_groups(ctx: Context, groups, messages, seed=0, block_check=False):
    """verifySignatureSetsSameMessage for many groups in ONE device call (Context.verify_same_message): groups[g] =
    [(pk96 or table index, signature bytes)] all signing messages[g]; a list with one list of bools per group, each
    what verify_signature_sets_same_message answers for that group.  An empty group gives an empty list.
    block_check: the groups' aggregates are checked 1024 groups at a time under one final exponentiation
    (native.SAME_BLOCK_CHECK) -- the same answers, fewer checks when most groups verify."""
    groups = [list(g) for g in groups]
    messages = [bytes(m)[:32].ljust(32, b"\0") for m in messages]
    if len(messages) != len(groups):
        raise ValueError("one message per group")
    if not groups:
        return []
    first = np.cumsum([0] + [len(g) for g in groups])
    pkb, pki, buf, sig_len, stride = _same_message_arrays([s for g in groups for s in g])
    if first[-1] == 0:
        pkb = b""  # no set at all: either key mode
    res, _, _ = ctx.verify_same_message(first, b"".join(messages), buf, pk_bytes=pkb, pk_index=pki, sig_len=sig_len,
                                        sig_stride=stride, seed=seed,
                                        flags=SAME_BLOCK_CHECK if block_check else 0)
    return [[int(r) == 1 for r in res[first[g]: first[g + 1]]] for g in range(len(groups))]


def verify_and_aggregate_same_message_groups(ctx: Context, groups, messages, include=None, seed=0, block_check=False):
    """verify_same_message_groups that also returns each group's aggregate of the signatures that verified, in ONE
    device call (Context.verify_same_message_agg).  include (optional): per group a list with one truthy / falsy entry
    per set, or None for all -- a falsy set is verified but left out of the aggregate (one the pool already holds).
    A list with one (bools, aggregate96 or None, count) per group: the aggregate is Signature.toBytes() of the sum
    over the `count` sets that verified and were included, None when there is none."""
    groups = [list(g) for g in groups]
    messages = [bytes(m)[:32].ljust(32, b"\0") for m in messages]
    if len(messages) != len(groups):
        raise ValueError("one message per group")
    if include is not None and len(include) != len(groups):
        raise ValueError("one include list (or None) per group")
    if not groups:
        return []
    first = np.cumsum([0] + [len(g) for g in groups])
    inc = None
    if include is not None:
        inc = np.ones(int(first[-1]), np.uint8)
        for g, m in enumerate(include):
            if m is None:
                continue
            if len(m) != len(groups[g]):
                raise ValueError(f"group {g}: one include entry per set")
            inc[first[g]: first[g + 1]] = [1 if x else 0 for x in m]
    pkb, pki, buf, sig_len, stride = _same_message_arrays([s for g in groups for s in g])
    if first[-1] == 0:
        pkb = b""  # no set at all: either key mode
    res, _, _, out, cnt = ctx.verify_same_message_agg(first, b"".join(messages), buf, pk_bytes=pkb, pk_index=pki,
                                                      sig_len=sig_len, sig_stride=stride, seed=seed,
                                                      flags=SAME_BLOCK_CHECK if block_check else 0, include=inc)
    return [([int(r) == 1 for r in res[first[g]: first[g + 1]]], out[g] if cnt[g] else None, int(cnt[g]))
            for g in range(len(groups))]


def verify_and_aggregate_same_message(ctx: Context, sets, message: bytes, seed=0):
    """verify_signature_sets_same_message and, from the same device call, the aggregate the attestation pool folds in:
    (a list with one bool per set, Signature.toBytes() (96 bytes) of the sum of the signatures that verified, or None
    when none did).  Raises BlstError("Empty signature set") for no sets."""
    sets = list(sets)
    if not sets:
        raise BlstError(10)
    bools, agg, _ = verify_and_aggregate_same_message_groups(ctx, [sets], [message], seed=seed)[0]
    return bools, agg
