"""ctypes binding of libblsgpu.so (include/blsgpu.h).  Loads the in-tree library and fails loudly if it
is missing -- there is no CPU fallback for verification."""
import ctypes
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BLSGPU_LIB") or os.path.join(PKG, "libblsgpu.so")  # override: tuning variants

# job / status codes (blsgpu_code)
OK = 0
BAD_ENCODING = 1
POINT_NOT_ON_CURVE = 2
POINT_NOT_IN_GROUP = 3
PK_IS_INFINITY = 6
INVALID_SIZE = 8
EMPTY_AGGREGATE = 9
EMPTY_SET = 10
DEVICE_ERROR = 11
ERR_ARGS = 100
ERR_NO_DEVICE = 101
ERR_CLOSED = 102
ERR_ENTROPY = 103
# blsgpu_batch.job_flags bits
JOB_BATCHABLE = 1
JOB_URGENT = 2  # VerifySignatureOpts.verifyOnMainThread: the device's urgent lane
# blsgpu_aggregate_signatures flags
AGG_VALIDATE = 1  # Signature.fromBytes(.., validate = true)
AGG_MAX_SIGS = 1 << 20
# blsgpu_debug_inject targets
INJECT_ENTROPY = 1
INJECT_DEVICE = 2

EXPORTED_SYMBOLS = [
    "blsgpu_init",
    "blsgpu_destroy",
    "blsgpu_device_count",
    "blsgpu_pubkeys_upload",
    "blsgpu_pubkeys_count",
    "blsgpu_verify",
    "blsgpu_submit",
    "blsgpu_set_option",
    "blsgpu_code_name",
    "blsgpu_debug_op",
    "blsgpu_aggregate_pubkeys",
    "blsgpu_key_validate",
    "blsgpu_signing_roots",
    "blsgpu_shard_jobs",
    "blsgpu_get_option",
    "blsgpu_chunkify",
    "blsgpu_batch_scalars",
    "blsgpu_debug_inject",
    "blsgpu_route_call",
    "blsgpu_aggregate_signatures",
    "blsgpu_sig_agg_lanes",
    "blsgpu_randomness_words",
    "blsgpu_aggregate_with_randomness",
    "blsgpu_awr_lanes",
    "blsgpu_verify_same_message",
    "blsgpu_same_message_form",
    "blsgpu_same_message_blocks",
    "blsgpu_aggregate_verify",
    "blsgpu_aggregate_verify_form",
    "blsgpu_verify_same_message_agg",
    "blsgpu_same_message_agg_lanes",
    "blsgpu_pubkeys_upload_compressed",
    "blsgpu_pubkeys_read",
    "blsgpu_committees_upload",
    "blsgpu_committees_count",
    "blsgpu_aggregate_pubkeys_bits",
    "blsgpu_committee_bits_mode",
    "blsgpu_committee_bits_lanes",
    "blsgpu_awr_parts",
]
PK_VALIDATE = 1  # BLSGPU_PK_VALIDATE: the uploaded keys are untrusted, KeyValidate each
BITS_NO_COMPLEMENT = 1  # BLSGPU_BITS_NO_COMPLEMENT: diagnostics / tests, always sum the participants
SAME_LANE_FORMS = 1
SAME_BLOCK_CHECK = 4  # BLSGPU_SAME_BLOCK_CHECK: one check per block of 1024 groups, then the descent
# blsgpu_aggregate_verify flags
AV_VALIDATE_KEYS = 1  # the keys are untrusted: KeyValidate each
AV_LANE_FORMS = 2  # diagnostics / tests: the large-call kernel forms whatever the size
ROOT_OBJECT = 0
ROOT_ATTESTATION_DATA = 1


class Batch(ctypes.Structure):
    _fields_ = [
        ("n_sets", ctypes.c_uint32),
        ("n_jobs", ctypes.c_uint32),
        ("job_first_set", ctypes.c_void_p),
        ("job_flags", ctypes.c_void_p),
        ("pk_bytes", ctypes.c_void_p),
        ("set_pk_first", ctypes.c_void_p),
        ("pk_index", ctypes.c_void_p),
        ("msgs", ctypes.c_void_p),
        ("sigs", ctypes.c_void_p),
        ("sig_len", ctypes.c_void_p),
        ("sig_stride", ctypes.c_uint32),
        ("seed", ctypes.c_uint64),
    ]


class Stats(ctypes.Structure):
    _fields_ = [
        ("groups", ctypes.c_uint32),
        ("batch_retries", ctypes.c_uint32),
        ("batch_sigs_success", ctypes.c_uint32),
        ("devices_used", ctypes.c_uint32),
        ("device_ms", ctypes.c_double),
        ("stage_ms", ctypes.c_double * 8),
        ("unique_messages", ctypes.c_uint32),
        ("pairing_units", ctypes.c_uint32),
        ("miller_chunks", ctypes.c_uint32),
        ("run_sets", ctypes.c_uint32),
        ("run_calls", ctypes.c_uint32),
        ("fallback_jobs", ctypes.c_uint32),
        ("fallback_miller", ctypes.c_uint32),
        ("urgent_lane", ctypes.c_uint32),
        ("host_ms", ctypes.c_double),
    ]


class SameMessageStats(ctypes.Structure):
    _fields_ = [
        ("groups_accepted", ctypes.c_uint32),
        ("groups_retried", ctypes.c_uint32),
        ("retry_sets", ctypes.c_uint32),
        ("unique_messages", ctypes.c_uint32),
        ("form", ctypes.c_uint32),
        ("device_ms", ctypes.c_double),
    ]


class AggregateVerifyStats(ctypes.Structure):
    _fields_ = [
        ("pairs", ctypes.c_uint32),
        ("unique_messages", ctypes.c_uint32),
        ("miller_items", ctypes.c_uint32),
        ("miller_chunks", ctypes.c_uint32),
        ("form", ctypes.c_uint32),
        ("jobs_checked", ctypes.c_uint32),
        ("device_ms", ctypes.c_double),
    ]


class CommitteeBitsStats(ctypes.Structure):
    _fields_ = [
        ("segments", ctypes.c_uint32),
        ("segments_complemented", ctypes.c_uint32),
        ("keys_present", ctypes.c_uint32),
        ("keys_added", ctypes.c_uint32),
        ("keys_subtracted", ctypes.c_uint32),
        ("lanes", ctypes.c_uint32),
        ("device_ms", ctypes.c_double),
    ]


STAGES = ["sig_decode", "hash_to_g2", "pk_aggregate", "pk_finish", "sig_msm", "miller_sets",
          "group_reduce", "group_check"]
# the kernels each stage's HIP-event interval covers (rocprof lists them separately; k_batch_inv runs in both the
# hash and the pubkey stage)
KERNEL_OF_STAGE = ["k_sig_decode+k_sig_subgroup2+k_sig_subgroup_coop",
                   "k_hash_prep+k_batch_inv+k_hash_map+k_hash_clear+k_hash_clear2+k_hash_clear_coop+k_h_affine",
                   "k_pk_aggregate+k_pk_aggregate_g", "k_pk_finish+k_batch_inv+k_pk_affine",
                   "k_job_mask+k_msm_bucket+k_msm_bucket2+k_msm_slice_pairs+k_msm_slice_pairs2+k_msm_window+k_msm_window2"
                   "+k_msm_horner+k_msm_horner_lane",
                   "k_miller_lines+k_miller_lines2+k_miller_acc+k_miller_acc2+k_miller_acc6+k_miller_accx+k_miller_coop",
                   "k_f_runs+k_f_pairs+k_f_gather", "k_group_sig_miller+k_group_check"]


DONE_CB = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int)

_lib = None


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: build it with `python -m lodestar_amd.build` (hipcc, gfx950). "
            "There is no CPU verification path."
        )
    lib = ctypes.CDLL(LIB_PATH)
    lib.blsgpu_init.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
    lib.blsgpu_init.restype = ctypes.c_int
    lib.blsgpu_destroy.argtypes = [ctypes.c_void_p]
    lib.blsgpu_destroy.restype = None
    lib.blsgpu_device_count.argtypes = [ctypes.c_void_p]
    lib.blsgpu_device_count.restype = ctypes.c_int
    lib.blsgpu_pubkeys_upload.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_uint32]
    lib.blsgpu_pubkeys_upload.restype = ctypes.c_int
    lib.blsgpu_pubkeys_count.argtypes = [ctypes.c_void_p]
    lib.blsgpu_pubkeys_count.restype = ctypes.c_uint32
    lib.blsgpu_verify.argtypes = [ctypes.c_void_p, ctypes.POINTER(Batch), ctypes.c_void_p, ctypes.POINTER(Stats)]
    lib.blsgpu_verify.restype = ctypes.c_int
    lib.blsgpu_submit.argtypes = [ctypes.c_void_p, ctypes.POINTER(Batch), ctypes.c_void_p, ctypes.POINTER(Stats),
                                  DONE_CB, ctypes.c_void_p]
    lib.blsgpu_submit.restype = ctypes.c_int
    lib.blsgpu_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int64]
    lib.blsgpu_set_option.restype = ctypes.c_int
    lib.blsgpu_code_name.argtypes = [ctypes.c_int]
    lib.blsgpu_code_name.restype = ctypes.c_char_p
    lib.blsgpu_debug_op.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_uint32,
                                    ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    lib.blsgpu_debug_op.restype = ctypes.c_int
    vp, u32 = ctypes.c_void_p, ctypes.c_uint32
    lib.blsgpu_aggregate_pubkeys.argtypes = [vp, ctypes.POINTER(Batch), vp, u32, vp]
    lib.blsgpu_key_validate.argtypes = [vp, u32, vp, u32, u32, vp, vp]
    lib.blsgpu_signing_roots.argtypes = [vp, ctypes.c_int, u32, vp, u32, vp, u32, vp]
    lib.blsgpu_shard_jobs.argtypes = [vp, vp, u32, u32, vp]
    lib.blsgpu_get_option.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int64)]
    lib.blsgpu_chunkify.argtypes = [u32, u32, vp, vp]
    lib.blsgpu_batch_scalars.argtypes = [ctypes.POINTER(Batch), vp]
    lib.blsgpu_batch_scalars.restype = ctypes.c_int
    lib.blsgpu_debug_inject.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.c_int64]
    lib.blsgpu_debug_inject.restype = ctypes.c_int
    lib.blsgpu_route_call.argtypes = [u32, u32, vp, ctypes.c_int64, u32, vp, vp]
    lib.blsgpu_route_call.restype = ctypes.c_int
    lib.blsgpu_aggregate_signatures.argtypes = [vp, u32, vp, vp, u32, vp, u32, vp, u32, vp, vp]
    lib.blsgpu_aggregate_signatures.restype = ctypes.c_int
    lib.blsgpu_sig_agg_lanes.argtypes = [u32, u32]
    lib.blsgpu_sig_agg_lanes.restype = u32
    lib.blsgpu_randomness_words.argtypes = [u32, ctypes.c_uint64, vp]
    lib.blsgpu_randomness_words.restype = ctypes.c_int
    lib.blsgpu_aggregate_with_randomness.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, ctypes.c_uint64, vp, u32, vp,
                                                     u32, vp, vp]
    lib.blsgpu_aggregate_with_randomness.restype = ctypes.c_int
    lib.blsgpu_awr_lanes.argtypes = [u32, u32]
    lib.blsgpu_awr_lanes.restype = u32
    lib.blsgpu_awr_parts.argtypes = [u32, vp, vp, vp, vp]
    lib.blsgpu_awr_parts.restype = ctypes.c_int
    lib.blsgpu_verify_same_message.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, vp, ctypes.c_uint64, u32, vp, vp, vp]
    lib.blsgpu_verify_same_message.restype = ctypes.c_int
    lib.blsgpu_same_message_form.argtypes = [u32, u32]
    lib.blsgpu_same_message_form.restype = u32
    lib.blsgpu_same_message_blocks.argtypes = [u32, u32]
    lib.blsgpu_same_message_blocks.restype = u32
    lib.blsgpu_verify_same_message_agg.argtypes = [vp, u32, vp, vp, vp, vp, vp, u32, vp, ctypes.c_uint64, u32, vp, vp,
                                                   vp, vp, vp, u32, vp]
    lib.blsgpu_verify_same_message_agg.restype = ctypes.c_int
    lib.blsgpu_same_message_agg_lanes.argtypes = [u32, u32]
    lib.blsgpu_same_message_agg_lanes.restype = u32
    lib.blsgpu_aggregate_verify.argtypes = [vp, u32, vp, vp, vp, u32, vp, vp, u32, vp, u32, vp, vp, vp]
    lib.blsgpu_aggregate_verify.restype = ctypes.c_int
    lib.blsgpu_aggregate_verify_form.argtypes = [u32, u32]
    lib.blsgpu_aggregate_verify_form.restype = u32
    lib.blsgpu_pubkeys_upload_compressed.argtypes = [vp, u32, vp, u32, u32, vp, vp]
    lib.blsgpu_pubkeys_upload_compressed.restype = ctypes.c_int
    lib.blsgpu_pubkeys_read.argtypes = [vp, u32, u32, vp, u32]
    lib.blsgpu_pubkeys_read.restype = ctypes.c_int
    lib.blsgpu_committees_upload.argtypes = [vp, u32, u32, vp, vp]
    lib.blsgpu_committees_upload.restype = ctypes.c_int
    lib.blsgpu_committees_count.argtypes = [vp]
    lib.blsgpu_committees_count.restype = u32
    lib.blsgpu_aggregate_pubkeys_bits.argtypes = [vp, u32, vp, vp, vp, vp, u32, vp, u32, vp, vp]
    lib.blsgpu_aggregate_pubkeys_bits.restype = ctypes.c_int
    lib.blsgpu_committee_bits_mode.argtypes = [u32, u32, u32]
    lib.blsgpu_committee_bits_mode.restype = u32
    lib.blsgpu_committee_bits_lanes.argtypes = [u32, u32]
    lib.blsgpu_committee_bits_lanes.restype = u32
    _lib = lib
    return lib


def code_name(code: int) -> str:
    n = load().blsgpu_code_name(code)
    return n.decode() if n else f"BLSGPU_{code}"


def shard_jobs(job_first_set, n_parts, set_pk_first=None):
    """The runtime's sharding rule (C-ABI blsgpu_shard_jobs, pure host code): [(job_begin, job_end)]."""
    jfs = np.ascontiguousarray(job_first_set, dtype=np.uint32)
    spf = None if set_pk_first is None else np.ascontiguousarray(set_pk_first, dtype=np.uint32)
    out = np.zeros(n_parts + 1, np.uint32)
    rc = load().blsgpu_shard_jobs(jfs.ctypes.data, None if spf is None else spf.ctypes.data, len(jfs) - 1, n_parts,
                                  out.ctypes.data)
    if rc != OK:
        raise ValueError(f"blsgpu_shard_jobs -> {code_name(rc)}")
    return [(int(out[k]), int(out[k + 1])) for k in range(n_parts)]


def route_call(n_sets, device_load, split_sets=16384, start=0):
    """The runtime's call routing (C-ABI blsgpu_route_call, pure host code): the devices, in shard order, a call of
    n_sets sets runs on given each device's queued cost."""
    dl = np.ascontiguousarray(device_load, dtype=np.int64)
    out = np.zeros(max(len(dl), 1), np.uint32)
    k = ctypes.c_uint32(0)
    rc = load().blsgpu_route_call(n_sets, len(dl), dl.ctypes.data, split_sets, start, out.ctypes.data,
                                  ctypes.addressof(k))
    if rc != OK:
        raise ValueError(f"blsgpu_route_call -> {code_name(rc)}")
    return [int(x) for x in out[: k.value]]


def sig_agg_lanes(n_groups, n_sigs):
    """Lanes per group blsgpu_aggregate_signatures gives a call of this shape (C-ABI blsgpu_sig_agg_lanes, pure host
    code): 64, 32, 16, 8 or 1."""
    return int(load().blsgpu_sig_agg_lanes(n_groups, n_sigs))


def aggregate_layout(sigs, group_first, sig_len=None, sig_stride=None, out_len=96):
    """The arrays of one blsgpu_aggregate_signatures call, checked on the host: (sigs uint8, group_first uint32,
    sig_len uint32, sig_stride).  Raises ValueError for a layout the library would refuse."""
    gf = np.ascontiguousarray(group_first, dtype=np.int64)
    if gf.ndim != 1 or len(gf) == 0:
        raise ValueError("group_first needs n_groups + 1 >= 1 entries")
    if gf[0] != 0 or (np.diff(gf) < 0).any():
        raise ValueError("group_first must start at 0 and never decrease")
    n = int(gf[-1])
    if n > AGG_MAX_SIGS:
        raise ValueError(f"at most {AGG_MAX_SIGS} signatures per call")
    if out_len not in (96, 192):
        raise ValueError("out_len must be 96 or 192")
    buf = _u8(sigs)
    if sig_stride is None:
        sig_stride = (len(buf) // n) if n else 96
    if sig_stride < 96:
        raise ValueError("sig_stride must be at least 96")
    if len(buf) < n * sig_stride:
        raise ValueError(f"{n} signatures of stride {sig_stride} need {n * sig_stride} bytes, got {len(buf)}")
    sl = np.full(n, sig_stride if sig_stride in (96, 192) else 96, np.uint32) if sig_len is None else \
        np.ascontiguousarray(sig_len, dtype=np.uint32)
    if sl.ndim != 1 or len(sl) != n:
        raise ValueError(f"sig_len needs one entry per signature ({n})")
    if sig_stride < 192 and (sl == 192).any():
        raise ValueError("a 192-byte signature needs sig_stride >= 192")
    return buf, gf.astype(np.uint32), sl, int(sig_stride)


def awr_lanes(n_groups, n_sets):
    """Lanes per group blsgpu_aggregate_with_randomness gives a call of this shape (C-ABI blsgpu_awr_lanes, pure host
    code): 64, 32, 16, 8 or 1."""
    return int(load().blsgpu_awr_lanes(n_groups, n_sets))


def awr_parts(group_first):
    """How the randomized sums of a same-message call with these groups are cut (C-ABI blsgpu_awr_parts, pure host
    code): (part_sets, part_first).  part_sets = L t sets per part, or 0 when the call is not split; part_first = the
    parts' first sets and n, a uint32 array of n_parts + 1 entries (group_first itself when not split).  ValueError
    for a group_first the calls would refuse."""
    gf = np.ascontiguousarray(group_first, dtype=np.int64)
    if gf.ndim != 1 or len(gf) == 0:
        raise ValueError("group_first needs n_groups + 1 >= 1 entries")
    if (gf < 0).any() or (gf > 0xFFFFFFFF).any():
        raise ValueError("group_first entries must be set counts")
    gf = gf.astype(np.uint32)
    n_groups = len(gf) - 1
    out = np.zeros(max(n_groups, 65536) + 1, np.uint32)
    part_sets, n_parts = ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = load().blsgpu_awr_parts(n_groups, gf.ctypes.data, ctypes.addressof(part_sets), ctypes.addressof(n_parts),
                                 out.ctypes.data)
    if rc != OK:
        raise ValueError(f"blsgpu_awr_parts -> {code_name(rc)}")
    return int(part_sets.value), out[: n_parts.value + 1].copy()


def same_message_form(n_items, flags=0):
    """The kernel forms blsgpu_verify_same_message gives a phase of n_items pairings (C-ABI blsgpu_same_message_form,
    pure host code): 0 = cooperative, 1 = lane forms."""
    return int(load().blsgpu_same_message_form(n_items, flags))


def same_message_agg_lanes(n_groups, n_sets):
    """Lanes per group the aggregate phase of blsgpu_verify_same_message_agg gives a call of this shape (C-ABI
    blsgpu_same_message_agg_lanes, pure host code): the rule of sig_agg_lanes."""
    return int(load().blsgpu_same_message_agg_lanes(n_groups, n_sets))


def same_message_blocks(n_groups, flags=0):
    """The blocks of groups blsgpu_verify_same_message checks under one final exponentiation each (C-ABI
    blsgpu_same_message_blocks, pure host code): 0 without SAME_BLOCK_CHECK, else ceil(n_groups / 1024)."""
    return int(load().blsgpu_same_message_blocks(n_groups, flags))


def aggregate_verify_form(n_items, flags=0):
    """The kernel forms blsgpu_aggregate_verify gives a call of n_items Miller items -- the pairs of its non-empty
    jobs plus one item per such job (C-ABI blsgpu_aggregate_verify_form, pure host code): 0 = cooperative, 1 = lane
    forms."""
    return int(load().blsgpu_aggregate_verify_form(n_items, flags))


def committee_bits_mode(size, present, flags=0):
    """How blsgpu_aggregate_pubkeys_bits takes a segment of `size` members of which `present` participate (C-ABI
    blsgpu_committee_bits_mode, pure host code): 0 = sums the participants, 1 = by complement."""
    return int(load().blsgpu_committee_bits_mode(size, present, flags))


def committee_bits_lanes(n_sets, n_items):
    """Lanes per set blsgpu_aggregate_pubkeys_bits gives a call of n_sets sets that gathers n_items points (C-ABI
    blsgpu_committee_bits_lanes, pure host code): 64, 32, 16 or 8."""
    return int(load().blsgpu_committee_bits_lanes(n_sets, n_items))


def randomness_words(n, seed):
    """The scalar words of a randomized aggregation of n sets (C-ABI blsgpu_randomness_words, pure host code): a
    uint64 array, never 0; seed 0 draws a fresh key per call.  RuntimeError when the OS gives no randomness."""
    out = np.zeros(max(n, 1), np.uint64)
    rc = load().blsgpu_randomness_words(n, seed, out.ctypes.data)
    if rc != OK:
        raise RuntimeError(f"blsgpu_randomness_words -> {code_name(rc)}")
    return out[:n]


def awr_layout(group_first, sigs, pk_bytes=None, pk_index=None, sig_len=None, sig_stride=None, out_pk_len=96,
               out_sig_len=192):
    """The arrays of one blsgpu_aggregate_with_randomness call, checked on the host: (group_first uint32, sigs uint8,
    sig_len uint32, sig_stride, pk_bytes uint8 or None, pk_index uint32 or None).  Raises ValueError for a layout the
    library would refuse."""
    if out_pk_len not in (48, 96):
        raise ValueError("out_pk_len must be 48 or 96")
    buf, gf, sl, stride = aggregate_layout(sigs, group_first, sig_len, sig_stride, out_sig_len)
    n = int(gf[-1])
    if (pk_bytes is None) == (pk_index is None):
        raise ValueError("exactly one of pk_bytes and pk_index")
    pkb = pki = None
    if pk_bytes is not None:
        pkb = _u8(pk_bytes)
        if len(pkb) != 96 * n:
            raise ValueError(f"{n} sets need {96 * n} pubkey bytes, got {len(pkb)}")
    else:
        idx = np.ascontiguousarray(pk_index, dtype=np.int64)
        if idx.ndim != 1 or len(idx) != n:
            raise ValueError(f"pk_index needs one entry per set ({n})")
        if n and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
            raise ValueError("pk_index entries must be table indices")
        pki = idx.astype(np.uint32)
    return gf, buf, sl, stride, pkb, pki


def chunkify(length, min_per_chunk):
    """chunkifyMaximizeChunkSize(range(length), min_per_chunk) (reference multithread/utils.ts:4-19) through the
    C-ABI (blsgpu_chunkify, pure host code): list of index lists."""
    out = np.zeros(length // max(min_per_chunk, 1) + 2, np.uint32)
    nc = ctypes.c_uint32(0)
    rc = load().blsgpu_chunkify(length, min_per_chunk, out.ctypes.data, ctypes.addressof(nc))
    if rc != OK:
        raise ValueError(f"blsgpu_chunkify -> {code_name(rc)}")
    return [list(range(int(out[k]), int(out[k + 1]))) for k in range(nc.value)]


def batch_scalars(job_first_set, job_flags=None, seed=0):
    """The batch scalar words a call would use (C-ABI blsgpu_batch_scalars, pure host code): uint64 array, one word
    per set (0 = r = 1).  Raises RuntimeError(ERR_ENTROPY) when seed is 0 and the OS gives no randomness."""
    jfs = np.ascontiguousarray(job_first_set, dtype=np.uint32)
    if len(jfs) == 0:
        raise ValueError("job_first_set needs n_jobs + 1 >= 1 entries")
    n = int(jfs[-1])
    b = Batch()
    b.n_sets = n
    b.n_jobs = len(jfs) - 1
    b.job_first_set = jfs.ctypes.data
    keep = [jfs]
    if job_flags is not None:
        fl = np.ascontiguousarray(job_flags, dtype=np.uint8)
        keep.append(fl)
        b.job_flags = fl.ctypes.data
    b.seed = seed
    out = np.zeros(max(n, 1), np.uint64)
    rc = load().blsgpu_batch_scalars(ctypes.byref(b), out.ctypes.data)
    if rc != OK:
        raise RuntimeError(f"blsgpu_batch_scalars -> {code_name(rc)}")
    return out[:n]


def debug_inject(what, skip=0, count=1):
    """Arms the library's fault injection (blsgpu_debug_inject): after `skip` more events, the next `count` entropy
    draws (INJECT_ENTROPY) or pipeline runs (INJECT_DEVICE) fail.  count 0 disarms."""
    rc = load().blsgpu_debug_inject(what, skip, count)
    if rc != OK:
        raise ValueError(f"blsgpu_debug_inject -> {code_name(rc)}")


def _u8(b):
    return np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray) else np.ascontiguousarray(b)


def make_batch(job_first_set, sigs, sig_len, msgs, pk_bytes=None, set_pk_first=None, pk_index=None,
               job_flags=None, sig_stride=None, seed=0x4C4F444553544152):
    """blsgpu_batch over numpy/bytes arrays: (Batch, keep-alive list).  Modes: pk_bytes alone (one key per
    set), pk_bytes + set_pk_first (bytes aggregate), set_pk_first + pk_index (device table)."""
    job_first_set = np.ascontiguousarray(job_first_set, dtype=np.uint32)
    sig_len = np.ascontiguousarray(sig_len, dtype=np.uint32)
    n_sets = len(sig_len)
    sigs, msgs = _u8(sigs), _u8(msgs)
    if sig_stride is None:
        sig_stride = (len(sigs) // n_sets) if n_sets else 96
    keep = [job_first_set, sig_len, sigs, msgs]
    b = Batch()
    b.n_sets = n_sets
    b.n_jobs = len(job_first_set) - 1
    b.job_first_set = job_first_set.ctypes.data
    if job_flags is not None:
        job_flags = np.ascontiguousarray(job_flags, dtype=np.uint8)
        keep.append(job_flags)
        b.job_flags = job_flags.ctypes.data
    if pk_bytes is not None:
        pk = _u8(pk_bytes)
        if len(pk) == 0:
            pk = np.zeros(1, np.uint8)
        keep.append(pk)
        b.pk_bytes = pk.ctypes.data
    if set_pk_first is not None:
        set_pk_first = np.ascontiguousarray(set_pk_first, dtype=np.uint32)
        keep.append(set_pk_first)
        b.set_pk_first = set_pk_first.ctypes.data
    if pk_index is not None:
        pk_index = np.ascontiguousarray(pk_index, dtype=np.uint32)
        keep.append(pk_index)
        b.pk_index = pk_index.ctypes.data if len(pk_index) else set_pk_first.ctypes.data
    b.msgs = msgs.ctypes.data if len(msgs) else 0
    b.sigs = sigs.ctypes.data if len(sigs) else 0
    b.sig_len = sig_len.ctypes.data if len(sig_len) else 0
    b.sig_stride = sig_stride
    b.seed = seed
    return b, keep


class Pending:
    """An asynchronous call of Context.submit_raw."""

    status = None
    t_done = None

    def wait(self, timeout=None):
        if not self.ev.wait(timeout):
            raise TimeoutError("blsgpu_submit: call not completed")
        if self.status != OK:
            raise RuntimeError(f"blsgpu_submit -> {code_name(self.status)}")
        return self.res[: self.n_jobs], self.st


class Context:
    """Owns a blsgpu_ctx on one or more HIP devices."""

    def __init__(self, devices=None):
        lib = load()
        self._lib = lib
        h = ctypes.c_void_p()
        if devices:
            arr = (ctypes.c_int * len(devices))(*devices)
            rc = lib.blsgpu_init(arr, len(devices), ctypes.byref(h))
        else:
            rc = lib.blsgpu_init(None, 0, ctypes.byref(h))
        if rc != OK:
            raise RuntimeError(f"blsgpu_init failed: {code_name(rc)} (no usable MI355X?)")
        self.h = h

    def close(self):
        if self.h:
            self._lib.blsgpu_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def device_count(self):
        return self._lib.blsgpu_device_count(self.h)

    def set_option(self, key: str, value: int):
        rc = self._lib.blsgpu_set_option(self.h, key.encode(), int(value))
        if rc != OK:
            raise ValueError(f"blsgpu_set_option({key}) -> {code_name(rc)}")

    def get_option(self, key: str) -> int:
        v = ctypes.c_int64(0)
        rc = self._lib.blsgpu_get_option(self.h, key.encode(), ctypes.byref(v))
        if rc != OK:
            raise ValueError(f"blsgpu_get_option({key}) -> {code_name(rc)}")
        return v.value

    def upload_pubkeys(self, first_index: int, pk96: bytes):
        n = len(pk96) // 96
        rc = self._lib.blsgpu_pubkeys_upload(self.h, first_index, pk96, n)
        if rc != OK:
            raise ValueError(f"blsgpu_pubkeys_upload -> {code_name(rc)}")

    def upload_pubkeys_compressed(self, first_index: int, pk48: bytes, validate=False):
        """Table entries [first_index, first_index + n) from 48-byte compressed keys, decompressed on the GPU (validate:
        KeyValidate each, BLSGPU_PK_VALIDATE).  Returns (status int8 array, first_bad): a rejected key is reported --
        status[k] its code, first_bad the lowest rejected index, nothing stored -- not raised; first_bad is 0xffffffff
        when every key was stored.  Raises only for a call-level failure (BLSGPU_ERR_*, DEVICE_ERROR)."""
        src = _u8(pk48)
        if len(src) % 48:
            raise ValueError("48-byte compressed pubkeys expected")
        n = len(src) // 48
        st = np.zeros(max(n, 1), np.int8)
        fb = ctypes.c_uint32(0xFFFFFFFF)
        rc = self._lib.blsgpu_pubkeys_upload_compressed(self.h, first_index, src.ctypes.data if n else None, n,
                                                        PK_VALIDATE if validate else 0, st.ctypes.data,
                                                        ctypes.byref(fb))
        if rc >= 100 or rc == DEVICE_ERROR:
            raise RuntimeError(f"blsgpu_pubkeys_upload_compressed -> {code_name(rc)}")
        return st[:n], fb.value

    def read_pubkeys(self, first_index: int, n: int, out_len=96) -> bytes:
        """Table entries [first_index, first_index + n) as 96-byte uncompressed or 48-byte compressed encodings."""
        out = np.zeros(max(n * out_len, 1), np.uint8)
        rc = self._lib.blsgpu_pubkeys_read(self.h, first_index, n, out.ctypes.data, out_len)
        if rc != OK:
            raise RuntimeError(f"blsgpu_pubkeys_read -> {code_name(rc)}")
        return out[: n * out_len].tobytes()

    @property
    def pubkeys_count(self):
        return self._lib.blsgpu_pubkeys_count(self.h)

    def upload_committees(self, first_committee: int, committee_first, members):
        """blsgpu_committees_upload: drops the stored committees with id >= first_committee, then stores committees
        [first_committee, first_committee + n), committee c of the call being the table indices
        members[committee_first[c]: committee_first[c + 1]].  ValueError for a refused call (BLSGPU_ERR_ARGS)."""
        cf = np.ascontiguousarray(committee_first, dtype=np.uint32)
        mem = np.ascontiguousarray(members, dtype=np.uint32)
        if cf.ndim != 1 or len(cf) == 0:
            raise ValueError("committee_first needs n + 1 >= 1 entries")
        n = len(cf) - 1
        if len(mem) != int(cf[-1]):
            raise ValueError(f"committee_first ends at {int(cf[-1])}, got {len(mem)} members")
        rc = self._lib.blsgpu_committees_upload(self.h, first_committee, n, cf.ctypes.data if n else None,
                                                mem.ctypes.data if n else None)
        if rc == ERR_ARGS:
            raise ValueError("blsgpu_committees_upload -> BLSGPU_ERR_ARGS")
        if rc != OK:
            raise RuntimeError(f"blsgpu_committees_upload -> {code_name(rc)}")

    @property
    def committees_count(self):
        return self._lib.blsgpu_committees_count(self.h)

    def aggregate_pubkeys_bits(self, set_seg_first, seg_committee, set_bits_first, bits, flags=0, out_len=96):
        """blsgpu_aggregate_pubkeys_bits: the aggregated key of every set from its committees' participation bits.
        Returns (list of out_len-byte encodings, status int8 array, CommitteeBitsStats).  ValueError for a refused
        call (BLSGPU_ERR_ARGS), RuntimeError for a call-level failure."""
        ssf = np.ascontiguousarray(set_seg_first, dtype=np.uint32)
        sbf = np.ascontiguousarray(set_bits_first, dtype=np.uint32)
        seg = np.ascontiguousarray(seg_committee, dtype=np.uint32)
        if ssf.ndim != 1 or len(ssf) == 0 or sbf.shape != ssf.shape:
            raise ValueError("set_seg_first and set_bits_first need n_sets + 1 >= 1 entries each")
        n = len(ssf) - 1
        buf = _u8(bits)
        if len(seg) < int(ssf[-1]) or len(buf) < int(sbf[-1]):
            raise ValueError("seg_committee / bits shorter than the offsets say")
        if len(seg) == 0:
            seg = np.zeros(1, np.uint32)
        if len(buf) == 0:
            buf = np.zeros(1, np.uint8)
        out = np.zeros(max(n, 1) * out_len, np.uint8)
        st = np.zeros(max(n, 1), np.int8)
        stats = CommitteeBitsStats()
        rc = self._lib.blsgpu_aggregate_pubkeys_bits(self.h, n, ssf.ctypes.data, seg.ctypes.data, sbf.ctypes.data,
                                                     buf.ctypes.data, flags, out.ctypes.data, out_len, st.ctypes.data,
                                                     ctypes.byref(stats))
        if rc == ERR_ARGS:
            raise ValueError("blsgpu_aggregate_pubkeys_bits -> BLSGPU_ERR_ARGS")
        if rc != OK:
            raise RuntimeError(f"blsgpu_aggregate_pubkeys_bits -> {code_name(rc)}")
        return [out[out_len * i: out_len * (i + 1)].tobytes() for i in range(n)], st[:n], stats

    def verify_raw(self, job_first_set, sigs, sig_len, msgs, pk_bytes=None, set_pk_first=None, pk_index=None,
                   job_flags=None, sig_stride=None, seed=0x4C4F444553544152):
        """Low-level call: numpy/bytes arrays in, (job_result int8 array, Stats) out."""
        b, keep = make_batch(job_first_set, sigs, sig_len, msgs, pk_bytes, set_pk_first, pk_index, job_flags,
                             sig_stride, seed)
        res = np.zeros(max(b.n_jobs, 1), dtype=np.int8)
        st = Stats()
        rc = self._lib.blsgpu_verify(self.h, ctypes.byref(b), res.ctypes.data, ctypes.byref(st))
        if rc != OK:
            raise RuntimeError(f"blsgpu_verify -> {code_name(rc)}")
        return res[: b.n_jobs], st

    def submit_raw(self, job_first_set, sigs, sig_len, msgs, pk_bytes=None, set_pk_first=None, pk_index=None,
                   job_flags=None, sig_stride=None, seed=0x4C4F444553544152):
        """Asynchronous call (blsgpu_submit: inputs copied before it returns): a Pending whose wait() gives
        (job_result int8 array, Stats) once the runtime's done callback ran."""
        import threading

        b, keep = make_batch(job_first_set, sigs, sig_len, msgs, pk_bytes, set_pk_first, pk_index, job_flags,
                             sig_stride, seed)
        p = Pending()
        p.res = np.zeros(max(b.n_jobs, 1), dtype=np.int8)
        p.n_jobs = b.n_jobs
        p.st = Stats()
        p.ev = threading.Event()

        def done(user, status):
            p.status = status
            p.t_done = __import__("time").perf_counter()
            p.ev.set()

        p.cb = DONE_CB(done)  # kept alive with the Pending until the callback ran
        rc = self._lib.blsgpu_submit(self.h, ctypes.byref(b), p.res.ctypes.data, ctypes.byref(p.st), p.cb, None)
        if rc != OK:
            raise RuntimeError(f"blsgpu_submit -> {code_name(rc)}")
        return p

    def aggregate_pubkeys(self, pk_bytes=None, set_pk_first=None, pk_index=None, out_len=96):
        """PublicKey.aggregate(...).toBytes() per set on the GPU: (list of bytes, status int8 array)."""
        n = (len(set_pk_first) - 1) if set_pk_first is not None else len(pk_bytes) // 96
        b, keep = make_batch(np.array([0, n]), b"", np.zeros(n, np.uint32), b"", pk_bytes, set_pk_first, pk_index)
        out = np.zeros(max(n, 1) * out_len, np.uint8)
        st = np.zeros(max(n, 1), np.int8)
        rc = self._lib.blsgpu_aggregate_pubkeys(self.h, ctypes.byref(b), out.ctypes.data, out_len, st.ctypes.data)
        if rc != OK:
            raise RuntimeError(f"blsgpu_aggregate_pubkeys -> {code_name(rc)}")
        return [out[out_len * i: out_len * (i + 1)].tobytes() for i in range(n)], st[:n]

    def aggregate_signatures(self, sigs, group_first, sig_len=None, sig_stride=None, validate=True, out_len=96):
        """Signature.aggregate(sigs.map(fromBytes)).toBytes() per group on the GPU.  Group g owns signatures
        [group_first[g], group_first[g + 1]) of sigs[sig_stride * k] (sig_len[k] bytes each; default: all sig_stride).
        Returns (list of out_len-byte encodings, status int8 array, first_bad uint32 array); a rejected or empty group
        gives zero bytes.  ValueError for a malformed layout, before the library is called."""
        buf, gf, sl, stride = aggregate_layout(sigs, group_first, sig_len, sig_stride, out_len)
        n = len(gf) - 1
        if len(buf) == 0:
            buf = np.zeros(1, np.uint8)
        if len(sl) == 0:
            sl = np.zeros(1, np.uint32)
        out = np.zeros(max(n, 1) * out_len, np.uint8)
        st = np.zeros(max(n, 1), np.int8)
        fb = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
        rc = self._lib.blsgpu_aggregate_signatures(self.h, n, gf.ctypes.data, buf.ctypes.data, stride, sl.ctypes.data,
                                                   AGG_VALIDATE if validate else 0, out.ctypes.data, out_len,
                                                   st.ctypes.data, fb.ctypes.data)
        if rc != OK:
            raise RuntimeError(f"blsgpu_aggregate_signatures -> {code_name(rc)}")
        return [out[out_len * i: out_len * (i + 1)].tobytes() for i in range(n)], st[:n], fb[:n]

    def aggregate_with_randomness(self, group_first, sigs, pk_bytes=None, pk_index=None, sig_len=None,
                                  sig_stride=None, seed=0, out_pk_len=96, out_sig_len=192):
        """blst aggregateWithRandomness per group on the GPU: group g owns sets [group_first[g], group_first[g + 1]),
        set k = (pk_bytes[96 k] or table entry pk_index[k], sigs[sig_stride * k] of sig_len[k] bytes).  Returns (list
        of P encodings, list of S encodings, status int8 array, first_bad uint32 array); a rejected or empty group
        gives zero bytes.  seed 0 = fresh scalars (production); else the words of randomness_words(n, seed).
        ValueError for a malformed layout, before the library is called."""
        gf, buf, sl, stride, pkb, pki = awr_layout(group_first, sigs, pk_bytes, pk_index, sig_len, sig_stride,
                                                   out_pk_len, out_sig_len)
        n = len(gf) - 1
        if len(buf) == 0:
            buf = np.zeros(1, np.uint8)
        if len(sl) == 0:
            sl = np.zeros(1, np.uint32)
        if pkb is not None and len(pkb) == 0:
            pkb = np.zeros(1, np.uint8)
        if pki is not None and len(pki) == 0:
            pki = np.zeros(1, np.uint32)
        opk = np.zeros(max(n, 1) * out_pk_len, np.uint8)
        osig = np.zeros(max(n, 1) * out_sig_len, np.uint8)
        st = np.zeros(max(n, 1), np.int8)
        fb = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
        rc = self._lib.blsgpu_aggregate_with_randomness(
            self.h, n, gf.ctypes.data, None if pkb is None else pkb.ctypes.data,
            None if pki is None else pki.ctypes.data, buf.ctypes.data, stride, sl.ctypes.data, seed, opk.ctypes.data,
            out_pk_len, osig.ctypes.data, out_sig_len, st.ctypes.data, fb.ctypes.data)
        if rc != OK:
            raise RuntimeError(f"blsgpu_aggregate_with_randomness -> {code_name(rc)}")
        return ([opk[out_pk_len * i: out_pk_len * (i + 1)].tobytes() for i in range(n)],
                [osig[out_sig_len * i: out_sig_len * (i + 1)].tobytes() for i in range(n)], st[:n], fb[:n])

    def verify_same_message(self, group_first, msgs, sigs, pk_bytes=None, pk_index=None, sig_len=None,
                            sig_stride=None, seed=0, flags=0):
        """verifySignatureSetsSameMessage for many groups in one device call (blsgpu_verify_same_message): group g owns
        sets [group_first[g], group_first[g + 1]) and signs msgs[32 g]; sets as in aggregate_with_randomness.  Returns
        (set_result int8 array: 1 / 0 / -code per set, group_result int8 array: 1 accepted / 0 verified set by set /
        -9 empty, SameMessageStats).  ValueError for a malformed layout, before the library is called; RuntimeError
        for a call-level failure."""
        gf, buf, sl, stride, pkb, pki = awr_layout(group_first, sigs, pk_bytes, pk_index, sig_len, sig_stride)
        n_groups = len(gf) - 1
        n = int(gf[-1])
        m = _u8(msgs)
        if len(m) != 32 * n_groups:
            raise ValueError(f"{n_groups} groups need {32 * n_groups} message bytes, got {len(m)}")
        if len(m) == 0:
            m = np.zeros(1, np.uint8)
        if len(buf) == 0:
            buf = np.zeros(1, np.uint8)
        if len(sl) == 0:
            sl = np.zeros(1, np.uint32)
        if pkb is not None and len(pkb) == 0:
            pkb = np.zeros(1, np.uint8)
        if pki is not None and len(pki) == 0:
            pki = np.zeros(1, np.uint32)
        res = np.zeros(max(n, 1), np.int8)
        gres = np.zeros(max(n_groups, 1), np.int8)
        st = SameMessageStats()
        rc = self._lib.blsgpu_verify_same_message(
            self.h, n_groups, gf.ctypes.data, m.ctypes.data, None if pkb is None else pkb.ctypes.data,
            None if pki is None else pki.ctypes.data, buf.ctypes.data, stride, sl.ctypes.data, seed, flags,
            res.ctypes.data, gres.ctypes.data, ctypes.byref(st))
        if rc != OK:
            raise RuntimeError(f"blsgpu_verify_same_message -> {code_name(rc)}")
        return res[:n], gres[:n_groups], st

    def verify_same_message_agg(self, group_first, msgs, sigs, pk_bytes=None, pk_index=None, sig_len=None,
                                sig_stride=None, seed=0, flags=0, include=None, out_sig_len=96):
        """verify_same_message that also returns each group's aggregate of the signatures that verified
        (blsgpu_verify_same_message_agg).  include (a byte per set, default all): a set with include 0 is verified
        but left out of the sum.  Returns (set_result, group_result, SameMessageStats -- all as verify_same_message
        answers --, out_sig: list of out_sig_len-byte encodings, zero bytes for a group that summed nothing,
        agg_count uint32 array: the sets summed per group).  ValueError for a malformed layout, before the library is
        called; RuntimeError for a call-level failure."""
        gf, buf, sl, stride, pkb, pki = awr_layout(group_first, sigs, pk_bytes, pk_index, sig_len, sig_stride)
        n_groups = len(gf) - 1
        n = int(gf[-1])
        if out_sig_len not in (96, 192):
            raise ValueError("out_sig_len must be 96 or 192")
        m = _u8(msgs)
        if len(m) != 32 * n_groups:
            raise ValueError(f"{n_groups} groups need {32 * n_groups} message bytes, got {len(m)}")
        inc = None
        if include is not None:
            inc = np.ascontiguousarray(include, dtype=np.uint8)
            if inc.shape != (n,):
                raise ValueError(f"{n} sets need {n} include bytes, got shape {inc.shape}")
            if n == 0:
                inc = None
        if len(m) == 0:
            m = np.zeros(1, np.uint8)
        if len(buf) == 0:
            buf = np.zeros(1, np.uint8)
        if len(sl) == 0:
            sl = np.zeros(1, np.uint32)
        if pkb is not None and len(pkb) == 0:
            pkb = np.zeros(1, np.uint8)
        if pki is not None and len(pki) == 0:
            pki = np.zeros(1, np.uint32)
        res = np.zeros(max(n, 1), np.int8)
        gres = np.zeros(max(n_groups, 1), np.int8)
        out = np.zeros(max(n_groups, 1) * out_sig_len, np.uint8)
        cnt = np.zeros(max(n_groups, 1), np.uint32)
        st = SameMessageStats()
        rc = self._lib.blsgpu_verify_same_message_agg(
            self.h, n_groups, gf.ctypes.data, m.ctypes.data, None if pkb is None else pkb.ctypes.data,
            None if pki is None else pki.ctypes.data, buf.ctypes.data, stride, sl.ctypes.data, seed, flags,
            res.ctypes.data, gres.ctypes.data, ctypes.byref(st), None if inc is None else inc.ctypes.data,
            out.ctypes.data, out_sig_len, cnt.ctypes.data)
        if rc != OK:
            raise RuntimeError(f"blsgpu_verify_same_message_agg -> {code_name(rc)}")
        return (res[:n], gres[:n_groups], st,
                [out[out_sig_len * g: out_sig_len * (g + 1)].tobytes() for g in range(n_groups)], cnt[:n_groups])

    def aggregate_verify(self, job_first, msgs, sigs, pk_bytes=None, pk_len=96, pk_index=None, sig_len=None,
                         sig_stride=None, flags=0):
        """AggregateVerify for many jobs in one device call (blsgpu_aggregate_verify): job j owns pairs [job_first[j],
        job_first[j + 1]), pair k = (pk_bytes[pk_len k] or table entry pk_index[k], msgs[32 k]), and has the one
        signature sigs[sig_stride * j] of sig_len[j] bytes (default: all sig_stride).  flags: AV_VALIDATE_KEYS (the
        keys are untrusted, pk_len 48 or 96), AV_LANE_FORMS.  Returns (job_result int8 array: 1 / 0 / -code per job,
        first_bad uint32 array: the call index of the job's rejected key or 0xffffffff, AggregateVerifyStats).
        ValueError for a malformed layout, before the library is called; RuntimeError for a call-level failure."""
        jf = np.ascontiguousarray(job_first, dtype=np.int64)
        if jf.ndim != 1 or len(jf) == 0:
            raise ValueError("job_first needs n_jobs + 1 >= 1 entries")
        if jf[0] != 0 or (np.diff(jf) < 0).any():
            raise ValueError("job_first must start at 0 and never decrease")
        n_jobs, n = len(jf) - 1, int(jf[-1])
        if n > AGG_MAX_SIGS:
            raise ValueError(f"at most {AGG_MAX_SIGS} pairs per call")
        # the signatures: one per job, laid out as one group of n_jobs signatures
        buf, _, sl, stride = aggregate_layout(sigs, [0, n_jobs], sig_len, sig_stride)
        if (pk_bytes is None) == (pk_index is None):
            raise ValueError("exactly one of pk_bytes and pk_index")
        m = _u8(msgs)
        if len(m) != 32 * n:
            raise ValueError(f"{n} pairs need {32 * n} message bytes, got {len(m)}")
        pkb = pki = None
        if pk_bytes is not None:
            if pk_len not in ((48, 96) if flags & AV_VALIDATE_KEYS else (96,)):
                raise ValueError("pk_len must be 96, or 48 / 96 with AV_VALIDATE_KEYS")
            pkb = _u8(pk_bytes)
            if len(pkb) != pk_len * n:
                raise ValueError(f"{n} pairs need {pk_len * n} pubkey bytes, got {len(pkb)}")
        else:
            if flags & AV_VALIDATE_KEYS:
                raise ValueError("AV_VALIDATE_KEYS needs pk_bytes: table entries are trusted")
            idx = np.ascontiguousarray(pk_index, dtype=np.int64)
            if idx.ndim != 1 or len(idx) != n:
                raise ValueError(f"pk_index needs one entry per pair ({n})")
            if n and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
                raise ValueError("pk_index entries must be table indices")
            pki = idx.astype(np.uint32)
        pad = lambda a, t: np.zeros(1, t) if a is not None and len(a) == 0 else a  # noqa: E731
        m, buf, sl, pkb, pki = pad(m, np.uint8), pad(buf, np.uint8), pad(sl, np.uint32), pad(pkb, np.uint8), \
            pad(pki, np.uint32)
        jf = jf.astype(np.uint32)
        res = np.zeros(max(n_jobs, 1), np.int8)
        fb = np.full(max(n_jobs, 1), 0xFFFFFFFF, np.uint32)
        st = AggregateVerifyStats()
        rc = self._lib.blsgpu_aggregate_verify(
            self.h, n_jobs, jf.ctypes.data, m.ctypes.data, None if pkb is None else pkb.ctypes.data, pk_len,
            None if pki is None else pki.ctypes.data, buf.ctypes.data, stride, sl.ctypes.data, flags,
            res.ctypes.data, fb.ctypes.data, ctypes.byref(st))
        if rc != OK:
            raise RuntimeError(f"blsgpu_aggregate_verify -> {code_name(rc)}")
        return res[:n_jobs], fb[:n_jobs], st

    def key_validate(self, pks: bytes, pk_len: int):
        """KeyValidate on the GPU: (96-byte uncompressed keys, status int8 array)."""
        n = len(pks) // pk_len
        src = _u8(pks)
        out = np.zeros(max(n, 1) * 96, np.uint8)
        st = np.zeros(max(n, 1), np.int8)
        rc = self._lib.blsgpu_key_validate(self.h, n, src.ctypes.data, pk_len, pk_len, out.ctypes.data, st.ctypes.data)
        if rc != OK:
            raise RuntimeError(f"blsgpu_key_validate -> {code_name(rc)}")
        return out[: 96 * n].tobytes(), st[:n]

    def signing_roots(self, kind: int, objects: bytes, domains: bytes):
        """computeSigningRoot on the GPU: one domain for all (32 B) or one per object."""
        obj_len = 32 if kind == ROOT_OBJECT else 128
        n = len(objects) // obj_len
        o, d = _u8(objects), _u8(domains)
        dstride = 0 if len(domains) == 32 else 32
        out = np.zeros(max(n, 1) * 32, np.uint8)
        rc = self._lib.blsgpu_signing_roots(self.h, kind, n, o.ctypes.data, obj_len, d.ctypes.data, dstride,
                                            out.ctypes.data)
        if rc != OK:
            raise RuntimeError(f"blsgpu_signing_roots -> {code_name(rc)}")
        return [out[32 * i: 32 * i + 32].tobytes() for i in range(n)]

    def debug_op(self, op: int, inputs: bytes, in_stride: int, out_stride: int):
        n = len(inputs) // in_stride
        inb = np.frombuffer(inputs, dtype=np.uint8).copy()
        out = np.zeros(n * out_stride, dtype=np.uint8)
        st = np.zeros(n, dtype=np.int32)
        rc = self._lib.blsgpu_debug_op(self.h, op, n, inb.ctypes.data, in_stride, out.ctypes.data, out_stride,
                                       st.ctypes.data)
        if rc != OK:
            raise RuntimeError(f"blsgpu_debug_op -> {code_name(rc)}")
        return out.tobytes(), st
