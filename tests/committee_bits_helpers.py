"""Inputs and oracle answers shared by the committee-bits tests (tests/test_committee_bits_host.py on the CPU,
tests/test_gpu_committee_bits*.py on the GPU).  The table holds 600 interop keys and five keys built to
cancel: P, -P (secret keys sk and r - sk), P', -P' and Q.  The sum of table keys is (sum of their secret keys mod r) G,
so the oracle's answer for a set is one scalar multiplication (cpu.sk_to_pk), the identity encoding when the secret
keys add up to 0 mod r."""
import functools
import hashlib

import numpy as np

from oracle import bls12_381 as bls
from oracle import cpu

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
N_INTEROP = 600
SIZES = [1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 512]
EMPTY_AGGREGATE = 9
NO_COMPLEMENT = 1


def interop_sk(i):
    return int.from_bytes(hashlib.sha256(i.to_bytes(32, "little")).digest(), "little") % R_ORDER


SK_P, SK_P2, SK_Q = interop_sk(1000), interop_sk(1001), interop_sk(1002)
# table indices of the cancelling keys
P, NEG_P, P2, NEG_P2, Q = (N_INTEROP + k for k in range(5))
SKS = [interop_sk(i) for i in range(N_INTEROP)] + [SK_P, R_ORDER - SK_P, SK_P2, R_ORDER - SK_P2, SK_Q]


def sks_bytes():
    return b"".join(s.to_bytes(32, "big") for s in SKS)


@functools.lru_cache(maxsize=None)
def table_pk96():
    """The table's keys, 96 bytes each, from the oracle."""
    return cpu.sk_to_pk(sks_bytes())


def identity(out_len):
    return bytes([0xC0 if out_len == 48 else 0x40]) + bytes(out_len - 1)


def oracle_sums(index_lists, out_len):
    """[(encoding, status)] of the aggregated key of every index list: the oracle's (sum of secret keys) G."""
    scalars = [sum(SKS[int(i)] for i in idx) % R_ORDER for idx in index_lists]
    finite = [k for k, idx in enumerate(index_lists) if len(idx) and scalars[k]]
    pk96 = cpu.sk_to_pk(b"".join(scalars[k].to_bytes(32, "big") for k in finite)) if finite else b""
    enc = {k: pk96[96 * j: 96 * j + 96] for j, k in enumerate(finite)}
    out = []
    for k, idx in enumerate(index_lists):
        if len(idx) == 0:
            out.append((bytes(out_len), EMPTY_AGGREGATE))
        elif k not in enc:
            out.append((identity(out_len), 0))
        else:
            out.append((enc[k] if out_len == 96 else bls.g1_compress(bls.g1_deserialize(enc[k])), 0))
    return out


def pack(bits):
    """SSZ bit order: bit i is byte[i // 8] >> (i % 8) & 1; the padding bits are zero."""
    return np.packbits(np.asarray(bits, dtype=bool), bitorder="little").tobytes()


@functools.lru_cache(maxsize=None)
def size_committees():
    """One committee per size of SIZES: distinct interop keys in a seeded random order."""
    rng = np.random.default_rng(0xC0117)
    return tuple(tuple(int(x) for x in rng.permutation(N_INTEROP)[:n]) for n in SIZES)


def participations(n, rng):
    """The participation patterns the tests run for a committee of n members: {name: bool array}.  The tie of the
    complement rule is absent + 1 == present, i.e. present = (n + 1) / 2: the three counts around it are taken (for an
    even n the rule has no exact tie; the counts on both sides of it are still those)."""
    def some(present):
        b = np.zeros(n, bool)
        b[rng.permutation(n)[:present]] = True
        return b

    out = {"none": np.zeros(n, bool), "all": np.ones(n, bool), "half": rng.random(n) < 0.5}
    for name, pos in (("first", 0), ("last", n - 1)):
        one, clear = np.zeros(n, bool), np.ones(n, bool)
        one[pos], clear[pos] = True, False
        out["one_" + name], out["clear_" + name] = one, clear
    p0 = (n + 1) // 2
    for name, present in (("tie_below", p0 - 1), ("tie", p0), ("tie_above", p0 + 1)):
        out[name] = some(min(max(present, 0), n))
    return out


def expand(committees, sets):
    """The index lists of `sets` -- a set is a list of (committee id, bool array) -- as getAttestingIndices gives them."""
    return [[committees[c][i] for c, bits in s for i in np.flatnonzero(bits)] for s in sets]


def call_arrays(sets):
    """(set_seg_first, seg_committee, set_bits_first, bits) of blsgpu_aggregate_pubkeys_bits for `sets`."""
    ssf, sbf, seg, parts = [0], [0], [], []
    for s in sets:
        seg += [c for c, _ in s]
        parts.append(pack(np.concatenate([np.asarray(b, bool) for _, b in s])) if s else b"")
        ssf.append(len(seg))
        sbf.append(sbf[-1] + len(parts[-1]))
    return (np.array(ssf, np.uint32), np.array(seg, np.uint32), np.array(sbf, np.uint32),
            np.frombuffer(b"".join(parts), np.uint8).copy())


def plan(committees, sets, no_complement=False):
    """What the host plan must say for `sets`, from the rule alone: a segment is complemented iff absent + 1 < present.
    {segments, segments_complemented, keys_present, keys_added, keys_subtracted, n_items}."""
    p = dict(segments=0, segments_complemented=0, keys_present=0, keys_added=0, keys_subtracted=0)
    for s in sets:
        for c, bits in s:
            size, present = len(committees[c]), int(np.count_nonzero(bits))
            p["segments"] += 1
            p["keys_present"] += present
            if not no_complement and size - present + 1 < present:
                p["segments_complemented"] += 1
                p["keys_subtracted"] += size - present
            else:
                p["keys_added"] += present
    p["n_items"] = p["keys_added"] + p["keys_subtracted"] + p["segments_complemented"]
    return p


def lanes_rule(n_sets, n_items):
    """The lane rule restated: the count rule of the pubkey aggregation capped by the mean items of a set."""
    if n_sets == 0:
        return 8
    chip = 1024 * 64
    by_count = 64 if n_sets * 64 <= chip else 32 if n_sets * 32 <= 2 * chip else 16 if n_sets * 16 <= 2 * chip else 8
    mean = -(-n_items // n_sets)
    by_size = 8 if mean <= 8 else 16 if mean <= 16 else 32 if mean <= 32 else 64
    return min(by_count, by_size)


# the cancellation cases: (name, committee of table indices, participation bits, the segment is complemented by default)
# Under the rule (absent + 1 < present) a three-member committee with one absent is summed directly, so each of those
# cases has a sibling with members repeated until the rule takes the complement.
_FILL = tuple(range(31))
_ACROSS = (1,) + (0,) * 31 + (1,) + (0,) * 31  # members 0 and 32: two lanes, met by the butterfly's addition
CANCELLATION = [
    ("sum_is_identity", (P, NEG_P), (1, 1), True),                      # the stored sum is the identity
    ("q_absent", (P, NEG_P, Q), (1, 1, 0), False),                      # P + (-P): opposite points
    ("q_absent_complement", (P, NEG_P, Q, P2, NEG_P2), (1, 1, 0, 1, 1), True),  # stored Q, minus Q: the identity
    ("absent_equals_sum", (P, P2, NEG_P2), (0, 1, 1), False),           # P' + (-P')
    ("absent_equals_sum_complement", (P, P2, NEG_P2, P2, NEG_P2), (0, 1, 1, 1, 1), True),  # stored P, minus P
    ("double_all", (P, P), (1, 1), True),                               # stored 2P: the doubling branch at upload
    ("double_one_absent", (P, P), (1, 0), False),                       # P
    ("double_direct", (P, P, P), (1, 1, 0), False),                     # P + P in the bits kernel: the doubling branch
    ("double_complement", (P, P, P, P), (1, 1, 1, 0), True),            # stored 4P, minus P
    ("equal_across_lanes", (P,) + _FILL + (P,) + _FILL, _ACROSS, False),       # lane 0 holds P, lane 1 holds P
    ("opposite_across_lanes", (P,) + _FILL + (NEG_P,) + _FILL, _ACROSS, False),  # lane 0 holds P, lane 1 holds -P
]
