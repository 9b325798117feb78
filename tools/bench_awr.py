#!/usr/bin/env python3
"""Times blsgpu_aggregate_with_randomness (blst aggregateWithRandomness on the GPU) on one device and prints one JSON
line.

Two calls over the same 16,384 device-made (key, message, signature) triples, bytes-mode keys, compressed signatures,
96- / 192-byte outputs, seed 0 (fresh scalars per call):
    128 groups of 128 sets (every set of a group signs the group's message)        16,384 groups of one set
Each is compared with two existing alternatives on the same library and the same sets:
    verify        blsgpu_verify of the sets as one-set batchable jobs (what a caller without the same-message path does)
    aggregate     blsgpu_aggregate_signatures of the same signatures in the same groups (decode + subgroup check + plain
                  G2 sums: the part of the work that has no scalar multiplication)
Every call is warmed up, then timed `--calls` times (>= 20) with a host clock around the C call, which ends in a
stream synchronise (blsgpu_verify: in its completion), so a time holds the input copy, every kernel and the output
copy.  Medians, minima and maxima are reported.  Kernel times come from a run of their own under
`rocprofv3 --kernel-trace --stats` (k_sig_decode, k_sig_subgroup*, k_awr_sum<fp / fp2, L>, k_awr_serialize).

    python tools/bench_awr.py [--calls 30] [--warmup 5] [--out FILE]
"""
import argparse
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SETS = 16384
SHAPES = [("128x128", 128, 128), ("16384x1", 16384, 1)]
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def workload(ctx, size):
    """16,384 (pubkey, message, signature) triples made on the device (debug ops 8 and 7, pinned to the oracle by
    tests/test_gpu_parity.py); set k signs message k // size."""
    sks = [(int.from_bytes(hashlib.sha256(i.to_bytes(32, "little")).digest(), "little") % R_ORDER).to_bytes(32, "big")
           for i in range(N_SETS)]
    msgs = [hashlib.sha256(b"bench_awr" + (j // size).to_bytes(4, "little")).digest() for j in range(N_SETS)]
    pks, st = ctx.debug_op(8, b"".join(sks), 32, 96)
    assert (st == 0).all()
    sigs, st = ctx.debug_op(7, b"".join(sk + m for sk, m in zip(sks, msgs)), 64, 96)
    assert (st == 0).all()
    return pks, b"".join(msgs), sigs


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


def time_shape(ctx, native, n_groups, size, calls, warmup):
    pks, msgs, sigs = workload(ctx, size)
    first = np.arange(n_groups + 1, dtype=np.uint32) * size
    buf = np.frombuffer(sigs, np.uint8)
    pkb = np.frombuffer(pks, np.uint8)
    sl = np.full(N_SETS, 96, np.uint32)
    last = {}

    def awr():
        last["awr"] = ctx.aggregate_with_randomness(first, buf, pk_bytes=pkb, sig_len=sl, sig_stride=96, seed=0)

    def aggregate():
        last["agg"] = ctx.aggregate_signatures(buf, first, sig_len=sl, sig_stride=96)

    verify_args = dict(job_first_set=np.arange(N_SETS + 1), sigs=sigs, sig_len=sl, msgs=msgs, pk_bytes=pks,
                       job_flags=np.ones(N_SETS), sig_stride=96, seed=0)

    def verify():
        last["ver"] = ctx.verify_raw(**verify_args)

    out = {"groups": n_groups, "group_size": size, "lanes": native.awr_lanes(n_groups, N_SETS)}
    out["aggregate_with_randomness"] = timed(awr, calls, warmup)
    out["aggregate_signatures"] = timed(aggregate, calls, warmup)
    out["verify"] = timed(verify, calls, warmup)
    assert not last["awr"][2].any() and not last["agg"][1].any() and (last["ver"][0] == 1).all()
    # the aggregates are what they claim to be: each (P, message, S) verifies
    p, s = last["awr"][0], last["awr"][1]
    res, _ = ctx.verify_raw(np.arange(n_groups + 1), b"".join(s), [192] * n_groups,
                            b"".join(msgs[32 * size * g: 32 * size * g + 32] for g in range(n_groups)),
                            pk_bytes=b"".join(p), job_flags=np.ones(n_groups), sig_stride=192)
    assert (res == 1).all()
    a = out["aggregate_with_randomness"]["median_ms"]
    out["ratio_to_verify"] = a / out["verify"]["median_ms"]
    out["ratio_to_aggregate_signatures"] = a / out["aggregate_signatures"]["median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    from lodestar_amd import native

    ctx = native.Context([0])  # fails loudly without a GPU: there is nothing to time elsewhere
    try:
        shapes = {name: time_shape(ctx, native, g, size, a.calls, a.warmup) for name, g, size in SHAPES}
    finally:
        ctx.close()
    line = json.dumps({"bench": "aggregate_with_randomness", "sets": N_SETS, "shapes": shapes})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
