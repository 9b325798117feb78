#!/usr/bin/env python3
"""Times blsgpu_aggregate_verify (batched AggregateVerify) against what the library offered before it for the same
pairs, on one device, in one process and library, and prints one JSON line.

Device-made keys and signatures (debug ops 8 and 7, pinned to the oracle by tests/test_gpu_parity.py).  Pair k is (key k,
message k): every message of a call is distinct.  A job's signature is the sum of its pairs' signatures
(Context.aggregate_signatures).  Shapes: 16,384 jobs x 1 pair, 4,096 x 4, 64 x 256.
Per shape:
    aggregate_verify  Context.aggregate_verify, trusted 96-byte keys: k + 1 Miller items with shared squarings and one
                      final exponentiation per job of k pairs
    verify            the yardstick, existing behaviour: Context.verify_raw of the same pairs as one-set non-batchable
                      jobs, each with its own signature -- 2 Miller loops and 1 final exponentiation per pair
Both answers are checked (every job 1) before anything is timed.  The legs are warmed up `--warmup` times and timed
`--calls` times, alternately (one call of each per round), with a host clock around the calls, which end in a stream
synchronise; medians, minima and maxima are reported.

    python tools/bench_aggregate_verify.py [--calls 30] [--warmup 5] [--out FILE] [--shapes 16384x1,4096x4,64x256]
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

SHAPES = [(16384, 1), (4096, 4), (64, 256)]
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def workload(ctx, n_jobs, size):
    n = n_jobs * size
    sks = [(int.from_bytes(hashlib.sha256(i.to_bytes(32, "little")).digest(), "little") % R_ORDER).to_bytes(32, "big")
           for i in range(n)]
    msgs = [hashlib.sha256(b"bench_aggregate_verify" + k.to_bytes(4, "little")).digest() for k in range(n)]
    pks, st = ctx.debug_op(8, b"".join(sks), 32, 96)
    assert (st == 0).all()
    sigs, st = ctx.debug_op(7, b"".join(sk + m for sk, m in zip(sks, msgs)), 64, 96)
    assert (st == 0).all()
    first = np.arange(n_jobs + 1, dtype=np.uint32) * size
    if size == 1:
        job_sigs = sigs
    else:
        out, st, _ = ctx.aggregate_signatures(sigs, first, sig_stride=96, validate=False)
        assert (st == 0).all()
        job_sigs = b"".join(out)
    return pks, b"".join(msgs), sigs, job_sigs, first


def timed(fns, calls, warmup):
    """Times the legs alternately (one call of each per round), so drift on a shared host falls on all of them alike."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    ms = {name: [] for name in fns}
    for _ in range(calls):
        for name, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": calls}
            for name, v in ms.items()}


def time_shape(ctx, n_jobs, size, calls, warmup):
    pks, msgs, sigs, job_sigs, first = workload(ctx, n_jobs, size)
    n = n_jobs * size
    pkb = np.frombuffer(pks, np.uint8)
    mb = np.frombuffer(msgs, np.uint8)
    jsb = np.frombuffer(job_sigs, np.uint8)
    sb = np.frombuffer(sigs, np.uint8)
    jl = np.full(n_jobs, 96, np.uint32)
    sl = np.full(n, 96, np.uint32)
    sets = np.arange(n + 1, dtype=np.uint32)
    flags = np.zeros(n, np.uint8)  # non-batchable one-set jobs: each its own pairing check
    last = {}

    def aggregate_verify():
        last["av"] = ctx.aggregate_verify(first, mb, jsb, pk_bytes=pkb, sig_len=jl, sig_stride=96)

    def verify():
        last["v"] = ctx.verify_raw(sets, sb, sl, mb, pk_bytes=pkb, job_flags=flags, sig_stride=96, seed=0)

    aggregate_verify()
    res, _, st = last["av"]
    assert (res == 1).all() and st.jobs_checked == n_jobs and st.miller_items == n + n_jobs
    verify()
    assert (last["v"][0] == 1).all()
    out = {"jobs": n_jobs, "pairs_per_job": size, "form": st.form, "miller_items": st.miller_items,
           "miller_chunks": st.miller_chunks, "unique_messages": st.unique_messages}
    out.update(timed({"aggregate_verify": aggregate_verify, "verify": verify}, calls, warmup))
    out["aggregate_verify"]["device_ms_last"] = last["av"][2].device_ms
    out["aggregate_verify_over_verify"] = out["aggregate_verify"]["median_ms"] / out["verify"]["median_ms"]
    # operation counts per call: Miller items (shared squarings within a job's chunks) and final exponentiations
    out["ops"] = {"aggregate_verify": {"miller_items": n + n_jobs, "final_exps": n_jobs},
                  "verify": {"miller_loops": 2 * n, "final_exps": n}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--shapes", default=",".join(f"{j}x{k}" for j, k in SHAPES), help="jobs x pairs, comma separated")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",")]
    from lodestar_amd import native

    ctx = native.Context([0])  # fails loudly without a GPU: there is nothing to time elsewhere
    try:
        res = {f"{j}x{k}": time_shape(ctx, j, k, a.calls, a.warmup) for j, k in shapes}
    finally:
        ctx.close()
    line = json.dumps({"bench": "aggregate_verify", "shapes": res})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
