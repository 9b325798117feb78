#!/usr/bin/env python3
"""Times blsgpu_aggregate_signatures (Signature.aggregate on the GPU) on one device and prints one JSON line.

Shapes, all compressed in and out, validate = true, over the same 16,384 device-made signatures:
    256 groups of 64        16,384 groups of 1        32 groups of 512
Each shape is warmed up, then timed `--calls` times (>= 20): a host clock around the C call, which ends in a stream
synchronise, so a call's time holds its input copy, the decode + subgroup check, the segmented sum, the serialization
and the output copy.  The median, the minimum and the maximum are reported, and one check per shape that the device's
answer did not change between the first and the last call.

Yardstick: the verify pipeline's own sig_decode stage (blsgpu_stats.stage_ms[0], option "profile" 1) of a 16,384-set
single-set call in the same process -- HIP-event kernel time of the part of aggregation that already existed (no
copies), median of `--calls` calls.  ratio = shape median / yardstick.

    python tools/bench_sig_aggregate.py [--calls 30] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SIGS = 16384
SHAPES = [("256x64", 256, 64), ("16384x1", 16384, 1), ("32x512", 32, 512)]
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def workload(ctx):
    """16,384 (pubkey, message, signature) triples made on the device (debug ops 8 and 7, pinned to the oracle by
    tests/test_gpu_parity.py)."""
    sks = [(int.from_bytes(hashlib.sha256(i.to_bytes(32, "little")).digest(), "little") % R_ORDER).to_bytes(32, "big")
           for i in range(N_SIGS)]
    msgs = [hashlib.sha256(b"bench_sig_aggregate" + j.to_bytes(4, "little")).digest() for j in range(N_SIGS)]
    pks, st = ctx.debug_op(8, b"".join(sks), 32, 96)
    assert (st == 0).all()
    sigs, st = ctx.debug_op(7, b"".join(sk + m for sk, m in zip(sks, msgs)), 64, 96)
    assert (st == 0).all()
    return pks, b"".join(msgs), sigs


def time_shape(ctx, lib, native, sigs, n_groups, size, calls, warmup):
    buf = np.frombuffer(sigs, np.uint8)
    first = (np.arange(n_groups + 1, dtype=np.uint32) * size).astype(np.uint32)
    sl = np.full(N_SIGS, 96, np.uint32)
    out = np.zeros(n_groups * 96, np.uint8)
    st = np.zeros(n_groups, np.int8)
    fb = np.zeros(n_groups, np.uint32)

    def call():
        rc = lib.blsgpu_aggregate_signatures(ctx.h, n_groups, first.ctypes.data, buf.ctypes.data, 96, sl.ctypes.data,
                                             native.AGG_VALIDATE, out.ctypes.data, 96, st.ctypes.data, fb.ctypes.data)
        if rc != native.OK:
            raise RuntimeError(f"blsgpu_aggregate_signatures -> {native.code_name(rc)}")

    call()
    ref = out.copy()
    assert not st.any(), "the workload's signatures are valid"
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    assert np.array_equal(out, ref) and not st.any()
    return {"groups": n_groups, "group_size": size, "lanes": native.sig_agg_lanes(n_groups, N_SIGS),
            "median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": calls}


def yardstick(ctx, pks, msgs, sigs, calls, warmup):
    ctx.set_option("profile", 1)
    args = dict(job_first_set=np.arange(N_SIGS + 1), sigs=sigs, sig_len=[96] * N_SIGS, msgs=msgs, pk_bytes=pks,
                job_flags=np.ones(N_SIGS), sig_stride=96)
    ms = []
    for k in range(warmup + calls):
        res, st = ctx.verify_raw(**args)
        assert (res == 1).all()
        if k >= warmup:
            ms.append(st.stage_ms[0])
    ctx.set_option("profile", 0)
    return {"sets": N_SIGS, "stage": "sig_decode", "median_ms": statistics.median(ms), "min_ms": min(ms),
            "max_ms": max(ms), "calls": calls}


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
        lib = native.load()
        pks, msgs, sigs = workload(ctx)
        y = yardstick(ctx, pks, msgs, sigs, a.calls, a.warmup)
        shapes = {}
        for name, g, size in SHAPES:
            r = time_shape(ctx, lib, native, sigs, g, size, a.calls, a.warmup)
            r["ratio_to_sig_decode"] = r["median_ms"] / y["median_ms"]
            shapes[name] = r
    finally:
        ctx.close()
    line = json.dumps({"bench": "sig_aggregate", "signatures": N_SIGS, "yardstick": y, "shapes": shapes})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
