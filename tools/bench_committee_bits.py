#!/usr/bin/env python3
"""Times pubkey aggregation from committee participation bits against aggregation from expanded index lists, at bench
config C4's shape, on one device, and prints one JSON line.

The workload is bench.py's build_c4 itself: a 2^20-key table, 2,048 committees of 512 (consecutive slices of its seeded
permutation), 32,768 aggregate sets with its 0-10 % dropout per set, signed on the device.  The committees go to the
committee store once; every set's participation bits are read off build_c4's index lists.

Aggregation legs (each a synchronous library call that ends in a stream synchronise; the same keys come back):
    a_index_lists     blsgpu_aggregate_pubkeys, table mode, on the expanded lists (4 bytes per participant go up)
    b_bits_direct     blsgpu_aggregate_pubkeys_bits with BLSGPU_BITS_NO_COMPLEMENT (bits go up, every participant added)
    c_bits            blsgpu_aggregate_pubkeys_bits as shipped (a nearly full committee: its stored sum minus the absent)
Verify legs, end to end:
    v_table           blsgpu_verify in table mode (the pipeline aggregates the expanded lists itself)
    v_bits_then_bytes leg c, then blsgpu_verify in bytes mode on the keys it returned (the round trip included)
Before anything is timed the three aggregation legs are compared byte for byte and both verify legs must accept every
job.  The legs are then warmed up `--warmup` times and timed `--calls` times alternately (one call of each per round)
with a host clock; median, minimum and maximum are reported, and `accepted`: c's median lies below a's by more than
the larger min-max spread of the two.

    python tools/bench_committee_bits.py [--calls 10] [--warmup 3] [--out FILE]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_VAL, N_COMM, CSIZE = 1 << 20, 2048, 512


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "committee_bits_bench.json"))
    args = ap.parse_args()

    import bench
    from lodestar_amd import native
    from lodestar_amd.native import Context

    lib = native.load()
    ctx = Context([0])
    w, n, desc, _ = bench.build_c4(ctx, 0, 1)
    spf, idx = w["set_pk_first"], w["pk_index"]
    # build_c4's committees: consecutive 512-slices of the first draw of its generator
    perm = np.random.default_rng(bench.SEED).permutation(N_VAL).astype(np.uint32)
    ctx.upload_committees(0, np.arange(0, N_VAL + 1, CSIZE), perm)
    assert ctx.committees_count == N_COMM
    committee = np.array(w["_mkey"], np.uint32)  # one message per committee: the message key is the committee
    bits = np.zeros((n, CSIZE // 8), np.uint8)
    for s in range(n):
        members = perm[committee[s] * CSIZE: (committee[s] + 1) * CSIZE]
        present = np.isin(members, idx[spf[s]: spf[s + 1]])
        assert int(present.sum()) == int(spf[s + 1] - spf[s])
        bits[s] = np.packbits(present, bitorder="little")
    ssf = np.arange(n + 1, dtype=np.uint32)
    sbf = (np.arange(n + 1, dtype=np.uint64) * (CSIZE // 8)).astype(np.uint32)
    bits = np.ascontiguousarray(bits.reshape(-1))

    b_table, keep_t = native.make_batch(w["job_first_set"], w["sigs"], w["sig_len"], w["msgs"], set_pk_first=spf,
                                        pk_index=idx, job_flags=w["job_flags"], sig_stride=96)
    outs = {k: np.zeros(n * 96, np.uint8) for k in "abc"}
    sts = {k: np.full(n, 99, np.int8) for k in "abc"}
    b_bytes, keep_b = native.make_batch(w["job_first_set"], w["sigs"], w["sig_len"], w["msgs"], pk_bytes=outs["c"],
                                        job_flags=w["job_flags"], sig_stride=96)
    assert b_bytes.pk_bytes == outs["c"].ctypes.data  # the batch reads leg c's output buffer in place
    stats = {k: native.CommitteeBitsStats() for k in "bc"}
    res = {k: np.zeros(b_table.n_jobs, np.int8) for k in ("table", "bytes")}
    vst = native.Stats()

    def a_index_lists():
        rc = lib.blsgpu_aggregate_pubkeys(ctx.h, ctypes.byref(b_table), outs["a"].ctypes.data, 96, sts["a"].ctypes.data)
        assert rc == 0

    def bits_call(k, flags):
        def run():
            rc = lib.blsgpu_aggregate_pubkeys_bits(ctx.h, n, ssf.ctypes.data, committee.ctypes.data, sbf.ctypes.data,
                                                   bits.ctypes.data, flags, outs[k].ctypes.data, 96, sts[k].ctypes.data,
                                                   ctypes.byref(stats[k]))
            assert rc == 0
        return run

    def v_table():
        assert lib.blsgpu_verify(ctx.h, ctypes.byref(b_table), res["table"].ctypes.data, ctypes.byref(vst)) == 0

    c_bits = bits_call("c", 0)

    def v_bits_then_bytes():
        c_bits()
        assert lib.blsgpu_verify(ctx.h, ctypes.byref(b_bytes), res["bytes"].ctypes.data, ctypes.byref(vst)) == 0

    fns = {"a_index_lists": a_index_lists, "b_bits_direct": bits_call("b", native.BITS_NO_COMPLEMENT),
           "c_bits": c_bits, "v_table": v_table, "v_bits_then_bytes": v_bits_then_bytes}
    for fn in fns.values():
        fn()
    assert not sts["a"].any() and (sts["a"] == sts["b"]).all() and (sts["a"] == sts["c"]).all()
    assert (outs["a"] == outs["b"]).all() and (outs["a"] == outs["c"]).all(), "the legs' keys differ"
    assert (res["table"] == 1).all() and (res["bytes"] == 1).all(), "a verify leg rejected a job"
    legs = timed(fns, args.calls, args.warmup)
    ctx.close()

    a, c = legs["a_index_lists"], legs["c_bits"]
    spread = max(a["max_ms"] - a["min_ms"], c["max_ms"] - c["min_ms"])
    count = lambda s: {f: getattr(s, f) for f, _ in s._fields_ if f != "device_ms"}  # noqa: E731
    out = {"tool": "tools/bench_committee_bits.py", "workload": desc["workload"], "sets": n,
           "keys_present": int(spf[-1]), "h2d_bytes": {"a_index_lists": int(4 * spf[-1] + 4 * (n + 1)),
                                                       "c_bits": int(len(bits) + 4 * (3 * n + 3))},
           "stats": {"b_bits_direct": count(stats["b"]), "c_bits": count(stats["c"])},
           "legs": legs, "outputs_equal": True,
           "ratio_a_over_c": a["median_ms"] / c["median_ms"],
           "ratio_v_table_over_v_bits": legs["v_table"]["median_ms"] / legs["v_bits_then_bytes"]["median_ms"],
           "accepted": bool(a["median_ms"] - c["median_ms"] > spread)}
    print(json.dumps(out), flush=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
