#!/usr/bin/env python3
"""Times blsgpu_verify_same_message (the whole same-message method in one device call) against the two-step method on
the same library and the same sets, on one device, and prints one JSON line.

16,384 device-made (key, message, signature) triples, bytes-mode keys, compressed signatures, seed 0:
    128x128          128 groups of 128 sets, all valid
    16384x1          16,384 groups of one set, all valid
    128x128 bad 1%   one set of 1% of the groups (1 group) carries a signature over another message
    128x128 bad 100% one such set in every group
Per shape:
    fused      Context.verify_same_message
    fused_blocks  the same call with native.SAME_BLOCK_CHECK: one pairing check per block of 1024 groups, the per-group
               descent of a block that fails, then the per-set retry
    two_step   the existing method, unchanged code: Context.aggregate_with_randomness, then Context.verify_raw of the
               (P, message, S) of every accepted group as one-set batchable jobs, then Context.verify_raw of every set
               of the groups that were rejected or did not verify, as one-set batchable jobs
    serial     the fused call with its three branches on one stream (BLSGPU_SAME_SERIAL=1, read once per process: a
               child process times it)
All answers are compared set by set before anything is timed.  fused, fused_blocks and two_step run in the same process,
are warmed up `--warmup` times and timed `--calls` times (>= 20), alternately (one call of each per round), with a host
clock
around the calls, which end in a stream synchronise; medians, minima and maxima are reported.

    python tools/bench_same_message.py [--calls 30] [--warmup 5] [--out FILE] [--no-serial]

--aggregate times blsgpu_verify_same_message_agg instead, on 128x128, 16384x1 and 128x128 bad 1%, each
with and without SAME_BLOCK_CHECK, three legs timed alternately in this process:
    two_call   verify_same_message, then aggregate_signatures (validate off) of the sets that verified, grouped as
               they were: the way to the groups' aggregates without the new call, both functions unchanged code
    one_call   verify_same_message_agg
    verify     verify_same_message alone: one_call minus this is the cost of the aggregate phase
The aggregates and counts of the two ways are compared byte for byte before anything is timed.
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_SETS = 16384
SAME_BLOCK_CHECK = 4  # native.SAME_BLOCK_CHECK
# name, groups, sets per group, groups with one bad set
SHAPES = [("128x128", 128, 128, 0), ("16384x1", 16384, 1, 0), ("128x128_bad_1pct", 128, 128, 1),
          ("128x128_bad_100pct", 128, 128, 128)]
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def workload(ctx, size, bad_groups):
    """16,384 (pubkey, signature) pairs made on the device (debug ops 8 and 7, pinned to the oracle by
    tests/test_gpu_parity.py); set k signs message k // size, except the first set of the first `bad_groups` groups,
    which signs another message."""
    sks = [(int.from_bytes(hashlib.sha256(i.to_bytes(32, "little")).digest(), "little") % R_ORDER).to_bytes(32, "big")
           for i in range(N_SETS)]
    gmsgs = [hashlib.sha256(b"bench_same_message" + g.to_bytes(4, "little")).digest() for g in range(N_SETS // size)]
    signed = [gmsgs[j // size] for j in range(N_SETS)]
    for g in range(bad_groups):
        signed[g * size] = hashlib.sha256(b"another message" + g.to_bytes(4, "little")).digest()
    pks, st = ctx.debug_op(8, b"".join(sks), 32, 96)
    assert (st == 0).all()
    sigs, st = ctx.debug_op(7, b"".join(sk + m for sk, m in zip(sks, signed)), 64, 96)
    assert (st == 0).all()
    return pks, b"".join(gmsgs), sigs


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


def time_shape(ctx, n_groups, size, bad_groups, calls, warmup, fused_only):
    pks, gmsgs, sigs = workload(ctx, size, bad_groups)
    first = np.arange(n_groups + 1, dtype=np.uint32) * size
    buf = np.frombuffer(sigs, np.uint8)
    pkb = np.frombuffer(pks, np.uint8)
    sl = np.full(N_SETS, 96, np.uint32)
    last = {}

    def fused():
        last["fused"] = ctx.verify_same_message(first, gmsgs, buf, pk_bytes=pkb, sig_len=sl, sig_stride=96, seed=0)

    def fused_blocks():
        last["blocks"] = ctx.verify_same_message(first, gmsgs, buf, pk_bytes=pkb, sig_len=sl, sig_stride=96, seed=0,
                                                 flags=SAME_BLOCK_CHECK)

    def two_step():
        p, s, st, _ = ctx.aggregate_with_randomness(first, buf, pk_bytes=pkb, sig_len=sl, sig_stride=96, seed=0)
        good = [g for g in range(n_groups) if st[g] == 0]
        ok = np.zeros(n_groups, bool)
        if good:
            res, _ = ctx.verify_raw(np.arange(len(good) + 1), b"".join(s[g] for g in good), [192] * len(good),
                                    b"".join(gmsgs[32 * g: 32 * g + 32] for g in good),
                                    pk_bytes=b"".join(p[g] for g in good), job_flags=np.ones(len(good)), sig_stride=192)
            ok[good] = res == 1
        out = np.repeat(ok, size).astype(np.int8)
        retry = [g for g in range(n_groups) if not ok[g]]
        if retry:
            idx = np.concatenate([np.arange(first[g], first[g + 1]) for g in retry])
            res, _ = ctx.verify_raw(np.arange(len(idx) + 1), buf.reshape(-1, 96)[idx].tobytes(), [96] * len(idx),
                                    b"".join(gmsgs[32 * g: 32 * g + 32] * size for g in retry),
                                    pk_bytes=pkb.reshape(-1, 96)[idx].tobytes(), job_flags=np.ones(len(idx)),
                                    sig_stride=96)
            out[idx] = res
        last["two"] = out

    fused()
    res, gres, st = last["fused"]
    want = np.ones(N_SETS, np.int8)
    want[[g * size for g in range(bad_groups)]] = 0
    assert (res == want).all() and st.groups_retried == bad_groups and st.retry_sets == bad_groups * size
    out = {"groups": n_groups, "group_size": size, "bad_groups": bad_groups, "form": st.form,
           "unique_messages": st.unique_messages}
    legs = {"fused": fused}
    if not fused_only:
        fused_blocks()
        bres, bgres, bst = last["blocks"]
        assert (bres == res).all() and (bgres == gres).all() and bst.retry_sets == st.retry_sets
        out["form_blocks"] = bst.form
        legs["fused_blocks"] = fused_blocks
        two_step()
        assert (last["two"] == want).all()
        legs["two_step"] = two_step
    out.update(timed(legs, calls, warmup))
    out["fused"]["device_ms_last"] = last["fused"][2].device_ms
    if not fused_only:
        out["fused_blocks"]["device_ms_last"] = last["blocks"][2].device_ms
        out["fused_over_two_step"] = out["fused"]["median_ms"] / out["two_step"]["median_ms"]
        out["fused_blocks_over_two_step"] = out["fused_blocks"]["median_ms"] / out["two_step"]["median_ms"]
        out["fused_blocks_over_fused"] = out["fused_blocks"]["median_ms"] / out["fused"]["median_ms"]
    return out


AGG_SHAPES = [SHAPES[0], SHAPES[1], SHAPES[2]]


def time_aggregate_shape(ctx, n_groups, size, bad_groups, flags, calls, warmup):
    pks, gmsgs, sigs = workload(ctx, size, bad_groups)
    first = np.arange(n_groups + 1, dtype=np.uint32) * size
    buf = np.frombuffer(sigs, np.uint8)
    pkb = np.frombuffer(pks, np.uint8)
    sl = np.full(N_SETS, 96, np.uint32)
    last = {}

    def verify():
        last["verify"] = ctx.verify_same_message(first, gmsgs, buf, pk_bytes=pkb, sig_len=sl, sig_stride=96, seed=0,
                                                 flags=flags)

    def two_call():
        res, _, _ = ctx.verify_same_message(first, gmsgs, buf, pk_bytes=pkb, sig_len=sl, sig_stride=96, seed=0,
                                            flags=flags)
        ok = res == 1
        if ok.all():
            out, st, _ = ctx.aggregate_signatures(buf, first, sig_len=sl, sig_stride=96, validate=False)
            cnt = np.diff(first)
        else:
            cnt = np.add.reduceat(ok.astype(np.int64), first[:-1].astype(np.int64))
            kept = np.concatenate([[0], np.cumsum(cnt)])
            out, st, _ = ctx.aggregate_signatures(buf.reshape(-1, 96)[ok].reshape(-1), kept, sig_len=sl[ok],
                                                  sig_stride=96, validate=False)
        last["two"] = (res, out, cnt)

    def one_call():
        last["one"] = ctx.verify_same_message_agg(first, gmsgs, buf, pk_bytes=pkb, sig_len=sl, sig_stride=96, seed=0,
                                                  flags=flags)

    two_call()
    one_call()
    res, gres, st, out, cnt = last["one"]
    want = np.ones(N_SETS, np.int8)
    want[[g * size for g in range(bad_groups)]] = 0
    assert (res == want).all() and (last["two"][0] == want).all()
    assert out == last["two"][1] and (cnt == last["two"][2]).all() and int(cnt.sum()) == N_SETS - bad_groups
    r = {"groups": n_groups, "group_size": size, "bad_groups": bad_groups, "flags": flags, "form": st.form,
         "agg_lanes": native_agg_lanes(n_groups)}
    r.update(timed({"two_call": two_call, "one_call": one_call, "verify": verify}, calls, warmup))
    r["one_call"]["device_ms_last"] = last["one"][2].device_ms
    r["one_call_over_two_call"] = r["one_call"]["median_ms"] / r["two_call"]["median_ms"]
    r["phase_ms"] = r["one_call"]["median_ms"] - r["verify"]["median_ms"]
    return r


def native_agg_lanes(n_groups):
    from lodestar_amd import native

    return native.same_message_agg_lanes(n_groups, N_SETS)


def main_aggregate(a):
    from lodestar_amd import native

    ctx = native.Context([0])
    try:
        shapes = {}
        for name, g, size, bad in AGG_SHAPES:
            for flags in (0, SAME_BLOCK_CHECK):
                shapes[name + ("_blocks" if flags else "")] = time_aggregate_shape(ctx, g, size, bad, flags, a.calls,
                                                                                   a.warmup)
    finally:
        ctx.close()
    line = json.dumps({"bench": "verify_same_message_agg", "sets": N_SETS, "shapes": shapes})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--fused-only", action="store_true", help="time the fused call alone (the serial child)")
    ap.add_argument("--no-serial", action="store_true", help="leave the serial child out")
    ap.add_argument("--aggregate", action="store_true", help="time verify_same_message_agg against the two-call method")
    a = ap.parse_args()
    if a.calls < 20:
        ap.error("--calls must be at least 20")
    if a.aggregate:
        return main_aggregate(a)
    from lodestar_amd import native

    ctx = native.Context([0])  # fails loudly without a GPU: there is nothing to time elsewhere
    try:
        shapes = {name: time_shape(ctx, g, size, bad, a.calls, a.warmup, a.fused_only)
                  for name, g, size, bad in SHAPES}
    finally:
        ctx.close()
    if not a.fused_only and not a.no_serial:
        # the same fused calls with the three branches of the group phase on one stream, in a process of their own
        env = dict(os.environ, BLSGPU_SAME_SERIAL="1")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused-only", "--calls", str(a.calls),
                                "--warmup", str(a.warmup)], env=env, capture_output=True, text=True, timeout=900)
        if child.returncode != 0:
            raise RuntimeError("serial child failed:\n" + child.stdout + child.stderr)
        serial = json.loads(child.stdout.strip().splitlines()[-1])["shapes"]
        for name in shapes:
            shapes[name]["serial"] = serial[name]["fused"]
            shapes[name]["fused_over_serial"] = shapes[name]["fused"]["median_ms"] / serial[name]["fused"]["median_ms"]
    line = json.dumps({"bench": "verify_same_message", "sets": N_SETS, "serial": bool(os.environ.get(
        "BLSGPU_SAME_SERIAL") == "1"), "shapes": shapes})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
