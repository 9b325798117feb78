#!/usr/bin/env python3
"""Times the same-message calls on groups larger than a wave, this library against a reference checkout (the parent
commit, built), and prints one JSON line.

Shapes (groups x sets; set k of group g signs message g; device-made keys and signatures, bytes-mode keys, compressed
signatures):
    split by awr_parts.hpp      128x128    16x1024    1x16384    4096x1+1x4096 (skewed)
    controls, not split         128x64     16384x1
Calls: blsgpu_aggregate_with_randomness (96- / 192-byte outputs) and blsgpu_verify_same_message (flags 0).  Only entry
points the reference has are used, so one script times both.

Each library is timed in child processes of its own that run this file from that library's checkout, alternating
reference, new, reference, new .. for `--rounds` rounds in one session.  A child first answers every shape with a
fixed seed and reports a digest of every output, which must agree between the libraries; then, per shape and call, 5
warm-up calls and `--calls` timed ones (seed 0: fresh scalars), a host clock around the synchronous call.  Per leg the
median over its rounds' samples with min - max.

Acceptance: on each split shape the new median is below the reference's by more than the larger of the two legs' min -
max spreads; on each control it is not above the reference's by more than that spread.

    python tools/bench_wide_groups.py --ref-root DIR [--calls 30] [--warmup 5] [--rounds 1] [--out FILE]
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
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SEED = 0x57494445
SHAPES = [  # name, group sizes, split
    ("128x128", [128] * 128, True),
    ("16x1024", [1024] * 16, True),
    ("1x16384", [16384], True),
    ("4096x1+1x4096", [1] * 4096 + [4096], True),
    ("128x64", [64] * 128, False),
    ("16384x1", [1] * 16384, False),
]
CALLS = ["aggregate_with_randomness", "verify_same_message"]


# ------------------------------------------------------------------------------------------------------- child
def workload(ctx, sizes):
    """(pubkeys, one message per group, signatures) made on the device (debug ops 8 and 7, pinned to the oracle by
    tests/test_gpu_parity.py); every set of group g signs message g."""
    n = sum(sizes)
    sks = [(int.from_bytes(hashlib.sha256(i.to_bytes(32, "little")).digest(), "little") % R_ORDER).to_bytes(32, "big")
           for i in range(n)]
    gmsgs = [hashlib.sha256(b"bench_wide_groups" + g.to_bytes(4, "little")).digest() for g in range(len(sizes))]
    per_set = [gmsgs[g] for g, size in enumerate(sizes) for _ in range(size)]
    pks, st = ctx.debug_op(8, b"".join(sks), 32, 96)
    assert (st == 0).all()
    sigs, st = ctx.debug_op(7, b"".join(sk + m for sk, m in zip(sks, per_set)), 64, 96)
    assert (st == 0).all()
    return pks, b"".join(gmsgs), sigs


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def child(root, calls, warmup, only):
    sys.path.insert(0, root)
    from lodestar_amd import native

    assert os.path.dirname(os.path.abspath(native.__file__)) == os.path.join(os.path.abspath(root), "lodestar_amd")
    ctx = native.Context([0])  # fails loudly without a GPU: there is nothing to time elsewhere
    out = {}
    try:
        for name, sizes, _ in SHAPES:
            if only and name not in only:
                continue
            n = sum(sizes)
            pks, gmsgs, sigs = workload(ctx, sizes)
            first = np.cumsum([0] + sizes).astype(np.uint32)
            args = dict(pk_bytes=np.frombuffer(pks, np.uint8), sig_len=np.full(n, 96, np.uint32), sig_stride=96)
            buf = np.frombuffer(sigs, np.uint8)

            def awr(seed=0):
                return ctx.aggregate_with_randomness(first, buf, seed=seed, **args)

            def verify(seed=0):
                return ctx.verify_same_message(first, gmsgs, buf, seed=seed, flags=0, **args)

            p, s, st, fb = awr(SEED)
            res, gres, stats = verify(SEED)
            assert not st.any() and (res == 1).all() and (gres == 1).all()
            digest = hashlib.sha256(b"".join(p) + b"".join(s) + st.tobytes() + fb.tobytes() + res.tobytes() +
                                    gres.tobytes()).hexdigest()
            out[name] = {"digest": digest, "lanes": native.awr_lanes(len(sizes), n),
                         "aggregate_with_randomness": timed(awr, calls, warmup),
                         "verify_same_message": timed(verify, calls, warmup)}
    finally:
        ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


# ------------------------------------------------------------------------------------------------------ parent
def run_child(root, a):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", root, "--calls", str(a.calls), "--warmup",
           str(a.warmup)] + (["--only", a.only] if a.only else [])
    env = dict(os.environ)
    env.pop("BLSGPU_LIB", None)  # each checkout loads its own library
    p = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True, timeout=a.child_timeout)
    if p.returncode != 0:
        raise SystemExit(f"the child for {root} ended with {p.returncode}; nothing more is started")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def leg(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples),
            "calls": len(samples)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-root", help="a checkout of the reference commit with its library built")
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--only", default=None, help="comma-separated shape names")
    ap.add_argument("--child-timeout", type=int, default=900)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.calls, a.warmup, a.only.split(",") if a.only else None)
    if not a.ref_root:
        ap.error("--ref-root is required")
    runs = {"ref": [], "new": []}
    for _ in range(a.rounds):
        runs["ref"].append(run_child(os.path.abspath(a.ref_root), a))
        runs["new"].append(run_child(ROOT, a))
    shapes, ok = {}, True
    for name, sizes, split in SHAPES:
        if name not in runs["new"][0]:
            continue
        digests = {r[name]["digest"] for side in runs.values() for r in side}
        assert len(digests) == 1, f"{name}: the libraries' answers differ"
        e = {"groups": len(sizes), "sets": sum(sizes), "split": split, "lanes": runs["new"][0][name]["lanes"],
             "answers_equal": True}
        for call in CALLS:
            ref = leg([x for r in runs["ref"] for x in r[name][call]])
            new = leg([x for r in runs["new"] for x in r[name][call]])
            spread = max(ref["max_ms"] - ref["min_ms"], new["max_ms"] - new["min_ms"])
            meets = new["median_ms"] < ref["median_ms"] - spread if split else \
                new["median_ms"] <= ref["median_ms"] + spread
            ok = ok and meets
            e[call] = {"ref": ref, "new": new, "spread_ms": spread, "ratio": new["median_ms"] / ref["median_ms"],
                       "meets": meets}
        shapes[name] = e
    line = json.dumps({"bench": "wide_groups", "rounds": a.rounds, "shapes": shapes, "acceptance_met": ok})
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    return 0 if ok else 3  # 3: measured, and a comparison is not met


if __name__ == "__main__":
    sys.exit(main())
