#!/usr/bin/env python3
"""Times the ways to fill the trusted pubkey table from a validator registry, on one device, and prints one JSON line
per key count.

The keys are made on the device (debug op 8, pinned to the oracle by tests/test_gpu_parity.py), uploaded once as 96
bytes and read back compressed (Context.read_pubkeys), so both encodings of the same keys exist on the host.  Legs,
each on a context of its own that already holds the range (every timed call overwrites [0, keys): no table growth in
any of them):
    a_compressed_trusted    blsgpu_pubkeys_upload_compressed, flags 0
    b_compressed_validate   blsgpu_pubkeys_upload_compressed, BLSGPU_PK_VALIDATE
    c_key_validate_then_96  today's route without blst on the host: blsgpu_key_validate (48 -> 96 bytes, back to the
                            host), then blsgpu_pubkeys_upload of those bytes -- both unchanged code
    d_upload_96             blsgpu_pubkeys_upload alone: the host already holds decompressed keys
Before anything is timed every leg runs once and the four tables are read back (Context.read_pubkeys) and compared byte
for byte.  The legs are then warmed up `--warmup` times and timed `--calls` times alternately (one call of each per
round) with a host clock around the library calls, which all end in a stream synchronise; median, minimum and maximum
are reported.  As context, the C oracle's cpu.pk_decode (decompression, no subgroup check) is timed on one host thread
over a sample of the keys.

    python tools/bench_pubkeys_upload.py [--keys 1048576 ...] [--calls 10] [--warmup 3] [--out FILE]
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

R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
CHUNK = 1 << 18  # keys made per debug-op call


def make_keys(ctx, n):
    """(pk96, pk48) numpy arrays of n valid keys."""
    pk96 = []
    for a in range(0, n, CHUNK):
        sks = b"".join((int.from_bytes(hashlib.sha256(i.to_bytes(8, "little")).digest(), "little") % R_ORDER or 1)
                       .to_bytes(32, "big") for i in range(a, min(n, a + CHUNK)))
        out, st = ctx.debug_op(8, sks, 32, 96)
        assert (st == 0).all()
        pk96.append(out)
    pk96 = b"".join(pk96)
    ctx.upload_pubkeys(0, pk96)
    pk48 = ctx.read_pubkeys(0, n, 48)
    assert ctx.read_pubkeys(0, n, 96) == pk96
    return np.frombuffer(pk96, np.uint8), np.frombuffer(pk48, np.uint8)


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


def bench(n, calls, warmup):
    from lodestar_amd import native
    from lodestar_amd.native import Context

    lib = native.load()
    names = ["a_compressed_trusted", "b_compressed_validate", "c_key_validate_then_96", "d_upload_96"]
    ctxs = {name: Context([0]) for name in names}
    try:
        pk96, pk48 = make_keys(ctxs["d_upload_96"], n)
        st = np.zeros(n, np.int8)
        fb = np.zeros(1, np.uint32)
        mid = np.zeros(96 * n, np.uint8)  # leg c's keys on their way back up

        def compressed(name, flags):
            def run():
                rc = lib.blsgpu_pubkeys_upload_compressed(ctxs[name].h, 0, pk48.ctypes.data, n, flags, st.ctypes.data,
                                                          fb.ctypes.data)
                assert rc == 0 and fb[0] == 0xFFFFFFFF
            return run

        def two_calls():
            h = ctxs["c_key_validate_then_96"].h
            assert lib.blsgpu_key_validate(h, n, pk48.ctypes.data, 48, 48, mid.ctypes.data, st.ctypes.data) == 0
            assert not st.any()
            assert lib.blsgpu_pubkeys_upload(h, 0, ctypes.c_char_p(mid.ctypes.data), n) == 0

        def upload_96():
            assert lib.blsgpu_pubkeys_upload(ctxs["d_upload_96"].h, 0, ctypes.c_char_p(pk96.ctypes.data), n) == 0

        fns = {"a_compressed_trusted": compressed("a_compressed_trusted", 0),
               "b_compressed_validate": compressed("b_compressed_validate", native.PK_VALIDATE),
               "c_key_validate_then_96": two_calls, "d_upload_96": upload_96}
        for fn in fns.values():
            fn()
        want = pk96.tobytes()
        for name in names:
            assert ctxs[name].pubkeys_count == n
            assert ctxs[name].read_pubkeys(0, n, 96) == want, f"{name}: table contents differ"
        legs = timed(fns, calls, warmup)
    finally:
        for c in ctxs.values():
            c.close()
    for v in legs.values():
        v["keys_per_s"] = n / (v["median_ms"] * 1e-3)
    out = {"keys": n, "legs": legs, "contents_equal": True}
    try:
        from oracle import cpu

        sample = min(n, 2000)
        keys = [pk48[48 * i: 48 * i + 48].tobytes() for i in range(sample)]
        cpu.pk_decode(keys[0])
        t0 = time.perf_counter()
        for k in keys:
            cpu.pk_decode(k)
        dt = time.perf_counter() - t0
        out["cpu_pk_decode"] = {"sample": sample, "keys_per_s_per_thread": sample / dt,
                                "ms_for_all_keys_one_thread": n * dt / sample * 1e3}
    except Exception as e:  # the C oracle is test infrastructure: absent from an installed package
        out["cpu_pk_decode"] = {"error": str(e)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=int, nargs="+", default=[1 << 20])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pubkeys_compressed_bench.json"))
    args = ap.parse_args()
    results = []
    for n in args.keys:
        r = bench(n, args.calls, args.warmup)
        print(json.dumps(r), flush=True)
        results.append(r)
        with open(args.out, "w") as f:  # after every key count: a later one that fails keeps the earlier results
            json.dump({"tool": "tools/bench_pubkeys_upload.py", "calls": args.calls, "warmup": args.warmup,
                       "results": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
