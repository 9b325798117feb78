"""ctypes driver of tests/native/run_plan_probe.cpp (the HIP-free plan of one pipeline run, csrc/run_plan.hpp), shared
by tests/test_run_plan.py (CPU) and tests/test_gpu_run_plan.py (the library runs the plan the probe computes)."""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "run_plan_probe.cpp")
LIB = os.path.join(HERE, "native", "librun_plan_probe.so")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
HDR = os.path.join(CSRC, "run_plan.hpp")
DEPS = [SRC, HDR] + [os.path.join(CSRC, h) for h in ("options.hpp", "helper_layout.hpp", "miller_plan.hpp")]

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
        L = ctypes.CDLL(LIB)
        for f in ("rp_options_new", "rp_plan", "rp_ftree", "rp_classify", "rp_fallback", "rp_pool"):
            getattr(L, f).restype = ctypes.c_void_p
        L.rp_next_fail_rate.restype = ctypes.c_double
        L.rp_option_key.restype = L.rp_extra_keys.restype = ctypes.c_char_p
        L.rp_option_default.restype = ctypes.c_int64
        _lib = L
    return _lib


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.uint32)


def _p32(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))


def _p8(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))


class Result:
    """What a probe call computed: r.vec(name) -> list of ints, r[name] -> number."""

    def __init__(self, handle, keep=()):
        self.h = ctypes.c_void_p(handle)
        self.keep = keep  # arrays the plan points into

    def vec(self, name):
        n = lib().rp_vec(self.h, name.encode(), None, 0)
        assert n != 0xFFFFFFFF, name
        out = np.zeros(max(n, 1), np.uint32)
        lib().rp_vec(self.h, name.encode(), _p32(out), n)
        return out[:n].astype(np.int64).tolist()

    def __getitem__(self, name):
        x = ctypes.c_double()
        assert lib().rp_num(self.h, name.encode(), ctypes.byref(x)) == 0, name
        assert x.value == int(x.value)
        return int(x.value)

    def __del__(self):
        if self.h:
            lib().rp_free(self.h)
            self.h = None


class Opts:
    def __init__(self, **kv):
        self.h = ctypes.c_void_p(lib().rp_options_new())
        for k, v in kv.items():
            assert lib().rp_option(self.h, k.encode(), ctypes.c_int64(int(v))) == 0, k

    def set_checked(self, key, value):
        """As blsgpu_set_option stores it; False = refused."""
        return lib().rp_option_checked(self.h, key.encode(), ctypes.c_int64(int(value))) == 0

    def __getitem__(self, key):
        v = ctypes.c_int64()
        assert lib().rp_option_get(self.h, key.encode(), ctypes.byref(v)) == 0, key
        return v.value

    def same_run(self, other):
        return bool(lib().rp_options_same_run(self.h, other.h))

    def __del__(self):
        lib().rp_options_free(self.h)


def option_rows():
    """The options table (csrc/options.hpp): [(key, is an ABI key, takes part in same_run, default)]."""
    rows, i = [], 0
    while lib().rp_option_key(i) is not None:
        rows.append((lib().rp_option_key(i).decode(), bool(lib().rp_option_abi(i)), bool(lib().rp_option_same_run(i)),
                     lib().rp_option_default(i)))
        i += 1
    return rows


def extra_keys():
    """(the keys that live on the context, the read-only keys): handled by name in runtime.cpp."""
    return tuple(set(lib().rp_extra_keys(ro).decode().split()) for ro in (0, 1))


def plan(counts, flags, msg_ids, *, opts=None, keys_per_set=None, pk_mode=1, sig_len=None, job_begin=0, job_end=None,
         urgent=False, alone=False, fail_rate=0.0, seed=7, pool=None):
    """The plan of a batch whose jobs have `counts` sets and `flags`, set i signing message msg_ids[i]."""
    jfs = _u32(np.concatenate([[0], np.cumsum(counts)]))
    n = int(jfs[-1])
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    msgs = np.zeros((n + 1, 32), np.uint8)
    msgs[:n, :8] = np.asarray(msg_ids, dtype="<u8").reshape(n, 1).view(np.uint8).reshape(n, 8) if n else 0
    sl = _u32(sig_len if sig_len is not None else [96] * n)
    sl = np.concatenate([sl, _u32([0])])
    spf = _u32(np.concatenate([[0], np.cumsum(keys_per_set if keys_per_set is not None else [1] * n)]))
    o = opts or Opts()
    pl = _u32(np.asarray(pool).reshape(-1)) if pool is not None else None
    if pl is not None and len(pl) == 0:
        pl = _u32([0])
    h = lib().rp_plan(_p32(jfs), _p8(fl), job_begin, len(counts) if job_end is None else job_end, _p8(msgs), _p32(sl),
                      _p32(spf), pk_mode, o.h, int(urgent), int(alone), ctypes.c_double(fail_rate),
                      ctypes.c_uint64(seed), _p32(pl) if pl is not None else None, len(pool) if pool is not None else 0)
    return Result(h, keep=(jfs, fl, msgs, sl, spf, o, pl))


def ftree(ranges_len, segs, f_run_max):
    gc, at = [], 0
    for ln in ranges_len:
        gc += [at, at + ln]
        at += ln
    g = _u32(gc if gc else [0])
    return Result(lib().rp_ftree(_p32(g), len(ranges_len), at, segs, ctypes.c_int64(f_run_max))), gc, at


def classify(p, job_err, group_ok, spec):
    je = np.ascontiguousarray(job_err, dtype=np.int8)
    ok = np.ascontiguousarray(list(group_ok) + [0], dtype=np.uint8)
    r = Result(lib().rp_classify(p.h, je.ctypes.data_as(ctypes.POINTER(ctypes.c_int8)), _p8(ok), int(spec)))
    return r, [x - 256 for x in r.vec("jr")]


def next_fail_rate(p, jr, rate):
    a = np.ascontiguousarray(jr, dtype=np.int32)
    return lib().rp_next_fail_rate(p.h, a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.c_double(rate))


def fallback(p, retry, opts, alone):
    r = _u32(retry if len(retry) else [0])
    return Result(lib().rp_fallback(p.h, _p32(r), len(retry), opts.h, int(alone)), keep=(opts,))


def pool_groups(counts, flags, job_begin=0, job_end=None):
    jfs = _u32(np.concatenate([[0], np.cumsum(counts)]))
    fl = np.ascontiguousarray(flags, dtype=np.uint8)
    return Result(lib().rp_pool(_p32(jfs), _p8(fl), job_begin, len(counts) if job_end is None else job_end))
