"""ctypes driver of tests/native/call_plan_probe.cpp (the HIP-free call side of the runtime, csrc/call_plan.hpp), used
by tests/test_call_plan.py."""
import ctypes
import os
import subprocess

import numpy as np

from lodestar_amd.native import Batch

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "call_plan_probe.cpp")
LIB = os.path.join(HERE, "native", "libcall_plan_probe.so")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")
DEPS = [SRC] + [os.path.join(CSRC, h) for h in ("call_plan.hpp", "run_plan.hpp", "options.hpp", "batch_rand.hpp",
                                                "helper_layout.hpp", "miller_plan.hpp")]
NULL = 0xFFFFFFFE  # cp_bytes: the merged batch's pointer is null

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in DEPS):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC, "-lpthread"])
        L = ctypes.CDLL(LIB)
        L.cp_new.restype = ctypes.c_void_p
        L.cp_num.restype = L.cp_shard_cost.restype = ctypes.c_int64
        L.cp_bytes.restype = L.cp_max_table_index.restype = ctypes.c_uint32
        _lib = L
    return _lib


class Call:
    """A call's arrays as a blsgpu_batch.  mode: 0 table indices, 1 one key per set, 2 key bytes per set range."""

    def __init__(self, counts, flags, mode, sig_len, stride, seed, keys_per_set=None, rng=None):
        rng = rng or np.random.default_rng(seed)
        self.mode = mode
        self.jfs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
        n = self.n = int(self.jfs[-1])
        self.flags = np.asarray(flags, np.uint8)
        self.sig_len = np.asarray(sig_len, np.uint32)
        assert len(self.sig_len) == n and len(self.flags) == len(counts)
        self.stride = stride
        self.sigs = rng.integers(1, 256, (n, stride), dtype=np.uint8)  # never 0: a row left zero shows
        self.msgs = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        kps = [1] * n if mode == 1 else list(keys_per_set)
        self.spf = np.concatenate([[0], np.cumsum(kps)]).astype(np.uint32)
        npk = int(self.spf[-1])
        self.pki = rng.integers(0, 1 << 20, npk, dtype=np.uint32)
        self.pkb = rng.integers(0, 256, (npk, 96), dtype=np.uint8)
        self.seed = seed
        self.result = np.full(len(counts), 77, np.int8)  # sentinel
        b = self.b = Batch()
        b.n_sets, b.n_jobs, b.sig_stride, b.seed = n, len(counts), stride, seed
        b.job_first_set, b.job_flags = self.jfs.ctypes.data, self.flags.ctypes.data
        b.msgs, b.sigs, b.sig_len = self.msgs.ctypes.data, self.sigs.ctypes.data, self.sig_len.ctypes.data
        b.pk_bytes = self.pkb.ctypes.data if mode else None
        b.set_pk_first = None if mode == 1 else self.spf.ctypes.data
        b.pk_index = self.pki.ctypes.data if mode == 0 else None

    def ref(self):
        return ctypes.byref(self.b)


class Merged:
    """Shards (call, job_begin, job_end) packed into the batch of one merged run."""

    def __init__(self, parts, thread_min_sets=4096):
        self.parts = parts
        self.h = ctypes.c_void_p(lib().cp_new())
        for c, jb, je in parts:
            lib().cp_add(self.h, c.ref(), jb, je, c.result.ctypes.data_as(ctypes.c_void_p))
        lib().cp_pack(self.h, ctypes.c_uint32(thread_min_sets))

    def bytes(self, name):
        """The named array as bytes, or None where the merged batch has a null pointer."""
        n = lib().cp_bytes(self.h, name.encode(), None, 0)
        assert n != 0xFFFFFFFF, name
        if n == NULL:
            return None
        out = np.zeros(max(n, 1), np.uint8)
        lib().cp_bytes(self.h, name.encode(), out.ctypes.data_as(ctypes.c_void_p), n)
        return out[:n]

    def u32(self, name):
        a = self.bytes(name)
        return None if a is None else a.view(np.uint32).astype(np.int64)

    def __getitem__(self, name):
        v = lib().cp_num(self.h, name.encode())
        assert v >= 0, name
        return v

    def scatter(self, res):
        res = np.ascontiguousarray(res, np.int8)
        assert len(res) == self["nj"]
        lib().cp_scatter(self.h, res.ctypes.data_as(ctypes.c_void_p))

    def __del__(self):
        lib().cp_free(self.h)


def shard_scalars(call, job_begin, job_end):
    out = np.zeros(max(int(call.jfs[job_end] - call.jfs[job_begin]), 1), np.uint64)
    lib().cp_shard_scalars(call.ref(), job_begin, job_end, out.ctypes.data_as(ctypes.c_void_p))
    return out[:int(call.jfs[job_end] - call.jfs[job_begin])]
