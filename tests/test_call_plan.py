"""The call side's host arithmetic (lodestar_amd/csrc/call_plan.hpp), CPU only, through
tests/native/call_plan_probe.cpp: the packing of several calls' shards into the batch of one merged run equals the
same jobs submitted as one call, each part's batch scalars are its own call's, results scatter back into the calls'
own job ranges, and validate_batch, max_table_index and table_covers refuse what they refused in runtime.cpp."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from lodestar_amd import native
from lodestar_amd.native import Batch
from tests import call_plan_probe as cp
from tests.test_batch_scalars import expected_words

ARRAYS = ["job_first_set", "job_flags", "sig_len", "sigs", "msgs", "set_pk_first", "pk_index", "pk_bytes", "scal",
          "set_off", "job_off", "key_off"]


def test_header_is_hip_free():
    src = open(os.path.join(cp.CSRC, "call_plan.hpp")).read()
    includes = [ln.split()[1] for ln in src.splitlines() if ln.startswith("#include")]
    assert sorted(includes) == sorted(["<pthread.h>", "<system_error>", "<thread>", '"batch_rand.hpp"', '"run_plan.hpp"'])
    # (tests/test_run_plan.py checks run_plan.hpp and what it includes)
    rand = open(os.path.join(cp.CSRC, "batch_rand.hpp")).read().splitlines()
    assert all("hip" not in ln and '"' not in ln for ln in rand if ln.startswith("#include"))


def _keys(n, mode, phase=0):
    """Aggregate sets of 1, 3 and 0 keys (modes 0 and 2; mode 1 is one key per set by definition)."""
    return [1] * n if mode == 1 else [(1, 3, 0)[(i + phase) % 3] for i in range(n)]


def _call(counts, flags, mode, sig_len, stride, seed, phase=0):
    return cp.Call(counts, flags, mode, sig_len, stride, seed, keys_per_set=_keys(sum(counts), mode, phase))


def _parts(mode):
    """Three parts of 5, 1 and 7 sets (the 7-set one with jobs of no sets at its start, in its middle and at its
    end; strides 96, 192 and 200, the last with a set of sig_len 0 and one of 100), then the middle shard (jobs 1
    and 2) of a four-job call, so that every re-basing has a nonzero origin."""
    a = _call([2, 3], [1, 1], mode, [96] * 5, 96, seed=11)
    b = _call([1], [0], mode, [192], 192, seed=12, phase=1)  # a lone non-batchable set: r = 1
    c = _call([0, 3, 0, 4, 0], [1, 1, 0, 1, 1], mode, [96, 0, 192, 96, 100, 192, 96], 200, seed=13, phase=2)
    d = _call([2, 1, 3, 2], [1, 0, 1, 1], mode, [96, 192, 96, 192, 96, 96, 192, 96], 192, seed=14)
    return [(a, 0, 2), (b, 0, 1), (c, 0, 5), (d, 1, 3)]


def _shard(part):
    c, jb, je = part
    return c, int(c.jfs[jb]), int(c.jfs[je])


def _single_call(parts):
    """The parts' jobs as ONE call, built by concatenation: its prefix arrays start at 0 and run through."""
    counts, flags, sig_len, msgs, kps, pki, pkb = [], [], [], [], [], [], []
    for part in parts:
        c, a, e = _shard(part)
        jb, je = part[1], part[2]
        counts += np.diff(c.jfs[jb:je + 1].astype(np.int64)).tolist()
        flags += c.flags[jb:je].tolist()
        sig_len += c.sig_len[a:e].tolist()
        msgs.append(c.msgs[a:e])
        kps += np.diff(c.spf[a:e + 1].astype(np.int64)).tolist()
        pki.append(c.pki[c.spf[a]:c.spf[e]])
        pkb.append(c.pkb[c.spf[a]:c.spf[e]])
    return dict(jfs=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), flags=np.array(flags, np.uint8),
                sig_len=np.array(sig_len, np.int64), msgs=np.concatenate(msgs),
                spf=np.concatenate([[0], np.cumsum(kps)]).astype(np.int64), pki=np.concatenate(pki).astype(np.int64),
                pkb=np.concatenate(pkb))


def _sig_rows(parts, sig_w):
    """The single call's signature rows at width sig_w: a 96- or 192-byte signature at the start of its row; a
    part already at that stride keeps its rows as they are, every other row is zero past the signature (and zero
    altogether for a signature of another length)."""
    rows = []
    for part in parts:
        c, a, e = _shard(part)
        if c.stride == sig_w:
            rows.append(c.sigs[a:e])
            continue
        r = np.zeros((e - a, sig_w), np.uint8)
        for i in range(a, e):
            ln = int(c.sig_len[i])
            if ln in (96, 192):
                r[i - a, :ln] = c.sigs[i, :ln]
        rows.append(r)
    return np.concatenate(rows)


def _check_equals_single_call(parts, mode, want_sig_w):
    m = cp.Merged(parts)
    one = _single_call(parts)
    n, nj = len(one["sig_len"]), len(one["flags"])
    assert (m["n_sets"], m["n_jobs"], m["mode"], m["sig_stride"]) == (n, nj, mode, want_sig_w)
    assert (m["n"], m["nj"]) == (n, nj)
    assert m.u32("job_first_set").tolist() == one["jfs"].tolist()
    assert m.bytes("job_flags").tolist() == one["flags"].tolist()
    assert m.u32("sig_len").tolist() == one["sig_len"].tolist()
    assert np.array_equal(m.bytes("msgs").reshape(n, 32), one["msgs"])
    got_sigs = m.bytes("sigs").reshape(n, want_sig_w)
    assert np.array_equal(got_sigs, _sig_rows(parts, want_sig_w))
    if mode == 1:
        assert m.bytes("set_pk_first") is None and m.bytes("pk_index") is None
        assert np.array_equal(m.bytes("pk_bytes").reshape(n, 96), one["pkb"])
    else:
        assert m.u32("set_pk_first").tolist() == one["spf"].tolist()
        assert m["npk"] == one["spf"][-1]
        if mode == 0:
            assert m.bytes("pk_bytes") is None
            assert m.u32("pk_index").tolist() == one["pki"].tolist()
        else:
            assert m.bytes("pk_index") is None
            assert np.array_equal(m.bytes("pk_bytes").reshape(-1, 96), one["pkb"])
    # the parts' offsets
    so = np.cumsum([0] + [e - a for _, a, e in map(_shard, parts)])
    jo = np.cumsum([0] + [je - jb for _, jb, je in parts])
    ko = np.cumsum([0] + [int(c.spf[e] - c.spf[a]) if mode != 1 else 0 for c, a, e in map(_shard, parts)])
    assert m.u32("set_off").tolist() == so[:-1].tolist() and m.u32("job_off").tolist() == jo[:-1].tolist()
    assert m.u32("key_off").tolist() == ko[:-1].tolist()
    return m


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_packing_equals_concatenation(mode):
    parts = _parts(mode)
    assert [e - a for _, a, e in map(_shard, parts)] == [5, 1, 7, 4]
    _check_equals_single_call(parts, mode, 192)
    _check_equals_single_call(parts[:1], mode, 96)  # (one part alone packs too)
    _check_equals_single_call(parts[3:], mode, 192)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_signature_strides(mode):
    """sig_w is 192 as soon as any live set of any part is 192 bytes long, else 96; rows are narrowed or widened to
    it, and a signature that is neither 96 nor 192 bytes long leaves its row zero."""
    s96 = _call([2, 3], [1, 1], mode, [96] * 5, 96, seed=21)
    s192 = _call([1, 2, 2], [1, 1, 1], mode, [96, 192, 96, 96, 192], 192, seed=22)
    s192c = _call([3], [1], mode, [96] * 3, 192, seed=23)  # a wide stride, every signature compressed
    s200 = _call([4, 3], [1, 1], mode, [96, 0, 96, 100, 96, 96, 96], 200, seed=24)
    s200u = _call([2], [1], mode, [192, 96], 200, seed=25)
    m = _check_equals_single_call([(s96, 0, 2), (s200, 0, 2), (s192c, 0, 1)], mode, 96)
    sig = m.bytes("sigs").reshape(-1, 96)
    assert not sig[5 + 1].any() and not sig[5 + 3].any() and sig[5].all() and sig[12].all()
    m = _check_equals_single_call([(s96, 0, 2), (s192, 0, 3), (s200, 0, 2)], mode, 192)
    sig = m.bytes("sigs").reshape(-1, 192)
    assert sig[0, :96].all() and not sig[0, 96:].any()  # widened
    assert not sig[10 + 1].any() and not sig[10 + 3].any()
    _check_equals_single_call([(s200, 0, 2), (s200u, 0, 1)], mode, 192)
    # only the shard's own sets count: jobs 0 and 2 of s192 hold its compressed signatures
    _check_equals_single_call([(s96, 0, 2), (s192, 0, 1)], mode, 96)
    _check_equals_single_call([(s96, 0, 2), (s192, 1, 2)], mode, 192)


def test_threaded_packing_is_the_serial_packing():
    """A part of 4,096 sets packs on its own thread (not the first part, which packs on the calling thread): byte
    for byte what the same parts give packed one after the other."""
    rng = np.random.default_rng(5)
    for mode in (0, 1, 2):
        n = 4096
        counts = rng.integers(0, 4, 2000).tolist()  # ~3,000 sets in jobs of 0 to 3, the rest in the last job
        counts.append(n - sum(counts))
        assert counts[-1] > 0
        sig_len = rng.choice([96, 192], n).tolist()
        big = _call(counts, rng.integers(0, 2, len(counts)).tolist(), mode, sig_len, 192, seed=31)
        big2 = _call([n], [1], mode, [96] * n, 96, seed=32)
        small = _call([2, 3], [1, 0], mode, [96] * 5, 96, seed=33)
        parts = [(small, 0, 2), (big, 0, len(counts)), (big2, 0, 1), (small, 1, 2)]
        threaded, serial = cp.Merged(parts, 4096), cp.Merged(parts, 0xFFFFFFFF)
        for name in ARRAYS:
            a, b = threaded.bytes(name), serial.bytes(name)
            assert (a is None) == (b is None), name
            assert a is None or np.array_equal(a, b), name
        assert threaded["n"] == 2 * n + 8 and threaded["sig_stride"] == 192
        one = _single_call(parts)
        assert threaded.u32("job_first_set").tolist() == one["jfs"].tolist()
        assert np.array_equal(threaded.bytes("sigs").reshape(-1, 192), _sig_rows(parts, 192))


@pytest.mark.parametrize("mode", [0, 2])
def test_scalars_are_each_calls_own(mode):
    """A part's words are shard_scalars of its own call: the call's keystream words at the call's OWN set indices
    (blsgpu_batch_scalars, pinned by tests/test_batch_scalars.py), 0 for a lone non-batchable set."""
    parts = _parts(mode)
    m = cp.Merged(parts)
    scal = m.bytes("scal").view(np.uint64)
    at = 0
    for part in parts:
        c, a, e = _shard(part)
        abi = native.batch_scalars(c.jfs, c.flags, c.seed)
        assert [int(x) for x in abi] == expected_words(c.jfs.tolist(), c.flags.tolist(), c.seed)
        assert np.array_equal(scal[at:at + e - a], abi[a:e])
        assert np.array_equal(cp.shard_scalars(c, part[1], part[2]), abi[a:e])
        at += e - a
    assert at == len(scal) == 17
    assert scal[5] == 0  # part b's lone non-batchable set
    d_words = scal[13:17]  # call d's sets 2..5: job 1 (one set, not batchable), then job 2's three sets
    assert d_words[0] == 0 and (d_words[1:] != 0).all()
    # two parts get different keys: the same shape under another seed shares no word
    a1 = _call([2, 3], [1, 1], mode, [96] * 5, 96, seed=11)
    a2 = _call([2, 3], [1, 1], mode, [96] * 5, 96, seed=99)
    s = cp.Merged([(a1, 0, 2), (a2, 0, 2)]).bytes("scal").view(np.uint64)
    assert np.array_equal(s[:5], scal[:5]) and (s[:5] != s[5:]).all()


def test_results_scatter_into_each_calls_own_job_range():
    parts = _parts(0)
    m = cp.Merged(parts)
    res = np.arange(1, m["nj"] + 1).astype(np.int8)  # 2 + 1 + 5 + 2 jobs
    assert len(res) == 10
    m.scatter(res)
    a, b, c, d = (p[0] for p in parts)
    assert a.result.tolist() == [1, 2] and b.result.tolist() == [3] and c.result.tolist() == [4, 5, 6, 7, 8]
    assert d.result.tolist() == [77, 9, 10, 77]  # the sentinel stays outside [job_begin, job_end)


def _raw(n_sets, n_jobs, jfs, sig_len=None, stride=96, spf=None, pki=None, pkb=None, msgs=True, sigs=True):
    keep = []

    def arr(a, dt):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dt)
        keep.append(a)
        return a.ctypes.data

    b = Batch()
    b.n_sets, b.n_jobs, b.sig_stride = n_sets, n_jobs, stride
    b.job_first_set = arr(jfs, np.uint32)
    b.sig_len = arr(sig_len, np.uint32)
    b.msgs = arr(np.zeros(32 * max(n_sets, 1)), np.uint8) if msgs else None
    b.sigs = arr(np.zeros(stride * max(n_sets, 1)), np.uint8) if sigs else None
    b.set_pk_first, b.pk_index, b.pk_bytes = arr(spf, np.uint32), arr(pki, np.uint32), arr(pkb, np.uint8)
    return b, keep


def _validate(*a, **kw):
    b, keep = _raw(*a, **kw)
    return cp.lib().cp_validate(ctypes.byref(b))


def test_validate_batch_refusals():
    pkb1, pkb2 = np.zeros(96), np.zeros(192)
    assert _validate(1, 1, [0, 1], [96], pkb=pkb1) == native.OK  # the smallest valid batch
    assert _validate(0, 0, [0]) == native.OK and _validate(0, 2, [0, 0, 0]) == native.OK
    assert cp.lib().cp_validate(None) == native.ERR_ARGS
    assert _validate(1, 1, None, [96], pkb=pkb1) == native.ERR_ARGS  # no job_first_set
    assert _validate(1, 1, [1, 1], [96], pkb=pkb1) == native.ERR_ARGS  # a first entry that is not 0
    assert _validate(2, 2, [0, 3, 2], [96, 96], pkb=pkb2) == native.ERR_ARGS  # a decreasing prefix
    assert _validate(2, 1, [0, 1], [96, 96], pkb=pkb2) == native.ERR_ARGS  # a last entry that is not n_sets
    assert _validate(1, 0, [0]) == native.ERR_ARGS  # no jobs, but sets
    assert _validate(1, 1, [0, 1], None, pkb=pkb1) == native.ERR_ARGS  # missing arrays: sig_len,
    assert _validate(1, 1, [0, 1], [96], pkb=pkb1, msgs=False) == native.ERR_ARGS  # msgs,
    assert _validate(1, 1, [0, 1], [96], pkb=pkb1, sigs=False) == native.ERR_ARGS  # sigs
    assert _validate(1, 1, [0, 1], [96], stride=95, pkb=pkb1) == native.ERR_ARGS  # a stride below 96
    assert _validate(1, 1, [0, 1], [192], stride=96, pkb=pkb1) == native.ERR_ARGS  # a signature longer than the stride
    assert _validate(1, 1, [0, 1], [192], stride=191, pkb=pkb1) == native.ERR_ARGS
    assert _validate(1, 1, [0, 1], [192], stride=192, pkb=pkb1) == native.OK
    assert _validate(1, 1, [0, 1], [97], stride=96, pkb=pkb1) == native.OK  # (another length is the kernel's to reject)
    assert _validate(1, 1, [0, 1], [96], spf=[0, 1]) == native.ERR_ARGS  # table mode without pk_index
    assert _validate(1, 1, [0, 1], [96], pki=[0]) == native.ERR_ARGS  # table mode without set_pk_first
    assert _validate(1, 1, [0, 1], [96], spf=[0, 1], pki=[0]) == native.OK
    assert _validate(1, 1, [0, 1], [96], spf=[1, 1], pki=[0]) == native.ERR_ARGS  # key prefix not from 0
    assert _validate(2, 1, [0, 2], [96, 96], spf=[0, 2, 1], pki=[0, 0]) == native.ERR_ARGS  # key prefix decreasing
    assert _validate(2, 1, [0, 2], [96, 96], spf=[0, 2, 1], pkb=pkb2) == native.ERR_ARGS  # (bytes aggregate too)


def test_max_table_index_and_table_covers():
    L = cp.lib()
    c = cp.Call([2, 0, 1, 2], [1, 1, 1, 1], 0, [96] * 5, 96, seed=3, keys_per_set=[2, 0, 0, 3, 1])
    c.pki[:] = [7, 41, 5, 40, 39, 2]
    assert L.cp_max_table_index(c.ref()) == 41
    for mode in (1, 2):  # key bytes: no table index
        assert L.cp_max_table_index(_call([2], [1], mode, [96] * 2, 96, seed=3).ref()) == 0
    b, keep = _raw(0, 1, [0, 0])  # a call without sets
    assert L.cp_max_table_index(ctypes.byref(b)) == 0

    def covers(jb, je, table_n, call=c, max_index=41):
        return bool(L.cp_table_covers(call.ref(), jb, je, max_index, table_n))

    assert covers(0, 4, 42) and not covers(0, 4, 41) and not covers(0, 4, 0)
    assert not covers(3, 4, 41)  # the CALL's largest index counts, whichever shard uses it
    assert covers(1, 2, 0)  # a shard with no sets
    assert covers(1, 3, 0)  # a shard with sets (set 2) and no keys
    assert covers(0, 0, 0) and not covers(0, 1, 0)
    for mode in (1, 2):  # key bytes never need the table
        assert covers(0, 1, 0, call=_call([2], [1], mode, [96] * 2, 96, seed=3), max_index=0)
    assert L.cp_shard_cost(c.ref(), 0, 4) == 256 * 5 + 6 and L.cp_shard_cost(c.ref(), 2, 4) == 256 * 3 + 4
    assert L.cp_shard_cost(_call([2], [1], 1, [96] * 2, 96, seed=3).ref(), 0, 1) == 512


def test_probe_program_under_sanitizers(tmp_path):
    """The probe's own main (these shapes, threaded and serial) as a stand-alone program under ASan + UBSan: a child
    process, never loaded into Python."""
    one = tmp_path / "one.cpp"
    one.write_text("int main() { return 0; }\n")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if subprocess.run(["g++", *flags, "-o", str(tmp_path / "one"), str(one)], capture_output=True).returncode != 0 or \
            subprocess.run([str(tmp_path / "one")], capture_output=True).returncode != 0:
        pytest.skip("no sanitized host build here")
    exe = tmp_path / "call_plan_probe"
    subprocess.check_call(["g++", *flags, "-DCALL_PLAN_PROBE_MAIN", "-o", str(exe), cp.SRC, "-lpthread"])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "merged runs, checksum" in r.stdout
