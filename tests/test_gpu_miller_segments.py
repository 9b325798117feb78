"""Step segments of the one-lane Miller accumulation on the device (miller_plan.hpp, k_miller_acc<.., SEG>, k_f_fold):
J lanes per chunk, each over its own step range, the F tree per (group, segment) and the per-group Horner fold, forced
by BLSGPU_MILLER_SEGMENTS = J with miller_k = k, miller_lanes = 1 and coop_max = 0 on calls far below the automatic
rule's 65,536 items, and once through the automatic rule itself.  Every case is compared job for job with
oracle/blscpu.c."""
import os

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import cpu
from tests.test_gpu_parity import THREADS, corrupted_single_sets, interop_sks, msg

pytestmark = pytest.mark.gpu

ENV = "BLSGPU_MILLER_SEGMENTS"


class forced:
    """A context created with BLSGPU_MILLER_SEGMENTS = J (blsgpu_init reads it), chunks of k on one lane."""

    def __init__(self, J, k):
        self.J, self.k = J, k

    def __enter__(self):
        from lodestar_amd.native import Context

        self.old = os.environ.get(ENV)
        os.environ[ENV] = str(self.J)
        try:
            self.ctx = Context([0])
        finally:
            if self.old is None:
                del os.environ[ENV]
            else:
                os.environ[ENV] = self.old
        self.ctx.set_option("miller_k", self.k)
        self.ctx.set_option("miller_lanes", 1)
        self.ctx.set_option("coop_max", 0)
        return self.ctx

    def __exit__(self, *exc):
        self.ctx.close()


@pytest.fixture(scope="module")
def ragged():
    """2,085 single-key one-set jobs (divisible by neither 4 nor 8: ragged last chunks), ~1% corrupted so the fallback
    runs beside the batch pass; the oracle's verdicts, computed once."""
    n = 2085
    sks, pks, msgs, sigs, sig_len = corrupted_single_sets(n, b"SEG", np.random.default_rng(2085))
    batch = dict(job_first_set=np.arange(n + 1), sigs=sigs, sig_len=sig_len, msgs=b"".join(msgs), sig_stride=192,
                 pk_bytes=pks, job_flags=np.ones(n))
    want, _ = cpu.verify_jobs(threads=THREADS, **batch)
    return n, batch, want


@pytest.mark.parametrize("J,k", [(2, 2), (3, 4), (4, 8), (8, 8)])
def test_ragged_chunks_and_fallback_vs_oracle(ragged, J, k):
    n, batch, want = ragged
    with forced(J, k) as ctx:
        got, st = ctx.verify_raw(**batch)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert (got == 1).sum() >= n - max(8, n // 100) and st.batch_retries >= 1 and st.fallback_miller > 0
    # chunks, not lanes: every group's items in chunks of <= k, the last one ragged
    assert n / k <= st.miller_chunks <= n / k + st.groups and st.miller_chunks * k != n


def test_automatic_rule_on_a_large_run_vs_oracle(ragged):
    """The automatic rule, which starts at 65,536 items: the 2,085 jobs above 32 times over in one call (66,720 sets,
    dedupe off so that every repeated set is its own pairing).  Jobs are independent, so the oracle's verdicts repeat
    with them.  Every group holds corrupted sets, so the fallback's whole-loop accumulations run after a batch pass
    that took chunks of 8 on step segments (miller_chunks counts chunks: ~ n / 8)."""
    from lodestar_amd.native import Context

    n0, base, want0 = ragged
    rep = 32
    n = n0 * rep
    batch = dict(job_first_set=np.arange(n + 1), sigs=bytes(base["sigs"]) * rep, sig_len=list(base["sig_len"]) * rep,
                 msgs=bytes(base["msgs"]) * rep, sig_stride=192, pk_bytes=bytes(base["pk_bytes"]) * rep,
                 job_flags=np.ones(n))
    ctx = Context([0])
    try:
        ctx.set_option("dedupe", 0)
        got, st = ctx.verify_raw(**batch)
    finally:
        ctx.close()
    assert np.array_equal(got, np.tile(want0, rep)), np.nonzero(got != np.tile(want0, rep))[0][:10]
    assert st.pairing_units == n and st.batch_retries >= 1 and st.fallback_miller > 0
    assert n / 8 <= st.miller_chunks <= n / 8 + st.groups


def test_same_message_units_vs_oracle():
    """2,048 sets over 300 distinct roots, dedupe on: the items are same-message units (k_miller_acc<true, SEG>)."""
    n, n_msg = 2048, 300
    sks = interop_sks(n, first=5000)
    msgs = [msg(i % n_msg, b"segment units") for i in range(n)]
    sigs = bytearray(cpu.sign(sks, b"".join(msgs), threads=THREADS))
    sigs[96 * 900: 96 * 901] = sigs[96 * 1200: 96 * 1201]  # the same root, another signer's signature
    batch = dict(job_first_set=np.arange(n + 1), sigs=bytes(sigs), sig_len=[96] * n, msgs=b"".join(msgs),
                 pk_bytes=cpu.sk_to_pk(sks, threads=THREADS), job_flags=np.ones(n))
    want, _ = cpu.verify_jobs(threads=THREADS, **batch)
    with forced(4, 8) as ctx:
        got, st = ctx.verify_raw(**batch)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert got[900] == 0 and (np.delete(got, 900) == 1).all()
    assert st.unique_messages == n_msg and st.pairing_units < n and st.miller_chunks < st.pairing_units


def test_tiny_and_empty_groups_vs_oracle():
    """Groups of one item (non-batchable one-set jobs: one chunk of one item on J lanes) among batchable jobs, and a
    group with no active item (a non-batchable job whose only set is malformed: every segment value is one)."""
    n = 600
    sks = interop_sks(n, first=7000)
    msgs = [msg(i, b"segment tiny") for i in range(n)]
    sigs = bytearray(cpu.sign(sks, b"".join(msgs), threads=THREADS))
    flags = np.ones(n)
    flags[[5, 77, 300, 599]] = 0
    sigs[96 * 77] = 0x00  # compressed flag cleared -> BAD_ENCODING: job 77 has no set that enters its equation
    sigs[96 * 300: 96 * 301] = sigs[96 * 301: 96 * 302]  # a one-item group that fails
    batch = dict(job_first_set=np.arange(n + 1), sigs=bytes(sigs), sig_len=[96] * n, msgs=b"".join(msgs),
                 pk_bytes=cpu.sk_to_pk(sks, threads=THREADS), job_flags=flags)
    want, _ = cpu.verify_jobs(threads=THREADS, **batch)
    with forced(4, 8) as ctx:
        got, st = ctx.verify_raw(**batch)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    assert got[77] == -bls.BLST_BAD_ENCODING and got[300] == 0 and (np.delete(got, [77, 300]) == 1).all()
    assert st.groups >= 5
