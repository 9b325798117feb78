"""The library runs the plan the probe computes: for a few small calls, the run's counts in blsgpu_stats (groups,
unique messages, pairing units, Miller chunks, retried jobs and their re-run Miller loops) equal those of
csrc/run_plan.hpp built on the host from the same arrays (tests/native/run_plan_probe.cpp), and the per-job results
equal the oracle's.  Each case has a fresh context with group_adapt 0, so no earlier run's failure rate plays a part."""
import numpy as np
import pytest

from oracle import cpu
from tests import run_plan_probe as rp
from tests.test_gpu_parity import THREADS, interop_sks, msg

pytestmark = pytest.mark.gpu

COUNTS = [2, 0, 1, 3, 1, 2, 1]  # seven jobs, ten sets (tests/test_run_plan.py)
FLAGS = [1, 1, 0, 1, 1, 1, 1]
MSGS = [5, 5, 6, 7, 5, 7, 7, 5, 8, 8]  # repeats inside a group and across groups


@pytest.fixture(scope="module")
def keys():
    sks = interop_sks(40, first=7000)
    return sks, cpu.sk_to_pk(sks, threads=THREADS)


def run_case(keys, counts, flags, msg_ids, options, bad=()):
    """One call on a fresh context: set i is key i over message msg_ids[i]; the sets in `bad` carry the next key's
    signature over their message (well-formed, invalid).  Returns (results, stats, the probe's plan, its options)."""
    from lodestar_amd.native import Context

    sks, pks = keys
    n = sum(counts)
    signer = [(i + 1) % n if i in bad else i for i in range(n)]
    sigs = cpu.sign(b"".join(sks[32 * k: 32 * k + 32] for k in signer), b"".join(msg(m, b"plan") for m in msg_ids),
                    threads=THREADS)
    batch = dict(job_first_set=np.concatenate([[0], np.cumsum(counts)]), sigs=sigs, sig_len=[96] * n,
                 msgs=b"".join(msg(m, b"plan") for m in msg_ids), pk_bytes=pks[:96 * n], job_flags=np.asarray(flags))
    opts = dict(group_adapt=0, **options)
    c = Context([0])
    try:
        for k, v in opts.items():
            c.set_option(k, v)
        got, st = c.verify_raw(**batch)
    finally:
        c.close()
    want, _ = cpu.verify_jobs(threads=THREADS, **batch)
    assert np.array_equal(got, want), (got, want)
    o = rp.Opts(**opts)
    first = {}
    p = rp.plan(counts, flags, [first.setdefault(m, i) for i, m in enumerate(msg_ids)], opts=o, alone=True)
    assert (st.groups, st.unique_messages, st.pairing_units, st.miller_chunks) == (
        p["ng0"], p["n_umsg"], p["n_items"], p["n_chunks"])
    return got, st, p, o


@pytest.mark.parametrize("options,merged,coop,mk", [
    (dict(group_sets=4), True, True, 1),             # merged units, cooperative forms
    (dict(group_sets=4, dedupe=0), False, True, 1),
    (dict(group_sets=4, miller_k=2), True, False, 2),  # stored lines and the lane accumulation
])
def test_seven_jobs(keys, options, merged, coop, mk):
    got, st, p, _ = run_case(keys, COUNTS, FLAGS, MSGS, options)
    assert (p["merged"], p["coop"], p["mk"]) == (merged, coop, mk)
    assert all(got[j] == 1 for j, c in enumerate(COUNTS) if c) and st.fallback_jobs == 0
    assert st.pairing_units == (6 if merged else 10) and st.groups == 4


@pytest.mark.parametrize("keep_f", [1, 0])
def test_failed_group_of_three_jobs(keys, keep_f):
    """One invalid signature in a three-job group: every job of the group is re-checked on its own, from the kept
    per-set Miller values (keep_f 1) or by re-running its Miller loops (keep_f 0)."""
    got, st, p, o = run_case(keys, [1, 1, 1], [1, 1, 1], [101, 102, 103], dict(keep_f=keep_f), bad=[1])
    assert got.tolist() == [1, 0, 1] and p["ng0"] == 1 and p["keep_f"] == keep_f
    c, _ = rp.classify(p, [0, 0, 0], [0], spec=p["spec"])
    f = rp.fallback(p, c.vec("retry"), o, alone=True)
    assert st.fallback_jobs == len(c.vec("retry")) == 3
    assert st.fallback_miller == (0 if keep_f else len(f.vec("ritems"))) and len(f.vec("ritems")) == (0 if keep_f else 3)


def test_two_round_fallback_with_a_one_job_last_sub_group(keys):
    """33 single-set jobs in one group, one invalid, not a small run: sub-groups of 16, 16 and 1 jobs, then the jobs of
    the failing sub-group one by one."""
    n = 33
    got, st, p, o = run_case(keys, [1] * n, [1] * n, [100 + i for i in range(n)], dict(group_sets=64, small_max=0),
                             bad=[20])
    c, _ = rp.classify(p, [0] * n, [0], spec=p["spec"])
    f = rp.fallback(p, c.vec("retry"), o, alone=True)
    assert p["ng0"] == 1 and not p["small"] and f["nsub"] == 3 and f.vec("subr")[-2:] == [32, 33]
    assert st.fallback_jobs == 33 == f["nr"]
    assert got.tolist() == [0 if j == 20 else 1 for j in range(n)]
