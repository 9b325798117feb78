"""The multi-lane engines on raw limbs, on the device, each in the launch shape its production kernels use: every
record of tests/coop_vectors.py through blsgpu_debug_op ops 108..157 (k_coop_debug.hip) -- lacc_fin, the lane-pair
field, tower, line-step and G2 point forms (DPP exchanges, the pair-combined zero test), the six-lane GT engine (__shfl
with the packed select tables, ten groups per wave beside four idle lanes), the 16-lane g2c groups (four per block,
live groups beside groups flagged off that run every phase on arbitrary words and must write nothing) and the
workgroup GT engine (operands in LDS, every aliasing of gtw_mul, the barrier schedules).  Each op is launched in two
record orders: interleaved (neighbouring pairs / groups hold different data on different branches) and grouped (whole
waves on one branch); every record sits at two different positions of its block.  The reference is the oracle and
Python integers (tests/coop_vectors.py); the host-compilable subset of the same records also runs in
tests/test_coop_contracts.py.
Run on the MI355X box:  timeout -k 10 300 python -u -m pytest tests/test_gpu_coop_contracts.py -q --durations=0"""
import numpy as np
import pytest

from tests import coop_vectors as kv
from tests import tower_vectors as tv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd.native import Context

    c = Context()
    yield c
    c.close()


def _input_rows(recs):
    return np.array([[x for l in r.ins for x in l] for r in recs], dtype=np.uint32)


@pytest.mark.parametrize("name", kv.OP_NAMES)
def test_coop_contract_device(ctx, name):
    op = kv.BY_NAME[name]
    recs = kv.records(name)
    n_out = max(op.n_out, 1)  # (a predicate writes nothing; its output row stays zero)
    rows_in = _input_rows(recs)
    for label, order in zip(("interleaved", "grouped"), kv.launch_orders(name)):
        order = np.array(order)
        out, st = ctx.debug_op(op.code, rows_in[order].tobytes(), 56 * op.n_in, 56 * n_out)
        rows = np.empty((len(recs), n_out * tv.NL), np.uint32)
        rows[order] = np.frombuffer(out, np.uint32).reshape(len(recs), n_out * tv.NL)  # back to the records' order
        status = np.empty(len(recs), np.int64)
        status[order] = st
        bad = kv.check(name, rows.tolist(), status.tolist())
        assert not bad, "%s order: %s" % (label, kv.format_failures(name, bad))


def test_coop_op_bad_strides_refused(ctx):
    """strides below an op's element or not word-aligned, and the op just above the range, are refused on the host:
    one op of every engine"""
    for name in ("lacc_fin", "fp6x_mul", "g6_line_mul", "g2c_add", "gtw_mul sparse", "gtw_miller_loop"):
        op = kv.BY_NAME[name]
        i, o = 56 * op.n_in, 56 * op.n_out
        inp = _input_rows(kv.records(name)[:3]).tobytes()
        out, st = ctx.debug_op(op.code, inp, i, o)
        assert len(st) == 3
        for in_stride, out_stride in ((i - 4, o), (i, o - 4), (i + 2, o), (i, o + 2)):
            with pytest.raises(RuntimeError, match="ERR_ARGS"):
                ctx.debug_op(op.code, inp, in_stride, out_stride)
    with pytest.raises(RuntimeError, match="ERR_ARGS"):
        ctx.debug_op(158, bytes(3 * 1344), 1344, 672)
