"""The one-lane point formulas on raw limbs, exceptional branches included, on the device: every record of
tests/curve_vectors.py through blsgpu_debug_op ops 69..107 (k_curve_debug.hip), two launches per op over the same
records.  The same records pass on the host build (tests/test_curve_contracts.py); here they run through what only the
device has -- hipcc's code for the shared source, the register-ABI product calls and the per-lane LDS slot of the Fp2
products, and lanes of one wave on different branches: in the interleaved order every 64-lane wave mixes the branch
classes (a nested jac_dbl inside jac_add next to lanes on the generic path, infinity next to both), in the grouped
order the waves are uniform wherever a class fills one.
Run on the MI355X box:  timeout -k 10 300 python -u -m pytest tests/test_gpu_curve_contracts.py -q --durations=0"""
import numpy as np
import pytest

from tests import curve_vectors as cv
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


@pytest.mark.parametrize("name", cv.OP_NAMES)
def test_curve_contract_device(ctx, name):
    op = cv.BY_NAME[name]
    recs = cv.records(name)
    assert len(recs) > 128 and len(recs) % 128  # more than one workgroup, the last one partly filled
    n_out = max(op.n_out, 1)  # (a predicate writes nothing; its output row stays zero)
    rows_in = _input_rows(recs)
    interleaved, grouped = cv.launch_orders(name)
    assert all(len(c) > 1 for c in cv.wave_classes(name, interleaved))
    assert any(len(c) == 1 for c in cv.wave_classes(name, grouped))
    for label, order in (("interleaved", interleaved), ("grouped", grouped)):
        order = np.array(order)
        out, st = ctx.debug_op(op.code, rows_in[order].tobytes(), 56 * op.n_in, 56 * n_out)
        rows = np.empty((len(recs), n_out * tv.NL), np.uint32)
        rows[order] = np.frombuffer(out, np.uint32).reshape(len(recs), n_out * tv.NL)  # back to the records' order
        status = np.empty(len(recs), np.int64)
        status[order] = st
        bad = cv.check(name, rows.tolist(), status.tolist())
        assert not bad, "%s order: %s" % (label, cv.format_failures(name, bad))


def test_curve_op_short_stride_refused(ctx):
    """strides below a curve op's element (G2 jac_add: 12 x 56 in, 6 x 56 out), or not word-aligned, are refused on
    the host"""
    inp = _input_rows(cv.records("g2_jac_add")[:4]).tobytes()
    out, st = ctx.debug_op(89, inp, 672, 336)
    assert len(st) == 4
    for in_stride, out_stride in ((668, 336), (672, 332), (674, 336), (672, 338)):
        with pytest.raises(RuntimeError, match="ERR_ARGS"):
            ctx.debug_op(89, inp, in_stride, out_stride)
