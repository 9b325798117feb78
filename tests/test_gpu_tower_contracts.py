"""The field tower at the edges of its operand contracts, on the device: every record of tests/tower_vectors.py through
blsgpu_debug_op ops 32..68 (k_tower_debug.hip), one call per operation.  The same records pass on the host build
(tests/test_tower_contracts.py); here they run through what only the device has -- the register-ABI product calls
(fp_mul_r, fp_sqr_r, fp2_mul_r, fp2_sqr_r, fp2_mul_fp_r), the per-lane LDS slot of the Fp2 products' second operand
at its full 128-lane width with different data in every lane, and hipcc's code for the shared source.
Run on the MI355X box:  python -u -m pytest tests/test_gpu_tower_contracts.py -q --durations=0"""
import numpy as np
import pytest

from tests import tower_vectors as tv

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from lodestar_amd.native import Context

    c = Context()
    yield c
    c.close()


def _input_bytes(recs):
    return np.array([[x for l in r.ins for x in l] for r in recs], dtype=np.uint32).tobytes()


@pytest.mark.parametrize("name", tv.OP_NAMES)
def test_tower_contract_device(ctx, name):
    op = tv.BY_NAME[name]
    recs = tv.records(name)
    assert len(recs) > 128 and len(recs) % 128  # more than one workgroup, the last one partly filled
    n_out = max(op.n_out, 1)  # (a predicate writes nothing; its output row stays zero)
    out, st = ctx.debug_op(op.code, _input_bytes(recs), 56 * op.n_in, 56 * n_out)
    rows = np.frombuffer(out, np.uint32).reshape(len(recs), n_out * tv.NL)
    bad = tv.check(name, rows.tolist(), st.tolist())
    assert not bad, tv.format_failures(name, bad)


def test_tower_op_short_stride_refused(ctx):
    """strides below a tower op's element (fp2_mul: 4 x 56 in, 2 x 56 out), or not word-aligned, are refused on the
    host"""
    inp = _input_bytes(tv.records("fp2_mul")[:4])
    out, st = ctx.debug_op(34, inp, 224, 112)
    assert len(st) == 4
    for in_stride, out_stride in ((220, 112), (224, 108), (226, 112), (224, 114)):
        with pytest.raises(RuntimeError, match="ERR_ARGS"):
            ctx.debug_op(34, inp, in_stride, out_stride)
