"""The field tower at the edges of its operand contracts, on the host build of the headers: every record of
tests/tower_vectors.py through tests/native/emu.cpp's emu_tower_op -- the dispatch (csrc/tower_debug.hpp) the device
kernel runs too.  This is what shows, without a GPU, that the vectors' expectations are right and that the arithmetic
stays inside every stated bound; tests/test_gpu_tower_contracts.py re-runs the same records on MI355X."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import tower_vectors as tv
from tests.emu_helpers import lib

U32P = ctypes.POINTER(ctypes.c_uint32)


def _run(fn, recs, n_in, n_out, with_op=None):
    """one call per record on its own rows of two arrays; returns the output rows and the status words"""
    inp = np.array([[x for l in r.ins for x in l] for r in recs], dtype=np.uint32).reshape(len(recs), n_in * tv.NL)
    out = np.zeros((len(recs), max(n_out, 1) * tv.NL), dtype=np.uint32)
    st = []
    ip, op = inp.ctypes.data, out.ctypes.data
    for i in range(len(recs)):
        a = ctypes.cast(ip + i * inp.strides[0], U32P)
        b = ctypes.cast(op + i * out.strides[0], U32P)
        st.append(fn(with_op, a, b) if with_op is not None else (fn(a, b), 0)[1])
    return out, st


@pytest.mark.parametrize("name", tv.OP_NAMES)
def test_tower_contract_host(name):
    L = lib()
    L.emu_tower_op.argtypes = [ctypes.c_int, U32P, U32P]
    L.emu_tower_op.restype = ctypes.c_int
    op = tv.BY_NAME[name]
    recs = tv.records(name)
    out, st = _run(L.emu_tower_op, recs, op.n_in, op.n_out, with_op=op.code)
    bad = tv.check(name, out.tolist(), st)
    assert not bad, tv.format_failures(name, bad)


def test_fp2_mul_both_bodies_at_the_closed_edge():
    """fp2_mul's records (values up to and including 8p, 8p also as the un-normalized 4p + 4p) through both product
    bodies: the schoolbook-offset body the build selects (< 1.1 p) and the lazy-reduction body (< 1.06 p)."""
    L = lib()
    recs = tv.records("fp2_mul")
    assert any(all(tv.val(l) == 8 * tv.P for l in r.ins) and max(r.ins[0]) >= 1 << 28 for r in recs)
    for fn, bound in ((L.emu_fp2_mul_sb_limbs, tv.lt_frac(11, 10)), (L.emu_fp2_mul_lazy_limbs, tv.lt_frac(106, 100))):
        fn.argtypes = [U32P, U32P]
        fn.restype = None
        out, st = _run(fn, recs, 4, 2)
        bad = tv.check("fp2_mul", out.tolist(), st)
        assert not bad, tv.format_failures("fp2_mul", bad)
        vals = [tv.val(row[:14]) for row in out.tolist()] + [tv.val(row[14:]) for row in out.tolist()]
        assert max(vals) <= bound


def test_vector_set_shape():
    """What the device test relies on: per operation more than one 128-lane workgroup and a partly filled last one,
    no two records with the same operands, operands inside the stated limb bounds; fp2_sqrt's square / non-square
    counts by the oracle and an input on each side of its t == 0 selection."""
    limb_bits = {"fp_mul": 30, "fp2_mul_fp": 30, "fp_sqr": 29, "fp2_mul": 29}
    value_max = {"fp_mul": 16 * tv.P - 1, "fp2_mul_fp": 16 * tv.P - 1, "fp_sqr": 4 * tv.P, "fp2_mul": 8 * tv.P,
                 "fp2_sqr": 4 * tv.P, "fp6_mul": 4 * tv.P, "fp6_mul_by_01": 4 * tv.P, "fp6_mul_by_12": 4 * tv.P}
    for name in tv.OP_NAMES:
        recs = tv.records(name)
        assert len(recs) > 128 and len(recs) % 128 != 0, name
        assert len({tuple(tuple(l) for l in r.ins) for r in recs}) == len(recs), name
        bits, vmax = limb_bits.get(name, 28), value_max.get(name, 2 * tv.P)
        arr = np.array([r.ins for r in recs], dtype=np.int64)  # (records, operands, limbs)
        assert arr.min() >= 0 and arr[:, :, :13].max() < (1 << bits), name
        vals = [tv.val(l) for l in arr.reshape(-1, tv.NL).tolist()]
        assert max(vals) == vmax, name  # nothing above the contract, and the closed edge itself is present
    sq = tv.records("fp2_sqrt")
    assert sum(r.status for r in sq) >= 20 and sum(1 - r.status for r in sq) >= 20
    assert any("[t == 0]" in r.name for r in sq if r.status) and any("[t == 0]" not in r.name for r in sq if r.status)


def test_op_sizes_match_the_library_table():
    """blsgpu_debug_op's kOpSizes rows (helpers.cpp) for the tower ops and the point-formula ops (tests/curve_vectors.py)
    are the vectors' operand / result counts at 56 bytes per Fp value, so a short stride is refused on the host."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lodestar_amd", "csrc",
                            "helpers.cpp")).read()
    table = src[src.index("kOpSizes[] ="):src.index("const OpSize* sz")]
    rows = {int(a): (int(b), int(c)) for a, b, c in re.findall(r"\{(\d+),\s*(\d+),\s*(\d+)\}", table)}
    for op in tv.OPS:
        assert rows[op.code] == (56 * op.n_in, 56 * op.n_out), op.name
    from tests import curve_vectors as cv  # the raw-limb ops are the tower's and the point formulas', nothing else

    for op in cv.OPS:
        assert rows[op.code] == (56 * op.n_in, 56 * op.n_out), op.name
    assert [c for c in sorted(rows) if 32 <= c <= 68] == [op.code for op in tv.OPS]
    assert sorted(c for c in rows if c >= 32) == [op.code for op in tv.OPS] + [op.code for op in cv.OPS]
