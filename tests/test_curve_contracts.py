"""The one-lane point formulas (csrc/curve.hpp, ops.hpp g1_in_subgroup) on raw limbs, exceptional branches included,
on the host build of the headers: every record of tests/curve_vectors.py through tests/native/emu.cpp's emu_curve_op --
the dispatch (csrc/curve_debug.hpp) the device kernel runs too.  This is what shows, without a GPU, that the vectors'
expectations are right; tests/test_gpu_curve_contracts.py re-runs the same records on MI355X.  (The kOpSizes rows of
these ops are checked with the tower's: tests/test_tower_contracts.py test_op_sizes_match_the_library_table.)"""
import ctypes
import random

import numpy as np
import pytest

from oracle import bls12_381 as bls
from tests import curve_vectors as cv
from tests import tower_vectors as tv
from tests.emu_helpers import lib
from tests.test_tower_contracts import U32P, _run


@pytest.mark.parametrize("name", cv.OP_NAMES)
def test_curve_contract_host(name):
    L = lib()
    L.emu_curve_op.argtypes = [ctypes.c_int, U32P, U32P]
    L.emu_curve_op.restype = ctypes.c_int
    op = cv.BY_NAME[name]
    recs = cv.records(name)
    out, st = _run(L.emu_curve_op, recs, op.n_in, op.n_out, with_op=op.code)
    bad = cv.check(name, out.tolist(), st)
    assert not bad, cv.format_failures(name, bad)


def test_affine_law_agrees_with_the_oracle():
    """aff_add (the reference for the pairs the oracle's API cannot take) against g1_add / g2_add: P + Q, P + P,
    P - P and the infinity cases, over the whole pool"""
    for G in (cv.G1, cv.G2):
        pts = [pt.aff for pt in cv.pool(G.tag)]
        rng = random.Random(11)
        for i, a in enumerate(pts):
            b = pts[rng.randrange(len(pts))]
            for p, q in ((a, b), (a, a), (a, G.neg(a)), (None, a), (a, None), (None, None)):
                assert cv.aff_add(G, p, q) == G.add(p, q), (G.tag, i)


def test_curve_vector_set_shape():
    """What the device test relies on: per op more than one 128-lane workgroup and a partly filled last one, distinct
    operands, every operand normalized and within [0, 2p]; the additions' records on every branch; at least two
    branch classes per op, mixed in every wave of the interleaved order and a uniform wave in the grouped one."""
    for name in cv.OP_NAMES:
        recs = cv.records(name)
        assert len(recs) > 128 and len(recs) % 128 != 0, name
        assert len({tuple(tuple(l) for l in r.ins) for r in recs}) == len(recs), name
        arr = np.array([r.ins for r in recs], dtype=np.int64)
        assert arr.min() >= 0 and arr[:, :, :13].max() < (1 << 28), name
        assert max(tv.val(l) for l in arr.reshape(-1, tv.NL).tolist()) <= 2 * tv.P, name
        inter, grouped = cv.launch_orders(name)
        assert sorted(inter) == sorted(grouped) == list(range(len(recs))), name
        assert all(len(c) > 1 for c in cv.wave_classes(name, inter)), name
        assert any(len(c) == 1 for c in cv.wave_classes(name, grouped)), name
    for tag in ("g1", "g2"):
        for fn, classes in (("jac_add", {"generic", "P+P", "P-P", "inf+Q", "P+inf", "inf+inf"}),
                            ("jac_add_aff", {"generic", "P+P", "P-P", "inf+Q"})):
            for body in ("", "_lazy", "_eager"):
                got = {r.cls for r in cv.records("%s_%s%s" % (tag, fn, body))}
                assert got >= classes, (tag, fn, body)
                assert tag == "g1" or got >= {"generic, x half-equal", "P-P, y half-equal"}


def test_chain_records_take_every_reachable_branch():
    """From the mirror of the [|z|] chain alone (curve_vectors.chain_branches): the table of the module docstring, and
    every branch an available small order reaches is taken by a record of each chain op of that group."""
    assert cv.chain_branches(3) == {"inf+P", "P+P", "-P+P", "dbl inf"}
    assert cv.chain_branches(11) == {"P+P"}
    assert cv.chain_branches(13) == {"inf+P", "-P+P", "dbl inf"}
    for m in (23, 2713, 10177, 11953):
        assert cv.chain_branches(m) == set()
    for tag, names in cv.CHAIN_OPS.items():
        for name in names:
            for branch in cv.CHAIN_REACHABLE[tag]:
                assert any(branch in r.branches for r in cv.records(name)), (name, branch)
    assert "P+P" not in cv.CHAIN_REACHABLE["g2"]  # (the docstring's unreachable pair)


def test_subgroup_records_follow_the_definition():
    """the subgroup predicates' expected answers are [r]P == O by the oracle: true on subgroup points in every
    representative, false on outside points and on every small-order point"""
    for tag in ("g1", "g2"):  # (pool() itself asserts in_subgroup == ([r]P is None) for every point)
        assert not any(pt.order and pt.in_subgroup for pt in cv.pool(tag))
    assert [bls.g2_in_subgroup_def(pt.aff) for pt in cv.pool("g2")] == [pt.in_subgroup for pt in cv.pool("g2")]
    for name in ("g1_in_subgroup", "g2_in_subgroup", "g2_in_subgroup_ld"):
        recs = cv.records(name)
        assert sum(r.status for r in recs) >= 20 and sum(1 - r.status for r in recs) >= 20

