"""The multi-lane engines on raw limbs, the part of them the host build of the headers can run: the records of
tests/coop_vectors.py through tests/native/emu.cpp's emu_coop_op (csrc/coop_debug.hpp coop_host_op) -- lacc_fin, the
g2c phases lane by lane (g2c_host_add, the doubling phases, the chain), gtw_mul_prod / gtw_mul_rec lane by lane in
every aliasing, and the Miller schedule.  Lanes run in turn here, so no cross-lane bug can show: this test shows that
the vectors' expectations are right and that the phase arithmetic stays inside its bounds;
tests/test_gpu_coop_contracts.py runs the same records on MI355X in the production launch shapes.
The lane-pair ops (fp2x.hpp, gtx.hpp: DPP exchanges) and the six-lane ops (gt6.hpp: __shfl), and gtw_cyc_sqr, gtw_conj,
gtw_frob, gtw_pow_z and gtw_final_exp, are device-only: their records are built and shape-checked here, and run on the
device only."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import coop_vectors as kv
from tests import tower_vectors as tv
from tests.emu_helpers import lib
from tests.test_tower_contracts import U32P, _run


# the classes of records on an op's ordinary path; every other class is an edge or an exceptional branch
PLAIN = {"random", "generic", "finite", "cyclotomic", "neither zero", "not one", "curve point"}
# the classes whose records take an exceptional branch of the point formulas (additions, chains)
EXCEPTIONAL = {"inf", "P+P", "P-P", "inf+Q", "P+inf", "inf+inf", "order 13: -P+P, dbl inf, inf+P"}


def _lib():
    L = lib()
    L.emu_coop_op.argtypes = [ctypes.c_int, U32P, U32P]
    L.emu_coop_op.restype = ctypes.c_int
    L.emu_lacc_audit_max.argtypes = [ctypes.c_int]
    L.emu_lacc_audit_max.restype = ctypes.c_double
    L.emu_lacc_audit_reset.restype = None
    return L


def _host_recs(name):
    """the records the host model can run: a g2c element flagged off exists on the device only"""
    return [r for r in kv.records(name) if r.cls != "off"]


@pytest.mark.parametrize("name", kv.HOST_OP_NAMES)
def test_coop_contract_host(name):
    L = _lib()
    op = kv.BY_NAME[name]
    recs = _host_recs(name)
    out, st = _run(L.emu_coop_op, recs, op.n_in, op.n_out, with_op=op.code)
    bad = kv.check(name, out.tolist(), st, recs=recs)
    assert not bad, kv.format_failures(name, bad)


def test_device_only_ops_are_refused_by_the_host_entry():
    L = _lib()
    buf = (ctypes.c_uint32 * (24 * tv.NL))()
    for op in kv.OPS:
        if not op.host:
            assert L.emu_coop_op(op.code, buf, buf) == -2, op.name
    assert L.emu_coop_op(158, buf, buf) == -2


def test_lacc_users_stay_inside_lacc_fin_range():
    """No caller of lacc_fin counts its own terms.  Over every record of the lacc users the host build runs, the
    largest positive-side and negative-side sums handed to lacc_fin (recorded by the BLS_LACC_AUDIT build of lacc.hpp,
    in units of p) stay inside what it requires: lacc.hpp promises at most 15 terms <= 2p per side, i.e. <= 30 p, and
    the quotient estimate needs pos + 32p - neg in [0, 64p)."""
    L = _lib()
    worst = [0.0, 0.0]
    for name in kv.LACC_USERS:
        op = kv.BY_NAME[name]
        L.emu_lacc_audit_reset()
        _run(L.emu_coop_op, _host_recs(name), op.n_in, op.n_out, with_op=op.code)
        m = [L.emu_lacc_audit_max(0), L.emu_lacc_audit_max(1)]
        print("%-16s largest lacc_fin sums: + %.3f p, - %.3f p" % (name, m[0], m[1]))
        assert 0 < m[0] <= 30 and 0 < m[1] <= 30, (name, m)
        worst = [max(a, b) for a, b in zip(worst, m)]
    assert worst[0] < 32 and worst[1] <= 32
    # the audit itself: 15 x 2p on both sides reads as 30 p
    op = kv.BY_NAME["lacc_fin"]
    L.emu_lacc_audit_reset()
    _run(L.emu_coop_op, [r for r in kv.records("lacc_fin") if r.cls == "15 x 2p"], op.n_in, op.n_out, with_op=op.code)
    assert abs(L.emu_lacc_audit_max(0) - 30) < 1e-9 and abs(L.emu_lacc_audit_max(1) - 30) < 1e-9


def test_coop_vector_set_shape():
    """What the device test relies on, for every op (the device-only ones included): distinct operands; more than one
    block of the engine's kernel and a partly filled last one (the ten-record chain ops aside); operands inside the
    contract; two orders in which every record changes its position within the block; different branch classes next
    to each other in the interleaved order; in the grouped order a whole wave on every class that can fill one, the
    point formulas' exceptional branches among them; records of every non-plain class at the first and last pair of a
    DPP row, in six-lane group 9 and in g2c group 3."""
    limb_bits = {"fp2x_mul": 29, "lacc_fin": 32}
    value_max = {"fp2x_mul": 8 * tv.P, "fp2x_sqr": 4 * tv.P, "fp6x_mul": 4 * tv.P}
    for name in kv.OP_NAMES:
        op = kv.BY_NAME[name]
        recs = kv.records(name)
        blk = kv.BLOCK[op.engine]
        assert len({tuple(tuple(l) for l in r.ins) for r in recs}) == len(recs), name
        if name in kv.CHAIN_OPS:
            assert 8 <= len(recs) <= 12, name
        elif blk > 1:
            assert len(recs) > blk and len(recs) % blk != 0, name
        inter, grouped = kv.launch_orders(name)
        assert sorted(inter) == sorted(grouped) == list(range(len(recs))), name
        if blk > 1:
            where = {r: j % blk for j, r in enumerate(inter)}
            assert all(where[r] != j % blk for j, r in enumerate(grouped)), name
        assert len({r.cls for r in recs}) > 1, name
        # the grouped order: every class that has a wave's worth of records fills a wave of its own
        wave = kv.WAVE[op.engine]
        uniform = {next(iter(c)) for c in kv.wave_classes(name, grouped) if len(c) == 1}
        for cls in {r.cls for r in recs}:
            assert sum(r.cls == cls for r in recs) < wave or cls in uniform or wave == 1, (name, cls)
        # and where a class is an exceptional branch of the point formulas, a whole wave takes that branch
        if op.engine in ("pair", "g2c"):
            assert EXCEPTIONAL & {r.cls for r in recs} <= uniform, (name, EXCEPTIONAL & {r.cls for r in recs} - uniform)
        # the required positions, for every class but the op's plain one (random / generic / finite / cyclotomic):
        # the first and the last pair of a 16-lane DPP row, six-lane group 9 beside the idle lanes, g2c group 3
        want_pos = {"pair": {0, 7}, "g6": {9}, "g2c": {3}}.get(op.engine)
        if want_pos and name not in kv.CHAIN_OPS:
            mod = 8 if op.engine == "pair" else blk
            for cls in {r.cls for r in recs} - PLAIN:
                seen = {j % mod for order in (inter, grouped) for j, r in enumerate(order) if recs[r].cls == cls}
                assert seen >= want_pos or sum(r.cls == cls for r in recs) < 2 * mod, (name, cls, seen)  # (a class
                # with fewer records than two rows / blocks need not reach them)
        if op.engine != "gtw" and name not in kv.CHAIN_OPS:
            mixed = [len(c) > 1 for c in kv.wave_classes(name, inter)]
            minor = len(recs) - max(sum(r.cls == c for r in recs) for c in {r.cls for r in recs})
            assert sum(mixed) >= min(len(mixed) - 1, minor // 2), name  # (as many waves as the small classes reach)
        if op.engine in ("g2c", "lane") or name == "fp2x_is_zero":
            continue  # (raw words / limb sums / checked below)
        arr = np.array([r.ins for r in recs], dtype=np.int64)
        assert arr.min() >= 0 and arr[:, :, :13].max() < (1 << limb_bits.get(name, 28)), name
        vmax = max(tv.val(l) for l in arr.reshape(-1, tv.NL).tolist())
        assert vmax <= value_max.get(name, 2 * tv.P), name  # nothing above the contract
        assert name in kv.CHAIN_OPS or vmax == value_max.get(name, 2 * tv.P), name  # and its closed edge is present
    # fp2x_mul: one fp_add_nr level, 8p - 1 reached independently per coefficient
    top = 8 * tv.P - 1
    for k in range(4):
        assert any(tv.val(r.ins[k]) == top and all(tv.val(r.ins[j]) == 0 for j in range(4) if j != k)
                   for r in kv.records("fp2x_mul")), k
    assert any(max(r.ins[0]) >= 1 << 28 for r in kv.records("fp2x_mul"))
    # g2c: live and off groups share blocks in the interleaved order; whole blocks are off in the grouped one
    for name in ("g2c_dbl", "g2c_add", "g2c_mul_zabs"):
        recs = kv.records(name)
        inter, grouped = kv.launch_orders(name)
        blocks = [[recs[i].cls == "off" for i in inter[b:b + 4]] for b in range(0, len(inter), 4)]
        assert sum(any(b) and not all(b) for b in blocks) >= 10, name
        blocks = [[recs[i].cls == "off" for i in grouped[b:b + 4]] for b in range(0, len(grouped), 4)]
        assert any(all(b) for b in blocks), name
        assert any(r.cls == "off" and all(x == 0xFFFFFFFF for l in r.ins[1:] for x in l) for r in recs), name
        # lane 0 takes the exceptional path while its neighbours take the regular one
        if name == "g2c_add":
            exc = {"P+P", "P-P", "inf+Q", "P+inf", "inf+inf"}
            assert {r.cls for r in recs} >= exc | {"generic", "off", "2p operands"}
            blocks = [[recs[i].cls for i in inter[b:b + 4]] for b in range(0, len(inter), 4)]
            assert sum(any(c in exc for c in b) and any(c == "generic" for c in b) for b in blocks) >= 10
    # the chain ops hit the exceptional branches inside the chain, with enough records to fill a wave of lane pairs
    for name in ("g2x_jac_mul_zabs", "g2c_mul_zabs"):
        n_exc = sum(r.cls == "order 13: -P+P, dbl inf, inf+P" for r in kv.records(name))
        assert n_exc >= kv.WAVE["pair"], (name, n_exc)
    # the squarings' lacc users: zero with 2p on one half of the coefficients only, beside the uniform zeros
    for name in ("g6_cyc_sqr", "gtw_cyc_sqr", "gtw_cyc_sqr D=A"):
        one_sided = [r for r in kv.records(name) if r.cls == "zero, one-sided 2p"]
        assert len(one_sided) == 12, name
        for r in one_sided:
            vals = [tv.val(l) for l in r.ins]
            assert vals.count(2 * tv.P) == 6 and all(v in (0, tv.P, 2 * tv.P) for v in vals) and r.want == [0] * 12


def test_coop_op_sizes_match_the_library_table():
    """blsgpu_debug_op's kCoopSizes rows (helpers.cpp) are the vectors' operand / result counts at 56 bytes per Fp
    value, so a short stride is refused on the host."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lodestar_amd", "csrc",
                            "helpers.cpp")).read()
    table = src[src.index("kCoopSizes[] ="):]
    table = table[:table.index("};")]
    rows = {int(a): (int(b), int(c)) for a, b, c in re.findall(r"\{(\d+),\s*(\d+),\s*(\d+)\}", table)}
    assert sorted(rows) == [op.code for op in kv.OPS]
    for op in kv.OPS:
        assert rows[op.code] == (56 * op.n_in, 56 * op.n_out), op.name
