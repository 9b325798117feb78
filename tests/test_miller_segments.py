"""Step segments of the Miller accumulation, on the host from the device headers (CPU only).

tests/native/miller_segments.cpp computes a chunk's segment values the way k_miller_acc does (miller_acc_step over each
segment's step range from f = 1, the squaring of the first step skipped) and folds them by the Horner pass of k_f_fold
(pairing.hpp miller_seg_fold).  The fold must equal the product of miller_loop over the chunk's pairs, byte for byte in
canonical form: integer arithmetic, no tolerance."""
import ctypes
import hashlib
import os
import subprocess

import pytest

from oracle import bls12_381 as bls
from tests import emu_helpers as eh

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "miller_segments.cpp")
LIB = os.path.join(HERE, "native", "libmiller_segments.so")
CSRC = os.path.join(os.path.dirname(HERE), "lodestar_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    deps = [SRC] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hpp")]
    if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", LIB, SRC])
    return ctypes.CDLL(LIB)


@pytest.fixture(scope="module")
def pairs():
    """Three random (P, Q): P = sk g1, Q = H(m), from the oracle; 288 bytes each."""
    out = []
    for i in range(3):
        sk = int.from_bytes(hashlib.sha256(b"segments sk %d" % i).digest(), "big") % bls.R
        q = bls.hash_to_g2(hashlib.sha256(b"segments msg %d" % i).digest())
        out.append(eh.g1b(bls.sk_to_pk(sk)) + eh.g2b(q))
    return out


ONE = (1).to_bytes(48, "big") + bytes(11 * 48)


def run_chunk(lib, pairs, active, J):
    n = len(pairs)
    segs = ctypes.create_string_buffer(576 * J)
    fold = ctypes.create_string_buffer(576)
    ref = ctypes.create_string_buffer(576)
    assert lib.seg_chunk(b"".join(pairs), bytes(active), n, J, segs, fold, ref) == 0
    return [segs.raw[576 * j:576 * (j + 1)] for j in range(J)], fold.raw, ref.raw


@pytest.mark.parametrize("J", range(1, 9))
@pytest.mark.parametrize("n", [1, 2, 3])
def test_fold_equals_product_of_miller_loops(lib, pairs, n, J):
    segs, fold, ref = run_chunk(lib, pairs[:n], [1] * n, J)
    assert ref != ONE
    assert fold == ref
    if J > 1:
        assert len(set(segs)) == J and ONE not in segs  # every lane did its own share


@pytest.mark.parametrize("J", range(1, 9))
def test_one_item_by_miller_acc_step(lib, pairs, J):
    """The same through miller_acc_step's own squaring rule (step index relative to the segment's first step)."""
    fold = ctypes.create_string_buffer(576)
    assert lib.seg_single(pairs[1], J, fold) == 0
    assert fold.raw == run_chunk(lib, pairs[1:2], [1], 1)[2]


@pytest.mark.parametrize("J", range(1, 9))
def test_inactive_items(lib, pairs, J):
    segs, fold, ref = run_chunk(lib, pairs, [0, 0, 0], J)  # a chunk with no active item: every segment value is one
    assert segs == [ONE] * J and fold == ONE and ref == ONE
    segs, fold, ref = run_chunk(lib, pairs, [1, 0, 1], J)  # an excluded set between two included ones
    assert fold == ref == run_chunk(lib, [pairs[0], pairs[2]], [1, 1], 1)[2]


def test_reference_is_the_oracles_miller_loop(lib, pairs):
    """miller_loop of the device headers against the emulator's own entry (itself checked against the oracle)."""
    out = ctypes.create_string_buffer(576)
    eh.lib().emu_miller(pairs[0][:96], pairs[0][96:], out)
    assert out.raw == run_chunk(lib, pairs[:1], [1], 4)[1]
