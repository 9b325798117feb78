"""Inputs and oracle answers shared by the compressed-upload tests (tests/test_pubkeys_compressed_host.py on the CPU,
tests/test_gpu_pubkeys_compressed*.py on the GPU).  Every expected value comes from the oracle: bls.g1_decompress /
g1_serialize / g1_compress, cpu.key_validate, cpu.sk_to_pk."""
import functools

from oracle import bls12_381 as bls
from oracle import cpu
from tests.test_gpu_parity import CACHED

NONE = 0xFFFFFFFF
INF48 = bytes([0xC0]) + bytes(47)
CACHED48 = [bytes.fromhex(p) for _, p in CACHED]
# the 199 candidates of test_gpu_parity.py::test_key_validate_classes_vs_oracle: x = t, either sign bit
SCAN = [bytes([0x80 | (t & 0x20)]) + bytes(45) + t.to_bytes(2, "big") for t in range(1, 200)]
# the identity, the infinity bit with another bit set, no compression bit, x >= p
SPECIAL = [INF48, bytes([0xE0]) + bytes(47), bytes(48), bytes([0x9F]) + bytes([0xFF]) * 47]


@functools.lru_cache(maxsize=None)
def valid_keys(n, first=1):
    """n valid keys, 48 bytes compressed: the oracle's sk_to_pk of secret keys first, first + 1, ..."""
    pk96 = cpu.sk_to_pk(b"".join((first + i).to_bytes(32, "big") for i in range(n)))
    return tuple(bls.g1_compress(bls.g1_deserialize(pk96[96 * i: 96 * i + 96])) for i in range(n))


@functools.lru_cache(maxsize=None)
def expected(pk48, validate):
    """(code, 96-byte uncompressed encoding or None) of one 48-byte key.  Trusted: the code of bls.g1_decompress, 6
    for the identity.  validate: cpu.key_validate."""
    try:
        pt = bls.g1_decompress(pk48)
        code = bls.BLST_PK_IS_INFINITY if pt is None else 0
    except bls.BlstError as e:
        pt, code = None, e.code
    if validate:
        code = cpu.key_validate(pk48)
    return code, (bls.g1_serialize(pt) if code == 0 else None)


@functools.lru_cache(maxsize=None)
def class_examples():
    """One key per error class, from the scan: {code: key}, with POINT_NOT_IN_GROUP an on-curve key outside G1."""
    out = {bls.BLST_BAD_ENCODING: SPECIAL[2], bls.BLST_PK_IS_INFINITY: INF48}
    for c in SCAN:
        code = expected(c, True)[0]
        if code in (bls.BLST_POINT_NOT_ON_CURVE, bls.BLST_POINT_NOT_IN_GROUP) and code not in out:
            out[code] = c
    assert len(out) == 4
    return out
