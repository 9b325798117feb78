"""blsgpu_pubkeys_upload_compressed / blsgpu_pubkeys_read on the GPU: the table filled from 48-byte
compressed keys holds what the oracle decompresses them to and what the 96-byte upload stores, rejected keys are
reported per key with nothing written, and the rows read back as 96- or 48-byte encodings.  The kernels run one lane per
key in 64-lane workgroups: the shapes are n = 1, 63, 64, 65, 130.  Expected values come from the oracle alone
(tests/pubkeys_compressed_helpers.py)."""
import json
import os

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import cpu
from tests.pubkeys_compressed_helpers import NONE, class_examples, expected, valid_keys

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FX = json.load(open(os.path.join(ROOT, "tests", "golden", "verify_sets.json")))
SHAPES = [1, 63, 64, 65, 130]


@pytest.fixture()
def ctx():
    from lodestar_amd.native import Context

    c = Context([0])
    yield c
    c.close()


def pk96_of(keys):
    return b"".join(expected(k, False)[1] for k in keys)


@pytest.mark.parametrize("validate", [False, True])
@pytest.mark.parametrize("n", SHAPES)
def test_upload_and_read(ctx, n, validate):
    keys = valid_keys(130)[:n]
    st, first_bad = ctx.upload_pubkeys_compressed(0, b"".join(keys), validate=validate)
    assert first_bad == NONE and len(st) == n and not st.any()
    assert ctx.pubkeys_count == n
    assert ctx.read_pubkeys(0, n, 96) == pk96_of(keys)
    assert ctx.read_pubkeys(0, n, 48) == b"".join(keys)
    assert ctx.read_pubkeys(0, 0, 96) == b"" and ctx.read_pubkeys(n, 0, 48) == b""


def test_read_crossing_a_workgroup_from_a_non_zero_first(ctx):
    keys = valid_keys(130)
    ctx.upload_pubkeys_compressed(0, b"".join(keys))
    for first, m in [(3, 70), (60, 10), (63, 2), (64, 66), (129, 1)]:
        assert ctx.read_pubkeys(first, m, 96) == pk96_of(keys[first: first + m])
        assert ctx.read_pubkeys(first, m, 48) == b"".join(keys[first: first + m])


def test_same_table_as_the_96_byte_path():
    """The golden keys compressed by the oracle: the golden cases in table mode answer as the fixture says, and
    aggregate_pubkeys over table indices equals the same call on a context filled by upload_pubkeys(96)."""
    from lodestar_amd.native import Context

    pk96 = [bytes.fromhex(k["pk"]) for k in FX["keys"]]
    pk48 = [bls.g1_compress(bls.g1_deserialize(p)) for p in pk96]
    a, b = Context([0]), Context([0])
    try:
        st, first_bad = a.upload_pubkeys_compressed(0, b"".join(pk48))
        assert first_bad == NONE and not st.any()
        b.upload_pubkeys(0, b"".join(pk96))
        assert a.pubkeys_count == b.pubkeys_count == len(pk96)
        assert a.read_pubkeys(0, len(pk96), 96) == b.read_pubkeys(0, len(pk96), 96) == b"".join(pk96)
        for c in FX["cases"]:
            jfs, order = [0], []
            for j in c["jobs"]:
                order += j
                jfs.append(len(order))
            sets = [FX["sets"][k] for k in order]
            sigs = [bytes.fromhex(s["sig"]) for s in sets]
            spf, idx = [0], []
            for s in sets:
                idx += s["pks"]
                spf.append(len(idx))
            res, _ = a.verify_raw(jfs, b"".join(s.ljust(192, b"\0")[:192] for s in sigs), [len(s) for s in sigs],
                                  b"".join(bytes.fromhex(s["msg"]) for s in sets), set_pk_first=spf, pk_index=idx,
                                  job_flags=[int(c["batchable"])] * len(c["jobs"]), sig_stride=192)
            assert list(res) == c["expected"], c["name"]
        rng = np.random.default_rng(5)
        spf = np.cumsum([0] + [int(x) for x in rng.integers(1, 9, 40)])
        idx = rng.integers(0, len(pk96), int(spf[-1]))
        for out_len in (48, 96):
            got, gst = a.aggregate_pubkeys(set_pk_first=spf, pk_index=idx, out_len=out_len)
            want, wst = b.aggregate_pubkeys(set_pk_first=spf, pk_index=idx, out_len=out_len)
            assert got == want and list(gst) == list(wst)
    finally:
        a.close()
        b.close()


@pytest.mark.parametrize("validate", [False, True])
def test_error_classes(ctx, validate):
    """130 keys, one key of each class at lanes 0, 63, 64 and 129, every other key valid: per-key status as the oracle,
    the return value and first_bad name the lowest one, and the table is as before the call."""
    from lodestar_amd import native

    before = valid_keys(70, first=1000)
    ctx.upload_pubkeys_compressed(0, b"".join(before))
    ex = class_examples()
    keys = list(valid_keys(130))
    lanes = {0: bls.BLST_POINT_NOT_IN_GROUP, 63: bls.BLST_POINT_NOT_ON_CURVE, 64: bls.BLST_PK_IS_INFINITY,
             129: bls.BLST_BAD_ENCODING}
    for lane, code in lanes.items():
        keys[lane] = ex[code]
    want = [expected(k, validate)[0] for k in keys]
    assert [want[lane] for lane in lanes] == ([3, 2, 6, 1] if validate else [0, 2, 6, 1])
    assert sum(1 for w in want if w) == (4 if validate else 3)
    src = np.frombuffer(b"".join(keys), np.uint8)
    st, fb = np.full(130, 77, np.int8), np.full(1, 0x12345678, np.uint32)
    rc = native.load().blsgpu_pubkeys_upload_compressed(ctx.h, 0, src.ctypes.data, 130,
                                                        native.PK_VALIDATE if validate else 0, st.ctypes.data,
                                                        fb.ctypes.data)
    low = 0 if validate else 63
    assert st.tolist() == want
    assert rc == want[low] and int(fb[0]) == low
    st2, fb2 = ctx.upload_pubkeys_compressed(0, b"".join(keys), validate=validate)  # the binding reports the same
    assert st2.tolist() == want and fb2 == low
    assert ctx.pubkeys_count == 70
    assert ctx.read_pubkeys(0, 70, 48) == b"".join(before)
    assert ctx.read_pubkeys(0, 70, 96) == pk96_of(before)
    # status and first_bad are both optional
    assert native.load().blsgpu_pubkeys_upload_compressed(ctx.h, 0, src.ctypes.data, 130,
                                                          native.PK_VALIDATE if validate else 0, None, None) == want[low]
    assert ctx.pubkeys_count == 70


def test_trusted_upload_stores_a_key_outside_g1(ctx):
    off = class_examples()[bls.BLST_POINT_NOT_IN_GROUP]
    st, fb = ctx.upload_pubkeys_compressed(0, off)
    assert st.tolist() == [0] and fb == NONE and ctx.pubkeys_count == 1
    assert ctx.read_pubkeys(0, 1, 96) == bls.g1_serialize(bls.g1_decompress(off))
    assert ctx.read_pubkeys(0, 1, 48) == off
    st, fb = ctx.upload_pubkeys_compressed(1, off, validate=True)
    assert st.tolist() == [bls.BLST_POINT_NOT_IN_GROUP] and fb == 0 and ctx.pubkeys_count == 1


def test_extend_and_overwrite(ctx):
    keys, other = valid_keys(130), valid_keys(10, first=2000)
    ctx.upload_pubkeys_compressed(0, b"".join(keys[:65]))
    st, fb = ctx.upload_pubkeys_compressed(60, b"".join(other), validate=True)
    assert fb == NONE and not st.any() and ctx.pubkeys_count == 70
    assert ctx.read_pubkeys(0, 70, 48) == b"".join(keys[:60] + other)
    assert ctx.read_pubkeys(0, 70, 96) == pk96_of(keys[:60] + other)
    with pytest.raises(RuntimeError, match="BLSGPU_ERR_ARGS"):
        ctx.upload_pubkeys_compressed(71, keys[0])
    assert ctx.pubkeys_count == 70
    # rows written by the 96-byte upload read back as those bytes
    pk96 = pk96_of(keys[100:130])
    ctx.upload_pubkeys(65, pk96)
    assert ctx.pubkeys_count == 95
    assert ctx.read_pubkeys(65, 30, 96) == pk96
    assert ctx.read_pubkeys(65, 30, 48) == b"".join(keys[100:130])
    assert ctx.read_pubkeys(0, 65, 48) == b"".join(keys[:60] + other[:5])


def test_refusals(ctx):
    from lodestar_amd import native

    lib = native.load()
    keys = valid_keys(4)
    ctx.upload_pubkeys_compressed(0, b"".join(keys))
    src = np.frombuffer(b"".join(keys), np.uint8)
    st, fb = np.full(4, 77, np.int8), np.full(1, 0x12345678, np.uint32)
    for first, n, flags in [(0, 4, 2), (0, 4, 3), (0, 4, 0x80000000), (0, 0, 2), (6, 4, 0), (0xFFFFFFFE, 4, 0)]:
        rc = lib.blsgpu_pubkeys_upload_compressed(ctx.h, first, src.ctypes.data, n, flags, st.ctypes.data,
                                                  fb.ctypes.data)
        assert rc == native.ERR_ARGS, (first, n, flags)
    assert lib.blsgpu_pubkeys_upload_compressed(ctx.h, 0, None, 4, 0, st.ctypes.data, fb.ctypes.data) == native.ERR_ARGS
    assert (st == 77).all() and fb[0] == 0x12345678  # a refused call writes neither
    assert lib.blsgpu_pubkeys_upload_compressed(ctx.h, 9, None, 0, 0, None, None) == native.OK  # n == 0
    assert ctx.pubkeys_count == 4 and ctx.read_pubkeys(0, 4, 48) == b"".join(keys)
    out = np.full(5 * 96, 0x5A, np.uint8)
    for first, n, out_len in [(0, 5, 96), (4, 1, 48), (5, 1, 96), (0xFFFFFFFF, 2, 96), (0, 1, 0), (0, 1, 47), (0, 1, 97)]:
        assert lib.blsgpu_pubkeys_read(ctx.h, first, n, out.ctypes.data, out_len) == native.ERR_ARGS, (first, n, out_len)
    assert lib.blsgpu_pubkeys_read(ctx.h, 0, 1, None, 96) == native.ERR_ARGS
    assert (out == 0x5A).all()
    assert lib.blsgpu_pubkeys_read(ctx.h, 0, 0, None, 96) == native.OK


def test_two_replicas():
    """Context([0, 0]) with route_split_sets 1: a compressed upload, then a 4-job table-mode call of valid and invalid
    sets whose shards land on both replicas answers as the oracle."""
    from lodestar_amd.native import Context

    n = 4
    keys = valid_keys(n)
    sks = b"".join((1 + i).to_bytes(32, "big") for i in range(n))
    msgs = [bytes([0x30 + i]) * 32 for i in range(n)]
    sigs = cpu.sign(sks, b"".join(msgs))
    msgs[1], msgs[2] = msgs[2], msgs[1]  # jobs 1 and 2 sign another message: well-formed, invalid
    batch = dict(job_first_set=np.arange(n + 1), sigs=sigs, sig_len=[96] * n, msgs=b"".join(msgs),
                 set_pk_first=np.arange(n + 1), pk_index=[0, 1, 2, 3], job_flags=np.ones(n), sig_stride=96)
    table = cpu.Table(pk96_of(keys))
    want, _ = cpu.verify_jobs(table=table, **batch)
    table.close()
    assert list(want) == [1, 0, 0, 1]
    c = Context([0, 0])
    try:
        c.set_option("route_split_sets", 1)
        st, fb = c.upload_pubkeys_compressed(0, b"".join(keys))
        assert fb == NONE and not st.any() and c.pubkeys_count == n
        got, stats = c.verify_raw(**batch)
        assert list(got) == list(want)
        assert stats.devices_used == 2
    finally:
        c.close()


def test_api_functions(ctx):
    from lodestar_amd import api

    keys = list(valid_keys(65))
    api.upload_pubkeys_compressed(ctx, 0, keys)
    assert ctx.pubkeys_count == 65
    assert api.read_pubkeys(ctx, 0, 65) == [expected(k, False)[1] for k in keys]
    assert api.read_pubkeys(ctx, 60, 5, compressed=True) == keys[60:65]
    assert api.read_pubkeys(ctx, 3, 0) == []
    ex = class_examples()
    bad = keys[:10]
    bad[7], bad[9] = ex[bls.BLST_POINT_NOT_IN_GROUP], ex[bls.BLST_POINT_NOT_ON_CURVE]
    with pytest.raises(api.BlstError, match="BLST_ERROR: BLST_POINT_NOT_ON_CURVE") as e:
        api.upload_pubkeys_compressed(ctx, 65, bad)  # trusted: the key outside G1 passes, lane 9 is the first rejected
    assert e.value.code == bls.BLST_POINT_NOT_ON_CURVE and e.value.index == 65 + 9
    with pytest.raises(api.BlstError, match="BLST_ERROR: BLST_POINT_NOT_IN_GROUP") as e:
        api.upload_pubkeys_compressed(ctx, 65, bad, validate=True)
    assert e.value.code == bls.BLST_POINT_NOT_IN_GROUP and e.value.index == 65 + 7
    assert ctx.pubkeys_count == 65
    with pytest.raises(ValueError):
        api.upload_pubkeys_compressed(ctx, 0, [keys[0][:47]])
    with pytest.raises(RuntimeError, match="BLSGPU_ERR_ARGS"):
        api.read_pubkeys(ctx, 60, 6)
