"""Shared by the AggregateVerify tests: a small world of interop keys and messages, and the reference answer of a job
composed from oracle/bls12_381.py alone.

Reference (include/blsgpu.h blsgpu_aggregate_verify): no pairs -> -9; the job's lowest-index rejected key -> -code and
its call index (KeyValidate with validate_keys, else g1_deserialize + an identity check); the signature through
signature_from_bytes -> -code; an identity signature -> 0; otherwise

    f12_is_one(final_exp(miller_loop(-g1, sig) * prod_k miller_loop(pk_k, hash_to_g2(m_k))))

miller_loop(pk, H(m)) is cached per (key bytes, message): a Miller loop costs ~30 ms in the Python oracle.  All
comparisons with the device are exact.
"""
import hashlib
from collections import namedtuple

from oracle import bls12_381 as bls
from oracle import cpu

THREADS = 16
K = 16  # interop keys
M = 16  # messages
NONE = 0xFFFFFFFF
INF96 = bytes([0xC0]) + bytes(95)
INF192 = bytes([0x40]) + bytes(191)
INF_PK48 = bytes([0xC0]) + bytes(47)

# pairs: [(key index, message index)]; sig: the job's signature bytes; keys: {position in the job: replacement key
# bytes} (bytes mode only)
Job = namedtuple("Job", "pairs sig keys", defaults=({},))


def sk32(x):
    return (x % bls.R).to_bytes(32, "big")


def msg(j, tag=b"aggregate-verify"):
    return hashlib.sha256(tag + j.to_bytes(4, "little")).digest()


class World:
    def __init__(self):
        self.sks = [bls.interop_secret_key(i) for i in range(K)]
        self.msgs = [msg(j) for j in range(M)]
        skb = b"".join(sk32(s) for s in self.sks)
        pk = cpu.sk_to_pk(skb, threads=THREADS)
        self.pk96 = [pk[96 * i: 96 * i + 96] for i in range(K)]
        self.pk48 = [bls.g1_compress(bls.g1_deserialize(p)) for p in self.pk96]
        # sk_i * H(m_j) for every (i, j), one oracle call
        sg = cpu.sign(b"".join(sk32(self.sks[i]) for i in range(K) for _ in range(M)), b"".join(self.msgs) * K,
                      threads=THREADS)
        self._sig96 = [[sg[96 * (M * i + j): 96 * (M * i + j) + 96] for j in range(M)] for i in range(K)]
        self._sig_pt, self._h, self._ml, self._key, self._job = {}, {}, {}, {}, {}

    def sig_point(self, i, j):
        if (i, j) not in self._sig_pt:
            self._sig_pt[(i, j)] = bls.signature_from_bytes(self._sig96[i][j], validate=False)
        return self._sig_pt[(i, j)]

    def sum_point(self, pairs):
        acc = None
        for i, j in pairs:
            acc = bls.g2_add(acc, self.sig_point(i, j))
        return acc

    def sign(self, pairs, wide=False):
        """The aggregate signature of the pairs: sum sk_i H(m_j), 96 bytes compressed (192 uncompressed when wide)."""
        pt = self.sum_point(pairs)
        return bls.g2_serialize(pt) if wide else bls.g2_compress(pt)

    def job(self, pairs, wide=False):
        return Job(list(pairs), self.sign(pairs, wide))

    def key_bytes(self, job, pos, pk_len=96):
        i = job.pairs[pos][0]
        return job.keys.get(pos, self.pk96[i] if pk_len == 96 else self.pk48[i])

    def h(self, j):
        if j not in self._h:
            self._h[j] = bls.hash_to_g2(self.msgs[j])
        return self._h[j]

    def key_point(self, kb, validate):
        """The key's affine point, or the code it is rejected with."""
        if (kb, validate) not in self._key:
            try:
                pt = bls.key_validate(kb) if validate else bls.g1_deserialize(kb)
                self._key[(kb, validate)] = pt if pt is not None else bls.BLST_PK_IS_INFINITY
            except bls.BlstError as e:
                self._key[(kb, validate)] = e.code
        return self._key[(kb, validate)]

    def miller(self, kb, pt, j):
        if (kb, j) not in self._ml:
            self._ml[(kb, j)] = bls.miller_loop(pt, self.h(j))
        return self._ml[(kb, j)]

    def expected(self, job, first, validate=False, pk_len=96):
        """(job_result, first_bad) of a job whose first pair has call index `first` (computed once per distinct job)."""
        key = (tuple(job.pairs), job.sig, tuple(sorted(job.keys.items())), validate, pk_len)
        if key not in self._job:
            self._job[key] = self._expected(job, validate, pk_len)
        res, pos = self._job[key]
        return res, (NONE if pos is None else first + pos)

    def _expected(self, job, validate, pk_len):
        """(job_result, position in the job of its rejected key or None)."""
        if not job.pairs:
            return -9, None
        pts = []
        for pos in range(len(job.pairs)):
            kb = self.key_bytes(job, pos, pk_len)
            pt = self.key_point(kb, validate)
            if isinstance(pt, int):
                return -pt, pos
            pts.append((kb, pt))
        try:
            sig = bls.signature_from_bytes(job.sig)
        except bls.BlstError as e:
            return -e.code, None
        if sig is None:
            return 0, None
        f = bls.miller_loop(bls.g1_neg(bls.G1_GEN), sig)
        for (kb, pt), (_, j) in zip(pts, job.pairs):
            f = bls.f12mul(f, self.miller(kb, pt, j))
        return (1 if bls.f12_is_one(bls.final_exp(f)) else 0), None


def call(ctx, world, jobs, table=False, flags=0, pk_len=96):
    """One Context.aggregate_verify call over the jobs: (job_result list, first_bad list, stats)."""
    stride = 192 if any(len(j.sig) > 96 for j in jobs) else 96
    first = [0]
    for j in jobs:
        first.append(first[-1] + len(j.pairs))
    buf = b"".join(j.sig[:stride].ljust(stride, b"\0") for j in jobs)
    msgs = b"".join(world.msgs[m] for j in jobs for _, m in j.pairs)
    if table:
        assert not any(j.keys for j in jobs)
        keys = dict(pk_index=[i for j in jobs for i, _ in j.pairs])
    else:
        keys = dict(pk_bytes=b"".join(world.key_bytes(j, p, pk_len) for j in jobs for p in range(len(j.pairs))),
                    pk_len=pk_len)
    res, fb, st = ctx.aggregate_verify(first, msgs, buf, sig_len=[len(j.sig) for j in jobs], sig_stride=stride,
                                       flags=flags, **keys)
    return [int(r) for r in res], [int(x) for x in fb], st


def expected_all(world, jobs, validate=False, pk_len=96):
    out, first = [], 0
    for j in jobs:
        out.append(world.expected(j, first, validate, pk_len))
        first += len(j.pairs)
    return [r for r, _ in out], [b for _, b in out]


_WORLD = []


def get_world():
    """The one World of the test process: its Miller-loop cache is shared by every AggregateVerify test module."""
    if not _WORLD:
        _WORLD.append(World())
    return _WORLD[0]
