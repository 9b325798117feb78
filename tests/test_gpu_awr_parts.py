"""Same-message groups larger than their lanes take at one go (csrc/awr_parts.hpp, k_awr_fold in csrc/k_awr.hip): the
randomized sums of such a call run over parts of the groups and a fold adds each group's parts.  Every answer is
compared with the oracle as tests/test_gpu_same_message.py compares it (its helpers build the calls and the expected
values: P = sk_to_pk(sum r_k sk_k), S = sign(sum r_k sk_k, m) with r_k = r_of_word(words[k]) of the call's seed).

Each test first asserts through native.awr_parts that its shape is cut the way it intends.  The fold is a segmented sum
on awr_parts::fold_lanes(groups, the largest group's parts) lanes per group -- for one group what sig_agg_lanes gives
its parts -- and the shapes walk every form of it: one lane (two or three parts per group), the butterflies of 8 (four
parts), 16 (ten) and 32 lanes (eighteen) and the wave form with its LDS tree (65 parts, two of them on lane 0).
"""
import copy

import numpy as np
import pytest

from oracle import bls12_381 as bls
from oracle import cpu
from tests.emu_helpers import r_of_word
from tests.test_gpu_same_message import (INF96, NONE, SEED, THREADS, K, Set, bad_key, check, corrupted, ctx,  # noqa: F401
                                         expected, msg, oracle_same_message, run, sk32, world)

pytestmark = pytest.mark.gpu

LANE_FORMS, BLOCK_CHECK = 1, 4


def cut(sizes):
    """(L, part_sets, part_first as a list) of a call with these group sizes, by the library's own rule."""
    from lodestar_amd import native

    first = np.cumsum([0] + list(sizes))
    part_sets, part_first = native.awr_parts(first)
    return native.awr_lanes(len(sizes), int(first[-1])), part_sets, part_first.tolist()


def model_parts(sizes, part_sets):
    out, at = [], 0
    for s in sizes:
        out += [at + j for j in range(0, max(s, 1), part_sets)]
        at += s
    return out + [at]


def valid_groups(world, sizes, stride=7, wide_every=0):
    groups, k = [], 0
    for n in sizes:
        groups.append([world.valid((stride * (k + j) + 3) % K, wide=bool(wide_every) and (k + j) % wide_every == 1)
                       for j in range(n)])
        k += n
    return groups


# ------------------------------------------------------------------------------------------- 1 smallest splits
@pytest.mark.parametrize("sizes", [[65], [128], [129], [192], [65, 1, 0, 130]], ids=str)
def test_smallest_splits(ctx, world, sizes):
    """One wave per part and a fold of two or three parts per group; 65 leaves a one-set last part (the wave form
    skips its tree there, not in its neighbour).  Table mode with compressed outputs, bytes mode with uncompressed
    ones, the same bytes underneath."""
    L, part_sets, part_first = cut(sizes)
    assert (L, part_sets) == (64, 64) and part_first == model_parts(sizes, 64)
    assert len(part_first) - 1 == sum(max(1, -(-s // 64)) for s in sizes) > len(sizes)
    groups = valid_groups(world, sizes, wide_every=3)
    want = expected(world, groups)
    got_t, lanes = run(ctx, world, groups, table=True, out_pk_len=48, out_sig_len=96)
    assert lanes == 64
    check(got_t, want, 48, 96)
    got_b, _ = run(ctx, world, groups, table=False, out_pk_len=96, out_sig_len=192)
    check(got_b, want, 96, 192)


# ------------------------------------------------------------------------- 2 every lane form with a split group
@pytest.mark.parametrize("sizes,lanes", [([2] * 40 + [100], 8), ([10] * 20 + [100], 16), ([24] * 10 + [100], 32)],
                         ids=["L8", "L16", "L32"])
def test_lane_forms_with_a_split_group(ctx, world, sizes, lanes):
    L, part_sets, part_first = cut(sizes)
    assert (L, part_sets) == (lanes, lanes) and part_first == model_parts(sizes, lanes)
    assert len(part_first) - 1 == len(sizes) - 1 + -(-100 // lanes)
    groups = valid_groups(world, sizes, stride=5)
    got, used = run(ctx, world, groups, table=True, out_sig_len=96)
    assert used == lanes
    check(got, expected(world, groups), 96, 96)


def test_one_lane_form_with_a_split_group(ctx, world):
    """8,193 one-set groups and one of five: a lane per part, the five-set group as five parts folded by one lane.
    Every group's status, first_bad and P against the oracle; S for every 64th group and the last eight."""
    sizes = [1] * 8193 + [5]
    L, part_sets, part_first = cut(sizes)
    assert (L, part_sets) == (1, 1) and part_first == list(range(8199))
    groups = valid_groups(world, sizes, stride=5)
    n = len(sizes)
    want = expected(world, groups, want_sig=lambda g: g % 64 == 0 or g >= n - 8)
    got, used = run(ctx, world, groups, table=True, out_sig_len=96)
    assert used == 1
    check(got, want, 96, 96)


# --------------------------------------------------------------------------------------- 3 exceptional folds
def own(world):
    """A copy of the module's world a test may append keys to: the shared one stays as it was made."""
    w = copy.copy(world)
    w.sks, w.pk96, w.sig96, w._sig192 = list(world.sks), list(world.pk96), list(world.sig96), dict(world._sig192)
    return w


def extra_key(world, sk):
    """A key the test chose the secret of: appended to the test's own world (bytes mode only, the table holds the
    first K)."""
    sk %= bls.R
    assert sk != 0
    world.sks.append(sk)
    world.pk96.append(cpu.sk_to_pk(sk32(sk), threads=1)[:96])
    world.sig96.append(cpu.sign(sk32(sk), world.m, threads=1)[:96])
    return len(world.sks) - 1


def weighted(world, keys, at, words):
    """sum r_k sk_k over the sets at call positions at, at + 1, .. holding these keys"""
    return sum(r_of_word(int(words[at + j]), raw=True) * world.sks[k] for j, k in enumerate(keys)) % bls.R


def solve_last(world, keys, at, words, target):
    """The secret for the set after `keys` (call position at + len(keys)) that makes the weighted sum of them all
    equal `target`."""
    r = r_of_word(int(words[at + len(keys)]), raw=True) % bls.R
    return (target - weighted(world, keys, at, words)) * pow(r, -1, bls.R) % bls.R


def run_same(ctx, world, groups, msgs, flags=0, agg=False, include=None, table=False, seed=SEED):
    flat = [s for g in groups for s in g]
    first = np.cumsum([0] + [len(g) for g in groups])
    keys = dict(pk_index=[s.key for s in flat]) if table else \
        dict(pk_bytes=b"".join(s.pk if s.pk is not None else world.pk96[s.key] for s in flat))
    args = dict(sig_len=[len(s.sig) for s in flat], sig_stride=96, seed=seed, flags=flags, **keys)
    buf = b"".join(s.sig.ljust(96, b"\0") for s in flat)
    if agg:
        return ctx.verify_same_message_agg(first, b"".join(msgs), buf, include=include, out_sig_len=96, **args)
    return ctx.verify_same_message(first, b"".join(msgs), buf, **args)


@pytest.mark.parametrize("sign", [1, -1], ids=["equal", "opposite"])
def test_equal_and_opposite_part_sums(ctx, world, sign):
    """A 128-set group whose last key makes its second part's sum r_k sk_k equal to the first part's (the fold of
    both sums doubles) or opposite to it (both sums are the identity): the oracle's bytes, the identity encodings, and
    from verify_same_message a group that is not accepted on its sum when P is infinite, with every set right on its
    own in the retry."""
    from lodestar_amd import native

    world = own(world)
    assert cut([128]) == (64, 64, [0, 64, 128])
    words = native.randomness_words(128, SEED)
    a_keys, b_keys = list(range(64)), list(range(64, 127))
    last = extra_key(world, solve_last(world, b_keys, 64, words, sign * weighted(world, a_keys, 0, words)))
    group = [world.valid(k) for k in a_keys + b_keys + [last]]
    assert weighted(world, b_keys + [last], 64, words) == sign * weighted(world, a_keys, 0, words) % bls.R
    (p, s, st, fb), _ = run(ctx, world, [group], out_pk_len=96, out_sig_len=96)
    assert list(st) == [0] and list(fb) == [NONE]
    if sign == 1:
        want = expected(world, [group])
        check((p, s, st, fb), want, 96, 96)
        assert want[0][1] is not None and p[0][0] != 0x40
    else:
        assert p[0] == bytes([0x40]) + bytes(95) and s[0] == INF96
    res, gres, stats = run_same(ctx, world, [group], [world.m])
    assert list(res) == [1] * 128
    assert list(gres) == ([1] if sign == 1 else [0])
    assert (stats.groups_accepted, stats.groups_retried, stats.retry_sets) == ((1, 0, 0) if sign == 1 else (0, 1, 128))


def test_butterfly_fold_with_equal_opposite_and_identity_operands(ctx, world):
    """One group of 256 sets is four parts on an eight-lane butterfly: level 2 adds part 2 to part 0 and part 3 to
    part 1, level 1 the two results.  Part 2's sum equals part 0's (a doubling) and part 3's is the opposite of part
    1's (the identity, which level 1 then adds)."""
    from lodestar_amd import native

    world = own(world)
    assert cut([256]) == (64, 64, [0, 64, 128, 192, 256])
    assert native.sig_agg_lanes(1, 4) == 8
    words = native.randomness_words(256, SEED)
    keys = [(3 * j + 1) % K for j in range(256)]
    k2 = extra_key(world, solve_last(world, keys[128:191], 128, words, weighted(world, keys[:64], 0, words)))
    keys[191] = k2
    k3 = extra_key(world, solve_last(world, keys[192:255], 192, words, -weighted(world, keys[64:128], 64, words)))
    keys[255] = k3
    group = [world.valid(k) for k in keys]
    (p, s, st, fb), _ = run(ctx, world, [group], out_pk_len=96, out_sig_len=96)
    check((p, s, st, fb), expected(world, [group]), 96, 96)
    # and the whole is twice part 0
    twice = 2 * weighted(world, keys[:64], 0, words) % bls.R
    assert p[0] == cpu.sk_to_pk(sk32(twice), threads=1)[:96]


# n sets in one group, the fold's lanes, and the two pairs of parts (a, b), (c, d) the fold's FIRST level adds (lane
# t takes lane t + lanes / 2: parts lanes / 2 apart): part b's sum is made equal to lane a's, part d's opposite to lane
# c's.  4,160 sets are 65 parts: lane 0 of the wave form walks parts 0 and 64 before the tree.
WIDE = [(600, 16, (0, 8), (1, 9)), (1100, 32, (0, 16), (1, 17)), (4160, 64, (0, 32), (1, 33))]


@pytest.mark.parametrize("n,lanes,equal,opposite", WIDE, ids=["fold16", "fold32", "fold64"])
def test_wide_folds(ctx, world, n, lanes, equal, opposite):
    """One large group on the 16- and 32-lane butterflies and on the wave form (LDS tree, error slots, two parts on
    lane 0): the oracle's bytes for a group in which one first-level addition doubles and another gives the identity;
    then, with two rejected signatures, the lower index whichever lane and part holds it."""
    from lodestar_amd import native

    world = own(world)
    n_parts = -(-n // 64)
    assert cut([n]) == (64, 64, list(range(0, n, 64)) + [n])
    assert native.sig_agg_lanes(1, n_parts) == lanes  # the fold's lanes: one group, so its parts are the mean
    words = native.randomness_words(n, SEED)
    keys = [(3 * j + 1) % K for j in range(n)]

    def part(p):
        return range(64 * p, min(n, 64 * p + 64))

    def lane_sum(t):  # what lane t holds before the first level: parts t, t + lanes, ..
        return sum(weighted(world, [keys[k] for k in part(p)], 64 * p, words) for p in range(t, n_parts, lanes))

    for (a, b), sign in ((equal, 1), (opposite, -1)):
        assert b == a + lanes // 2 and b + lanes >= n_parts  # lane b holds part b alone
        ks = list(part(b))
        keys[ks[-1]] = extra_key(world, solve_last(world, [keys[k] for k in ks[:-1]], ks[0], words, sign * lane_sum(a)))
        assert lane_sum(b) % bls.R == sign * lane_sum(a) % bls.R != 0
    group = [world.valid(k) for k in keys]
    got, used = run(ctx, world, [group], out_pk_len=96, out_sig_len=96)
    assert used == 64
    check(got, expected(world, [group]), 96, 96)
    # a bad signature in the last part and another in an earlier one; then only the late one
    late, early = n - 3, 64 * equal[1] + 5
    bad = {j: corrupted(world, "not_in_group", keys[j] % K, (keys[j] + 1) % K) for j in (late, early)}
    for touched in ((late, early), (late,)):
        g = list(group)
        for j in touched:
            g[j] = bad[j]
        (p, s, st, fb), _ = run(ctx, world, [g], out_pk_len=96, out_sig_len=96)
        assert (int(st[0]), int(fb[0])) == (bls.BLST_POINT_NOT_IN_GROUP, min(touched))
        assert p[0] == bytes(96) and s[0] == bytes(96)


def test_skewed_call_folds_on_lanes(ctx, world):
    """Many one-set groups and one large group: the fold's lanes follow the largest group (here 13 parts: 16 lanes),
    not the mean, and the one-part groups ride through the butterfly untouched."""
    sizes = [1] * 60 + [100]
    L, part_sets, part_first = cut(sizes)
    assert (L, part_sets) == (8, 8) and len(part_first) - 1 == 60 + 13
    groups = valid_groups(world, sizes, stride=5)
    got, used = run(ctx, world, groups, table=True, out_sig_len=96)
    assert used == 8
    check(got, expected(world, groups), 96, 96)


def test_part_of_identity_signatures(ctx, world):
    """The second part holds identity signatures only: its S is the identity, its keys still count in P."""
    sizes = [128, 3]
    assert cut(sizes)[1:] == (64, [0, 64, 128, 131])
    groups = valid_groups(world, sizes)
    groups[0][64:] = [Set(s.key, INF96, []) for s in groups[0][64:]]
    want = expected(world, groups)
    got, _ = run(ctx, world, groups, table=True, out_sig_len=96)
    check(got, want, 96, 96)
    assert want[0][1] is not None and got[1][0] != INF96
    only = [[Set(s.key, INF96, []) for s in groups[0]]]  # every part's S is the identity
    (p, s, st, fb), _ = run(ctx, world, only, table=True, out_sig_len=96)
    assert list(st) == [0] and s[0] == INF96 and p[0] == got[0][0]


# ------------------------------------------------------------------------------------- 4 errors across parts
def test_first_error_across_parts(ctx, world):
    """A 192-set group (three parts) between two clean groups, one of them split too.  The group's error is its
    lowest rejected set wherever its part lies, the key's code when key and signature of that set are rejected; the
    other groups answer as without it."""
    sizes = [5, 192, 70]
    assert cut(sizes)[1:] == (64, [0, 5, 69, 133, 197, 261, 267])
    clean = valid_groups(world, sizes)
    at = 5  # the large group's first set

    def with_sets(changes):
        g = [list(x) for x in clean]
        for j, s in changes.items():
            g[1][j] = s
        return g

    def key_of(j):
        return clean[1][j].key

    bad_sig = {j: corrupted(world, "not_in_group", key_of(j), key_of(j + 1)) for j in (74, 131)}
    x_ge_p = corrupted(world, "x_ge_p", key_of(100), key_of(101))
    cases = {
        # a bad signature in the second part and another in the third
        "two signatures": (with_sets({74: bad_sig[74], 131: bad_sig[131]}), True, (bad_sig[74].code, at + 74)),
        # bytes mode: a bad key in a later part than a bad signature
        "key after signature": (with_sets({74: bad_sig[74], 150: bad_key(world, key_of(150), "off_curve")}), False,
                                (bad_sig[74].code, at + 74)),
        # bytes mode: a bad signature in a later part than a bad key
        "signature after key": (with_sets({131: bad_sig[131], 10: bad_key(world, key_of(10), "infinity")}), False,
                                (bls.BLST_PK_IS_INFINITY, at + 10)),
        # bytes mode: a bad key and a bad signature on the same set, in the second part
        "both on one set": (with_sets({100: bad_key(world, key_of(100), "off_curve")._replace(
            sig=x_ge_p.sig, terms=[], code=bls.BLST_BAD_ENCODING), 140: bad_sig[131]._replace(key=key_of(140))}), False,
            (bls.BLST_POINT_NOT_ON_CURVE, at + 100)),
    }
    assert bad_sig[74].code == bad_sig[131].code == bls.BLST_POINT_NOT_IN_GROUP and x_ge_p.code == bls.BLST_BAD_ENCODING
    want_clean = expected(world, clean)
    for name, (groups, table, err) in cases.items():
        want = expected(world, groups)
        assert want[1] == err, name
        assert want[0] == want_clean[0] and want[2] == want_clean[2], name
        modes = (True, False) if table else (False,)
        for t in modes:
            got, _ = run(ctx, world, groups, table=t, out_sig_len=96)
            check(got, want, 96, 96)


# ------------------------------------------------------------------------------------ 5 the verifying calls
@pytest.fixture(scope="module")
def verify_case(world):
    """[130, 3]: a split group signing world.m and a small one signing another message; the same call with set 70 (the
    first group's second part) signing the wrong message."""
    sizes = [130, 3]
    groups = valid_groups(world, sizes, stride=11)
    m1 = msg(1, b"parts")
    sigs1 = cpu.sign(b"".join(sk32(world.sks[s.key]) for s in groups[1]), m1 * 3, threads=THREADS)
    groups[1] = [Set(s.key, sigs1[96 * j: 96 * j + 96], [(world.sks[s.key], m1)]) for j, s in enumerate(groups[1])]
    wrong = [list(g) for g in groups]
    k70 = groups[0][70].key
    wrong[0][70] = Set(k70, cpu.sign(sk32(world.sks[k70]), m1, threads=1)[:96], [(world.sks[k70], m1)])

    def plain_sum(sets, m):
        return cpu.sign(sk32(sum(world.sks[s.key] for s in sets)), m, threads=1)[:96]

    return sizes, groups, wrong, [world.m, m1], plain_sum


@pytest.mark.parametrize("flags", [0, LANE_FORMS, BLOCK_CHECK], ids=["coop", "lane", "blocks"])
def test_verify_same_message_with_a_split_group(ctx, world, verify_case, flags):
    sizes, groups, wrong, msgs, plain_sum = verify_case
    assert cut(sizes) == (64, 64, [0, 64, 128, 130, 133])
    # all valid
    res, gres, stats = run_same(ctx, world, groups, msgs, flags, table=True)
    assert list(res) == [1] * 133 and list(gres) == [1, 1] and stats.retry_sets == 0
    res, gres, stats, out, cnt = run_same(ctx, world, groups, msgs, flags, agg=True)
    assert list(res) == [1] * 133 and list(gres) == [1, 1] and list(cnt) == [130, 3]
    assert out == [plain_sum(groups[0], msgs[0]), plain_sum(groups[1], msgs[1])]
    # set 70 signs another message: its group fails, the retry finds the set, the aggregate leaves it out
    keys = [s.key for s in wrong[0]]
    want0 = oracle_same_message(world, keys, [s.sig for s in wrong[0]], msgs[0])
    assert want0 == [j != 70 for j in range(130)]
    res, gres, stats = run_same(ctx, world, wrong, msgs, flags, table=True)
    assert [bool(r) for r in res[:130]] == want0 and list(res[130:]) == [1, 1, 1] and list(gres) == [0, 1]
    assert (stats.groups_accepted, stats.groups_retried, stats.retry_sets) == (1, 1, 130)
    include = np.ones(133, np.uint8)
    include[[5, 70, 131]] = 0
    res, gres, stats, out, cnt = run_same(ctx, world, wrong, msgs, flags, agg=True, include=include)
    assert [bool(r) for r in res[:130]] == want0 and list(gres) == [0, 1] and list(cnt) == [128, 2]
    assert out == [plain_sum([s for j, s in enumerate(wrong[0]) if j not in (5, 70)], msgs[0]),
                   plain_sum([groups[1][0], groups[1][2]], msgs[1])]


# ---------------------------------------------------------------------------------- 6 not split means untouched
@pytest.mark.parametrize("sizes", [[64] * 128, [1] * 300], ids=["128x64", "300x1"])
def test_calls_that_are_not_split(ctx, world, sizes):
    from lodestar_amd import native

    L, part_sets, part_first = cut(sizes)
    assert part_sets == 0 and part_first == np.cumsum([0] + sizes).tolist() and L == (64 if sizes[0] == 64 else 1)
    groups = valid_groups(world, sizes, stride=5)
    got, used = run(ctx, world, groups, table=True, out_sig_len=96)
    assert used == L == native.awr_lanes(len(sizes), sum(sizes))
    check(got, expected(world, groups), 96, 96)
