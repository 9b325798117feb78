"""The options table (lodestar_amd/csrc/options.hpp), CPU only, through tests/native/run_plan_probe.cpp: what
blsgpu_set_option accepts, refuses and stores for every key of the table, which members keep two calls out of one
pipeline run (Options::same_run), and the defaults.  The expectations are written out here, not read from the
table: a row the test has no expectation for fails it."""
import pytest

from tests import run_plan_probe as rp

# any value is accepted, value != 0 is stored
FLAGS = ["profile", "dedupe", "serial", "copy_stream", "tail_on_msg", "early_release", "merge_balance", "msm_tree",
         "rsig_spec", "spec_large", "spec_gsm", "fb_force_busy", "keep_f", "keep_copy", "urgent_lane", "urgent_excl",
         "group_adapt"]
AT_LEAST = {"group_sets": 1, "max_devices": 1, "route_split_sets": 1, "merge_sets": 0, "fb_lane_min": 0,
            "urgent_max_sets": 0, "fb_direct_min": 0, "small_max": 0, "acc6_max": 0, "lane_tail_min": 0}
RANGES = {"miller_k": (0, 64), "group_policy": (0, 1), "miller_pairs": (0, 1), "merge_wait_us": (0, 1000000),
          "idle_wait_us": (0, 1000000), "pipeline_depth": (1, 64), "lines_lanes": (1, 2), "coop_max": (0, 1 << 24),
          "coop_g2_max": (0, 1 << 24), "coop_excl_max": (0, 1 << 24), "urgent_wait_us": (0, 100000),
          "fb_check6": (0, 2), "lane_tail_parts": (0, 3), "msm_slice_mid": (8, 256)}  # 256 = MSM_SLICE
SPECIAL = {"miller_lanes": ([0, 1, 2, 3, 6], [-1, 4, 5, 7, 8]),
           "f_run_max": ([1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024], [0, -1, -2, 3, 6, 12, 1023, 1025, 2048])}
NO_KEY = ["miller_segments"]  # a member without an ABI key: blsgpu_init sets it from the environment
NOT_IN_SAME_RUN = ["max_devices", "merge_sets", "merge_wait_us", "idle_wait_us", "pipeline_depth", "route_split_sets",
                   "urgent_lane", "urgent_max_sets", "urgent_excl", "urgent_wait_us"]
DEFAULTS = {
    "group_sets": 1024, "max_devices": 64, "profile": 0, "dedupe": 1, "miller_k": 0, "merge_sets": 131072,
    "merge_wait_us": 2000, "idle_wait_us": 0, "pipeline_depth": 3, "group_policy": 0, "serial": 0,
    "miller_segments": 0, "miller_lanes": 0, "f_run_max": 16, "lane_tail_min": 0, "lane_tail_parts": 3,
    "msm_slice_mid": 32, "lines_lanes": 2, "merge_balance": 0, "early_release": 0, "tail_on_msg": 0, "copy_stream": 0,
    "msm_tree": 1, "coop_max": 512, "coop_g2_max": 4096, "coop_excl_max": 512, "rsig_spec": 1, "spec_large": 1,
    "spec_gsm": 0, "fb_lane_min": 256, "route_split_sets": 16384, "acc6_max": 16384, "miller_pairs": 0,
    "small_max": 4096, "fb_direct_min": 1024, "fb_check6": 2, "keep_f": 1, "keep_copy": 0, "fb_force_busy": 0,
    "urgent_lane": 1, "urgent_max_sets": 512, "urgent_excl": 0, "urgent_wait_us": 300, "group_adapt": 1,
}
I64_MAX = (1 << 63) - 1
I64_MIN = -(1 << 63)


def _rows():
    return rp.option_rows()


def test_every_row_has_an_expectation_and_only_once():
    keys = [key for key, _, _, _ in _rows()]
    assert len(keys) == len(set(keys)) == 44
    expected = FLAGS + list(AT_LEAST) + list(RANGES) + list(SPECIAL) + NO_KEY
    assert len(expected) == len(set(expected))
    assert sorted(keys) == sorted(expected)
    assert sorted(key for key, abi, _, _ in _rows() if not abi) == NO_KEY
    assert set(NOT_IN_SAME_RUN) <= set(keys)
    context_keys, read_only = rp.extra_keys()
    assert context_keys == {"slots", "urgent_cus", "urgent_isolate", "blocking_sync", "pipeline_prio"}
    assert read_only == {"hw_queues", "abi_version", "spurious_groups"}
    assert not (context_keys | read_only) & set(keys)


def test_defaults():
    assert {key: d for key, _, _, d in _rows()} == DEFAULTS
    o = rp.Opts()
    assert {key: o[key] for key in DEFAULTS} == DEFAULTS


def _accepts(key, value, stored=None):
    o = rp.Opts()
    assert o.set_checked(key, value), (key, value)
    assert o[key] == (value if stored is None else stored), (key, value)


def _refuses(key, value):
    """A refused value leaves the old one in place (the default, and a value set before)."""
    o = rp.Opts()
    assert not o.set_checked(key, value), (key, value)
    assert o[key] == DEFAULTS[key], (key, value)


@pytest.mark.parametrize("key", FLAGS)
def test_flags_normalise(key):
    for value, stored in [(0, 0), (1, 1), (5, 1), (-1, 1), (I64_MAX, 1), (I64_MIN, 1)]:
        _accepts(key, value, stored)


@pytest.mark.parametrize("key", sorted(AT_LEAST))
def test_at_least(key):
    lo = AT_LEAST[key]
    for value in (lo, lo + 1, 1 << 40, I64_MAX):
        _accepts(key, value)
    for value in (lo - 1, -5, I64_MIN):
        _refuses(key, value)


@pytest.mark.parametrize("key", sorted(RANGES))
def test_ranges(key):
    lo, hi = RANGES[key]
    for value in (lo, hi, (lo + hi) // 2):
        _accepts(key, value)
    for value in (lo - 1, hi + 1, I64_MIN, I64_MAX):
        _refuses(key, value)


@pytest.mark.parametrize("key", sorted(SPECIAL))
def test_special_forms(key):
    good, bad = SPECIAL[key]
    for value in good:
        _accepts(key, value)
    for value in bad + [I64_MIN, I64_MAX]:
        _refuses(key, value)


def test_refused_value_keeps_the_one_set_before():
    o = rp.Opts()
    assert o.set_checked("miller_k", 7) and not o.set_checked("miller_k", 65) and o["miller_k"] == 7
    assert o.set_checked("f_run_max", 64) and not o.set_checked("f_run_max", 65) and o["f_run_max"] == 64
    assert o.set_checked("miller_lanes", 6) and not o.set_checked("miller_lanes", 5) and o["miller_lanes"] == 6


def test_unknown_and_keyless_names_are_refused():
    o = rp.Opts()
    for key in ("miller_segments", "no_such_option", "", "slots", "hw_queues", "Group_sets", "group_sets "):
        assert not o.set_checked(key, 1), key
    assert {key: o[key] for key in DEFAULTS} == DEFAULTS
    # the probe's raw setter reaches the keyless row, with no check
    assert rp.Opts(miller_segments=3)["miller_segments"] == 3
    assert rp.Opts(miller_k=1000)["miller_k"] == 1000


@pytest.mark.parametrize("key", sorted(DEFAULTS))
def test_same_run_reads_exactly_the_listed_members(key):
    """Changing one member from its default keeps two calls out of one run unless the member is read only before a
    run forms (routing, merging, the urgent lane)."""
    row = {k: run for k, _, run, _ in _rows()}
    a, b = rp.Opts(), rp.Opts(**{key: DEFAULTS[key] + 1})
    assert a.same_run(a) and b.same_run(b)
    assert a.same_run(b) == b.same_run(a) == (key in NOT_IN_SAME_RUN)
    assert row[key] == (key not in NOT_IN_SAME_RUN)
