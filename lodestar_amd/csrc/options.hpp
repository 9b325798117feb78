// The runtime options: the Options snapshot a call takes, and ONE table with a row per member -- its key, how
// blsgpu_set_option checks and stores a value, and whether the member decides which calls may share a pipeline run
// (Options::same_run).  blsgpu_set_option, blsgpu_get_option (runtime.cpp) and the probes' setters
// (tests/native/run_plan_probe.cpp) are loops over the table; the keys that live on the context, and the read-only
// ones, are named below it, so this file lists every key.  No HIP here.
#pragma once
#include <stdint.h>
#include <string.h>

#ifndef MSM_SLICE  // sets per MSM slice (kernels.h has the same guarded default; a build may override both with -D)
#define MSM_SLICE 256
#endif

namespace blsgpu_rt __attribute__((visibility("hidden"))) {

struct Options {  // snapshot taken at the start of each call
  int64_t group_sets = 1024;
  int64_t max_devices = 64;
  int64_t profile = 0;
  int64_t dedupe = 1;
  int64_t miller_k = 0;  // pairings per Miller accumulator (shared squarings); 0 = by run size (miller_k_auto)
  int64_t merge_sets = 131072;  // queued calls a slot merges into one pipeline run (sets), 0 = never
  int64_t merge_wait_us = 2000;  // while runs are in flight, a slot waits this long for more calls to merge
  int64_t idle_wait_us = 0;  // on an idle device, a slot waits up to this long while calls keep arriving (bursts)
  int64_t pipeline_depth = 3;    // runs a device has in flight (taken by a slot, batch pass not yet complete)
  int64_t group_policy = 0;    // 0 = groups of >= group_sets sets; 1 = the reference pool's jobs / requests / chunks
  int64_t serial = 0;  // diagnostics: every branch of a run on one stream (each kernel alone on the chip)
  int64_t miller_segments = 0;  // diagnostics (BLSGPU_MILLER_SEGMENTS, read by blsgpu_init; no option key): step
                                // segments of the one-lane accumulation, 0 = by run size (miller_plan.hpp plan_auto)
  int64_t miller_lanes = 0;  // lanes per pairing of the one-item-chunk Miller accumulation: 0 = by run size, 1, 2
  int64_t f_run_max = 16;    // merged runs: longest lane-serial run of the F product tree before the cooperative pairs
  int64_t lane_tail_min = 0;  // runs of >= this many sets take the lane forms of the Horner passes and the groups'
                                  // MillerLoop(-g1, S) (0 = never)
  int64_t lane_tail_parts = 3;    // bit 0: Horner passes, bit 1: MillerLoop(-g1, S)
  int64_t msm_slice_mid = 32;     // MSM slice length of runs of 1k-32k sets
  int64_t lines_lanes = 2;        // lanes per message of the Miller lines (1, or 2 = lane pairs: fp2x.hpp)
  int64_t merge_balance = 0;      // a backlog above merge_sets is cut into equal runs
  int64_t early_release = 0;      // a run leaves the pipeline count when its message branch is done
  int64_t tail_on_msg = 0;        // the group stage runs on the pair's high-priority message stream
  int64_t copy_stream = 0;        // a run's input copy on the table stream (not behind the pair's previous tail)
  int64_t msm_tree = 1;           // those runs sum each range's slices by a pairwise tree
  int64_t coop_max = 512;         // runs of <= this many pairings take the cooperative Miller loops (k_miller_coop)
  int64_t coop_g2_max = 4096;     // runs of <= this many sets take the cooperative [|z|] chains (clearing, subgroup)
  int64_t coop_excl_max = 512;    // cooperative workgroups take a CU each only in runs of <= this many items
  int64_t rsig_spec = 1;          // small idle runs form every r_i sig_i beside the batch pass (for the fallback)
  int64_t spec_large = 1;         // runs above small_max on an idle device take the speculative MSM too
  int64_t spec_gsm = 0;           // a speculative run's MillerLoop(-g1, S) follows its MSM on the other pair's stream
  int64_t fb_lane_min = 256;      // fallback check launches of >= this many checks take one lane per check (0 = never)
  int64_t route_split_sets = 16384;  // a call is split over min(devices, sets / this) devices, else routed whole
  int64_t acc6_max = 16384;       // one-item-chunk runs of <= this many chunks take the six-lane accumulation
  int64_t miller_pairs = 0;       // larger runs: the lane-pair accumulation (k_miller_accx, two waves per SIMD)
  int64_t small_max = 4096;       // runs of <= this many sets are latency-first (speculation, cooperative fallback checks)
  int64_t fb_direct_min = 1024;   // large runs under load with >= this many retried jobs check each directly (0 = never)
  int64_t fb_check6 = 2;          // those runs' lane checks: 0 one lane per check; 1 MillerLoop(-g1, S) one lane and the
                                  // final exponentiation six lanes per check (gt6.hpp); 2 both on six lanes
  int64_t keep_f = 1;             // the fallback reuses the batch pass's per-set Miller values (0: re-runs the loops)
  int64_t keep_copy = 0;          // how they are copied aside: 0 hipMemcpyAsync, 1 a copy kernel on the same stream
  int64_t fb_force_busy = 0;      // tests: every run's fallback takes the under-load forms
  int64_t urgent_lane = 1;        // calls with a BLSGPU_JOB_URGENT job run on the device's urgent lane
  int64_t urgent_max_sets = 512;  // larger urgent calls go to the head of the device queue instead
  int64_t urgent_excl = 0;        // urgent runs may use the exclusive-CU padding of the cooperative kernels
  int64_t urgent_wait_us = 300;   // the urgent dispatcher lingers this long for more urgent calls of a burst
  int64_t group_adapt = 1;        // batch groups shrink below group_sets while the device sees invalid sets (DESIGN
                                  // §5.2: safe once outgrown buffers stay allocated, DevBuf::ensure)
  // May a call with these options share a pipeline run with one that has `o`?  (Every row of the table marked run.)
  inline bool same_run(const Options& o) const;
};

// How blsgpu_set_option checks a value: a flag takes any value and stores value != 0; a range takes lo <= value <= hi;
// `lanes` one of {0, 1, 2, 3, 6}; `pow2` a power of two in [lo, hi].  A refused value changes nothing.
struct OptCheck {
  enum Kind { flag, range, lanes, pow2 } kind;
  int64_t lo, hi;
};
constexpr OptCheck kFlag{OptCheck::flag, 0, 1}, kLanes{OptCheck::lanes, 0, 6};
constexpr OptCheck in_range(int64_t lo, int64_t hi) { return {OptCheck::range, lo, hi}; }
constexpr OptCheck at_least(int64_t lo) { return {OptCheck::range, lo, INT64_MAX}; }
constexpr OptCheck pow2_in(int64_t lo, int64_t hi) { return {OptCheck::pow2, lo, hi}; }

struct OptionRow {
  const char* key;
  int64_t Options::*member;
  OptCheck check;
  bool run;         // takes part in same_run: calls that differ here never merge
  bool abi = true;  // a key of blsgpu_set_option / blsgpu_get_option (false: set by blsgpu_init and the probes only)
};
constexpr bool kRun = true, kAnyRun = false;  // kAnyRun: read before a run forms (routing, merging, the urgent lane)
#define OPT_ROW(name, ...) {#name, &Options::name, __VA_ARGS__}
constexpr OptionRow kOptionRows[] = {
    OPT_ROW(group_sets, at_least(1), kRun),
    OPT_ROW(max_devices, at_least(1), kAnyRun),
    OPT_ROW(profile, kFlag, kRun),
    OPT_ROW(dedupe, kFlag, kRun),
    OPT_ROW(miller_k, in_range(0, 64), kRun),
    OPT_ROW(merge_sets, at_least(0), kAnyRun),
    OPT_ROW(merge_wait_us, in_range(0, 1000000), kAnyRun),
    OPT_ROW(idle_wait_us, in_range(0, 1000000), kAnyRun),
    OPT_ROW(pipeline_depth, in_range(1, 64), kAnyRun),
    OPT_ROW(group_policy, in_range(0, 1), kRun),
    OPT_ROW(serial, kFlag, kRun),
    OPT_ROW(miller_segments, at_least(0), kRun, false),
    OPT_ROW(miller_lanes, kLanes, kRun),
    OPT_ROW(f_run_max, pow2_in(1, 1024), kRun),
    OPT_ROW(lane_tail_min, at_least(0), kRun),
    OPT_ROW(lane_tail_parts, in_range(0, 3), kRun),
    OPT_ROW(msm_slice_mid, in_range(8, MSM_SLICE), kRun),
    OPT_ROW(lines_lanes, in_range(1, 2), kRun),
    OPT_ROW(merge_balance, kFlag, kRun),
    OPT_ROW(early_release, kFlag, kRun),
    OPT_ROW(tail_on_msg, kFlag, kRun),
    OPT_ROW(copy_stream, kFlag, kRun),
    OPT_ROW(msm_tree, kFlag, kRun),
    OPT_ROW(coop_max, in_range(0, 1 << 24), kRun),
    OPT_ROW(coop_g2_max, in_range(0, 1 << 24), kRun),
    OPT_ROW(coop_excl_max, in_range(0, 1 << 24), kRun),
    OPT_ROW(rsig_spec, kFlag, kRun),
    OPT_ROW(spec_large, kFlag, kRun),
    OPT_ROW(spec_gsm, kFlag, kRun),
    OPT_ROW(fb_lane_min, at_least(0), kRun),
    OPT_ROW(route_split_sets, at_least(1), kAnyRun),
    OPT_ROW(acc6_max, at_least(0), kRun),
    OPT_ROW(miller_pairs, in_range(0, 1), kRun),
    OPT_ROW(small_max, at_least(0), kRun),
    OPT_ROW(fb_direct_min, at_least(0), kRun),
    OPT_ROW(fb_check6, in_range(0, 2), kRun),
    OPT_ROW(keep_f, kFlag, kRun),
    OPT_ROW(keep_copy, kFlag, kRun),
    OPT_ROW(fb_force_busy, kFlag, kRun),
    OPT_ROW(urgent_lane, kFlag, kAnyRun),
    OPT_ROW(urgent_max_sets, at_least(0), kAnyRun),
    OPT_ROW(urgent_excl, kFlag, kAnyRun),  // (the plan reads it, Forms::excl: an open question)
    OPT_ROW(urgent_wait_us, in_range(0, 100000), kAnyRun),
    OPT_ROW(group_adapt, kFlag, kRun),
};
#undef OPT_ROW
static_assert(sizeof(Options) == sizeof kOptionRows / sizeof kOptionRows[0] * sizeof(int64_t), "a row per member");

// The row of `key`; with abi_only, only a key of the ABI.  nullptr: no such option.
inline const OptionRow* find_option(const char* key, bool abi_only) {
  for (const OptionRow& r : kOptionRows)
    if ((r.abi || !abi_only) && strcmp(r.key, key) == 0) return &r;
  return nullptr;
}

// Stores `value` as blsgpu_set_option does; false = refused (out of range), nothing changed.
inline bool store_option(Options& o, const OptionRow& r, int64_t value) {
  const OptCheck& c = r.check;
  if (c.kind == OptCheck::flag) value = value != 0;
  else if (value < c.lo || value > c.hi) return false;
  else if (c.kind == OptCheck::lanes && (value == 4 || value == 5)) return false;
  else if (c.kind == OptCheck::pow2 && (value & (value - 1))) return false;
  o.*r.member = value;
  return true;
}

inline bool Options::same_run(const Options& o) const {
  for (const OptionRow& r : kOptionRows)
    if (r.run && this->*r.member != o.*r.member) return false;
  return true;
}

// The keys outside the table, handled by name in runtime.cpp: those that live on the context (blsgpu_ctx, with their
// own locks; all but slots before the first call only), then the read-only ones.
enum class CtxKey { slots, urgent_cus, urgent_isolate, blocking_sync, pipeline_prio, hw_queues, abi_version,
                    spurious_groups, none };
constexpr const char* kCtxKeys[] = {"slots",         "urgent_cus", "urgent_isolate", "blocking_sync",
                                    "pipeline_prio", "hw_queues",  "abi_version",    "spurious_groups"};
constexpr int kCtxKeysSettable = 5;  // the first five; the rest are read-only
static_assert(sizeof kCtxKeys / sizeof kCtxKeys[0] == (size_t)CtxKey::none, "a name per key");
inline CtxKey ctx_key(const char* key) {
  for (int i = 0; i < (int)CtxKey::none; i++)
    if (strcmp(kCtxKeys[i], key) == 0) return (CtxKey)i;
  return CtxKey::none;
}

}  // namespace blsgpu_rt
