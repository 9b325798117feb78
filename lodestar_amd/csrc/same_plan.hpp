// Host decisions of the same-message verification calls (helpers.cpp verify_same_message; k_same.hip is the device
// side).  No HIP here: tests/native/same_plan_probe.cpp includes this header alone and tests/test_same_plan.py compares
// every function with the rules below restated in Python.
//
// A call has n sets in G groups and runs up to five phases: group, block (BLSGPU_SAME_BLOCK_CHECK), descent, retry and
// aggregate.  The host decides three things.  The form of each phase: a phase of at most kCoopMax pairings takes the
// cooperative kernels (a workgroup per Miller loop and per check: latency), a larger one the lane forms (throughput).
// After the block phase, which groups the descent checks one by one: the included groups of every block whose check
// failed, except that a failed block with a single included group has its answer already (that group failed).  After
// the group verdicts, which sets the retry phase verifies on their own: every set of each non-empty group whose
// result is not 1, with the group's message index.  The last two are pure functions of a few byte arrays read back
// from the device, so they are tested here and not only through the GPU.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/blsgpu.h"

// (hidden, as blsgpu_rt is: none of this reaches the library's dynamic symbol table)
namespace same_plan __attribute__((visibility("hidden"))) {

// Pairings up to which a phase is cooperative: the coop_max option's default, taken as a constant because the helper
// calls read no option.  blsgpu_aggregate_verify's rule (aggverify_plan::kCoopMax) is the same number; helpers.cpp
// asserts that the two agree.
constexpr uint32_t kCoopMax = 512;
// BLSGPU_SAME_BLOCK_CHECK: groups per block, the group_sets option's default as a constant (kernels.h
// SAME_BLOCK_GROUPS; include/blsgpu.h documents it)
constexpr uint32_t kBlockGroups = 1024;

// blsgpu_same_message_stats.form (include/blsgpu.h)
constexpr uint32_t kFormGroupLane = 1;     // the group phase took the lane forms
constexpr uint32_t kFormRetryLane = 2;     // the retry phase did
constexpr uint32_t kFormBlocks = 4;        // the block phase ran
constexpr uint32_t kFormDescent = 8;       // some block failed and the per-group descent ran
constexpr uint32_t kFormDescentLane = 16;  // the descent's checks took the lane forms

// The message index's key: the same-message calls derive it from the call's hash key as plan_run does
// (run_plan.hpp); equality is by memcmp, the key only spreads the table's probes.
inline uint64_t msg_key(uint64_t hash_key) { return hash_key ^ 0x6a09e667f3bcc908ull; }

// blsgpu_same_message_form: 0 = cooperative forms, 1 = lane forms for a phase of n_items pairings
inline uint32_t form(uint32_t n_items, uint32_t flags) {
  return (flags & BLSGPU_SAME_LANE_FORMS) || n_items > kCoopMax ? 1u : 0u;
}

// blsgpu_same_message_blocks: no block without the flag, else ceil(n_groups / kBlockGroups)
inline uint32_t blocks(uint32_t n_groups, uint32_t flags) {
  return flags & BLSGPU_SAME_BLOCK_CHECK ? n_groups / kBlockGroups + (n_groups % kBlockGroups ? 1u : 0u) : 0u;
}

// The groups the descent checks individually, ascending.  Block b = groups [kBlockGroups b, min(n_groups,
// kBlockGroups (b + 1))) failed when any[b] (it has an included group) and not ok[b]; it lists its groups with
// include[g], or nothing when that is a single group.
inline std::vector<uint32_t> descent_list(uint32_t n_groups, uint32_t n_blocks, const uint8_t* any, const uint8_t* ok,
                                          const uint8_t* include) {
  std::vector<uint32_t> listed;
  for (uint32_t b = 0; b < n_blocks; b++) {
    if (!any[b] || ok[b]) continue;
    const uint64_t first = (uint64_t)b * kBlockGroups, end = first + kBlockGroups;
    const uint32_t last = end < n_groups ? (uint32_t)end : n_groups;
    const size_t before = listed.size();
    for (uint32_t g = (uint32_t)first; g < last; g++)
      if (include[g]) listed.push_back(g);
    if (listed.size() - before == 1) listed.pop_back();
  }
  return listed;
}

// The retry phase's sets: every set of each non-empty group whose result is not 1, ascending, and per listed set its
// group's message index (group_msg[g]).  Empty groups count as neither accepted nor retried.
struct Retry {
  std::vector<uint32_t> sets, msg;
  uint32_t groups_accepted = 0, groups_retried = 0;
};
inline Retry retry_list(const uint32_t* group_first, uint32_t n_groups, const int8_t* group_result,
                        const uint32_t* group_msg) {
  Retry r;
  for (uint32_t g = 0; g < n_groups; g++) {
    if (group_first[g + 1] == group_first[g]) continue;
    if (group_result[g] == 1) {
      r.groups_accepted++;
      continue;
    }
    r.groups_retried++;
    for (uint32_t k = group_first[g]; k < group_first[g + 1]; k++) {
      r.sets.push_back(k);
      r.msg.push_back(group_msg[g]);
    }
  }
  return r;
}

}  // namespace same_plan
