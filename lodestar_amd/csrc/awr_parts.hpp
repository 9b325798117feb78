// How the segmented randomized sums of the same-message calls (k_awr.hip) are laid over the chip: the lanes per group
// (blsgpu_awr_lanes) and the cut of groups larger than their lanes can take at one go into parts (blsgpu_awr_parts).
// No HIP here: tests/native/awr_parts_probe.cpp includes this header alone and tests/test_awr_parts_host.py compares
// it with the rule restated in Python.
//
// A call has n sets in G groups of sizes size_g and L = awr_lanes(G, n) lanes per group; the kernels run one wave per
// SIMD, so the chip holds kAwrChipLanes lanes at a time.  A lane's time is its number of sets, so a group larger than
// L sets is bound by sets per lane while the rest of the chip idles.  The rule: with t the smallest integer >= 1 for
// which
//     sum over g of max(1, ceil(size_g / (L t))) L  <=  kAwrChipLanes,
// group g is cut into max(1, ceil(size_g / (L t))) consecutive parts of L t sets (the last one shorter; an empty group
// is one empty part), each part is summed as a group of its own on L lanes -- no lane takes more than t sets -- and a
// fold adds each group's parts (k_awr_fold).  The sum is non-increasing in t and one part per group satisfies it, so t
// is found by bisection.  A call with G L > kAwrChipLanes (the chip is full as it is), or one in which no group has
// more than L t sets, is not split: it runs as it always did.  A group's sum is the same point however it is cut.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

// the chip's lanes for kernels that run one wave per SIMD: 1,024 waves of 64
constexpr uint32_t kAwrChipLanes = 1024 * 64;

// Lanes per group of the segmented randomized sum (blsgpu_awr_lanes).  A set costs two scalar multiplications (~50
// point operations each), a combine level one Jacobian addition per sum, so -- unlike sig_agg_lanes -- a lane per set
// pays off from two sets on: the fewest lanes of 8, 16, 32, 64 that cover the mean group size (one lane for one-set
// groups), capped by the group count: the kernels run one wave per SIMD (the scaling takes the whole register file),
// so the chip holds 1,024 waves = 65,536 lanes at a time and lanes beyond that only queue: the most lanes of 64, 32,
// 16, 8 with n_groups * L <= 65,536, then one lane per group.  Non-increasing in n_groups for a given n_sets.
inline uint32_t awr_lanes(uint32_t n_groups, uint32_t n_sets) {
  if (n_groups == 0) return 1;
  const uint64_t n = n_groups, lanes = kAwrChipLanes;
  const uint32_t by_count = n * 64 <= lanes ? 64 : n * 32 <= lanes ? 32 : n * 16 <= lanes ? 16 : n * 8 <= lanes ? 8 : 1;
  const uint64_t mean = ((uint64_t)n_sets + n - 1) / n;
  const uint32_t by_size = mean <= 1 ? 1 : mean <= 8 ? 8 : mean <= 16 ? 16 : mean <= 32 ? 32 : 64;
  return by_count < by_size ? by_count : by_size;
}

// (hidden, as blsgpu_rt is: none of this reaches the library's dynamic symbol table)
namespace awr_parts __attribute__((visibility("hidden"))) {

// Lanes the parts of a call take when a part has at most `part_sets` sets
inline uint64_t lanes_of(const uint32_t* group_first, uint32_t n_groups, uint32_t L, uint64_t part_sets) {
  uint64_t parts = 0;
  for (uint32_t g = 0; g < n_groups; g++) {
    const uint64_t size = group_first[g + 1] - group_first[g], p = (size + part_sets - 1) / part_sets;
    parts += p ? p : 1;
  }
  return parts * L;
}

// Lanes per group of the fold of a split call (k_awr_fold), a plain segmented sum of each group's parts: by the
// LARGEST group's parts -- one lane up to three parts (a combine level costs an addition, as in sig_agg_lanes), else the
// fewest lanes of 8, 16, 32, 64 that cover them -- so that no lane walks a large group's parts alone in a call of many
// small groups; capped by the group count as sig_agg_lanes caps its lanes (64 up to 1,024 groups, then 32, 16, 8 while
// n_groups * L <= twice the chip's lanes, then one lane per group): the fold's waves are short and may queue.
inline uint32_t fold_lanes(uint32_t n_groups, uint32_t max_parts) {
  if (n_groups == 0) return 1;
  const uint64_t n = n_groups, lanes = kAwrChipLanes;
  const uint32_t by_count = n * 64 <= lanes ? 64 : n * 32 <= 2 * lanes ? 32 : n * 16 <= 2 * lanes ? 16
                            : n * 8 <= 2 * lanes ? 8 : 1;
  const uint32_t by_size = max_parts <= 3 ? 1 : max_parts <= 8 ? 8 : max_parts <= 16 ? 16 : max_parts <= 32 ? 32 : 64;
  return by_count < by_size ? by_count : by_size;
}

// The cut of one call.  group_first: [n_groups + 1], non-decreasing from 0 (the caller has checked it).
struct Plan {
  uint32_t L = 1;          // awr_lanes(n_groups, n)
  uint32_t part_sets = 0;  // L t, or 0: the call is not split
  uint32_t n_parts = 0;    // n_groups when not split
  uint32_t L_fold = 1;     // split calls: fold_lanes(n_groups, the largest group's parts)
  // split calls only: the parts' first sets and n, [n_parts + 1]; group g's parts are [group_part[g],
  // group_part[g + 1]), [n_groups + 1]
  std::vector<uint32_t> part_first, group_part;
  bool split() const { return part_sets != 0; }
};
inline Plan plan(const uint32_t* group_first, uint32_t n_groups) {
  Plan p;
  p.n_parts = n_groups;
  if (n_groups == 0) return p;
  const uint32_t G = n_groups, L = p.L = awr_lanes(G, group_first[G]);
  if ((uint64_t)G * L > kAwrChipLanes) return p;
  uint32_t largest = 0;
  for (uint32_t g = 0; g < G; g++)
    if (group_first[g + 1] - group_first[g] > largest) largest = group_first[g + 1] - group_first[g];
  // the smallest t that fits: hi always fits (one part per group), lo - 1 never does
  uint64_t lo = 1, hi = ((uint64_t)largest + L - 1) / L;
  if (hi < 1) hi = 1;
  while (lo < hi) {
    const uint64_t mid = (lo + hi) / 2;
    if (lanes_of(group_first, G, L, mid * L) <= kAwrChipLanes)
      hi = mid;
    else
      lo = mid + 1;
  }
  const uint64_t part = lo * L;
  if (largest <= part) return p;
  p.part_sets = (uint32_t)part;
  p.L_fold = fold_lanes(G, (uint32_t)((largest + part - 1) / part));
  p.group_part.reserve((size_t)G + 1);
  for (uint32_t g = 0; g < G; g++) {
    p.group_part.push_back((uint32_t)p.part_first.size());
    const uint32_t first = group_first[g], last = group_first[g + 1];
    p.part_first.push_back(first);
    for (uint64_t k = (uint64_t)first + part; k < last; k += part) p.part_first.push_back((uint32_t)k);
  }
  p.n_parts = (uint32_t)p.part_first.size();
  p.group_part.push_back(p.n_parts);
  p.part_first.push_back(group_first[G]);
  return p;
}

}  // namespace awr_parts
