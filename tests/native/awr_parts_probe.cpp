// Host probe of lodestar_amd/csrc/awr_parts.hpp and of hl::AwrParts (helper_layout.hpp; tests/test_awr_parts_host.py):
// HIP-free headers alone.  With -DAWR_PARTS_PROBE_MAIN it is a program that walks a few shapes (for a sanitizer build
// on the host).
#include "../../lodestar_amd/csrc/awr_parts.hpp"
#include "../../lodestar_amd/csrc/helper_layout.hpp"

#include <string.h>

namespace hl = helper_layout;

extern "C" {

uint32_t probe_chip_lanes() { return kAwrChipLanes; }
uint32_t probe_awr_lanes(uint32_t n_groups, uint32_t n_sets) { return awr_lanes(n_groups, n_sets); }

uint32_t probe_fold_lanes(uint32_t n_groups, uint32_t max_parts) { return awr_parts::fold_lanes(n_groups, max_parts); }

// out = (L, part_sets, n_parts, L_fold); part_first has room for max(n_groups, chip lanes) + 1 entries, group_part for
// n_groups + 1; both are written only for a split call.  Returns 1 when the call is split.
int probe_plan(uint32_t n_groups, const uint32_t* group_first, uint32_t* out, uint32_t* part_first,
               uint32_t* group_part) {
  const awr_parts::Plan p = awr_parts::plan(group_first, n_groups);
  out[0] = p.L, out[1] = p.part_sets, out[2] = p.n_parts, out[3] = p.L_fold;
  if (!p.split()) return p.part_first.empty() && p.group_part.empty() ? 0 : -1;
  if (p.part_first.size() != (size_t)p.n_parts + 1 || p.group_part.size() != (size_t)n_groups + 1) return -1;
  memcpy(part_first, p.part_first.data(), p.part_first.size() * 4);
  memcpy(group_part, p.group_part.data(), p.group_part.size() * 4);
  return 1;
}

// every field of hl::AwrParts, in declaration order; returns the field count
int probe_parts_layout(uint64_t G, uint64_t n_parts, uint64_t* out) {
  const hl::AwrParts l(G, n_parts);
  static_assert(sizeof l % sizeof(size_t) == 0 && sizeof(size_t) == sizeof(uint64_t), "size_t fields only");
  memcpy(out, &l, sizeof l);
  return (int)(sizeof l / sizeof(uint64_t));
}
// the d_work fields of hl::Awr and hl::Same that depend on the launched lanes: (w_tab, w_sum_pk, w_sum_sig,
// work_words) and (w_tab, w_tab_pk, w_sum_pk, w_sum_sig, work_words)
void probe_awr_work(uint64_t G, uint64_t n, uint64_t lanes, uint64_t* out) {
  const hl::Awr l(G, n, 96, true, 96, 192, lanes);
  out[0] = l.w_tab, out[1] = l.w_sum_pk, out[2] = l.w_sum_sig, out[3] = l.work_words;
}
void probe_same_work(uint64_t G, uint64_t n, uint64_t U, uint64_t lanes, uint64_t* out) {
  const hl::Same l(G, n, U, 96, true, lanes);
  out[0] = l.w_tab, out[1] = l.w_tab_pk, out[2] = l.w_sum_pk, out[3] = l.w_sum_sig, out[4] = l.work_words;
}
}

#ifdef AWR_PARTS_PROBE_MAIN
#include <stdio.h>
int main() {
  uint64_t sum = 0, lay[16];
  const std::vector<std::vector<uint32_t>> shapes = {
      {65}, {64}, {65, 1, 0, 130}, {}, {0}, {0, 0, 0}, {16384}, {1u << 20}, std::vector<uint32_t>(128, 128),
      std::vector<uint32_t>(1024, 65), std::vector<uint32_t>(1023, 65), std::vector<uint32_t>(70000, 1)};
  for (std::vector<uint32_t> sizes : shapes)
    for (uint32_t extra : {0u, 5u, 100u, 4096u}) {
      if (extra) sizes.push_back(extra);
      const uint32_t G = (uint32_t)sizes.size();
      std::vector<uint32_t> gf(G + 1, 0);
      for (uint32_t g = 0; g < G; g++) gf[g + 1] = gf[g] + sizes[g];
      if (gf[G] > 1u << 20) continue;
      std::vector<uint32_t> part_first((G > kAwrChipLanes ? G : kAwrChipLanes) + 1), group_part(G + 1);
      uint32_t out[4];
      const int split = probe_plan(G, gf.data(), out, part_first.data(), group_part.data());
      if (split < 0) return 1;
      sum += out[0] + out[1] + out[2] + (split ? part_first[out[2]] + group_part[G] : 0);
      sum += probe_parts_layout(G, out[2], lay) + lay[6];
    }
  printf("checksum %llu\n", (unsigned long long)sum);
  return 0;
}
#endif
