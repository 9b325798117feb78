// Host probe of lodestar_amd/csrc/miller_plan.hpp (tests/test_miller_plan.py): the header alone, no HIP.
#include "../../lodestar_amd/csrc/miller_plan.hpp"

namespace mp = miller_plan;

extern "C" {

int probe_is_doubling(uint32_t s) { return mp::is_doubling_step(s) ? 1 : 0; }

// first[0 .. J], dbl[0 .. J); returns the segment count
int probe_segments(uint32_t J, uint32_t* first, uint32_t* dbl) {
  const mp::Segments sg = mp::segments(J);
  for (uint32_t j = 0; j <= sg.n; j++) first[j] = sg.first[j];
  for (uint32_t j = 0; j < sg.n; j++) dbl[j] = sg.dbl[j];
  return (int)sg.n;
}

uint64_t probe_count_chunks(const uint32_t* group_len, uint64_t n_groups, uint32_t k) {
  return mp::count_chunks(group_len, n_groups, k);
}

uint32_t probe_fit(uint64_t n_chunks, uint32_t want, uint64_t capacity) { return mp::fit_segments(n_chunks, want, capacity); }

int probe_allowed(uint64_t n_items, uint64_t n_chunks, uint32_t k, uint32_t J, uint64_t capacity) {
  return mp::pair_allowed(n_items, n_chunks, k, J, capacity) ? 1 : 0;
}

int probe_hold(double fail_rate, double sets_per_group) { return mp::hold_kept_values(fail_rate, sets_per_group) ? 1 : 0; }

// out = (k, J)
void probe_plan(uint32_t n_items, const uint32_t* group_len, uint64_t n_groups, uint64_t capacity, int explicit_k,
                uint32_t k_today, uint32_t* out) {
  const mp::Plan p = mp::plan_auto(n_items, group_len, n_groups, capacity, explicit_k != 0, k_today);
  out[0] = p.k, out[1] = p.segs;
}

// chunks of the item range [a, e): first[0 .. n_chunks] (relative to items[0]) and the items; returns n_chunks
uint32_t probe_chunks(uint32_t a, uint32_t e, uint32_t k, int interleave, uint32_t* first, uint32_t* items) {
  std::vector<uint32_t> f{0}, it;
  const auto cr = mp::add_chunks(f, it, a, e, k, interleave != 0);
  for (size_t i = 0; i < f.size(); i++) first[i] = f[i];
  for (size_t i = 0; i < it.size(); i++) items[i] = it[i];
  return cr.second - cr.first;
}
}
