// Host plan of the Miller accumulation's chunks and step segments (run_plan.hpp plan_run; k_miller.hip k_miller_acc reads the
// boundaries).  No HIP here: tests/native/miller_plan_probe.cpp includes this header alone.
//
// The Miller value of a chunk is prod_s l_s^(2^D(s)) over the 68 steps, D(s) = the doubling steps after step s.  Cut
// the steps into J contiguous segments, each starting at a doubling step; lane (chunk c, segment j) runs the chunk
// loop over its own steps from f = 1 (skipping the squaring of its first step) and gives g_{c,j}.  With d_j the
// doubling steps of segment j and e_j = d_{j+1} + ... + d_{J-1},
//   F_group = prod_j (prod_c g_{c,j})^(2^(e_j)):  R = G_0;  R = R^(2^(d_j)) G_j for j = 1 .. J - 1  (k_group.hip k_f_fold)
// so a chunk's 63 squarings are spread over its J lanes instead of repeated, and a run of n items in chunks of k keeps
// J n / k lanes: k can be J times larger at the same lane count.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <utility>
#include <vector>

namespace miller_plan {

constexpr uint32_t kSteps = 68;                       // MILLER_STEPS (kernels.h; pipeline.cpp asserts that they agree)
constexpr uint32_t kDoublings = 63;                   // bits of |z| below its top bit
constexpr uint64_t kZAbs = 0xd201000000010000ull;     // |z| (bls_constants.hpp BLS_Z_ABS)
constexpr uint32_t kMaxSegments = 8;
constexpr uint32_t kFillLanes = 65536;                // every SIMD gets a wave: 1,024 one-wave workgroups

// step s of the kernels' schedule is a doubling step (with its line), else the addition step of the bit before it
inline bool is_doubling_step(uint32_t s) {
  int bit = 62;
  bool add_next = false, dbl = true;
  for (uint32_t t = 0; t <= s; t++) {
    dbl = !add_next;
    if (!add_next) {
      add_next = (kZAbs >> bit) & 1ull;
      bit--;
    } else {
      add_next = false;
    }
  }
  return dbl;
}

// Segment boundaries for J segments: first[0] = 0 < first[1] < ... < first[J] = 68, step counts as equal as the
// doubling-step rule allows (an ideal boundary on an addition step moves to the doubling step before it: at most one
// step off), and dbl[j] = the doubling steps of segment j (sum 63).
struct Segments {
  uint32_t n;
  uint32_t first[kMaxSegments + 1];
  uint32_t dbl[kMaxSegments];
};
inline Segments segments(uint32_t J) {
  Segments sg{};
  sg.n = std::min(std::max(J, 1u), kMaxSegments);
  for (uint32_t j = 0; j <= sg.n; j++) {
    uint32_t s = (kSteps * j + sg.n / 2) / sg.n;
    if (s < kSteps && !is_doubling_step(s)) s--;
    sg.first[j] = s;
  }
  for (uint32_t j = 0; j < sg.n; j++) {
    sg.dbl[j] = 0;
    for (uint32_t s = sg.first[j]; s < sg.first[j + 1]; s++) sg.dbl[j] += is_doubling_step(s) ? 1 : 0;
  }
  return sg;
}

// chunks of <= k items a group of len items makes
inline uint32_t group_chunks(uint32_t len, uint32_t k) { return (len + k - 1) / k; }
inline uint64_t count_chunks(const uint32_t* group_len, size_t n_groups, uint32_t k) {
  uint64_t c = 0;
  for (size_t g = 0; g < n_groups; g++) c += group_chunks(group_len[g], k);
  return c;
}

// the most segments <= want that keep n_chunks * J slots within f_chunk's capacity (>= 1: a chunk has its own slot)
inline uint32_t fit_segments(uint64_t n_chunks, uint32_t want, uint64_t capacity) {
  uint32_t J = std::min(std::max(want, 1u), kMaxSegments);
  while (J > 1 && n_chunks * J > capacity) J--;
  return J;
}

// The automatic (k, J) of a run that takes the one-lane or two-lane chunk forms with k_today items per chunk
// (run_plan.hpp miller_k_auto): below 65,536 items, or with miller_k set (explicit), (k_today, 1).  Otherwise k is the
// largest of 8, 4 for which some J <= k gives n_chunks J >= 65,536 lanes, and J the smallest such.  A pair is allowed
// only if its n_chunks J slots fit capacity (the slots of f_chunk; ragged last chunks make n_chunks more than n / k)
// and its chunks are at least half full on average (a run of tiny groups gains nothing from k: it keeps today's
// form); with no allowed pair that fills the chip the run keeps (k_today, 1).  k stops at 8: op_counts.json and the
// benchmark's pricing know chunks of 1, 2, 4 and 8.
struct Plan {
  uint32_t k, segs;
};
inline bool pair_allowed(uint64_t n_items, uint64_t n_chunks, uint32_t k, uint32_t J, uint64_t capacity) {
  return J >= 1 && J <= k && J <= kMaxSegments && n_chunks * J <= capacity && 2 * n_items >= n_chunks * k;
}
inline Plan plan_auto(uint32_t n_items, const uint32_t* group_len, size_t n_groups, uint64_t capacity, bool explicit_k,
                      uint32_t k_today) {
  if (explicit_k || n_items < kFillLanes) return {k_today, 1};
  for (uint32_t k : {8u, 4u}) {
    const uint64_t nc = count_chunks(group_len, n_groups, k);
    for (uint32_t J = 1; J <= k && J <= kMaxSegments; J++)
      if (nc * J >= kFillLanes) {  // the smallest J that fills the chip: a larger one only needs more slots
        if (pair_allowed(n_items, nc, k, J, capacity)) return {k, J};
        break;
      }
  }
  return {k_today, 1};
}

// A run of one-item chunks keeps every set's Miller value for the fallback (run_plan.hpp keep_f); chunks of k > 1 give
// that up, and a failed group's jobs re-run their Miller loops.  By op_counts.json the plan saves
// 4,348 x 1.12 - 2,740 = ~2,100 products per set (two-lane k = 1 against k = 8) and a re-run costs ~4,900, so the plan
// pays while fewer than ~0.43 of the sets sit in failing groups; a run holds on to one-item chunks from half that on:
// with invalid sets at rate f (the device's estimate, group_adapt) a group of g sets fails at rate 1 - (1 - f)^g.
inline bool hold_kept_values(double fail_rate, double sets_per_group) {
  if (!(fail_rate > 0)) return false;
  double ok = 1.0;  // (1 - f)^g by squaring: no <cmath> here
  double b = fail_rate >= 1 ? 0.0 : 1.0 - fail_rate;
  for (uint64_t e = sets_per_group < 1 ? 1 : (uint64_t)sets_per_group; e; e >>= 1, b *= b)
    if (e & 1) ok *= b;
  return 1.0 - ok >= 0.2;
}

// Splits items [a, e) of one group into chunks of <= k items: appends to first / items, returns [chunk_begin, end).
// interleave: chunk c of the group's nc chunks takes items a + c, a + c + nc, a + c + 2 nc, ... so the lanes of a wave
// (consecutive chunks) read consecutive line-table columns at every item iteration; else consecutive items per chunk.
inline std::pair<uint32_t, uint32_t> add_chunks(std::vector<uint32_t>& first, std::vector<uint32_t>& items, uint32_t a,
                                                uint32_t e, uint32_t k, bool interleave = false,
                                                const uint32_t* map = nullptr) {
  const uint32_t c0 = (uint32_t)first.size() - 1;
  if (interleave) {
    const uint32_t nc = group_chunks(e - a, k);
    for (uint32_t c = 0; c < nc; c++) {
      for (uint32_t y = a + c; y < e; y += nc) items.push_back(map ? map[y] : y);
      first.push_back((uint32_t)items.size());
    }
  } else {
    for (uint32_t x = a; x < e; x += k) {
      for (uint32_t y = x; y < std::min(e, x + k); y++) items.push_back(map ? map[y] : y);
      first.push_back((uint32_t)items.size());
    }
  }
  return {c0, (uint32_t)first.size() - 1};
}

}  // namespace miller_plan
