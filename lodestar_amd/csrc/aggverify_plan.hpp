// Host plan of blsgpu_aggregate_verify's Miller accumulation (helpers.cpp; k_aggverify.hip writes the items).  No HIP
// here: tests/native/aggverify_probe.cpp includes this header alone.
//
// A call has n pairs in J jobs.  Pair k is item k and job j's signature item -- the pair (-g1, sig_j), which sits in
// the job's accumulators like any other pair -- is item n + j, so a job of k pairs is k + 1 Miller items with shared
// squarings and one final exponentiation.  A planned job lists its pairs in order, then its signature item; the list
// is cut into chunks of <= k items through miller_plan::add_chunks, never across two jobs, and f_ranges holds each
// job's chunk range [f_ranges[2j], f_ranges[2j + 1]) for the product F_j.  The call plans every non-empty job before
// the device has decoded anything (planned == nullptr): the items of a job the device rejects are switched off by
// their include bytes and its accumulators stay 1.
#pragma once
#include <stdint.h>
#include <vector>

#include "miller_plan.hpp"

namespace aggverify_plan {

// Miller items up to which a call takes the cooperative forms: same_plan::kCoopMax (helpers.cpp asserts it)
constexpr uint32_t kCoopMax = 512;
// The message index's key (run_plan.hpp dedupe_messages).  The call draws no randomness, so it is a constant: the key
// only spreads the table's probes, equality is by memcmp.
constexpr uint64_t kMsgKey = 0xbb67ae8584caa73bull;
constexpr uint32_t kLaneChunk = 8;   // most items per accumulator in the lane form; the cooperative form has one
constexpr uint32_t kLaneReduceMax = 8;  // chunks per job, on average, up to which one lane multiplies a job's chunk values

// 0 = cooperative forms, 1 = lane forms for a call that plans n_items Miller items
inline uint32_t form(uint32_t n_items, bool lane_flag) { return lane_flag || n_items > kCoopMax ? 1u : 0u; }

inline bool is_planned(const uint32_t* job_first, uint32_t j, const uint8_t* planned) {
  return planned ? planned[j] != 0 : job_first[j + 1] > job_first[j];
}

// Miller items and chunks of the planned jobs with k items per chunk
struct Counts {
  uint32_t jobs, items, chunks;
};
inline Counts count(const uint32_t* job_first, uint32_t n_jobs, const uint8_t* planned, uint32_t k) {
  Counts c{0, 0, 0};
  for (uint32_t j = 0; j < n_jobs; j++) {
    if (!is_planned(job_first, j, planned)) continue;
    const uint32_t len = job_first[j + 1] - job_first[j] + 1;
    c.jobs++, c.items += len, c.chunks += miller_plan::group_chunks(len, k);
  }
  return c;
}

// Items per accumulator.  Cooperative form: 1 (a workgroup per item).  Lane form: one lane runs a chunk's 68 steps one
// after the other -- measured at ~2.7 ms for the shared squarings plus ~3.7 ms per item of the chunk --
// and the chip holds miller_plan::kFillLanes lanes at one wave per SIMD, so sharing an accumulator pays only once a
// lane per item no longer fits: the smallest of 1, 2, 4, 8 whose chunk count is within kFillLanes, else 8.  With
// lane_flag (BLSGPU_AV_LANE_FORMS, "the large-call forms whatever the size") always 8, the shape of the largest calls.
inline uint32_t chunk_items_for(const uint32_t* job_first, uint32_t n_jobs, uint32_t form, bool lane_flag) {
  if (!form) return 1;
  if (lane_flag) return kLaneChunk;
  for (uint32_t k : {1u, 2u, 4u})
    if (count(job_first, n_jobs, nullptr, k).chunks <= miller_plan::kFillLanes) return k;
  return kLaneChunk;
}

struct Plan {
  uint32_t n_pairs = 0, n_jobs = 0;
  std::vector<uint32_t> items;        // the item list: each planned job's pairs, then its signature item
  std::vector<uint32_t> chunk_first;  // [n_chunks + 1] into chunk_items
  std::vector<uint32_t> chunk_items;
  std::vector<uint32_t> f_ranges;     // [2 n_jobs]: job j's chunks (empty range for a job that is not planned)
  uint32_t n_chunks() const { return (uint32_t)chunk_first.size() - 1; }
};
inline Plan build(const uint32_t* job_first, uint32_t n_jobs, const uint8_t* planned, uint32_t k) {
  Plan p;
  p.n_jobs = n_jobs, p.n_pairs = job_first[n_jobs];
  p.chunk_first.push_back(0);
  p.f_ranges.resize(2 * (size_t)n_jobs);
  for (uint32_t j = 0; j < n_jobs; j++) {
    const uint32_t a = (uint32_t)p.items.size();
    if (is_planned(job_first, j, planned)) {
      for (uint32_t i = job_first[j]; i < job_first[j + 1]; i++) p.items.push_back(i);
      p.items.push_back(p.n_pairs + j);
    }
    const uint32_t e = (uint32_t)p.items.size();
    const auto r = miller_plan::add_chunks(p.chunk_first, p.chunk_items, a, e, k, false, p.items.data());
    p.f_ranges[2 * (size_t)j] = r.first, p.f_ranges[2 * (size_t)j + 1] = r.second;
  }
  return p;
}

// What a call decides before the device has decoded anything.  Every non-empty job is planned: which of them the
// device rejects is known only after the decodes, and their items are switched off by the include bytes (one
// synchronize less than reading the status back first).
struct CallPlan {
  Counts planned;
  bool lane, lane_reduce;  // the forms; one lane, not one wave, multiplies a job's chunk values (jobs of few chunks)
  uint32_t k, n_chunks;    // items per chunk, chunks
  Plan plan;
};
inline CallPlan plan_call(const uint32_t* job_first, uint32_t n_jobs, bool lane_flag) {
  CallPlan p;
  p.planned = count(job_first, n_jobs, nullptr, 1);
  p.lane = form(p.planned.items, lane_flag) != 0;
  p.k = chunk_items_for(job_first, n_jobs, p.lane ? 1 : 0, lane_flag);
  p.plan = build(job_first, n_jobs, nullptr, p.k);
  p.n_chunks = p.plan.n_chunks();
  p.lane_reduce = p.lane && (uint64_t)p.n_chunks <= (uint64_t)kLaneReduceMax * p.planned.jobs;
  return p;
}

}  // namespace aggverify_plan
