// Host plan of one pipeline run (pipeline.cpp run_shard): everything a run decides on the host before and after its
// kernels, as plain arithmetic on the batch's arrays -- the batch groups, the message dedupe, the same-message units,
// the run's forms, Miller chunks and step segments, MSM slices, the F product tree, the device arenas, the sorting
// of the group verdicts, the fallback's lists and the pool policy's groups.  No HIP here:
// tests/native/run_plan_probe.cpp includes this header alone and tests/test_run_plan.py checks what the arrays mean.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <utility>
#include <vector>

#include "../../include/blsgpu.h"
#include "helper_layout.hpp"
#include "miller_plan.hpp"
#include "options.hpp"  // Options (the snapshot a call takes) and MSM_SLICE

namespace blsgpu_rt __attribute__((visibility("hidden"))) {

// words per element as kernels.h defines them (pipeline.cpp asserts that the two agree)
using helper_layout::Carve;
using helper_layout::kFp;
using helper_layout::kFp12;
using helper_layout::kG1A;
using helper_layout::kG1J;
using helper_layout::kG2A;
using helper_layout::kG2J;
using helper_layout::kMillerLineWords;
constexpr uint32_t kMsmSlice = MSM_SLICE;
constexpr size_t kMsmBucketWords = 128 * kG2J, kMsmWindowWords = 16 * kG2J;

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// One device's part of a call: contiguous jobs and their sets.
struct Shard {
  uint32_t job_begin, job_end;  // job range
  uint32_t set_begin, set_end;  // set range
  uint32_t dev = 0;             // device index (routing)
  int64_t cost = 0;             // routing cost, x256 (Device::load)
};

// pubkey mode of a batch: 0 table, 1 one key per set (bytes), 2 bytes aggregate
inline int pk_mode(const blsgpu_batch& b) { return !b.pk_bytes ? 0 : (b.set_pk_first ? 2 : 1); }

// ---- message deduplication: open addressing on the 32-byte signing roots ----------------------------------
struct MsgIndex {
  std::vector<uint32_t> slot;  // 1 + unique index, 0 = empty
  uint64_t key;
  explicit MsgIndex(uint32_t n, uint64_t k) : key(k) {
    size_t cap = 16;
    while (cap < (size_t)n * 2) cap <<= 1;
    slot.assign(cap, 0);
  }
  static uint64_t mix(uint64_t z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
  }
  size_t hash(const uint8_t* msgs, uint32_t i) const {
    uint64_t w[4];
    memcpy(w, msgs + (size_t)i * 32, 32);
    return (size_t)(mix(w[0] ^ key) ^ mix(w[1] + key) ^ w[2] ^ (w[3] << 1)) & (slot.size() - 1);
  }
  // returns the unique index of msg; appends to `uniq` (set indices of first occurrences) when new
  uint32_t find_or_add(const uint8_t* msgs, uint32_t i, std::vector<uint32_t>& uniq) {
    return find_or_add_h(msgs, i, hash(msgs, i), uniq);
  }
  uint32_t find_or_add_h(const uint8_t* msgs, uint32_t i, size_t h, std::vector<uint32_t>& uniq) {
    const size_t mask = slot.size() - 1;
    for (;;) {
      const uint32_t s = slot[h];
      if (!s) {
        uniq.push_back(i);
        slot[h] = (uint32_t)uniq.size();
        return (uint32_t)uniq.size() - 1;
      }
      if (memcmp(msgs + (size_t)uniq[s - 1] * 32, msgs + (size_t)i * 32, 32) == 0) return s - 1;
      h = (h + 1) & mask;
    }
  }
};

// The message index of n sets (ms: their 32-byte roots): msg_idx[i] = the unique index of set i's message, uniq[u] =
// the first set that signs unique message u.
inline void dedupe_messages(const uint8_t* ms, uint32_t n, uint64_t key, std::vector<uint32_t>& msg_idx,
                            std::vector<uint32_t>& uniq) {
  MsgIndex mi(n, key);
  msg_idx.resize(n);
  uniq.reserve(n);
  // hashes a few sets ahead, their table slots prefetched: the probes of a 131k-set run's 1 MB table were cache
  // misses one after another (~1.3-2.6 ms per run on the host)
  constexpr uint32_t kAhead = 16;
  size_t hq[kAhead];
  for (uint32_t i = 0; i < std::min(n, kAhead); i++) {
    hq[i] = mi.hash(ms, i);
    __builtin_prefetch(&mi.slot[hq[i]]);
  }
  for (uint32_t i = 0; i < n; i++) {
    const size_t h = hq[i % kAhead];
    if (i + kAhead < n) {
      hq[i % kAhead] = mi.hash(ms, i + kAhead);
      __builtin_prefetch(&mi.slot[hq[i % kAhead]]);
    }
    msg_idx[i] = mi.find_or_add_h(ms, i, h, uniq);
  }
}

// The same for a helper call (helpers.cpp): msg_idx as above; the value is the unique messages packed in that order.
inline std::vector<uint8_t> unique_messages(const uint8_t* ms, uint32_t n, uint64_t key, std::vector<uint32_t>& msg_idx) {
  std::vector<uint32_t> uniq;
  dedupe_messages(ms, n, key, msg_idx, uniq);
  std::vector<uint8_t> packed(uniq.size() * 32);
  for (size_t u = 0; u < uniq.size(); u++) memcpy(packed.data() + u * 32, ms + (size_t)uniq[u] * 32, 32);
  return packed;
}

// chunkifyMaximizeChunkSize (reference multithread/utils.ts:4-19): floor(len / min) chunks of ceil(len / count)
// items, or one chunk when that count is <= 1.  Returns the items per chunk.
inline uint32_t chunk_size(uint32_t len, uint32_t min_per_chunk) {
  const uint32_t count = min_per_chunk ? len / min_per_chunk : 0;
  return count <= 1 ? len : (len + count - 1) / count;
}

// A batch group: jobs [first, end) of the (shard-relative) job list; `batchable` = a chunk of batchable jobs (the
// reference's batch attempt, counted by the batchRetries / batchSigsSuccess metrics).
struct GroupPlanEntry {
  uint32_t first, end;
  bool batchable;
};

// Pairings per Miller accumulator when the option is 0: shared squarings save work (k = 4: 3,483 products per
// pairing vs 5,162 at k = 1, lodestar_amd/op_counts.json) but leave n / k lanes.  The accumulation is one wave per
// SIMD, so k doubles only while n / 2k still gives every SIMD a wave (>= 65,536 lanes = 1,024 waves): below that
// the stage would hold fewer SIMDs for longer on the run's critical path (r03c trace: k = 2 at 54k sets held 341
// waves for 14 ms).  This is the rule of whole-loop lanes (one segment): runs below 65,536 items, the fallback's own
// accumulations and every run the step-segment plan leaves alone.  From 65,536 items on, plan_run asks
// miller_plan::plan_auto for (k, J): J lanes per chunk, each over its own step range, keep the lane count of a J
// times smaller k, so such runs take k = 8 (or 4) at the lane count that stopped this rule at 1 or 2.
inline uint32_t miller_k_auto(uint32_t n_items) {
  uint32_t k = 1;
  while (k < 4 && n_items / (2 * k) >= 65536) k *= 2;
  return k;
}

// The Miller accumulation of a run's chunks: six lanes per chunk (k_miller_acc6) for runs of one-item chunks up to
// acc6_max chunks, two lanes (k_miller_acc2) for larger one-item-chunk runs while one lane per chunk would leave SIMDs
// idle (< 65,536 chunks = 1,024 waves), else one lane per chunk.
enum class AccForm { six, pairs, two, one };
inline AccForm acc_form(uint32_t mk, uint32_t n_chunks, int64_t lanes_opt, int64_t acc6_max, bool pairs) {
  if (lanes_opt == 6 || (lanes_opt == 0 && mk == 1 && (int64_t)n_chunks <= acc6_max)) return AccForm::six;
  // lane pairs, every Fp2 split (gtx.hpp): two waves per SIMD
  if (lanes_opt == 3 || (lanes_opt == 0 && pairs)) return AccForm::pairs;
  // two lanes per chunk: f never on one lane, no spills (r4zd/r4ze A/B, PMC r4f); auto: one-item chunks
  return lanes_opt == 2 || (lanes_opt == 0 && mk == 1) ? AccForm::two : AccForm::one;
}

// Splits set ranges into MSM slices of <= len (<= MSM_SLICE) sets: appends to slices (pairs), returns the range's
// [first slice, end slice)
inline void add_slices(std::vector<uint32_t>& slices, std::vector<uint32_t>& range_slices, uint32_t a, uint32_t e,
                       uint32_t len = kMsmSlice) {
  for (uint32_t x = a; x < e; x += len) {
    slices.push_back(x);
    slices.push_back(std::min<uint32_t>(e, x + len));
  }
  range_slices.push_back((uint32_t)(slices.size() / 2));
}

// Batch-group size for a run (group_adapt), f = the device's invalid-set rate estimate.  A group costs a fixed ~14.7k
// Montgomery multiplications (its MillerLoop(-g1, S) 5,747, final exponentiation 7,835, MSM range 1,085;
// lodestar_amd/op_counts.json), and when it fails
// every clean job in it is re-checked: per set 1.3k (the set's r_i sig_i; its Miller value is reused) plus its job's
// share of a sub-group check, ~13.6k per 16 jobs (the fallback's level 1, one final exponentiation per kFbSub jobs;
// only failing sub-groups check job by job).  With invalid sets at rate f a group of g sets fails with probability
// 1 - (1 - f)^g, so the expected cost per set is 14.7k / g + (1 - (1 - f)^g) * retry: the size that minimises it over
// powers of two in [8, group_sets].  All valid (f = 0): group_sets (1,024); the reference pool's 1% invalid gossip
// (C5, jobs of 1-3 sets): 32.  C5 by fixed group size (profiles/r06_c5_groups.json): 16 sets 721-797k sets/s, 32
// 753-830k, 64 795-809k, 128 706-724k, 1,024 617-739k; the first form of this model (retry priced at one final
// exponentiation per job) chose 16: 693k.  Per-job results do not depend on the grouping (each job's verdict is its
// own, as the reference's per-job re-verification); only the work does.
inline uint32_t adapt_group_sets(double f, int64_t group_sets, double sets_per_job) {
  const uint32_t gmax = (uint32_t)std::max<int64_t>(1, group_sets);
  if (f <= 0 || gmax <= 8) return gmax;
  const double retry = 13600.0 / (16.0 * std::max(1.0, sets_per_job)) + 1300.0, fixed = 14700.0;
  uint32_t best = gmax;
  double best_c = fixed / gmax + (1.0 - std::pow(1.0 - f, (double)gmax)) * retry;
  for (uint32_t g = 8; g < gmax; g *= 2) {
    const double c = fixed / g + (1.0 - std::pow(1.0 - f, (double)g)) * retry;
    if (c < best_c) best_c = c, best = g;
  }
  return best;
}

// F_g = prod of the group's Miller chunks as a product tree (launch_group_tree): with more than 16384 chunks (merged
// runs), runs of f_k consecutive chunks first (lane-serial: a 128-lane cooperative product costs ~6x the lane
// time) down to <= 8192 heads, then pair levels of stride f_k, 2 f_k, ... (one cooperative workgroup per pair);
// ftree = runs, then the pairs.  Up to 16384 chunks (a 16k call) the tree starts at the chunks: its latency.
// With step segments the tree runs per (segment, group) over the segment-major slots: range j * ng + g = the
// slots j * n_chunks + (group g's chunks); one segment: the groups' chunk ranges themselves.
struct FTree {
  std::vector<uint32_t> f_rng;        // [first slot, end slot) per (segment, group)
  std::vector<uint32_t> ftree;        // n_fruns runs [a, e), then the levels' pairs (dst, src)
  std::vector<uint32_t> f_level_end;  // pairs up to and including each level
  uint32_t n_fruns = 0, f_k = 1, n_franges = 0;
};
inline FTree plan_f_tree(const uint32_t* g_chunks, uint32_t ng, uint32_t n_chunks, uint32_t segs, int64_t f_run_max) {
  FTree t;
  uint32_t f_max = 0;
  const uint32_t n_slots = n_chunks * segs;
  t.n_franges = ng * segs;
  t.f_rng.resize(2 * (size_t)t.n_franges);
  for (uint32_t j = 0; j < segs; j++)
    for (uint32_t g = 0; g < ng; g++) {
      t.f_rng[2 * ((size_t)j * ng + g)] = j * n_chunks + g_chunks[2 * g];
      t.f_rng[2 * ((size_t)j * ng + g) + 1] = j * n_chunks + g_chunks[2 * g + 1];
    }
  if (n_slots > 16384)
    for (const uint32_t heads = f_run_max > 16 ? 256u : 8192u; n_slots / t.f_k > heads && t.f_k < (uint32_t)f_run_max;)
      t.f_k *= 2;
  for (uint32_t g = 0; g < ng; g++) f_max = std::max(f_max, g_chunks[2 * g + 1] - g_chunks[2 * g]);
  if (t.f_k > 1)
    for (uint32_t r = 0; r < t.n_franges; r++)
      for (uint32_t x = t.f_rng[2 * r], e = t.f_rng[2 * r + 1]; x < e; x += t.f_k)
        if (std::min(e, x + t.f_k) - x > 1) {
          t.ftree.push_back(x);
          t.ftree.push_back(std::min(e, x + t.f_k));
        }
  t.n_fruns = (uint32_t)(t.ftree.size() / 2);
  for (uint32_t st = t.f_k; st < f_max; st *= 2) {
    for (uint32_t r = 0; r < t.n_franges; r++)
      for (uint32_t i = t.f_rng[2 * r], e = t.f_rng[2 * r + 1]; i + st < e; i += 2 * st) {
        t.ftree.push_back(i);
        t.ftree.push_back(i + st);
      }
    t.f_level_end.push_back((uint32_t)(t.ftree.size() / 2) - t.n_fruns);
  }
  return t;
}

// What a run's forms depend on besides the batch and the options
struct RunEnv {
  bool urgent = false;          // the urgent slot's run (Slot::urgent)
  bool alone = false;           // no other run was in flight when the slot took this one (Slot::alone)
  double fail_rate = 0;         // the device's invalid-set rate estimate (Device::fail_rate), read once per run
  bool stream_pairs = true;     // BLSGPU_STREAM_PAIRS
  bool exclusive_small = true;  // BLSGPU_EXCLUSIVE_SMALL
};

// The forms a run's kernels take
struct Forms {
  bool coop, coop_g2, excl, small, spec, rsig_spec, keep_f, lane_tail, interleave;
  bool seg_plan;  // the automatic rule chose (mk, segs): the batch pass takes the one-lane kernel
  // mk_whole: the items per chunk of whole-loop lanes (one step segment), which the fallback's own accumulations keep
  uint32_t mk, mk_whole, segs, slice_len;
  uint32_t msm_tree;  // most slices of a range, when the tree sums them
};

// d_in / h_in (bytes, 256-B aligned sections): scalars | job_first_set | sigs (sig_w B each) | sig_len | unique msgs |
// msg_idx | set ranges | f ranges | units (first, sets, msg) | chunks | agg sets | MSM slices | F tree | pk section.
// The pk section: per-set key ranges (pk_first) and table indices or key bytes (pk_keys); one key per set: the
// key bytes alone (pk_first == pk_keys).
struct InArena {
  size_t scal, jobs, sigs, siglen, umsg, midx, ranges, franges, ufirst, usets, umsgi, cfirst, citems, agg, slices,
      rslices, ftree, pk_first, pk_keys, bytes;
};
// d_bytes: flags n | mflags nm | unit_ok n | status 3n | include n | spec n
struct ByteArena {
  size_t flags, mflags, unit_ok, status, include, spec, total;
};
// d_res / h_res: job_err nj | ok per group
struct ResArena {
  size_t job_err, ok, bytes;
  uint32_t max_ranges;
};
// d_work (words): per set sig_aff, pk_jac, pk_aff, f_chunk, the G1 window table of r_i pk_i (+ per unit unit_p),
// inv_buf, the pubkey branch's own inv_buf; per message h_aff, h_jac, h_norm, h_prep, h_q
struct WorkArena {
  size_t sig_aff, pk_jac, pk_aff, f_chunk, scal_tab, unit_p, inv_buf, inv_buf_pk, h_aff, h_jac, h_norm, h_prep, h_q,
      words;
};

struct RunPlan {
  // the shard: n sets from set s0, nj jobs; stride = max(n, 1) (the per-set arrays' length on the device)
  uint32_t n = 0, nj = 0, s0 = 0, stride = 1;
  const uint32_t* jfs = nullptr;  // the batch's job_first_set from the shard's first job on (it outlives the plan)
  bool table_mode = false, bytes_agg = false, pool = false;  // pool: the groups are a pool-policy list
  uint32_t pk_base = 0, npk = 0;
  // groups: [first job, end job) (shard-relative); group_batchable with a pool-policy list only
  std::vector<std::pair<uint32_t, uint32_t>> group_jobs;
  std::vector<uint8_t> group_batchable;
  uint32_t ng0 = 0;
  // dedupe
  std::vector<uint32_t> msg_idx, uniq;
  uint32_t n_umsg = 0, nm = 1;
  // units: within each group, one unit per distinct message (merged: fewer units than sets)
  std::vector<uint32_t> unit_of_set, unit_msg, unit_first, unit_sets, g_unit_first;
  bool merged = false;
  uint32_t n_units = 0, n_items = 0;
  Forms f{};
  // Miller chunks of the batch pass: each group's items (sets, or units) in chunks of mk
  std::vector<uint32_t> chunk_first, chunk_items, g_chunks;
  uint32_t n_chunks = 0;
  miller_plan::Segments segments{};
  // MSM slices of the groups' set ranges (S_g = sum r_i sig_i)
  std::vector<uint32_t> slices, range_slices;
  uint32_t n_slices = 0;
  FTree ft;
  // sets that aggregate >= 2 keys (one wave each in k_pk_aggregate); one-key sets are read by k_pk_finish
  std::vector<uint32_t> agg_sets;
  // signatures at a 96-byte stride when no set carries a 192-byte (uncompressed) one: half the staging and copy
  uint32_t sig_w = 96;
  InArena in{};
  ByteArena by{};
  ResArena res{};
  WorkArena work{};
  double t_dedupe_ms = 0, t_struct_ms = 0;  // host trace (plan_run's now_ms)

  std::pair<uint32_t, uint32_t> job_sets(uint32_t j) const { return {jfs[j] - s0, jfs[j + 1] - s0}; }
  std::pair<uint32_t, uint32_t> group_sets(uint32_t g) const {
    return {job_sets(group_jobs[g].first).first, job_sets(group_jobs[g].second - 1).second};
  }
  std::pair<uint32_t, uint32_t> group_items(uint32_t g) const {
    if (merged) return {g_unit_first[g], g_unit_first[g + 1]};
    return group_sets(g);
  }
  // sizes (words) of the slot buffers the batch pass grows
  size_t S_words() const { return kG2J * res.max_ranges; }
  size_t F_words() const { return kFp12 * res.max_ranges; }
  size_t G_words() const { return kFp12 * std::max<uint32_t>(ng0, 1); }
  size_t msmB_words() const { return kMsmBucketWords * std::max<uint32_t>(n_slices, 1); }
  size_t msmW_words() const { return kMsmWindowWords * res.max_ranges; }
  size_t lines_words() const { return (size_t)nm * kMillerLineWords; }
  size_t fkeep_words() const { return (size_t)stride * kFp12; }   // under keep_f
  size_t fseg_words() const { return kFp12 * ft.n_franges; }      // with more than one segment
  size_t fb_words() const { return (size_t)stride * 9 * kG2J; }   // r_i sig_i and their G2 window tables
};

inline void carve_arenas(RunPlan& p) {
  const size_t n = p.n, nj = p.nj, stride = p.stride, nm = p.nm;
  Carve c;
  InArena& a = p.in;
  a.scal = c.take(n * 8), a.jobs = c.take((nj + 1) * 4), a.sigs = c.take(n * p.sig_w), a.siglen = c.take(n * 4);
  a.umsg = c.take((size_t)p.n_umsg * 32), a.midx = c.take(n * 4), a.ranges = c.take((size_t)std::max(p.ng0, 1u) * 8);
  a.franges = c.take((size_t)std::max(p.ft.n_franges, 1u) * 8), a.ufirst = c.take((size_t)(p.n_units + 1) * 4);
  a.usets = c.take(p.unit_sets.size() * 4), a.umsgi = c.take((size_t)p.n_units * 4);
  a.cfirst = c.take((size_t)(p.n_chunks + 1) * 4), a.citems = c.take(p.chunk_items.size() * 4);
  a.agg = c.take(p.agg_sets.size() * 4), a.slices = c.take(p.slices.size() * 4);
  a.rslices = c.take(p.range_slices.size() * 4), a.ftree = c.take(p.ft.ftree.size() * 4);
  if (p.table_mode || p.bytes_agg) {
    a.pk_first = c.take((n + 1) * 4), a.pk_keys = c.take((size_t)p.npk * (p.table_mode ? 4 : 96));
  } else {
    a.pk_first = a.pk_keys = c.take(n * 96);
  }
  a.bytes = c.end;
  Carve b;
  p.by.flags = b.take(n), p.by.mflags = b.take(nm), p.by.unit_ok = b.take(n), p.by.status = b.take(3 * stride);
  p.by.include = b.take(stride), p.by.spec = b.take(stride), p.by.total = b.at;
  Carve r;
  p.res.max_ranges = std::max<uint32_t>(std::max(p.ng0, p.nj), 1);
  p.res.job_err = r.take(nj), p.res.ok = r.take(p.res.max_ranges), p.res.bytes = r.end;
  Carve w{1};
  WorkArena& k = p.work;
  k.sig_aff = w.take(stride * kG2A), k.pk_jac = w.take(stride * kG1J), k.pk_aff = w.take(stride * kG1A);
  k.f_chunk = w.take(stride * kFp12), k.scal_tab = w.take(stride * 8 * kG1J);
  k.unit_p = p.merged ? w.take(stride * kG1A) : w.at;
  k.inv_buf = w.take(stride * kFp);     // n_umsg <= n
  k.inv_buf_pk = w.take(stride * kFp);  // the pubkey branch's own (it runs beside the hash branch)
  k.h_aff = w.take(nm * kG2A), k.h_jac = w.take(nm * kG2J), k.h_norm = w.take(nm * kFp);
  k.h_prep = w.take(nm * 14 * kFp), k.h_q = w.take(nm * 2 * kG2J), k.words = w.end;
}

// The plan of one run.  With `pool` (group_policy 1) the groups are the list's job ranges instead of >= group_sets
// packing.  seed: the message index's hash key.  now_ms (host trace): a clock read after the dedupe and at the end.
inline RunPlan plan_run(const blsgpu_batch& b, const Shard& sh, const Options& opt, const RunEnv& env, uint64_t seed,
                        const std::vector<GroupPlanEntry>* pool = nullptr, double (*now_ms)() = nullptr) {
  RunPlan p;
  const uint32_t n = p.n = sh.set_end - sh.set_begin, nj = p.nj = sh.job_end - sh.job_begin;
  const uint32_t s0 = p.s0 = sh.set_begin;
  p.stride = std::max<uint32_t>(n, 1);
  p.jfs = b.job_first_set + sh.job_begin;
  p.table_mode = b.pk_bytes == nullptr;
  p.bytes_agg = b.pk_bytes && b.set_pk_first;
  p.pool = pool != nullptr;
  p.pk_base = b.set_pk_first ? b.set_pk_first[s0] : 0;
  p.npk = b.set_pk_first ? b.set_pk_first[sh.set_end] - p.pk_base : 0;

  // ---- groups (contiguous job ranges) ------------------------------------------------------------------------
  if (pool) {
    for (const GroupPlanEntry& g : *pool) {
      uint32_t sets = 0;
      for (uint32_t j = g.first; j < g.end; j++) sets += p.jfs[j + 1] - p.jfs[j];
      if (!sets) continue;  // empty jobs are rejected by the job mask, they join no group
      p.group_jobs.push_back({g.first, g.end});
      p.group_batchable.push_back(g.batchable);
    }
  } else {
    // group size: group_sets, or smaller while this device has seen invalid sets (group_adapt, adapt_group_sets)
    const uint32_t gs = opt.group_adapt ? adapt_group_sets(env.fail_rate, opt.group_sets, (double)n / std::max(nj, 1u))
                                        : (uint32_t)opt.group_sets;
    uint32_t cur_sets = 0;
    bool open = false;
    for (uint32_t j = 0; j < nj; j++) {
      const uint32_t a = p.jfs[j] - s0, e = p.jfs[j + 1] - s0;
      const bool batchable = b.job_flags && (b.job_flags[sh.job_begin + j] & 1u);
      if (e == a) {
        open = false;
        continue;
      }
      if (!batchable) {
        p.group_jobs.push_back({j, j + 1});
        open = false;
        continue;
      }
      if (!open || cur_sets >= gs) {
        p.group_jobs.push_back({j, j});
        cur_sets = 0;
        open = true;
      }
      p.group_jobs.back().second = j + 1;
      cur_sets += e - a;
    }
  }
  const uint32_t ng0 = p.ng0 = (uint32_t)p.group_jobs.size();

  // ---- message dedupe and same-message units ----------------------------------------------------------------
  if (opt.dedupe && n) {
    dedupe_messages(b.msgs + (size_t)s0 * 32, n, seed ^ 0x6a09e667f3bcc908ull, p.msg_idx, p.uniq);
  } else {
    p.msg_idx.resize(n);
    p.uniq.resize(n);
    for (uint32_t i = 0; i < n; i++) p.msg_idx[i] = p.uniq[i] = i;
  }
  const uint32_t n_umsg = p.n_umsg = (uint32_t)p.uniq.size();
  p.nm = std::max<uint32_t>(n_umsg, 1);
  if (now_ms) p.t_dedupe_ms = now_ms();
  // units: within each group, one unit per distinct message
  p.unit_of_set.assign(n, UINT32_MAX);
  p.g_unit_first.assign(ng0 + 1, 0);
  if (opt.dedupe && n_umsg < n) {
    std::vector<uint32_t> stamp(n_umsg, UINT32_MAX), unit_of_msg(n_umsg, 0);
    for (uint32_t g = 0; g < ng0; g++) {
      p.g_unit_first[g] = (uint32_t)p.unit_msg.size();
      const auto ae = p.group_sets(g);
      for (uint32_t i = ae.first; i < ae.second; i++) {
        const uint32_t m = p.msg_idx[i];
        if (stamp[m] != g) {
          stamp[m] = g;
          unit_of_msg[m] = (uint32_t)p.unit_msg.size();
          p.unit_msg.push_back(m);
        }
        p.unit_of_set[i] = unit_of_msg[m];
      }
    }
    p.g_unit_first[ng0] = (uint32_t)p.unit_msg.size();
    p.merged = p.unit_msg.size() < (size_t)n;
    if (p.merged) {
      const uint32_t nu = (uint32_t)p.unit_msg.size();
      p.unit_first.assign(nu + 1, 0);
      for (uint32_t i = 0; i < n; i++)
        if (p.unit_of_set[i] != UINT32_MAX) p.unit_first[p.unit_of_set[i] + 1]++;
      for (uint32_t u = 0; u < nu; u++) p.unit_first[u + 1] += p.unit_first[u];
      p.unit_sets.resize(p.unit_first[nu]);
      std::vector<uint32_t> fill(p.unit_first.begin(), p.unit_first.end() - 1);
      for (uint32_t i = 0; i < n; i++)
        if (p.unit_of_set[i] != UINT32_MAX) p.unit_sets[fill[p.unit_of_set[i]]++] = i;
    }
  }
  const bool merged = p.merged;
  p.n_units = merged ? (uint32_t)p.unit_msg.size() : 0;

  // ---- forms, Miller chunks and step segments ----------------------------------------------------------------
  // Small and mid-size runs (<= opt.coop_max pairings, miller_k auto or 1): one cooperative workgroup per pairing
  // (k_miller_coop, lines on the fly) -- 1/6 of the lane-per-chunk loop's latency, at a fraction of its lane
  // efficiency.  The [|z|] chains of the cofactor clearing and the subgroup check go cooperative below opt.coop_g2_max
  // sets.  Up to opt.coop_excl_max items every cooperative workgroup takes a CU to itself (k_common.hpp
  // exclusive_cu_lds): with more workgroups than CUs the padding would serialize them.
  Forms& f = p.f;
  const uint32_t n_items = p.n_items = merged ? p.n_units : n;
  f.coop = n_items <= (uint32_t)opt.coop_max && opt.miller_k <= 1;
  f.coop_g2 = n <= (uint32_t)opt.coop_g2_max;
  // (an urgent run takes the padding only with urgent_excl: on a small CU partition, or beside throughput runs, a
  // workgroup that needs a whole CU waits for one)
  f.excl = env.exclusive_small && n_items <= (uint32_t)opt.coop_excl_max && (!env.urgent || opt.urgent_excl);
  f.mk_whole = f.coop ? 1u : opt.miller_k > 0 ? (uint32_t)opt.miller_k : miller_k_auto(n_items);
  // Step segments (miller_plan.hpp): a run of >= 65,536 items that would take the one-lane or two-lane chunk form takes
  // chunks of 8 (or 4) items on the one-lane kernel with J lanes per chunk, each over its own step range, so that
  // n_chunks J lanes still give every SIMD a wave; the F tree then runs per (group, segment) and k_f_fold folds the J
  // heads of a group.  Such a run no longer has one chunk per set, so it gives up keep_f (below): a failed group's
  // jobs re-run their Miller loops; while the device sees enough invalid sets to fail a fifth of the groups, a run
  // that would keep its per-set values stays as it is (miller_plan::hold_kept_values).
  // BLSGPU_MILLER_SEGMENTS = J (diagnostics) switches the rule off: the one-lane form then runs min(J, k) segments
  // at any run size, every other form as ever.
  const AccForm form_whole = acc_form(f.mk_whole, n_items, opt.miller_lanes, opt.acc6_max, opt.miller_pairs != 0);
  f.mk = f.mk_whole, f.segs = 1;
  if (opt.miller_segments > 0) {
    if (!f.coop && form_whole == AccForm::one) f.segs = (uint32_t)std::min<int64_t>(opt.miller_segments, f.mk);
  } else if (!f.coop && opt.miller_lanes == 0 && (form_whole == AccForm::one || form_whole == AccForm::two)) {
    std::vector<uint32_t> g_len(ng0);
    for (uint32_t g = 0; g < ng0; g++) g_len[g] = p.group_items(g).second - p.group_items(g).first;
    // many failing groups: the kept per-set Miller values are worth more than the plan
    const bool hold = opt.keep_f && !merged && f.mk_whole == 1 && ng0 &&
                      miller_plan::hold_kept_values(env.fail_rate, (double)n / ng0);
    const miller_plan::Plan pl =
        miller_plan::plan_auto(n_items, g_len.data(), ng0, p.stride, opt.miller_k > 0 || hold, f.mk_whole);
    f.seg_plan = pl.k != f.mk_whole || pl.segs > 1;
    f.mk = pl.k, f.segs = pl.segs;
  }
  f.interleave = f.segs > 1 || f.seg_plan;  // (a one-segment run outside the rule keeps consecutive items)
  p.chunk_first.assign(1, 0);
  p.g_chunks.resize(2 * (size_t)ng0);
  p.chunk_items.reserve(n);
  for (uint32_t g = 0; g < ng0; g++) {
    const auto ae = p.group_items(g);
    const auto cr = miller_plan::add_chunks(p.chunk_first, p.chunk_items, ae.first, ae.second, f.mk, f.interleave);
    p.g_chunks[2 * g] = cr.first;
    p.g_chunks[2 * g + 1] = cr.second;
  }
  const uint32_t n_chunks = p.n_chunks = (uint32_t)p.chunk_first.size() - 1;
  // slot j * n_chunks + c of f_chunk (stride words apart)
  f.segs = miller_plan::fit_segments(n_chunks, f.segs, p.stride);
  p.segments = miller_plan::segments(f.segs);
  // Per-set pairings (no same-message units, one item per chunk): chunk c is set c (the groups cover every set of a
  // non-empty job, in order), so the batch pass's Miller values f_c = MillerLoop(r_c pk_c, H(m_c)) are exactly what a
  // failed group's per-job checks need.  They are copied aside before the F tree multiplies chunks in place, and the
  // fallback takes F_j = prod of its sets' kept values instead of re-running the Miller loops.
  f.keep_f = opt.keep_f && !merged && f.mk == 1 && n_chunks == n;
  // A small run (<= opt.small_max sets) leaves most of the chip idle whatever its kernel forms: on an idle device it takes
  // the other stream pair too (speculative MSM, parallel pubkey branch, r_i sig_i), and its fallback checks stay
  // cooperative (latency) instead of lane-per-check (throughput).
  f.small = n <= (uint32_t)opt.small_max;
  // speculative MSM (enqueue_batch_pass); spec_large: larger runs on an idle device too
  f.spec = env.stream_pairs && (f.small || opt.spec_large) && env.alone && !opt.serial;
  // A small run on an idle device also forms every r_i sig_i (k_sig_scale) on the idle pubkey stream once its pubkeys
  // and the decode are done: the chip has room, and a failed group's per-job checks then start from the sums instead
  // of a 1.7 ms scaling launch on the fallback's critical path (the batch pass itself never reads them).
  f.rsig_spec = f.spec && f.small && opt.rsig_spec;
  // Large (merged) runs meet a chip full of one-wave-per-SIMD stage kernels: the signature branch's cooperative tails
  // (Horner passes, MillerLoop(-g1, S)) waited for free SIMD groups there, so they run on single lanes
  f.lane_tail = opt.lane_tail_min > 0 && n >= (uint32_t)opt.lane_tail_min;

  // ---- MSM slices --------------------------------------------------------------------------------------------
  // Runs up to 32k sets (an isolated block's or
  // gossip call's latency) take half slices: twice the bucket workgroups at half the chain, 16k isolated sig_msm
  // 3.55 -> 2.80 ms; merged runs keep full slices (fewer bucket sums to combine: 100-step C2 3.13M vs 3.01M).
  // Small runs (<= 1024 sets) take 32-set slices: a bucket lane's chain of mixed additions is ~len / 8 plus its
  // spread (128 sets: ~25 additions on the slowest lane, 1.26 ms), the window lanes add the few slices up.
  // Up to 32k sets the slice length is opt.msm_slice_mid (default 32: a 16k call's bucket pass is 512 workgroups, every
  // SIMD a wave, ~4 additions per lane) and each range's slices are summed by a pairwise tree of launches
  // (launch_sig_msm tree_slices) instead of the window lanes' serial chain.
  constexpr uint32_t kMsmHalfSliceMaxSets = 32768, kMsmSmallSliceMaxSets = 1024;
  f.slice_len = n <= kMsmSmallSliceMaxSets ? 32 : n <= kMsmHalfSliceMaxSets ? (uint32_t)opt.msm_slice_mid : kMsmSlice;
  p.range_slices.assign(1, 0);
  for (uint32_t g = 0; g < ng0; g++) {
    const auto ae = p.group_sets(g);
    add_slices(p.slices, p.range_slices, ae.first, ae.second, f.slice_len);
  }
  p.n_slices = (uint32_t)(p.slices.size() / 2);
  // (runs of <= 1,024 sets too: a 1,024-set call's 32 slices summed serially by the window lanes took 2.0 ms beside the
  // cooperative Miller loops and made the signature branch its critical path -- r05 trace)
  f.msm_tree = 0;
  if (n <= kMsmHalfSliceMaxSets && opt.msm_tree) {
    for (uint32_t g = 0; g < ng0; g++) f.msm_tree = std::max(f.msm_tree, p.range_slices[g + 1] - p.range_slices[g]);
    // the tree's launches are sized n_ranges x (most slices of a range): only when the ranges are about equal (one
    // large job beside many single-set groups would launch ~n_ranges x max_pairs idle lanes per level)
    if ((uint64_t)ng0 * f.msm_tree > 2ull * p.n_slices) f.msm_tree = 0;
  }
  p.ft = plan_f_tree(p.g_chunks.data(), ng0, n_chunks, f.segs, opt.f_run_max);
  if (p.table_mode || p.bytes_agg)
    for (uint32_t i = 0; i < n; i++)
      if (b.set_pk_first[s0 + i + 1] - b.set_pk_first[s0 + i] >= 2) p.agg_sets.push_back(i);
  if (now_ms) p.t_struct_ms = now_ms();
  for (uint32_t i = 0; i < n; i++)
    if (b.sig_len[s0 + i] == 192) {
      p.sig_w = 192;
      break;
    }
  carve_arenas(p);
  return p;
}

// ---- per-job results of the batch pass ----------------------------------------------------------------------
// jr[j]: 1 valid, 0 invalid, 2 pending (in retry), < 0 the job's error code.  With a pool-policy list the
// batchRetries / batchSigsSuccess metrics count the list's batchable chunks the way the worker does (worker.ts:
// 56-84: a chunk that throws or returns false is one retry; a chunk that verifies adds all its sets).
struct Classified {
  std::vector<int> jr;
  std::vector<uint32_t> retry;     // clean jobs of failed groups, each re-checked on its own
  std::vector<uint32_t> failed_g;  // groups whose own equation failed (their clean jobs are in retry)
  uint32_t batch_retries = 0, batch_sigs_success = 0;
};
inline Classified classify_groups(const RunPlan& p, const int8_t* job_err, const uint8_t* group_ok, bool spec) {
  Classified c;
  c.jr.assign(p.nj, 0);
  for (uint32_t j = 0; j < p.nj; j++) {
    const int err = job_err[j];
    c.jr[j] = err ? -err : 2;  // 2 = pending
  }
  std::vector<uint32_t> clean;
  for (uint32_t g = 0; g < p.ng0; g++) {
    const uint32_t first = p.group_jobs[g].first, end = p.group_jobs[g].second;
    clean.clear();
    bool dropped = false;  // a rejected job of the group has sets (they may sit in a speculative S_g)
    for (uint32_t j = first; j < end; j++) {
      if (c.jr[j] == 2)
        clean.push_back(j);
      else if (p.job_sets(j).second > p.job_sets(j).first)
        dropped = true;
    }
    // Speculative MSM (spec): S_g summed every decoded set of the group, so a group with a rejected job is not the
    // equation of its clean jobs -- its verdict (pass or fail) is not read; every clean job is re-checked on its own
    // with exact masks (the fallback's own S_j, F_j).  Only the failure path pays.  The subgroup check's writes to
    // sig_aff, unordered with the speculative MSM's reads, can likewise only reach such a group.
    if (spec && dropped && !clean.empty()) {
      if (p.pool && p.group_batchable[g]) c.batch_retries++;
      if (!p.pool && clean.size() > 1) c.batch_retries++;
      c.retry.insert(c.retry.end(), clean.begin(), clean.end());
      continue;
    }
    if (p.pool) {  // the worker's metrics: a chunk with a throwing job or a failed equation is one retry
      if (!p.group_batchable[g]) {
      } else if (clean.size() == end - first && group_ok[g]) {
        c.batch_sigs_success += p.group_sets(g).second - p.group_sets(g).first;
      } else {
        c.batch_retries++;
      }
    }
    if (clean.empty()) continue;
    // A failed group's clean jobs are re-verified one by one, also when the group held a single clean job (its
    // equation was that job's own): the reference re-verifies every job of a failed chunk whatever its size
    // (worker.ts:76-98), so a job's false is always its own check's answer, never only its group's.
    if (group_ok[g]) {
      for (uint32_t j : clean) c.jr[j] = 1;
      if (!p.pool && end - first > 1)
        for (uint32_t j : clean) c.batch_sigs_success += p.job_sets(j).second - p.job_sets(j).first;
    } else {
      if (!p.pool && clean.size() > 1) c.batch_retries++;
      c.retry.insert(c.retry.end(), clean.begin(), clean.end());
      c.failed_g.push_back(g);
    }
  }
  return c;
}

// The device's invalid-set rate estimate after a run (group_adapt): a group "failed" when any of its non-empty jobs was
// not valid; with groups of s sets failing at rate pf, a set is invalid at rate f = 1 - (1 - pf)^(1/s).  Returns the
// new estimate from the old one (the caller holds Device::fail_mu); needs at least one group.
inline double next_fail_rate(const RunPlan& p, const std::vector<int>& jr, double rate) {
  uint32_t failed = 0;
  for (uint32_t g = 0; g < p.ng0; g++)
    for (uint32_t j = p.group_jobs[g].first; j < p.group_jobs[g].second; j++)
      if (jr[j] != 1 && p.job_sets(j).second > p.job_sets(j).first) {
        failed++;
        break;
      }
  const double pf = std::min((double)failed, p.ng0 - 0.5) / p.ng0;
  const double f = 1.0 - std::pow(1.0 - pf, (double)p.ng0 / std::max(p.n, 1u));
  return 0.5 * rate + 0.5 * f;
}

// ---- fallback: every clean job of every failed group gets its own verdict ---------------------------------
// The reference re-verifies each job of a failed chunk (worker.ts:76-98).  Here each retried job j gets its
// own Miller accumulation (its sets, miller_k per chunk) F_j and its own S_j = sum r_i sig_i -- a bucket MSM for
// large jobs, per-set scalings (k_sig_scale) plus a sum when the jobs are small (a 1-3-set job would leave a
// 128-lane MSM workgroup idle) -- and then, as group testing:
//   level 1: sub-groups of kFbSub consecutive retried jobs are checked with one final exponentiation each
//            (F_s = prod F_j, S_s = sum S_j); a passing sub-group validates its jobs;
//   level 2: every job of a failing sub-group is checked on its own.
// Per-job answers are the reference's (valid iff every set of the job verifies); with few invalid jobs the
// final exponentiations drop from one per job to about one per kFbSub jobs.
constexpr uint32_t kFbSub = 16;
// from this many sub-groups on, one lane per sub-group combines its 16 entries (instead of a wave per
// sub-group).  The checks stay one 128-lane workgroup each: a lane-per-check final exponentiation gave the
// same C5 throughput at 56% more latency (profiles/r02_configs_fallback.json), and its call frames need
// 8-12 KB/lane of scratch, which the per-queue scratch reservation does not always get.
constexpr uint32_t kFbLaneMin = 128;
// A small run (cooperative forms: the chip is far from full) checks every retried job directly in ONE launch --
// up to kFbDirectMax checks run side by side (4 cooperative workgroups per CU) -- instead of sub-groups, a host
// round trip and then the jobs of the failing sub-groups: one check round instead of two.  (Cooperative checks slow
// down with their number -- 96 in 3.1 ms, 257 in 5.7, 675 in 8.1, 1,024 in 16 ms: profiles/r05_fallback_* -- so
// beyond ~640 jobs two rounds of few checks are faster; C5's 514 retried jobs: p50 14.7 ms direct, 16.6 in two
// rounds.)
constexpr uint32_t kFbDirectMax = 640;

struct FallbackPlan {
  uint32_t nr = 0;  // retried jobs
  // per retried job: its set range (rr), its F range (rf: kept per-set values, or chunks of rfirst / ritems), its MSM
  // slices (rrs into rsl); rset: every retried set; subr: the sub-groups' ranges of retried jobs
  std::vector<uint32_t> rr, rf, rfirst, ritems, rsl, rrs, rset, subr;
  bool small_jobs = false, busy = false, direct = false;
  uint32_t nsub = 0, nc = 0, nrs = 0;
  int64_t fb_lane_min = 0;
  // d_list / h_list (words): rr | rf | rfirst | ritems | rsl | rrs | rset | subr | sel (the jobs checked on their own)
  size_t o_rf = 0, o_rfirst = 0, o_ritems = 0, o_rsl = 0, o_rrs = 0, o_rset = 0, o_sub = 0, o_sel = 0, words = 0;
  // a check launch of `count` checks takes the lane forms
  bool lane_checks(uint32_t count) const { return busy && fb_lane_min > 0 && count >= (uint32_t)fb_lane_min; }
};
inline FallbackPlan plan_fallback(const RunPlan& p, const std::vector<uint32_t>& retry, const Options& opt,
                                  bool alone) {
  FallbackPlan fp;
  const uint32_t nr = fp.nr = (uint32_t)retry.size();
  fp.rfirst.assign(1, 0), fp.rrs.assign(1, 0);
  fp.rr.resize(2 * (size_t)nr), fp.rf.resize(2 * (size_t)nr);
  for (uint32_t q = 0; q < nr; q++) {
    const auto js = p.job_sets(retry[q]);
    fp.rr[2 * q] = js.first;
    fp.rr[2 * q + 1] = js.second;
    add_slices(fp.rsl, fp.rrs, js.first, js.second);
    for (uint32_t i = js.first; i < js.second; i++) fp.rset.push_back(i);
    if (p.f.keep_f) {  // F_j from the kept per-set values: chunk = set
      fp.rf[2 * q] = js.first;
      fp.rf[2 * q + 1] = js.second;
      continue;
    }
    const auto cr = miller_plan::add_chunks(fp.rfirst, fp.ritems, js.first, js.second, p.f.mk_whole);
    fp.rf[2 * q] = cr.first;
    fp.rf[2 * q + 1] = cr.second;
  }
  // per-set scalings instead of per-job MSMs while the jobs are small (a 1-3-set job would leave a 128-lane MSM
  // workgroup idle); the speculative batch-pass scalings (rsig_spec) then save the scaling launch.  Large retried jobs
  // (e.g. two failing 1k-set block jobs) take the bucket MSM and the wave-per-job reduce even when the run made the
  // scalings: one lane summing a job's thousands of r_i sig_i and multiplying its Fp12 values in series is slower.
  fp.small_jobs = fp.rset.size() < (size_t)32 * nr;
  // Large runs under load (other runs in flight: merged calls, throughput first) take lane-per-check launches of many
  // checks, and with many retried jobs (>= fb_direct_min: dense failures, e.g. C5's 1% invalid sets fail every
  // group) check every job directly in ONE lane launch: three times the checks of the sub-group round trip, but one
  // ~25 ms lane round instead of two, and the run's call latency is what bounds a loaded device's throughput
  // (calls in flight / latency).  Small runs and runs on an idle device keep the cooperative checks' latency.
  fp.busy = (!p.f.small && !alone) || opt.fb_force_busy;
  fp.fb_lane_min = opt.fb_lane_min;
  fp.direct =
      (p.f.small && nr <= kFbDirectMax) || (fp.busy && opt.fb_direct_min > 0 && nr >= (uint32_t)opt.fb_direct_min);
  fp.nsub = !fp.direct && nr >= 2 * kFbSub ? (nr + kFbSub - 1) / kFbSub : 0;
  fp.subr.resize(2 * (size_t)fp.nsub);
  for (uint32_t t = 0; t < fp.nsub; t++) {
    fp.subr[2 * t] = t * kFbSub;
    fp.subr[2 * t + 1] = std::min(nr, (t + 1) * kFbSub);
  }
  fp.nc = (uint32_t)fp.rfirst.size() - 1;
  fp.nrs = (uint32_t)(fp.rsl.size() / 2);
  Carve c{1};
  c.take(fp.rr.size());  // rr, at 0
  fp.o_rf = c.take(fp.rf.size()), fp.o_rfirst = c.take(fp.rfirst.size()), fp.o_ritems = c.take(fp.ritems.size());
  fp.o_rsl = c.take(fp.rsl.size()), fp.o_rrs = c.take(fp.rrs.size()), fp.o_rset = c.take(fp.rset.size());
  fp.o_sub = c.take(fp.subr.size()), fp.o_sel = c.take(nr), fp.words = c.end;
  return fp;
}

// ---- group_policy 1: the reference pool's grouping ---------------------------------------------------------
// A call's sets are split into jobs of <= 128 sets (chunkifyMaximizeChunkSize(sets, 128), multithread/index.ts:156),
// consecutive jobs are packed into worker requests of >= 128 sets (prepareWork, index.ts:386-401), and each request's
// batchable jobs are checked in chunks of >= 16 jobs, its other jobs one by one (worker.ts:40-92).
struct PoolSub {
  uint32_t call, a, e;  // the call's job, its sets [a, e)
  bool batchable;
};
struct PoolPlan {
  std::vector<PoolSub> subs;
  std::vector<uint32_t> order;  // sub-job indices in group order
  std::vector<GroupPlanEntry> groups;
};
inline PoolPlan plan_pool_groups(const uint32_t* job_first_set, const uint8_t* job_flags, uint32_t job_begin,
                                 uint32_t job_end) {
  PoolPlan pp;
  std::vector<PoolSub>& subs = pp.subs;
  for (uint32_t j = job_begin; j < job_end; j++) {
    const uint32_t a = job_first_set[j], e = job_first_set[j + 1];
    const bool bt = job_flags && (job_flags[j] & 1u);
    if (a == e) {
      subs.push_back({j, a, a, bt});
      continue;
    }
    const uint32_t per = chunk_size(e - a, 128);
    for (uint32_t k = a; k < e; k += per) subs.push_back({j, k, std::min(e, k + per), bt});
  }
  for (size_t q = 0; q < subs.size();) {
    size_t q1 = q;
    uint32_t total = 0;
    while (q1 < subs.size() && total < 128) total += subs[q1].e - subs[q1].a, q1++;
    std::vector<uint32_t> bat, rest;
    for (size_t x = q; x < q1; x++) (subs[x].batchable && subs[x].e > subs[x].a ? bat : rest).push_back((uint32_t)x);
    if (!bat.empty()) {
      const uint32_t per = chunk_size((uint32_t)bat.size(), 16);
      for (size_t k = 0; k < bat.size(); k += per) {
        GroupPlanEntry g{(uint32_t)pp.order.size(), 0, true};
        for (size_t x = k; x < std::min(bat.size(), k + per); x++) pp.order.push_back(bat[x]);
        g.end = (uint32_t)pp.order.size();
        pp.groups.push_back(g);
      }
    }
    for (uint32_t x : rest) {
      pp.groups.push_back({(uint32_t)pp.order.size(), (uint32_t)pp.order.size() + 1, false});
      pp.order.push_back(x);
    }
    q = q1;
  }
  return pp;
}

}  // namespace blsgpu_rt
