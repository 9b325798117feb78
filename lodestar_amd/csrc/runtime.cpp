// Host runtime of libblsgpu: the C ABI declared in include/blsgpu.h.
//
// Replaces BlsMultiThreadWorkerPool's job plumbing (reference packages/beacon-node/src/chain/bls/
// multithread/index.ts:134-412) and the worker's batch/fallback policy (multithread/worker.ts:32-108)
// with HIP streams on MI355X and no host threads doing arithmetic:
//   * a call (one verifySignatureSets submission) is split into contiguous, cost-balanced shards of jobs,
//     one per device it uses (never splitting a job); shards go to their device's task queue;
//   * each device owns several slots (a HIP stream + its staging and work buffers) and ONE long-lived
//     dispatcher thread per slot that takes shards from the device queue, so concurrent calls overlap on
//     the GPU -- the way the reference keeps all its workers busy -- with no thread created per call;
//   * each shard runs the stage kernels (k_*.hip): signature decode + subgroup check, hash_to_G2 of every
//     DISTINCT signing root, pubkey aggregation, r_i scaling, the job mask, same-message unit sums, Miller
//     loops (per set, or per (group, message) unit), then the batch-group tail;
//   * batchable jobs are packed into groups of >= group_sets sets (random linear combination, one final
//     exponentiation per group); non-batchable jobs are their own group; a single-set non-batchable job
//     uses r = 1 (= CoreVerify, maybe_batch.ts:34-38);
//   * a failed group is resolved by ONE parallel launch that re-checks every clean job of every failed
//     group on its own (the reference re-verifies each job of a failed chunk, worker.ts:76-98): per job the
//     answer is the reference's, valid iff every set of the job verifies.
// There is no CPU verification path: without a usable GPU blsgpu_init fails.
#include <pthread.h>
#include <stdio.h>
#include <sys/random.h>

#include <cmath>
#include <string>
#include <system_error>

#include "runtime_internal.hpp"
#include "miller_plan.hpp"

using namespace blsgpu_rt;

namespace {

// Device-failure injection (blsgpu_debug_inject, tests only): the next `count` pipeline runs after `skip` more fail as
// if a HIP call had failed once their batch pass completed.
std::atomic<int64_t> g_fail_run_skip{0}, g_fail_run_count{0};
// set on the runtime's dispatcher threads (a "slots" change from a done callback would join its own thread)
thread_local bool tl_dispatcher = false;

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
// accumulations and every run the step-segment plan leaves alone.  From 65,536 items on, run_shard asks
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
// (segs: step segments, one-lane form only)
void launch_miller_acc_auto(const PipelineBuffers& pb, bool units, hipStream_t st, uint32_t mk, int64_t lanes_opt,
                            int64_t acc6_max, bool pairs, const MillerSegs* segs = nullptr) {
  switch (acc_form(mk, pb.n_chunks, lanes_opt, acc6_max, pairs)) {
    case AccForm::six: launch_miller_acc6(pb, units, st); break;
    case AccForm::pairs: launch_miller_accx(pb, units, st); break;
    case AccForm::two: launch_miller_acc2(pb, units, st); break;
    case AccForm::one: launch_miller_acc(pb, units, st, segs); break;
  }
}

using miller_plan::add_chunks;  // item ranges -> Miller chunks of <= k items (miller_plan.hpp)
static_assert(miller_plan::kSteps == MILLER_STEPS && miller_plan::kMaxSegments == MILLER_MAX_SEGS, "miller_plan.hpp");

// Splits set ranges into MSM slices of <= len (<= MSM_SLICE) sets: appends to slices (pairs), returns the range's
// [first slice, end slice)
inline void add_slices(std::vector<uint32_t>& slices, std::vector<uint32_t>& range_slices, uint32_t a, uint32_t e,
                       uint32_t len = MSM_SLICE) {
  for (uint32_t x = a; x < e; x += len) {
    slices.push_back(x);
    slices.push_back(std::min<uint32_t>(e, x + len));
  }
  range_slices.push_back((uint32_t)(slices.size() / 2));
}

}  // namespace

namespace blsgpu_rt __attribute__((visibility("hidden"))) {  // (Task, in runtime_internal.hpp, points to a Call)

struct Shard {
  uint32_t job_begin, job_end;  // job range
  uint32_t set_begin, set_end;  // set range
  uint32_t dev = 0;             // device index (routing)
  int64_t cost = 0;             // routing cost, x256 (Device::load)
};

// Inputs owned by an asynchronous call (the caller may reuse its buffers once blsgpu_submit returns)
struct Owned {
  std::vector<uint32_t> jfs, siglen, pkfirst, pkidx;
  std::vector<uint8_t> jflags, pkb, msgs, sigs;
};

struct Call {
  blsgpu_ctx* ctx = nullptr;
  blsgpu_batch b{};
  Owned* owned = nullptr;
  int8_t* job_result = nullptr;
  blsgpu_stats* stats = nullptr;
  uint64_t seed = 0;       // message-index hash key (batch_rand::hash_key of the call key)
  batch_rand::Key key{};   // batch scalars: ChaCha20 keystream under this key (batch_rand.hpp)
  uint32_t max_index = 0;  // largest pubkey-table index of the call (table mode)
  Options opt;
  std::vector<Shard> shards;
  std::vector<blsgpu_stats> sst;
  std::vector<int> rc;
  std::atomic<uint32_t> remaining{0};
  std::chrono::steady_clock::time_point t0;
  // completion: async callback, or a waiting synchronous caller
  blsgpu_done_cb done = nullptr;
  void* user = nullptr;
  bool sync = false;
  std::mutex m;
  std::condition_variable cv;
  bool finished = false;
  int status = BLSGPU_OK;
};

}  // namespace blsgpu_rt

namespace {

// ---- contiguous cost-balanced sharding (the rule lodestar_amd/shard.py restates) ------------------------
// cost of a job = its sets + 1/256 per aggregated pubkey; part k ends at the largest job boundary whose
// prefix cost is <= total (k+1)/n_parts; the last part takes the rest.
void shard_rule(const uint32_t* jfs, const uint32_t* spf, uint32_t n_jobs, uint32_t n_parts, uint32_t* out) {
  const uint32_t n_sets = n_jobs ? jfs[n_jobs] : 0;
  std::vector<double> set_prefix(n_sets + 1, 0.0);
  for (uint32_t i = 0; i < n_sets; i++)
    set_prefix[i + 1] = set_prefix[i] + 1.0 + (spf ? (double)(spf[i + 1] - spf[i]) / 256.0 : 0.0);
  std::vector<double> cost(n_jobs + 1);
  for (uint32_t j = 0; j <= n_jobs; j++) cost[j] = set_prefix[n_jobs ? jfs[j] : 0];
  uint32_t j0 = 0;
  out[0] = 0;
  for (uint32_t k = 0; k < n_parts; k++) {
    uint32_t j1;
    if (k + 1 == n_parts) {
      j1 = n_jobs;
    } else {
      const double target = cost[n_jobs] * (k + 1) / n_parts;
      // largest j1 >= j0 with cost[j1] <= target
      j1 = (uint32_t)(std::upper_bound(cost.begin(), cost.end(), target) - cost.begin());
      j1 = j1 ? j1 - 1 : 0;
      j1 = std::max(j0, j1);
    }
    out[k + 1] = j1;
    j0 = j1;
  }
}

// ---- routing calls over devices (the rule lodestar_amd/shard.py route_call restates) ---------------------------
// A call is split over k = min(devices, max(1, n_sets / split_sets)) devices and otherwise routed WHOLE: a gossip
// call (<= 16k sets at the default) runs on one device at the latency of its full size instead of becoming 2k-set
// shards on 8 devices (mid-size runs, each no faster than the whole call), while an epoch-scale call (C4: 32,768 sets)
// still splits.  The k devices are the least loaded (queued + running cost); ties go by distance from the rotating
// `start`, so equal loads spread.  out[0 .. k) = device indices in shard order; returns k.
uint32_t route_rule(uint32_t n_sets, uint32_t n_dev, const int64_t* load, int64_t split_sets, uint32_t start,
                    uint32_t* out) {
  if (n_dev == 0) return 0;
  const uint64_t per = (uint64_t)std::max<int64_t>(1, split_sets);
  const uint32_t k = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n_dev, n_sets / per));
  std::vector<uint32_t> order(n_dev);
  for (uint32_t d = 0; d < n_dev; d++) order[d] = d;
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    if (load[a] != load[b]) return load[a] < load[b];
    return (a + n_dev - start % n_dev) % n_dev < (b + n_dev - start % n_dev) % n_dev;
  });
  std::sort(order.begin(), order.begin() + k);  // shard order = device order (contiguous job ranges)
  for (uint32_t i = 0; i < k; i++) out[i] = order[i];
  return k;
}


// Batch-group size for a run (group_adapt).  A group costs a fixed ~14.7k Montgomery multiplications (its
// MillerLoop(-g1, S) 5,747, final exponentiation 7,835, MSM range 1,085; lodestar_amd/op_counts.json), and when it fails
// every clean job in it is re-checked: per set 1.3k (the set's r_i sig_i; its Miller value is reused) plus its job's
// share of a sub-group check, ~13.6k per 16 jobs (the fallback's level 1, one final exponentiation per kFbSub jobs;
// only failing sub-groups check job by job).  With invalid sets at rate f a group of g sets fails with probability
// 1 - (1 - f)^g, so the expected cost per set is 14.7k / g + (1 - (1 - f)^g) * retry: the size that minimises it over
// powers of two in [8, group_sets].  All valid (f = 0): group_sets (1,024); the reference pool's 1% invalid gossip
// (C5, jobs of 1-3 sets): 32.  C5 by fixed group size (profiles/r06_c5_groups.json): 16 sets 721-797k sets/s, 32
// 753-830k, 64 795-809k, 128 706-724k, 1,024 617-739k; the first form of this model (retry priced at one final
// exponentiation per job) chose 16: 693k.  Per-job results do not depend on the grouping (each job's verdict is its
// own, as the reference's per-job re-verification); only the work does.
uint32_t adapt_group_sets(Device& d, int64_t group_sets, double sets_per_job) {
  double f;
  {
    std::lock_guard<std::mutex> lk(d.fail_mu);
    f = d.fail_rate;
  }
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

// Runs one device's shard on one slot.  Writes job_result[job_begin..job_end).
// A slot's run leaves the device's in-flight count (once): its batch pass is complete on the GPU, so another slot
// may start the next run while this one finishes on the host (results, fallback round trips).
// Host-side timing of run formation (diagnostics): BLSGPU_HOST_TRACE=1 prints, per run, the milliseconds spent
// merging calls, in the host prep before the input copy, and in total before the batch pass is queued.
static bool host_trace() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_HOST_TRACE");
    return v && v[0] == '1';
  }();
  return on;
}
thread_local std::chrono::steady_clock::time_point tl_run_t0;
thread_local double tl_merge_ms = 0;

void release_inflight(Device& d, Slot& sl) {
  {
    std::lock_guard<std::mutex> lk(d.q_mu);
    if (!sl.in_flight) return;
    sl.in_flight = false;
    d.runs_inflight--;
  }
  d.q_cv.notify_all();
}

// With `plan` (group_policy 1), the groups are the plan's job ranges instead of >= group_sets packing, and the
// batchRetries / batchSigsSuccess metrics count the plan's batchable chunks the way the worker does (worker.ts:
// 56-84: a chunk that throws or returns false is one retry; a chunk that verifies adds all its sets).
// scal_words: the shard's batch scalar words (shard_scalars' rule, in the batch's set order); seed: the message
// index's hash key.
int run_shard(Device& d, Slot& sl, const blsgpu_batch& b, const Shard& sh, int8_t* job_result, uint64_t seed,
              const Options& opt, uint32_t max_index, blsgpu_stats& st, const uint64_t* scal_words,
              const std::vector<GroupPlanEntry>* plan = nullptr) {
  const uint32_t n = sh.set_end - sh.set_begin;
  const uint32_t nj = sh.job_end - sh.job_begin;
  if (nj == 0) return BLSGPU_OK;
  HIPCHK(hipSetDevice(d.id));
  const auto t_prep0 = std::chrono::steady_clock::now();
  const uint64_t grow0 = tl_async_grow;
  const uint32_t s0 = sh.set_begin;
  const uint32_t stride = std::max<uint32_t>(n, 1);
  const bool table_mode = b.pk_bytes == nullptr;
  const bool bytes_agg = b.pk_bytes && b.set_pk_first;
  const uint32_t pk_base = b.set_pk_first ? b.set_pk_first[s0] : 0;
  const uint32_t npk = b.set_pk_first ? b.set_pk_first[sh.set_end] - pk_base : 0;
  // the device's table must hold every index of the call (checked per device, under its table lock: a
  // call may race an upload that has reached some devices only)
  if (table_mode && npk && max_index >= d.table_n) return BLSGPU_ERR_ARGS;

  // ---- host-side job structure: groups (contiguous job ranges), scalars ------------------------------------
  std::vector<uint64_t> scal(n);
  std::vector<std::pair<uint32_t, uint32_t>> group_jobs;  // [first job, end job) (shard-relative)
  std::vector<uint8_t> group_batchable;                   // plan only: the group is a batchable chunk
  if (plan) {
    for (const GroupPlanEntry& g : *plan) {
      uint32_t sets = 0;
      for (uint32_t j = g.first; j < g.end; j++)
        sets += b.job_first_set[sh.job_begin + j + 1] - b.job_first_set[sh.job_begin + j];
      if (!sets) continue;  // empty jobs are rejected by the job mask, they join no group
      group_jobs.push_back({g.first, g.end});
      group_batchable.push_back(g.batchable);
    }
  } else {
    // group size: group_sets, or smaller while this device has seen invalid sets (group_adapt, adapt_group_sets)
    const uint32_t gs = opt.group_adapt ? adapt_group_sets(d, opt.group_sets, (double)n / std::max(nj, 1u))
                                        : (uint32_t)opt.group_sets;
    uint32_t cur_sets = 0;
    bool open = false;
    for (uint32_t j = 0; j < nj; j++) {
      const uint32_t gj = sh.job_begin + j;
      const uint32_t a = b.job_first_set[gj] - s0, e = b.job_first_set[gj + 1] - s0;
      const bool batchable = b.job_flags && (b.job_flags[gj] & 1u);
      if (e == a) {
        open = false;
        continue;
      }
      if (!batchable) {
        group_jobs.push_back({j, j + 1});
        open = false;
        continue;
      }
      if (!open || cur_sets >= gs) {
        group_jobs.push_back({j, j});
        cur_sets = 0;
        open = true;
      }
      group_jobs.back().second = j + 1;
      cur_sets += e - a;
    }
  }
  // scalars: the caller applies shard_scalars' rule (each merged call its own key, in the calls' own set order)
  memcpy(scal.data(), scal_words, (size_t)n * 8);
  auto job_sets = [&](uint32_t j) {
    const uint32_t gj = sh.job_begin + j;
    return std::make_pair(b.job_first_set[gj] - s0, b.job_first_set[gj + 1] - s0);
  };
  const uint32_t ng0 = (uint32_t)group_jobs.size();

  // ---- message dedupe and same-message units ----------------------------------------------------------------
  std::vector<uint32_t> msg_idx(n), uniq;
  if (opt.dedupe) {
    MsgIndex mi(n, seed ^ 0x6a09e667f3bcc908ull);
    uniq.reserve(n);
    // hashes a few sets ahead, their table slots prefetched: the probes of a 131k-set run's 1 MB table were cache
    // misses one after another (~1.3-2.6 ms per run on the host)
    const uint8_t* ms = b.msgs + (size_t)s0 * 32;
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
  } else {
    uniq.resize(n);
    for (uint32_t i = 0; i < n; i++) msg_idx[i] = uniq[i] = i;
  }
  const uint32_t n_umsg = (uint32_t)uniq.size();
  const uint32_t nm = std::max<uint32_t>(n_umsg, 1);
  const double t_dedupe_ms = host_trace() ? ms_since(t_prep0) : 0;
  // units: within each group, one unit per distinct message
  std::vector<uint32_t> unit_of_set(n, UINT32_MAX), unit_msg, unit_first, unit_sets, g_unit_first(ng0 + 1, 0);
  bool merged = false;
  if (opt.dedupe && n_umsg < n) {
    std::vector<uint32_t> stamp(n_umsg, UINT32_MAX), unit_of_msg(n_umsg, 0);
    for (uint32_t g = 0; g < ng0; g++) {
      g_unit_first[g] = (uint32_t)unit_msg.size();
      const uint32_t a = job_sets(group_jobs[g].first).first, e = job_sets(group_jobs[g].second - 1).second;
      for (uint32_t i = a; i < e; i++) {
        const uint32_t m = msg_idx[i];
        if (stamp[m] != g) {
          stamp[m] = g;
          unit_of_msg[m] = (uint32_t)unit_msg.size();
          unit_msg.push_back(m);
        }
        unit_of_set[i] = unit_of_msg[m];
      }
    }
    g_unit_first[ng0] = (uint32_t)unit_msg.size();
    merged = unit_msg.size() < (size_t)n;
    if (merged) {
      const uint32_t nu = (uint32_t)unit_msg.size();
      unit_first.assign(nu + 1, 0);
      for (uint32_t i = 0; i < n; i++)
        if (unit_of_set[i] != UINT32_MAX) unit_first[unit_of_set[i] + 1]++;
      for (uint32_t u = 0; u < nu; u++) unit_first[u + 1] += unit_first[u];
      unit_sets.resize(unit_first[nu]);
      std::vector<uint32_t> fill(unit_first.begin(), unit_first.end() - 1);
      for (uint32_t i = 0; i < n; i++)
        if (unit_of_set[i] != UINT32_MAX) unit_sets[fill[unit_of_set[i]]++] = i;
    }
  }
  const uint32_t n_units = merged ? (uint32_t)unit_msg.size() : 0;
  // Miller chunks of the batch pass: each group's items (sets, or units) in chunks of miller_k
  // Small and mid-size runs (<= opt.coop_max pairings, miller_k auto or 1): one cooperative workgroup per pairing
  // (k_miller_coop, lines on the fly) -- 1/6 of the lane-per-chunk loop's latency, at a fraction of its lane
  // efficiency.  The [|z|] chains of the cofactor clearing and the subgroup check go cooperative below opt.coop_g2_max
  // sets.  Up to opt.coop_excl_max items every cooperative workgroup takes a CU to itself (k_common.hpp
  // exclusive_cu_lds): with more workgroups than CUs the padding would serialize them.
  const uint32_t n_items = merged ? n_units : n;
  const bool coop = n_items <= (uint32_t)opt.coop_max && opt.miller_k <= 1;
  const bool coop_g2 = n <= (uint32_t)opt.coop_g2_max;
  // (an urgent run takes the padding only with urgent_excl: on a small CU partition, or beside throughput runs, a
  // workgroup that needs a whole CU waits for one)
  const bool excl = BLSGPU_EXCLUSIVE_SMALL && n_items <= (uint32_t)opt.coop_excl_max && (!sl.urgent || opt.urgent_excl);
  // mk_whole: the items per chunk of whole-loop lanes (one step segment), which the fallback's own accumulations keep
  const uint32_t mk_whole = coop ? 1u : opt.miller_k > 0 ? (uint32_t)opt.miller_k : miller_k_auto(n_items);
  auto group_items = [&](uint32_t g) -> std::pair<uint32_t, uint32_t> {
    if (merged) return {g_unit_first[g], g_unit_first[g + 1]};
    return {job_sets(group_jobs[g].first).first, job_sets(group_jobs[g].second - 1).second};
  };
  // Step segments (miller_plan.hpp): a run of >= 65,536 items that would take the one-lane or two-lane chunk form takes
  // chunks of 8 (or 4) items on the one-lane kernel with J lanes per chunk, each over its own step range, so that
  // n_chunks J lanes still give every SIMD a wave; the F tree then runs per (group, segment) and k_f_fold folds the J
  // heads of a group.  Such a run no longer has one chunk per set, so it gives up keep_f (below): a failed group's
  // jobs re-run their Miller loops; while the device sees enough invalid sets to fail a fifth of the groups, a run
  // that would keep its per-set values stays as it is (miller_plan::hold_kept_values).
  // BLSGPU_MILLER_SEGMENTS = J (diagnostics) switches the rule off: the one-lane form then runs min(J, k) segments
  // at any run size, every other form as ever.
  const AccForm form_whole = acc_form(mk_whole, n_items, opt.miller_lanes, opt.acc6_max, opt.miller_pairs != 0);
  uint32_t mk = mk_whole, segs = 1;
  bool seg_plan = false;  // the automatic rule chose (mk, segs): the batch pass takes the one-lane kernel
  if (opt.miller_segments > 0) {
    if (!coop && form_whole == AccForm::one) segs = (uint32_t)std::min<int64_t>(opt.miller_segments, mk);
  } else if (!coop && opt.miller_lanes == 0 && (form_whole == AccForm::one || form_whole == AccForm::two)) {
    std::vector<uint32_t> g_len(ng0);
    for (uint32_t g = 0; g < ng0; g++) g_len[g] = group_items(g).second - group_items(g).first;
    bool hold = false;  // many failing groups: the kept per-set Miller values are worth more than the plan
    if (opt.keep_f && !merged && mk_whole == 1 && ng0) {
      std::lock_guard<std::mutex> lk(d.fail_mu);
      hold = miller_plan::hold_kept_values(d.fail_rate, (double)n / ng0);
    }
    const miller_plan::Plan pl =
        miller_plan::plan_auto(n_items, g_len.data(), ng0, stride, opt.miller_k > 0 || hold, mk_whole);
    seg_plan = pl.k != mk_whole || pl.segs > 1;
    mk = pl.k, segs = pl.segs;
  }
  const bool interleave = segs > 1 || seg_plan;  // (a one-segment run outside the rule keeps consecutive items)
  std::vector<uint32_t> chunk_first{0}, chunk_items, g_chunks(2 * (size_t)ng0);
  chunk_items.reserve(n);
  for (uint32_t g = 0; g < ng0; g++) {
    const auto ae = group_items(g);
    const auto cr = add_chunks(chunk_first, chunk_items, ae.first, ae.second, mk, interleave);
    g_chunks[2 * g] = cr.first;
    g_chunks[2 * g + 1] = cr.second;
  }
  const uint32_t n_chunks = (uint32_t)chunk_first.size() - 1;
  segs = miller_plan::fit_segments(n_chunks, segs, stride);  // slot j * n_chunks + c of f_chunk (stride words apart)
  MillerSegs msegs{};
  {
    const miller_plan::Segments sg = miller_plan::segments(segs);
    msegs.n = sg.n;
    for (uint32_t j = 0; j <= sg.n; j++) msegs.first[j] = sg.first[j];
    for (uint32_t j = 0; j < sg.n; j++) msegs.dbl[j] = sg.dbl[j];
  }
  // Per-set pairings (no same-message units, one item per chunk): chunk c is set c (the groups cover every set of a
  // non-empty job, in order), so the batch pass's Miller values f_c = MillerLoop(r_c pk_c, H(m_c)) are exactly what a
  // failed group's per-job checks need.  They are copied aside before the F tree multiplies chunks in place, and the
  // fallback takes F_j = prod of its sets' kept values instead of re-running the Miller loops.
  const bool keep_f = opt.keep_f && !merged && mk == 1 && n_chunks == n;
  // A small run (<= opt.small_max sets) leaves most of the chip idle whatever its kernel forms: on an idle device it takes
  // the other stream pair too (speculative MSM, parallel pubkey branch, r_i sig_i), and its fallback checks stay
  // cooperative (latency) instead of lane-per-check (throughput).
  const bool small = n <= (uint32_t)opt.small_max;
  // speculative MSM (kernel pipeline below); spec_large: larger runs on an idle device too
  const bool spec = BLSGPU_STREAM_PAIRS && (small || opt.spec_large) && sl.alone && !opt.serial;
  // A small run on an idle device also forms every r_i sig_i (k_sig_scale) on the idle pubkey stream once its pubkeys
  // and the decode are done: the chip has room, and a failed group's per-job checks then start from the sums instead
  // of a 1.7 ms scaling launch on the fallback's critical path (the batch pass itself never reads them).
  const bool rsig_spec = spec && small && opt.rsig_spec;
  // MSM slices of the groups' set ranges (S_g = sum r_i sig_i).  Runs up to 32k sets (an isolated block's or
  // gossip call's latency) take half slices: twice the bucket workgroups at half the chain, 16k isolated sig_msm
  // 3.55 -> 2.80 ms; merged runs keep full slices (fewer bucket sums to combine: 100-step C2 3.13M vs 3.01M).
  // Small runs (<= 1024 sets) take 32-set slices: a bucket lane's chain of mixed additions is ~len / 8 plus its
  // spread (128 sets: ~25 additions on the slowest lane, 1.26 ms), the window lanes add the few slices up.
  // Up to 32k sets the slice length is opt.msm_slice_mid (default 32: a 16k call's bucket pass is 512 workgroups, every
  // SIMD a wave, ~4 additions per lane) and each range's slices are summed by a pairwise tree of launches
  // (launch_sig_msm tree_slices) instead of the window lanes' serial chain.
  constexpr uint32_t kMsmHalfSliceMaxSets = 32768, kMsmSmallSliceMaxSets = 1024;
  const uint32_t slice_len = n <= kMsmSmallSliceMaxSets  ? 32
                             : n <= kMsmHalfSliceMaxSets ? (uint32_t)opt.msm_slice_mid
                                                         : MSM_SLICE;
  std::vector<uint32_t> slices, range_slices{0};
  uint32_t msm_tree = 0;  // most slices of a range, when the tree sums them
  for (uint32_t g = 0; g < ng0; g++)
    add_slices(slices, range_slices, job_sets(group_jobs[g].first).first, job_sets(group_jobs[g].second - 1).second,
               slice_len);
  const uint32_t n_slices = (uint32_t)(slices.size() / 2);
  // (runs of <= 1,024 sets too: a 1,024-set call's 32 slices summed serially by the window lanes took 2.0 ms beside the
  // cooperative Miller loops and made the signature branch its critical path -- r05 trace)
  if (n <= kMsmHalfSliceMaxSets && opt.msm_tree) {
    for (uint32_t g = 0; g < ng0; g++) msm_tree = std::max(msm_tree, range_slices[g + 1] - range_slices[g]);
    // the tree's launches are sized n_ranges x (most slices of a range): only when the ranges are about equal (one
    // large job beside many single-set groups would launch ~n_ranges x max_pairs idle lanes per level)
    if ((uint64_t)ng0 * msm_tree > 2ull * n_slices) msm_tree = 0;
  }
  // F_g = prod of the group's Miller chunks as a product tree (launch_group_tree): with more than 16384 chunks (merged
  // runs), runs of f_k consecutive chunks first (lane-serial: a 128-lane cooperative product costs ~6x the lane
  // time) down to <= 8192 heads, then pair levels of stride f_k, 2 f_k, ... (one cooperative workgroup per pair);
  // ftree = runs, then the pairs.  Up to 16384 chunks (a 16k call) the tree starts at the chunks: its latency.
  std::vector<uint32_t> ftree, f_level_end;
  uint32_t f_k = 1, f_max = 0;
  // With step segments the tree runs per (segment, group) over the segment-major slots: range j * ng0 + g = the
  // slots j * n_chunks + (group g's chunks); one segment: the groups' chunk ranges themselves.
  const uint32_t n_slots = n_chunks * segs, n_franges = ng0 * segs;
  std::vector<uint32_t> f_rng(2 * (size_t)n_franges);
  for (uint32_t j = 0; j < segs; j++)
    for (uint32_t g = 0; g < ng0; g++) {
      f_rng[2 * ((size_t)j * ng0 + g)] = j * n_chunks + g_chunks[2 * g];
      f_rng[2 * ((size_t)j * ng0 + g) + 1] = j * n_chunks + g_chunks[2 * g + 1];
    }
  if (n_slots > 16384)
    for (const uint32_t heads = opt.f_run_max > 16 ? 256u : 8192u;
         n_slots / f_k > heads && f_k < (uint32_t)opt.f_run_max;)
      f_k *= 2;
  for (uint32_t g = 0; g < ng0; g++) f_max = std::max(f_max, g_chunks[2 * g + 1] - g_chunks[2 * g]);
  if (f_k > 1)
    for (uint32_t r = 0; r < n_franges; r++)
      for (uint32_t x = f_rng[2 * r], e = f_rng[2 * r + 1]; x < e; x += f_k)
        if (std::min(e, x + f_k) - x > 1) {
          ftree.push_back(x);
          ftree.push_back(std::min(e, x + f_k));
        }
  const uint32_t n_fruns = (uint32_t)(ftree.size() / 2);
  for (uint32_t st = f_k; st < f_max; st *= 2) {
    for (uint32_t r = 0; r < n_franges; r++)
      for (uint32_t i = f_rng[2 * r], e = f_rng[2 * r + 1]; i + st < e; i += 2 * st) {
        ftree.push_back(i);
        ftree.push_back(i + st);
      }
    f_level_end.push_back((uint32_t)(ftree.size() / 2) - n_fruns);
  }
  // sets that aggregate >= 2 keys (one wave each in k_pk_aggregate); one-key sets are read by k_pk_finish
  std::vector<uint32_t> agg_sets;
  if (table_mode || bytes_agg)
    for (uint32_t i = 0; i < n; i++)
      if (b.set_pk_first[s0 + i + 1] - b.set_pk_first[s0 + i] >= 2) agg_sets.push_back(i);

  // ---- stage inputs in the pinned arena and copy it to the device in one transfer ------------------------
  // arena (256-B aligned sections): scalars | job_first_set | sigs (192 B each) | sig_len | unique msgs |
  // msg_idx | set ranges | f ranges | units (first, sets, msg) | chunks | agg sets | MSM slices | F tree | pk section
  const double t_struct_ms = host_trace() ? ms_since(t_prep0) : 0;
  // signatures at a 96-byte stride when no set carries a 192-byte (uncompressed) one: half the staging and copy
  uint32_t sig_w = 96;
  for (uint32_t i = 0; i < n; i++)
    if (b.sig_len[s0 + i] == 192) {
      sig_w = 192;
      break;
    }
  const size_t o_scal = 0, o_jobs = al256(o_scal + (size_t)n * 8), o_sigs = al256(o_jobs + (size_t)(nj + 1) * 4),
               o_siglen = al256(o_sigs + (size_t)n * sig_w), o_umsg = al256(o_siglen + (size_t)n * 4),
               o_midx = al256(o_umsg + (size_t)n_umsg * 32), o_ranges = al256(o_midx + (size_t)n * 4),
               o_franges = al256(o_ranges + (size_t)std::max(ng0, 1u) * 8),
               o_ufirst = al256(o_franges + (size_t)std::max(n_franges, 1u) * 8),
               o_usets = al256(o_ufirst + (size_t)(n_units + 1) * 4), o_umsgi = al256(o_usets + (size_t)unit_sets.size() * 4),
               o_cfirst = al256(o_umsgi + (size_t)n_units * 4), o_citems = al256(o_cfirst + (size_t)(n_chunks + 1) * 4),
               o_agg = al256(o_citems + chunk_items.size() * 4), o_slices = al256(o_agg + agg_sets.size() * 4),
               o_rslices = al256(o_slices + slices.size() * 4), o_ftree = al256(o_rslices + range_slices.size() * 4),
               o_pk = al256(o_ftree + ftree.size() * 4);
  size_t in_bytes;
  if (table_mode)
    in_bytes = al256(o_pk + (size_t)(n + 1) * 4) + (size_t)npk * 4;
  else if (bytes_agg)
    in_bytes = al256(o_pk + (size_t)(n + 1) * 4) + (size_t)npk * 96;
  else
    in_bytes = o_pk + (size_t)n * 96;
  const size_t o_pk2 = al256(o_pk + (size_t)(n + 1) * 4);
  // the urgent slot runs on its own two stream pairs (Device::ust), every run on pair 0 with pair 1 idle beside it
  hipStream_t* const dst = sl.urgent ? d.ust : d.st;
  const int npairs = sl.urgent ? 2 : d.npairs;
  const int par = sl.urgent ? 0 : BLSGPU_STREAM_PAIRS ? (int)(d.run_seq.fetch_add(1) % (uint32_t)npairs) : 0;
  const int other = (par + 1) % npairs;
  hipStream_t s = BLSGPU_STREAM_PAIRS ? dst[2 * par] : dst[kSig];
  sl.set_stream(s);  // buffer growth of the batch pass, ordered before the input copy on the same stream
  sl.h_in.ensure(in_bytes);
  sl.d_in.ensure(in_bytes);
  uint8_t* const hin = sl.h_in.p;
  memcpy(hin + o_scal, scal.data(), (size_t)n * 8);
  uint32_t* hjobs = reinterpret_cast<uint32_t*>(hin + o_jobs);
  for (uint32_t j = 0; j < nj; j++) hjobs[j] = job_sets(j).first;
  hjobs[nj] = n;
  uint8_t* hsigs = hin + o_sigs;
  uint32_t* hsiglen = reinterpret_cast<uint32_t*>(hin + o_siglen);
  if (b.sig_stride == sig_w) {  // one block (the decoder reads only the bytes a set's length makes valid)
    memcpy(hsigs, b.sigs + (size_t)s0 * sig_w, (size_t)n * sig_w);
    memcpy(hsiglen, b.sig_len + s0, (size_t)n * 4);
  } else {
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t len = b.sig_len[s0 + i];
      const uint32_t cl = (len == 96 || len == 192) ? len : 0;
      memcpy(hsigs + (size_t)i * sig_w, b.sigs + (size_t)(s0 + i) * b.sig_stride, cl);
      hsiglen[i] = len;
    }
  }
  for (uint32_t u = 0; u < n_umsg; u++) memcpy(hin + o_umsg + (size_t)u * 32, b.msgs + (size_t)(s0 + uniq[u]) * 32, 32);
  memcpy(hin + o_midx, msg_idx.data(), (size_t)n * 4);
  uint32_t* hranges = reinterpret_cast<uint32_t*>(hin + o_ranges);
  uint32_t* hfranges = reinterpret_cast<uint32_t*>(hin + o_franges);
  for (uint32_t g = 0; g < ng0; g++) {
    hranges[2 * g] = job_sets(group_jobs[g].first).first;
    hranges[2 * g + 1] = job_sets(group_jobs[g].second - 1).second;
  }
  memcpy(hfranges, f_rng.data(), f_rng.size() * 4);
  memcpy(hin + o_cfirst, chunk_first.data(), chunk_first.size() * 4);
  memcpy(hin + o_citems, chunk_items.data(), chunk_items.size() * 4);
  if (!agg_sets.empty()) memcpy(hin + o_agg, agg_sets.data(), agg_sets.size() * 4);
  if (!slices.empty()) memcpy(hin + o_slices, slices.data(), slices.size() * 4);
  memcpy(hin + o_rslices, range_slices.data(), range_slices.size() * 4);
  if (!ftree.empty()) memcpy(hin + o_ftree, ftree.data(), ftree.size() * 4);
  if (merged) {
    memcpy(hin + o_ufirst, unit_first.data(), (size_t)(n_units + 1) * 4);
    memcpy(hin + o_usets, unit_sets.data(), unit_sets.size() * 4);
    memcpy(hin + o_umsgi, unit_msg.data(), (size_t)n_units * 4);
  }
  if (table_mode || bytes_agg) {
    uint32_t* hpkfirst = reinterpret_cast<uint32_t*>(hin + o_pk);
    for (uint32_t i = 0; i <= n; i++) hpkfirst[i] = b.set_pk_first[s0 + i] - pk_base;
    if (table_mode)
      memcpy(hin + o_pk2, b.pk_index + pk_base, (size_t)npk * 4);
    else
      memcpy(hin + o_pk2, b.pk_bytes + (size_t)pk_base * 96, (size_t)npk * 96);
  } else {
    memcpy(hin + o_pk, b.pk_bytes + (size_t)s0 * 96, (size_t)n * 96);
  }

  // byte arrays: flags n | mflags nm | unit_ok n | status 3n | include n ; results: job_err nj | ok ng
  const size_t ob_flags = 0, ob_mflags = al256(n), ob_unit = al256(ob_mflags + nm), ob_status = al256(ob_unit + n),
               ob_include = al256(ob_status + 3 * (size_t)stride), ob_spec = al256(ob_include + stride),
               bytes_total = al256(ob_spec + stride);
  sl.d_bytes.ensure(bytes_total);
  const uint32_t max_ranges = std::max<uint32_t>(std::max(ng0, nj), 1);
  const size_t o_ok = al256(nj), res_bytes = o_ok + max_ranges;
  sl.d_res.ensure(res_bytes);
  sl.h_res.ensure(res_bytes);
  sl.d_S.ensure((size_t)W_G2J * max_ranges);
  sl.d_F.ensure((size_t)W_FP12 * max_ranges);
  sl.d_G.ensure((size_t)W_FP12 * std::max<uint32_t>(ng0, 1));
  sl.d_msmB.ensure((size_t)MSM_BUCKET_WORDS * std::max<uint32_t>(n_slices, 1));
  sl.d_msmW.ensure((size_t)MSM_WINDOW_WORDS * max_ranges);
  // work area: per set sig_aff, pk_jac, pk_aff, f_chunk, the G1 window table of r_i pk_i, inv_buf (+ per unit
  // unit_p), per message h_aff, h_jac, h_norm, h_prep
  const size_t per_set = W_G2A + W_G1J + W_G1A + W_FP12 + 8 * W_G1J + 2 * W_FP + (merged ? W_G1A : 0);
  sl.d_work.ensure((size_t)stride * per_set + (size_t)nm * (W_G2A + W_G2J + W_FP + 14 * W_FP + 2 * W_G2J));
  sl.d_lines.ensure((size_t)nm * kMillerLineWords);
  if (keep_f) sl.d_fkeep.ensure((size_t)stride * W_FP12);
  if (segs > 1) sl.d_fseg.ensure((size_t)W_FP12 * n_franges);
  if (rsig_spec) sl.d_fb.ensure((size_t)stride * 9 * W_G2J);
  uint8_t* const din = sl.d_in.p;
  uint8_t* const d_ok0 = sl.d_res.p + o_ok;

  PipelineBuffers pb;
  memset(&pb, 0, sizeof pb);
  pb.n = stride;
  pb.sigs = din + o_sigs;
  pb.sig_len = reinterpret_cast<uint32_t*>(din + o_siglen);
  pb.sig_stride = sig_w;
  pb.pk_bytes = table_mode ? nullptr : din + (bytes_agg ? o_pk2 : o_pk);
  pb.set_pk_first = (table_mode || bytes_agg) ? reinterpret_cast<uint32_t*>(din + o_pk) : nullptr;
  pb.pk_index = table_mode ? reinterpret_cast<uint32_t*>(din + o_pk2) : nullptr;
  pb.pk_table = d.table.p;
  pb.pk_table_n = d.table_n;
  pb.agg_sets = reinterpret_cast<uint32_t*>(din + o_agg);
  pb.n_agg = (uint32_t)agg_sets.size();
  pb.pk_direct1 = 1;
  pb.scalars = reinterpret_cast<uint64_t*>(din + o_scal);
  pb.job_first_set = reinterpret_cast<uint32_t*>(din + o_jobs);
  pb.n_jobs = nj;
  pb.umsgs = din + o_umsg;
  pb.msg_idx = reinterpret_cast<uint32_t*>(din + o_midx);
  pb.n_umsg = n_umsg;
  pb.nm = nm;
  pb.n_units = n_units;
  pb.unit_set_first = reinterpret_cast<uint32_t*>(din + o_ufirst);
  pb.unit_sets = reinterpret_cast<uint32_t*>(din + o_usets);
  pb.unit_msg = reinterpret_cast<uint32_t*>(din + o_umsgi);
  uint32_t* w = sl.d_work.p;
  pb.sig_aff = w; w += (size_t)stride * W_G2A;
  pb.pk_jac = w; w += (size_t)stride * W_G1J;
  pb.pk_aff = w; w += (size_t)stride * W_G1A;
  pb.rsig = nullptr;  // S comes from the MSM (k_msm.hip), not from per-set scalings
  pb.f_chunk = w; w += (size_t)stride * W_FP12;
  pb.scal_tab = w; w += (size_t)stride * 8 * W_G1J;
  if (merged) {
    pb.unit_p = w; w += (size_t)stride * W_G1A;
  }
  pb.n_chunks = n_chunks;
  pb.chunk_first = reinterpret_cast<uint32_t*>(din + o_cfirst);
  pb.chunk_items = reinterpret_cast<uint32_t*>(din + o_citems);
  pb.inv_buf = w; w += (size_t)stride * W_FP;  // n_umsg <= n
  pb.inv_buf_pk = w; w += (size_t)stride * W_FP;  // the pubkey branch's own (it runs beside the hash branch)
  pb.h_aff = w; w += (size_t)nm * W_G2A;
  pb.h_jac = w; w += (size_t)nm * W_G2J;
  pb.h_norm = w; w += (size_t)nm * W_FP;
  pb.h_prep = w; w += (size_t)nm * 14 * W_FP;
  pb.h_q = w;
  pb.lines = sl.d_lines.p;
  uint8_t* const db = sl.d_bytes.p;
  pb.flags = db + ob_flags;
  pb.mflags = db + ob_mflags;
  pb.unit_ok = db + ob_unit;
  pb.status = reinterpret_cast<int8_t*>(db + ob_status);
  pb.include = db + ob_include;
  pb.job_err = reinterpret_cast<int8_t*>(sl.d_res.p);

  // ---- kernel pipeline ------------------------------------------------------------------------------------
  // DAG of one run on the device's streams (shared by its slots):
  //   signatures (s):    input copy -> decode -> [pubkeys done] job mask -> MSM -> MillerLoop(-g1, S_g)
  //   messages (sm):     hash_to_G2 -> affine -> Miller lines -> [job mask done] Miller accumulation -> F reduction
  //   pubkeys (sp):      aggregate -> r_i pk_i -> affine
  //   tail (stl):        [S_g Miller + F done] final exponentiation per group -> results copy
  // With stream pairs (BLSGPU_STREAM_PAIRS) the pubkey and tail branches run on the run's signature stream (they are
  // short next to the message branch; see sp below for small runs) and consecutive runs use the other pair; without,
  // each branch has its own stream shared by every run.
  const bool prof = opt.profile;
  // Large (merged) runs meet a chip full of one-wave-per-SIMD stage kernels: the signature branch's cooperative tails
  // (Horner passes, MillerLoop(-g1, S)) waited for free SIMD groups there, so they run on single lanes
  const bool lane_tail = opt.lane_tail_min > 0 && n >= (uint32_t)opt.lane_tail_min;
  // A small run that found the device idle puts its pubkey branch on the other pair's (idle) signature stream, beside
  // its own signature decode and subgroup checks instead of in front of them: the signature branch was a small
  // call's critical path (C1 serial trace: 7.25 ms vs the message branch's 6.15).
  hipStream_t sm = BLSGPU_STREAM_PAIRS ? dst[2 * par + 1] : dst[kMsg],
              sp = BLSGPU_STREAM_PAIRS ? (small && sl.alone ? dst[2 * other] : s) : dst[kPk],
              stl = BLSGPU_STREAM_PAIRS ? s : dst[kTail];
  if (opt.serial) sm = sp = stl = s;
  auto beg = [&](int k, hipStream_t st) {
    if (prof) HIPCHK(hipEventRecord(sl.ev[2 * k], st));
  };
  auto end = [&](int k, hipStream_t st) {
    if (prof) HIPCHK(hipEventRecord(sl.ev[2 * k + 1], st));
  };
  {
    std::unique_lock<std::mutex> enq(d.enq_mu, std::defer_lock);
    if (!sl.urgent) enq.lock();  // the urgent lane's streams are its own: nothing to keep in order with
    st.host_ms = ms_since(tl_run_t0);  // the slot picked the run -> its input copy is queued
    if (host_trace())
      fprintf(stderr,
              "[blsgpu host] run %u sets: merge %.2f ms, prep %.2f ms (dedupe %.2f, structure %.2f), pick-to-copy %.2f "
              "ms, %zu B in, %u Miller chunks of %u x %u segments\n",
              n, tl_merge_ms, ms_since(t_prep0), t_dedupe_ms, t_struct_ms, ms_since(tl_run_t0), in_bytes, n_chunks, mk,
              segs);
    // The input copy goes on the run's signature stream, or (copy_stream, when none of the run's buffers was
    // reallocated in that stream's order) on the device's table stream: a previous run's tail still queued on the
    // signature stream of this pair then delays only this run's signature branch, not its message branch
    const bool own_copy = opt.copy_stream && !opt.serial && !sl.urgent && tl_async_grow == grow0;
    hipStream_t sc = own_copy ? d.table_stream : s;
    HIPCHK(hipMemcpyAsync(din, hin, in_bytes, hipMemcpyHostToDevice, sc));
    HIPCHK(hipEventRecord(sl.join_in, sc));
    if (own_copy) HIPCHK(hipStreamWaitEvent(s, sl.join_in, 0));
    HIPCHK(hipStreamWaitEvent(sm, sl.join_in, 0));
    HIPCHK(hipStreamWaitEvent(sp, sl.join_in, 0));
    // messages
    beg(1, sm);
    launch_hash_to_g2(pb, sm, coop_g2, excl);
    launch_h_affine(pb, sm);
    end(1, sm);
    beg(kStages, sm);
    if (!coop) {
      // two lanes per message while one lane each would leave SIMDs idle (the same rule as the accumulation's)
      const bool two = opt.lines_lanes == 2;  // lane pairs, two waves per SIMD: C2 +2-4% (profiles/r05_pairs_ab.json)
      if (two)
        launch_miller_lines2(pb, sm);
      else
        launch_miller_lines(pb, sm);
    }
    end(kStages, sm);
    // pubkeys
    beg(2, sp);
    if ((table_mode || bytes_agg) && pb.n_agg) launch_pk_aggregate(pb, n, sp);
    end(2, sp);
    beg(3, sp);
    launch_pk_finish(pb, n, sp);
    launch_pk_affine(pb, n, sp);
    end(3, sp);
    HIPCHK(hipEventRecord(sl.join_pk, sp));
    // signatures, then the batch equation.  A small run on an idle device starts its MSM speculatively right after
    // the decode, on the other pair's (idle) message stream, over the sets that decoded (spec mask), while the
    // subgroup checks, the pubkeys and the job mask finish: S then includes the sets the job mask drops later (a
    // failed subgroup check or pubkey, a job's other sets).  That only changes the failure path: a group whose S
    // holds a dropped set fails its equation (barring a negligible r_i coincidence; an infinity signature never
    // enters, and a dropped valid signature is in G2, so its term e(-g1, r sig) != 1) and its jobs are re-checked one
    // by one with exact masks (the fallback), while a clean group's S is exact.  Saves the MSM's ~1.5 ms on the
    // signature branch of a 128-set call.
    hipStream_t smsm = spec ? dst[2 * other + 1] : s;
    PipelineBuffers pbm = pb;
    if (spec) pbm.include = db + ob_spec;
    beg(0, s);
    launch_sig_decode(pb, n, s, coop_g2, spec ? sl.join_dec : nullptr, excl);
    end(0, s);
    const uint32_t* d_slices = reinterpret_cast<uint32_t*>(din + o_slices);
    const uint32_t* d_rslices = reinterpret_cast<uint32_t*>(din + o_rslices);
    if (rsig_spec) {  // after the pubkey branch on sp (its own work comes first) and the decode (+ subgroup checks)
      HIPCHK(hipEventRecord(sl.join_rsig, s));
      HIPCHK(hipStreamWaitEvent(sp, sl.join_rsig, 0));
      PipelineBuffers pq = pb;
      pq.rsig = sl.d_fb.p;
      pq.scal_tab = sl.d_fb.p + (size_t)stride * W_G2J;
      launch_sig_scale(pq, n, sp);
      HIPCHK(hipEventRecord(sl.join_rsig, sp));
    }
    if (spec) {
      HIPCHK(hipStreamWaitEvent(smsm, sl.join_dec, 0));
      launch_spec_mask(pb, n, pbm.include, smsm);
      launch_sig_msm(pbm, d_slices, n_slices, d_rslices, ng0, sl.d_msmB.p, sl.d_msmW.p, sl.d_S.p, smsm, false,
                     msm_tree);
      HIPCHK(hipEventRecord(sl.join_msm, smsm));
    }
    HIPCHK(hipStreamWaitEvent(s, sl.join_pk, 0));
    beg(4, s);
    launch_job_mask(pb, s);
    HIPCHK(hipEventRecord(sl.join_mask, s));
    // the message branch continues with the Miller accumulation once the include mask exists
    HIPCHK(hipStreamWaitEvent(sm, sl.join_mask, 0));
    beg(5, sm);
    if (merged) launch_unit_aggregate(pb, sm);
    if (coop)
      launch_miller_coop(pb, merged, sm, excl);
    else if (seg_plan)
      launch_miller_acc(pb, merged, sm, &msegs);
    else
      launch_miller_acc_auto(pb, merged, sm, mk, opt.miller_lanes, opt.acc6_max, opt.miller_pairs != 0, &msegs);
    end(5, sm);
    if (keep_f && opt.keep_copy == 1)
      launch_copy_words(sl.d_fkeep.p, pb.f_chunk, (size_t)stride * W_FP12, sm);
    else if (keep_f)
      HIPCHK(hipMemcpyAsync(sl.d_fkeep.p, pb.f_chunk, (size_t)stride * W_FP12 * 4, hipMemcpyDeviceToDevice, sm));
    const uint32_t* d_franges = reinterpret_cast<uint32_t*>(din + o_franges);
    beg(6, sm);
    const uint32_t* d_ftree = reinterpret_cast<uint32_t*>(din + o_ftree);
    launch_group_tree(pb, d_franges, ng0, d_ftree, n_fruns, d_ftree + 2 * (size_t)n_fruns, f_level_end, sl.d_F.p, sm,
                      &msegs, sl.d_fseg.p);
    end(6, sm);
    HIPCHK(hipEventRecord(sl.join_msg, sm));
    if (spec)
      HIPCHK(hipStreamWaitEvent(s, sl.join_msm, 0));
    else
      launch_sig_msm(pb, d_slices, n_slices, d_rslices, ng0, sl.d_msmB.p, sl.d_msmW.p, sl.d_S.p, s,
                     lane_tail && (opt.lane_tail_parts & 1), msm_tree);
    end(4, s);
    // MillerLoop(-g1, S_g) of every group now, while the message branch still runs -- or (tail_on_msg) after it, on
    // the pair's high-priority message stream with the final exponentiations: a run's cooperative tail kernels then
    // take free SIMDs before the next runs' stage kernels, and they never hold the signature stream the next run on
    // this pair copies its inputs on
    const bool tail_msg = opt.tail_on_msg && !opt.serial && BLSGPU_STREAM_PAIRS;
    hipStream_t sg = s;
    // spec_gsm: a speculative run (the device was idle when it formed) runs MillerLoop(-g1, S) right behind its MSM on
    // the other pair's message stream (high priority, nothing else queued on it yet): it starts on a nearly idle chip.
    // On the signature stream it would wait behind the run's own Miller accumulation and then behind the next run's
    // stage kernels -- a three-wave workgroup gets no CU while another run's waves fill every SIMD -- and it held the
    // burst's first run, and so the pair, for ~36 ms of the driver's 20-step window.  Measured equal (the next runs then
    // wait behind it on the other pair instead, profiles/r06_ramp_ab.json): off by default.
    if (spec && opt.spec_gsm && !tail_msg) sg = smsm;
    if (tail_msg) {
      HIPCHK(hipEventRecord(sl.join_gsm, s));
      HIPCHK(hipStreamWaitEvent(sm, sl.join_gsm, 0));
      sg = stl = sm;
    }
    beg(kStages + 1, sg);
    launch_group_sig_miller(sl.d_S.p, ng0, sl.d_G.p, sg, excl && coop,
                            lane_tail && (opt.lane_tail_parts & 2));
    end(kStages + 1, sg);
    HIPCHK(hipEventRecord(sl.join_gsm, sg));
    HIPCHK(hipStreamWaitEvent(stl, sl.join_gsm, 0));
    HIPCHK(hipStreamWaitEvent(stl, sl.join_msg, 0));
    if (rsig_spec) HIPCHK(hipStreamWaitEvent(stl, sl.join_rsig, 0));  // the run completes with its r_i sig_i
    beg(7, stl);
    launch_group_check(sl.d_S.p, sl.d_F.p, ng0, d_ok0, stl, nullptr, 0, sl.d_G.p, excl && coop);
    end(7, stl);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sl.h_res.p, sl.d_res.p, o_ok + ng0, hipMemcpyDeviceToHost, stl));
    HIPCHK(hipEventRecord(sl.done, stl));
  }
  if (opt.early_release && !opt.serial) {
    // the run leaves the in-flight count once its message branch is done: its remaining tail (the signature side's
    // window sums / Horner / MillerLoop(-g1, S) and the final exponentiations) is short on a chip with room and must
    // not hold a pipeline place while the next runs' heavy kernels starve it
    HIPCHK(hipEventSynchronize(sl.join_msg));
    release_inflight(d, sl);
  }
  HIPCHK(hipEventSynchronize(sl.done));
  if (batch_rand::take_injection(g_fail_run_skip, g_fail_run_count)) throw HipError{hipErrorLaunchFailure};
  release_inflight(d, sl);
  st.groups += ng0;
  st.unique_messages += n_umsg;
  st.pairing_units += merged ? n_units : n;
  st.miller_chunks += n_chunks;
  st.run_sets = n;
  if (prof) {
    for (int k = 0; k < kStages; k++) {
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, sl.ev[2 * k], sl.ev[2 * k + 1]));
      if (k == 5 || k == 7) {  // Miller stage = lines + accumulation; group check = MillerLoop(-g1, S) + final exp.
        const int x = k == 5 ? kStages : kStages + 1;
        float ml = 0;
        HIPCHK(hipEventElapsedTime(&ml, sl.ev[2 * x], sl.ev[2 * x + 1]));
        ms += ml;
      }
      st.stage_ms[k] += ms;
    }
  }

  // ---- per-job results -------------------------------------------------------------------------------------
  std::vector<int> jr(nj, 0);
  for (uint32_t j = 0; j < nj; j++) {
    const int err = (int8_t)sl.h_res.p[j];
    jr[j] = err ? -err : 2;  // 2 = pending
  }
  std::vector<uint32_t> retry;  // clean jobs of failed groups, each re-checked on its own
  std::vector<uint32_t> failed_g;  // groups whose own equation failed (their clean jobs are in retry)
  for (uint32_t g = 0; g < ng0; g++) {
    std::vector<uint32_t> clean;
    bool dropped = false;  // a rejected job of the group has sets (they may sit in a speculative S_g)
    for (uint32_t j = group_jobs[g].first; j < group_jobs[g].second; j++) {
      if (jr[j] == 2)
        clean.push_back(j);
      else if (job_sets(j).second > job_sets(j).first)
        dropped = true;
    }
    // Speculative MSM (spec): S_g summed every decoded set of the group, so a group with a rejected job is not the
    // equation of its clean jobs -- its verdict (pass or fail) is not read; every clean job is re-checked on its own
    // with exact masks (the fallback's own S_j, F_j).  Only the failure path pays.  The subgroup check's writes to
    // sig_aff, unordered with the speculative MSM's reads, can likewise only reach such a group.
    if (spec && dropped && !clean.empty()) {
      if (plan && group_batchable[g]) st.batch_retries++;
      if (!plan && clean.size() > 1) st.batch_retries++;
      retry.insert(retry.end(), clean.begin(), clean.end());
      continue;
    }
    if (plan) {  // the worker's metrics: a chunk with a throwing job or a failed equation is one retry
      if (!group_batchable[g]) {
      } else if (clean.size() == group_jobs[g].second - group_jobs[g].first && sl.h_res.p[o_ok + g]) {
        st.batch_sigs_success += job_sets(group_jobs[g].second - 1).second - job_sets(group_jobs[g].first).first;
      } else {
        st.batch_retries++;
      }
    }
    if (clean.empty()) continue;
    // A failed group's clean jobs are re-verified one by one, also when the group held a single clean job (its
    // equation was that job's own): the reference re-verifies every job of a failed chunk whatever its size
    // (worker.ts:76-98), so a job's false is always its own check's answer, never only its group's.
    if (plan) {
      if (sl.h_res.p[o_ok + g]) {
        for (uint32_t j : clean) jr[j] = 1;
      } else {
        retry.insert(retry.end(), clean.begin(), clean.end());
        failed_g.push_back(g);
      }
      continue;
    }
    if (sl.h_res.p[o_ok + g]) {
      for (uint32_t j : clean) jr[j] = 1;
      if (group_jobs[g].second - group_jobs[g].first > 1)
        for (uint32_t j : clean) st.batch_sigs_success += job_sets(j).second - job_sets(j).first;
    } else {
      if (clean.size() > 1) st.batch_retries++;
      retry.insert(retry.end(), clean.begin(), clean.end());
      failed_g.push_back(g);
    }
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
  if (!retry.empty()) {
    constexpr uint32_t kFbSub = 16;
    // from this many sub-groups on, one lane per sub-group combines its 16 entries (instead of a wave per
    // sub-group).  The checks stay one 128-lane workgroup each: a lane-per-check final exponentiation gave the
    // same C5 throughput at 56% more latency (profiles/r02_configs_fallback.json), and its call frames need
    // 8-12 KB/lane of scratch, which the per-queue scratch reservation does not always get.
    constexpr uint32_t kFbLaneMin = 128;
    const uint32_t nr = (uint32_t)retry.size();
    // the fallback runs on the slot's own stream (the batch pass is complete: sl.done was waited for), its buffers grow
    // there
    const hipStream_t sfb = sl.fb ? sl.fb : stl;
    sl.set_stream(sfb);
    std::vector<uint32_t> rfirst{0}, ritems, rr(2 * (size_t)nr), rf(2 * (size_t)nr), rsl, rrs{0}, rset;
    for (uint32_t q = 0; q < nr; q++) {
      const auto js = job_sets(retry[q]);
      rr[2 * q] = js.first;
      rr[2 * q + 1] = js.second;
      add_slices(rsl, rrs, js.first, js.second);
      for (uint32_t i = js.first; i < js.second; i++) rset.push_back(i);
      if (keep_f) {  // F_j from the kept per-set values: chunk = set
        rf[2 * q] = js.first;
        rf[2 * q + 1] = js.second;
        continue;
      }
      const auto cr = add_chunks(rfirst, ritems, js.first, js.second, mk_whole);
      rf[2 * q] = cr.first;
      rf[2 * q + 1] = cr.second;
    }
    // per-set scalings instead of per-job MSMs while the jobs are small (a 1-3-set job would leave a 128-lane MSM
    // workgroup idle); the speculative batch-pass scalings (rsig_spec) then save the scaling launch.  Large retried jobs
    // (e.g. two failing 1k-set block jobs) take the bucket MSM and the wave-per-job reduce even when the run made the
    // scalings: one lane summing a job's thousands of r_i sig_i and multiplying its Fp12 values in series is slower.
    const bool small_jobs = rset.size() < (size_t)32 * nr;
    // A small run (cooperative forms: the chip is far from full) checks every retried job directly in ONE launch --
    // up to kFbDirectMax checks run side by side (4 cooperative workgroups per CU) -- instead of sub-groups, a host
    // round trip and then the jobs of the failing sub-groups: one check round instead of two.  (Cooperative checks slow
    // down with their number -- 96 in 3.1 ms, 257 in 5.7, 675 in 8.1, 1,024 in 16 ms: profiles/r05_fallback_* -- so
    // beyond ~640 jobs two rounds of few checks are faster; C5's 514 retried jobs: p50 14.7 ms direct, 16.6 in two
    // rounds.)
    constexpr uint32_t kFbDirectMax = 640;
    // Large runs under load (other runs in flight: merged calls, throughput first) take lane-per-check launches of many
    // checks, and with many retried jobs (>= fb_direct_min: dense failures, e.g. C5's 1% invalid sets fail every
    // group) check every job directly in ONE lane launch: three times the checks of the sub-group round trip, but one
    // ~25 ms lane round instead of two, and the run's call latency is what bounds a loaded device's throughput
    // (calls in flight / latency).  Small runs and runs on an idle device keep the cooperative checks' latency.
    const bool busy = (!small && !sl.alone) || opt.fb_force_busy;
    auto lane_checks = [&](uint32_t count) { return busy && opt.fb_lane_min > 0 && count >= (uint32_t)opt.fb_lane_min; };
    const bool direct = (small && nr <= kFbDirectMax) || (busy && opt.fb_direct_min > 0 && nr >= (uint32_t)opt.fb_direct_min);
    const uint32_t nsub = !direct && nr >= 2 * kFbSub ? (nr + kFbSub - 1) / kFbSub : 0;
    // One check launch of `count` entries (sel null: entries 0 .. ng): cooperative checks (small runs, idle device), or
    // for many checks under load MillerLoop(-g1, S) one lane per entry and the final exponentiation on six lanes per
    // check (fb_check6, gt6.hpp), or everything one lane per check
    auto fb_check = [&](const uint32_t* S, const uint32_t* F, uint32_t ng, uint8_t* ok, const uint32_t* sel,
                        uint32_t count) {
      if (lane_checks(count) && opt.fb_check6 == 2) {  // the Miller loop on six lanes too, from stored lines
        sl.d_lines.ensure((size_t)ng * kMillerLineWords);
        sl.d_fbflags.ensure(ng);
        launch_check6_miller(S, F, ng, ok, sfb, sel, count, sl.d_lines.p, sl.d_fbflags.p);
      } else if (lane_checks(count) && opt.fb_check6) {
        sl.d_G.ensure((size_t)W_FP12 * ng);
        launch_group_sig_miller_sel(S, ng, sel, count, sl.d_G.p, sfb);
        launch_group_check6(F, sl.d_G.p, ng, ok, sfb, sel, count);
      } else {
        launch_group_check(S, F, ng, ok, sfb, sel, count, nullptr, false, lane_checks(count));
      }
    };
    std::vector<uint32_t> subr(2 * (size_t)nsub);
    for (uint32_t t = 0; t < nsub; t++) {
      subr[2 * t] = t * kFbSub;
      subr[2 * t + 1] = std::min(nr, (t + 1) * kFbSub);
    }
    const uint32_t nc = (uint32_t)rfirst.size() - 1;
    const uint32_t nrs = (uint32_t)(rsl.size() / 2);
    const size_t o_rsl = 4 * (size_t)nr + rfirst.size() + ritems.size(), o_rrs = o_rsl + rsl.size(),
                 o_rset = o_rrs + rrs.size(), o_sub = o_rset + rset.size(), o_sel = o_sub + subr.size();
    const size_t words = o_sel + nr;
    sl.h_list.ensure(words);
    sl.d_list.ensure(words);
    uint32_t* hl = sl.h_list.p;
    memcpy(hl, rr.data(), rr.size() * 4);
    memcpy(hl + 2 * (size_t)nr, rf.data(), rf.size() * 4);
    memcpy(hl + 4 * (size_t)nr, rfirst.data(), rfirst.size() * 4);
    memcpy(hl + 4 * (size_t)nr + rfirst.size(), ritems.data(), ritems.size() * 4);
    memcpy(hl + o_rsl, rsl.data(), rsl.size() * 4);
    memcpy(hl + o_rrs, rrs.data(), rrs.size() * 4);
    memcpy(hl + o_rset, rset.data(), rset.size() * 4);
    if (nsub) memcpy(hl + o_sub, subr.data(), subr.size() * 4);
    sl.d_ok.ensure(nr + nsub);
    sl.h_ok.ensure(nr + nsub);
    sl.d_S.ensure((size_t)W_G2J * (nr + nsub));
    sl.d_F.ensure((size_t)W_FP12 * (nr + nsub));
    uint32_t* const dS = sl.d_S.p;  // per-job S_j, F_j (stride nr), then the sub-groups' (stride nsub)
    uint32_t* const dF = sl.d_F.p;
    uint32_t* const dS_sub = sl.d_S.p + (size_t)W_G2J * nr;
    uint32_t* const dF_sub = sl.d_F.p + (size_t)W_FP12 * nr;
    HIPCHK(hipMemcpyAsync(sl.d_list.p, hl, o_sel * 4, hipMemcpyHostToDevice, sfb));
    PipelineBuffers pr = pb;
    pr.n_chunks = nc;
    pr.chunk_first = sl.d_list.p + 4 * (size_t)nr;
    pr.chunk_items = sl.d_list.p + 4 * (size_t)nr + rfirst.size();
    if (keep_f) {
      pr.f_chunk = sl.d_fkeep.p;  // the batch pass's values: no Miller loop is recomputed
    } else {
      st.fallback_miller += (uint32_t)ritems.size();
      if (coop)  // no stored lines in a cooperative run: the per-job chunks hold one set each (mk = 1)
        launch_miller_coop(pr, false, sfb);
      else
        launch_miller_acc_auto(pr, false, sfb, mk_whole, opt.miller_lanes, opt.acc6_max, opt.miller_pairs != 0);
    }
    st.fallback_jobs += nr;
    if (small_jobs) {
      // r_i sig_i for the retried sets (G2 window tables and results in the fallback's own buffers), unless the batch
      // pass already formed them (rsig_spec: every set of the run, by set index)
      if (!rsig_spec) sl.d_fb.ensure((size_t)stride * 9 * W_G2J);
      pr.rsig = sl.d_fb.p;
      pr.scal_tab = sl.d_fb.p + (size_t)stride * W_G2J;
      if (!rsig_spec) launch_sig_scale(pr, (uint32_t)rset.size(), sfb, sl.d_list.p + o_rset);
      launch_group_reduce_lane(pr, sl.d_list.p, sl.d_list.p + 2 * (size_t)nr, nr, dS, dF, sfb);
    } else {
      sl.d_msmB.ensure((size_t)MSM_BUCKET_WORDS * std::max<uint32_t>(nrs, 1));
      sl.d_msmW.ensure((size_t)MSM_WINDOW_WORDS * nr);
      launch_sig_msm(pr, sl.d_list.p + o_rsl, nrs, sl.d_list.p + o_rrs, nr, sl.d_msmB.p, sl.d_msmW.p, dS, sfb);
      launch_group_reduce(pr, sl.d_list.p + 2 * (size_t)nr, nr, dF, sfb);
    }
    std::vector<uint32_t> sel;  // jobs to check on their own
    if (nsub) {
      if (nsub >= kFbLaneMin)
        launch_range_combine_lane(dS, dF, nr, sl.d_list.p + o_sub, nsub, dS_sub, dF_sub, sfb);
      else
        launch_range_combine(dS, dF, nr, sl.d_list.p + o_sub, nsub, dS_sub, dF_sub, sfb);
      fb_check(dS_sub, dF_sub, nsub, sl.d_ok.p + nr, nullptr, nsub);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(sl.h_ok.p + nr, sl.d_ok.p + nr, nsub, hipMemcpyDeviceToHost, sfb));
      HIPCHK(hipEventRecord(sl.done, sfb));
      HIPCHK(hipEventSynchronize(sl.done));
      for (uint32_t t = 0; t < nsub; t++)
        for (uint32_t q = subr[2 * t]; q < subr[2 * t + 1]; q++) {
          if (sl.h_ok.p[nr + t]) jr[retry[q]] = 1;
          else sel.push_back(q);
        }
    } else {
      for (uint32_t q = 0; q < nr; q++) sel.push_back(q);
    }
    if (!sel.empty()) {
      const uint32_t ns = (uint32_t)sel.size();
      memcpy(hl + o_sel, sel.data(), (size_t)ns * 4);
      HIPCHK(hipMemcpyAsync(sl.d_list.p + o_sel, hl + o_sel, (size_t)ns * 4, hipMemcpyHostToDevice, sfb));
      fb_check(dS, dF, nr, sl.d_ok.p, sl.d_list.p + o_sel, ns);
      HIPCHK(hipGetLastError());
      HIPCHK(hipMemcpyAsync(sl.h_ok.p, sl.d_ok.p, ns, hipMemcpyDeviceToHost, sfb));
      HIPCHK(hipEventRecord(sl.done, sfb));
      HIPCHK(hipEventSynchronize(sl.done));
      for (uint32_t k = 0; k < ns; k++) jr[retry[sel[k]]] = sl.h_ok.p[k] ? 1 : 0;
    }
    if (fb_verify() && small_jobs) {
      // Diagnostics (BLSGPU_FB_VERIFY=1): the fallback again from its inputs into fresh buffers once the device is idle
      // -- r_i sig_i, S_j / F_j, one cooperative check per job -- compared with the first pass's S_j, F_j (as they
      // are now in dS / dF), its uploaded lists, its results as read and as they are now in d_ok, and the answers.
      HIPCHK(hipDeviceSynchronize());
      const size_t wS = (size_t)W_G2J * nr, wF = (size_t)W_FP12 * nr;
      std::vector<uint32_t> S1(wS), F1(wF), S2(wS), F2(wF), L(o_sel);
      std::vector<uint8_t> ok_now(sel.size() + 1), ok2(nr);
      HIPCHK(hipMemcpy(S1.data(), dS, wS * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(F1.data(), dF, wF * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(L.data(), sl.d_list.p, o_sel * 4, hipMemcpyDeviceToHost));
      if (!sel.empty()) HIPCHK(hipMemcpy(ok_now.data(), sl.d_ok.p, sel.size(), hipMemcpyDeviceToHost));
      uint32_t *t_rs = nullptr, *t_S = nullptr, *t_F = nullptr;
      uint8_t* t_ok = nullptr;
      HIPCHK(hipMalloc((void**)&t_rs, (size_t)stride * 9 * W_G2J * 4));
      HIPCHK(hipMalloc((void**)&t_S, wS * 4));
      HIPCHK(hipMalloc((void**)&t_F, wF * 4));
      HIPCHK(hipMalloc((void**)&t_ok, nr));
      PipelineBuffers pq = pr;
      pq.rsig = t_rs;
      pq.scal_tab = t_rs + (size_t)stride * W_G2J;
      launch_sig_scale(pq, (uint32_t)rset.size(), sfb, sl.d_list.p + o_rset);
      launch_group_reduce_lane(pq, sl.d_list.p, sl.d_list.p + 2 * (size_t)nr, nr, t_S, t_F, sfb);
      launch_group_check(t_S, t_F, nr, t_ok, sfb, nullptr, 0, nullptr, false, false);
      HIPCHK(hipStreamSynchronize(sfb));
      HIPCHK(hipMemcpy(S2.data(), t_S, wS * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(F2.data(), t_F, wF * 4, hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(ok2.data(), t_ok, nr, hipMemcpyDeviceToHost));
      (void)hipFree(t_rs), (void)hipFree(t_S), (void)hipFree(t_F), (void)hipFree(t_ok);
      // S / F are stored structure-of-arrays (word w of job q at w * nr + q)
      uint32_t sdiff = 0, fdiff = 0, vdiff = 0, stale = 0, ldiff = 0, first_v = UINT32_MAX, last_v = 0;
      for (uint32_t q = 0; q < nr; q++) {
        bool ds = false, df = false;
        for (size_t w = 0; w < W_G2J && !ds; w++) ds = S1[w * nr + q] != S2[w * nr + q];
        for (size_t w = 0; w < W_FP12 && !df; w++) df = F1[w * nr + q] != F2[w * nr + q];
        sdiff += ds, fdiff += df;
        if ((jr[retry[q]] == 1) != (ok2[q] != 0)) {
          vdiff++;
          first_v = std::min(first_v, q);
          last_v = q;
        }
      }
      for (size_t k = 0; k < o_sel; k++) ldiff += L[k] != hl[k];
      for (size_t k = 0; k < sel.size(); k++) stale += (ok_now[k] != 0) != (sl.h_ok.p[k] != 0);
      if (vdiff || sdiff || fdiff || stale || ldiff)
        fprintf(stderr, "[blsgpu fbverify] %u-set run, %u retried jobs (nsub %u, direct %d, busy %d, keep_f %d, rsig_spec "
                "%d, spec %d, coop %d, lanes %d): answers that differ on re-check %u (q %u-%u), S_j differ %u, F_j differ "
                "%u, results read vs now %u, list words %zu\n", n, nr, nsub, (int)direct, (int)busy, (int)keep_f,
                (int)rsig_spec, (int)spec, (int)coop, (int)lane_checks((uint32_t)sel.size()), vdiff, first_v, last_v,
                sdiff, fdiff, stale, (size_t)ldiff);
      else
        fprintf(stderr, "[blsgpu fbverify] ok: %u-set run, %u retried jobs\n", n, nr);
    }
  }
  // a failed group whose clean jobs all verify on their own: its batch equation was computed wrong (the random
  // combination of valid sets always holds)
  for (uint32_t g : failed_g) {
    bool all_ok = true;
    for (uint32_t j = group_jobs[g].first; j < group_jobs[g].second && all_ok; j++)
      if (jr[j] != 1 && jr[j] >= 0) all_ok = false;  // errors (negative) are not in the equation
    if (all_ok) {
      d.spurious_groups.fetch_add(1, std::memory_order_relaxed);
      fprintf(stderr, "[blsgpu] device %d: batch group %u (jobs %u-%u) of a %u-set run failed its equation while "
              "every job verifies on its own (spec %d, merged %d, coop %d, mk %u)\n", d.id, g, group_jobs[g].first,
              group_jobs[g].second - 1, n, (int)spec, (int)merged, (int)coop, mk);
    }
  }
  for (uint32_t j = 0; j < nj; j++) job_result[sh.job_begin + j] = (int8_t)jr[j];
  // the device's invalid-set rate estimate (group_adapt): a group "failed" when any of its non-empty jobs was not
  // valid; with groups of s sets failing at rate pf, a set is invalid at rate f = 1 - (1 - pf)^(1/s)
  if (!plan && ng0) {
    uint32_t failed = 0;
    for (uint32_t g = 0; g < ng0; g++)
      for (uint32_t j = group_jobs[g].first; j < group_jobs[g].second; j++)
        if (jr[j] != 1 && job_sets(j).second > job_sets(j).first) {
          failed++;
          break;
        }
    const double pf = std::min((double)failed, ng0 - 0.5) / ng0;
    const double f = 1.0 - std::pow(1.0 - pf, (double)ng0 / std::max(n, 1u));
    std::lock_guard<std::mutex> lk(d.fail_mu);
    d.fail_rate = 0.5 * d.fail_rate + 0.5 * f;
  }
  return BLSGPU_OK;
}

uint32_t max_table_index(const blsgpu_batch* b) {
  uint32_t m = 0;
  if (!b->pk_bytes && b->n_sets)
    for (uint32_t k = 0; k < b->set_pk_first[b->n_sets]; k++) m = std::max(m, b->pk_index[k]);
  return m;
}

int validate_batch(const blsgpu_batch* b) {
  if (!b || !b->job_first_set) return BLSGPU_ERR_ARGS;
  if (b->n_jobs == 0) return b->n_sets == 0 ? BLSGPU_OK : BLSGPU_ERR_ARGS;
  if (b->job_first_set[0] != 0 || b->job_first_set[b->n_jobs] != b->n_sets) return BLSGPU_ERR_ARGS;
  for (uint32_t j = 0; j < b->n_jobs; j++)
    if (b->job_first_set[j + 1] < b->job_first_set[j]) return BLSGPU_ERR_ARGS;
  if (b->n_sets == 0) return BLSGPU_OK;
  if (!b->msgs || !b->sigs || !b->sig_len) return BLSGPU_ERR_ARGS;
  if (b->sig_stride < 96) return BLSGPU_ERR_ARGS;
  for (uint32_t i = 0; i < b->n_sets; i++)
    if (b->sig_len[i] > b->sig_stride && (b->sig_len[i] == 96 || b->sig_len[i] == 192)) return BLSGPU_ERR_ARGS;
  if (!b->pk_bytes && (!b->set_pk_first || !b->pk_index)) return BLSGPU_ERR_ARGS;
  if (b->set_pk_first) {
    if (b->set_pk_first[0] != 0) return BLSGPU_ERR_ARGS;
    for (uint32_t i = 0; i < b->n_sets; i++)
      if (b->set_pk_first[i + 1] < b->set_pk_first[i]) return BLSGPU_ERR_ARGS;
  }
  return BLSGPU_OK;
}


void finish_call(Call* c) {
  blsgpu_stats local{};
  int status = BLSGPU_OK;
  for (int k = 0; k < kStages; k++) local.stage_ms[k] = c->sst.empty() ? 0 : c->sst[0].stage_ms[k];
  for (size_t k = 0; k < c->shards.size(); k++) {
    local.groups += c->sst[k].groups;
    local.batch_retries += c->sst[k].batch_retries;
    local.batch_sigs_success += c->sst[k].batch_sigs_success;
    local.unique_messages += c->sst[k].unique_messages;
    local.pairing_units += c->sst[k].pairing_units;
    local.miller_chunks += c->sst[k].miller_chunks;
    local.fallback_jobs += c->sst[k].fallback_jobs;
    local.fallback_miller += c->sst[k].fallback_miller;
    local.urgent_lane |= c->sst[k].urgent_lane;
    local.host_ms = std::max(local.host_ms, c->sst[k].host_ms);
    if (c->rc[k] != BLSGPU_OK && c->rc[k] != BLSGPU_DEVICE_ERROR) status = c->rc[k];
  }
  local.run_sets = c->sst.empty() ? 0 : c->sst[0].run_sets;
  local.run_calls = c->sst.empty() ? 0 : c->sst[0].run_calls;
  local.devices_used = (uint32_t)c->shards.size();
  local.device_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - c->t0).count();
  if (c->stats) *c->stats = local;
  blsgpu_ctx* ctx = c->ctx;
  if (c->sync) {
    // notify under the lock: the waiter may destroy *c as soon as it can re-acquire it
    std::lock_guard<std::mutex> lk(c->m);
    c->status = status;
    c->finished = true;
    c->cv.notify_all();
  } else {
    blsgpu_done_cb done = c->done;
    void* user = c->user;
    delete c->owned;
    delete c;
    // a throwing callback must not unwind the dispatcher thread (std::terminate would take the host process down)
    if (done) try {
        done(user, status);
      } catch (...) {
      }
  }
  leave(ctx);
}

// pubkey mode of a batch: 0 table, 1 one key per set (bytes), 2 bytes aggregate
inline int pk_mode(const blsgpu_batch& b) { return !b.pk_bytes ? 0 : (b.set_pk_first ? 2 : 1); }

// Batch scalar words of a shard (shard-relative): single-set non-batchable jobs use r = 1 (word 0, CoreVerify,
// maybeBatch.ts:34-38), every other set i the call's keystream word i (batch_rand.hpp).
void shard_scalars(const blsgpu_batch& b, const Shard& sh, const batch_rand::Key& key, uint64_t* out) {
  if (sh.set_end > sh.set_begin) batch_rand::words(key, sh.set_begin, sh.set_end - sh.set_begin, out);
  for (uint32_t j = sh.job_begin; j < sh.job_end; j++) {
    const uint32_t a = b.job_first_set[j], e = b.job_first_set[j + 1];
    const bool batchable = b.job_flags && (b.job_flags[j] & 1u);
    if (!batchable && e - a == 1) out[a - sh.set_begin] = 0;
  }
}

// group_policy 1: the reference pool's grouping on the GPU.  A call's sets are split into jobs of <= 128 sets
// (chunkifyMaximizeChunkSize(sets, 128), multithread/index.ts:156), consecutive jobs are packed into worker requests
// of >= 128 sets (prepareWork, index.ts:386-401), and each request's batchable jobs are checked in chunks of >= 16
// jobs, its other jobs one by one (worker.ts:40-92).  The jobs are laid out group after group (one permuted batch),
// run as one pipeline with that group plan, and each call gets the first rejection of its jobs in job order, else
// false if a job is false, else true (Promise.all over the call's jobs, index.ts:165-173; oracle/blscpu.c
// blscpu_verify_jobs applies the same rule).
int run_pool_policy(Device& d, Slot& sl, const blsgpu_batch& b, const Shard& sh, int8_t* job_result, uint64_t seed,
                    const Options& opt, uint32_t max_index, blsgpu_stats& st, const uint64_t* scal_words) {
  const uint32_t s0 = sh.set_begin, n = sh.set_end - sh.set_begin;
  std::vector<uint64_t> scal0(std::max<uint32_t>(n, 1));
  memcpy(scal0.data(), scal_words, (size_t)n * 8);
  struct Sub {
    uint32_t call, a, e;
    bool batchable;
  };
  std::vector<Sub> subs;
  for (uint32_t j = sh.job_begin; j < sh.job_end; j++) {
    const uint32_t a = b.job_first_set[j], e = b.job_first_set[j + 1];
    const bool bt = b.job_flags && (b.job_flags[j] & 1u);
    if (a == e) {
      subs.push_back({j, a, a, bt});
      continue;
    }
    const uint32_t per = chunk_size(e - a, 128);
    for (uint32_t k = a; k < e; k += per) subs.push_back({j, k, std::min(e, k + per), bt});
  }
  std::vector<uint32_t> order;  // sub-job indices in group order
  std::vector<GroupPlanEntry> plan;
  for (size_t q = 0; q < subs.size();) {
    size_t q1 = q;
    uint32_t total = 0;
    while (q1 < subs.size() && total < 128) total += subs[q1].e - subs[q1].a, q1++;
    std::vector<uint32_t> bat, rest;
    for (size_t x = q; x < q1; x++) (subs[x].batchable && subs[x].e > subs[x].a ? bat : rest).push_back((uint32_t)x);
    if (!bat.empty()) {
      const uint32_t per = chunk_size((uint32_t)bat.size(), 16);
      for (size_t k = 0; k < bat.size(); k += per) {
        GroupPlanEntry g{(uint32_t)order.size(), 0, true};
        for (size_t x = k; x < std::min(bat.size(), k + per); x++) order.push_back(bat[x]);
        g.end = (uint32_t)order.size();
        plan.push_back(g);
      }
    }
    for (uint32_t x : rest) {
      plan.push_back({(uint32_t)order.size(), (uint32_t)order.size() + 1, false});
      order.push_back(x);
    }
    q = q1;
  }
  const int mode = pk_mode(b);
  const uint32_t ns = (uint32_t)subs.size();
  std::vector<uint32_t> jfs{0}, siglen, spf{0}, pki;
  std::vector<uint8_t> flags, msgs, sigs, pkb;
  std::vector<uint64_t> scal;
  jfs.reserve(ns + 1);
  siglen.reserve(n);
  scal.reserve(n);
  msgs.reserve((size_t)n * 32);
  sigs.reserve((size_t)n * b.sig_stride);
  for (uint32_t x : order) {
    const Sub& u = subs[x];
    jfs.push_back(jfs.back() + u.e - u.a);
    flags.push_back(u.batchable ? 1 : 0);
    for (uint32_t i = u.a; i < u.e; i++) {
      siglen.push_back(b.sig_len[i]);
      sigs.insert(sigs.end(), b.sigs + (size_t)i * b.sig_stride, b.sigs + (size_t)(i + 1) * b.sig_stride);
      msgs.insert(msgs.end(), b.msgs + (size_t)i * 32, b.msgs + (size_t)i * 32 + 32);
      scal.push_back(scal0[i - s0]);
      if (mode == 1) {
        pkb.insert(pkb.end(), b.pk_bytes + (size_t)i * 96, b.pk_bytes + (size_t)(i + 1) * 96);
      } else {
        const uint32_t k0 = b.set_pk_first[i], k1 = b.set_pk_first[i + 1];
        spf.push_back(spf.back() + k1 - k0);
        if (mode == 0)
          pki.insert(pki.end(), b.pk_index + k0, b.pk_index + k1);
        else
          pkb.insert(pkb.end(), b.pk_bytes + (size_t)k0 * 96, b.pk_bytes + (size_t)k1 * 96);
      }
    }
  }
  blsgpu_batch pb{};
  pb.n_sets = n;
  pb.n_jobs = ns;
  pb.job_first_set = jfs.data();
  pb.job_flags = flags.data();
  pb.pk_bytes = mode ? pkb.data() : nullptr;
  pb.set_pk_first = mode == 1 ? nullptr : spf.data();
  pb.pk_index = mode == 0 ? pki.data() : nullptr;
  pb.msgs = msgs.data();
  pb.sigs = sigs.data();
  pb.sig_len = siglen.data();
  pb.sig_stride = b.sig_stride;
  std::vector<int8_t> sub_res(std::max<uint32_t>(ns, 1), 0);
  const Shard all{0, ns, 0, n};
  const int rc = run_shard(d, sl, pb, all, sub_res.data(), seed, opt, max_index, st, scal.data(), &plan);
  if (rc != BLSGPU_OK) return rc;
  std::vector<uint32_t> pos(ns);
  for (uint32_t k = 0; k < ns; k++) pos[order[k]] = k;
  std::vector<uint8_t> seen(sh.job_end - sh.job_begin, 0);
  for (uint32_t j = sh.job_begin; j < sh.job_end; j++) job_result[j] = 1;
  for (uint32_t x = 0; x < ns; x++) {
    const uint32_t call = subs[x].call;
    const int8_t r = sub_res[pos[x]];
    if (seen[call - sh.job_begin]) continue;
    if (r < 0) {
      job_result[call] = r;
      seen[call - sh.job_begin] = 1;
    } else if (r == 0) {
      job_result[call] = 0;
    }
  }
  return BLSGPU_OK;
}

// One shard of a call (or a merged batch) under the call's group policy.
int run_call_shard(Device& d, Slot& sl, const blsgpu_batch& b, const Shard& sh, int8_t* job_result, uint64_t seed,
                   const Options& opt, uint32_t max_index, blsgpu_stats& st, const uint64_t* scal_words) {
  if (opt.group_policy == 1) return run_pool_policy(d, sl, b, sh, job_result, seed, opt, max_index, st, scal_words);
  return run_shard(d, sl, b, sh, job_result, seed, opt, max_index, st, scal_words);
}

// Does the device's table hold every index the call's shard uses?  (Checked per device under its table lock: a
// call may race an upload that has reached some devices only.)
inline bool table_covers(const Device& d, const Call* c, const Shard& sh) {
  const blsgpu_batch& b = c->b;
  if (b.pk_bytes || !b.set_pk_first || sh.set_end == sh.set_begin) return true;
  if (b.set_pk_first[sh.set_end] == b.set_pk_first[sh.set_begin]) return true;
  return c->max_index < d.table_n;
}

// Several queued shards (of different calls) run as ONE pipeline: their inputs are concatenated into one
// batch (jobs and results stay per call), so a launch fills the chip instead of one call's 16k-set share --
// the device-side counterpart of the pool packing queued jobs into one worker request (prepareWork,
// multithread/index.ts:386-401).  Jobs never interact, so every job's result is the one it gets alone.  A call
// that cannot run (a table index beyond the device's table) is completed with ERR_ARGS on its own and never
// joins the run; a failure of the run completes its calls with DEVICE_ERROR (every job rejected, never `false`).
// The caller holds the device's table lock (shared).
void run_merged(Device& d, Slot& sl, const std::vector<Task>& parts, std::vector<int>& rcs) {
  const auto t_merge0 = std::chrono::steady_clock::now();
  std::vector<size_t> live;
  for (size_t p = 0; p < parts.size(); p++) {
    const Call* c = parts[p].call;
    if (c->ctx->closed && !c->sync)
      rcs[p] = BLSGPU_ERR_CLOSED;
    else if (!table_covers(d, c, c->shards[parts[p].shard]))
      rcs[p] = BLSGPU_ERR_ARGS;
    else
      live.push_back(p);
  }
  if (live.empty()) return;
  int rc = BLSGPU_OK;
  blsgpu_stats st{};
  std::vector<int8_t> res;
  try {
    const Call* c0 = parts[live[0]].call;
    const int mode = pk_mode(c0->b);
    uint32_t n = 0, nj = 0, npk = 0, max_index = 0;
    for (size_t p : live) {
      const Task& t = parts[p];
      const Shard& sh = t.call->shards[t.shard];
      const blsgpu_batch& b = t.call->b;
      n += sh.set_end - sh.set_begin;
      nj += sh.job_end - sh.job_begin;
      if (b.set_pk_first) npk += b.set_pk_first[sh.set_end] - b.set_pk_first[sh.set_begin];
      max_index = std::max(max_index, t.call->max_index);
    }
    // the parts' offsets (sets, jobs, pubkeys), then every part packed in parallel into its own ranges: the batch
    // scalars (ChaCha20, ~0.4 ms per 16k-set call) and the copies of a 131k-set run took ~2.5 ms on one thread
    uint32_t sig_w = 96;
    std::vector<uint32_t> p_so, p_jo, p_ko;
    {
      uint32_t so = 0, jo = 0, ko = 0;
      for (size_t p : live) {
        const Task& t = parts[p];
        const Shard& sh = t.call->shards[t.shard];
        const blsgpu_batch& b = t.call->b;
        p_so.push_back(so);
        p_jo.push_back(jo);
        p_ko.push_back(ko);
        so += sh.set_end - sh.set_begin;
        jo += sh.job_end - sh.job_begin;
        if (b.set_pk_first) ko += b.set_pk_first[sh.set_end] - b.set_pk_first[sh.set_begin];
        for (uint32_t i = sh.set_begin; i < sh.set_end && sig_w == 96; i++)
          if (b.sig_len[i] == 192) sig_w = 192;
      }
    }
    std::vector<uint32_t> jfs(nj + 1), siglen(n), spf(mode == 1 ? 1 : n + 1), pki(mode == 0 ? npk : 0);
    std::vector<uint8_t> flags(nj), pkb(mode == 1 ? (size_t)n * 96 : mode == 2 ? (size_t)npk * 96 : 0),
        msgs((size_t)n * 32), sigs((size_t)n * sig_w, 0);
    std::vector<uint64_t> scal(std::max<uint32_t>(n, 1));
    jfs[0] = 0;
    spf[0] = 0;
    auto pack = [&](size_t q) {
      if (q) pthread_setname_np(pthread_self(), "blsgpu-pack");
      const Task& t = parts[live[q]];
      const Shard& sh = t.call->shards[t.shard];
      const blsgpu_batch& b = t.call->b;
      const uint32_t so = p_so[q], jo = p_jo[q], ko = p_ko[q], ns = sh.set_end - sh.set_begin;
      shard_scalars(b, sh, t.call->key, scal.data() + so);
      for (uint32_t j = sh.job_begin; j < sh.job_end; j++) {
        jfs[jo + (j - sh.job_begin) + 1] = so + b.job_first_set[j + 1] - sh.set_begin;
        flags[jo + (j - sh.job_begin)] = b.job_flags ? b.job_flags[j] : 0;
      }
      memcpy(siglen.data() + so, b.sig_len + sh.set_begin, (size_t)ns * 4);
      if (b.sig_stride == sig_w) {
        memcpy(sigs.data() + (size_t)so * sig_w, b.sigs + (size_t)sh.set_begin * sig_w, (size_t)ns * sig_w);
      } else {
        for (uint32_t i = sh.set_begin; i < sh.set_end; i++) {
          const uint32_t len = b.sig_len[i];
          if (len == 96 || len == 192)
            memcpy(sigs.data() + (size_t)(so + i - sh.set_begin) * sig_w, b.sigs + (size_t)i * b.sig_stride, len);
        }
      }
      memcpy(msgs.data() + (size_t)so * 32, b.msgs + (size_t)sh.set_begin * 32, (size_t)ns * 32);
      if (mode == 1) {
        memcpy(pkb.data() + (size_t)so * 96, b.pk_bytes + (size_t)sh.set_begin * 96, (size_t)ns * 96);
      } else {
        const uint32_t k0 = b.set_pk_first[sh.set_begin], k1 = b.set_pk_first[sh.set_end];
        for (uint32_t i = sh.set_begin; i < sh.set_end; i++)
          spf[so + (i - sh.set_begin) + 1] = ko + b.set_pk_first[i + 1] - k0;
        if (mode == 0)
          memcpy(pki.data() + ko, b.pk_index + k0, (size_t)(k1 - k0) * 4);
        else
          memcpy(pkb.data() + (size_t)ko * 96, b.pk_bytes + (size_t)k0 * 96, (size_t)(k1 - k0) * 96);
      }
    };
    {  // parts of >= 4,096 sets on their own threads (a small part packs faster than a thread starts)
      struct Joiner {  // joins the started threads on every exit, so none is destroyed while joinable
        std::vector<std::thread> th;
        ~Joiner() {
          for (auto& x : th)
            if (x.joinable()) x.join();
        }
      } j;
      std::vector<uint8_t> inline_pack(live.size(), 0);
      for (size_t q = 0; q < live.size(); q++) {
        const Shard& sh = parts[live[q]].call->shards[parts[live[q]].shard];
        inline_pack[q] = q == 0 || sh.set_end - sh.set_begin < 4096;
        if (inline_pack[q]) continue;
        try {
          j.th.emplace_back(pack, q);
        } catch (std::system_error&) {  // no thread: this part packs on the current one
          inline_pack[q] = 1;
        }
      }
      for (size_t q = 0; q < live.size(); q++)
        if (inline_pack[q]) pack(q);
    }
    blsgpu_batch mb{};
    mb.n_sets = n;
    mb.n_jobs = nj;
    mb.job_first_set = jfs.data();
    mb.job_flags = flags.data();
    mb.pk_bytes = mode ? pkb.data() : nullptr;
    mb.set_pk_first = mode == 1 ? nullptr : spf.data();
    mb.pk_index = mode == 0 ? pki.data() : nullptr;
    mb.msgs = msgs.data();
    mb.sigs = sigs.data();
    mb.sig_len = siglen.data();
    mb.sig_stride = sig_w;
    res.assign(std::max<uint32_t>(nj, 1), 0);
    const Shard all{0, nj, 0, n};
    tl_merge_ms = ms_since(t_merge0);
    rc = run_call_shard(d, sl, mb, all, res.data(), c0->seed, c0->opt, max_index, st, scal.data());
  } catch (...) {
    rc = BLSGPU_DEVICE_ERROR;
  }
  st.run_calls = (uint32_t)live.size();
  uint32_t jo = 0;
  for (size_t k = 0; k < live.size(); k++) {
    const size_t p = live[k];
    Call* c = parts[p].call;
    const Shard& sh = c->shards[parts[p].shard];
    for (uint32_t j = sh.job_begin; j < sh.job_end; j++, jo++) {
      if (rc == BLSGPU_OK)
        c->job_result[j] = res[jo];
      else if (rc == BLSGPU_DEVICE_ERROR)  // a device failure rejects every job, never `false`
        c->job_result[j] = -BLSGPU_DEVICE_ERROR;
    }
    blsgpu_stats& cs = c->sst[parts[p].shard];
    if (k == 0) {
      cs = st;  // the merged run's counters (and stage times) go to its first call
    } else {
      cs = blsgpu_stats{};
      cs.run_calls = st.run_calls;
    }
    rcs[p] = rc;
  }
}

void run_task(Device& d, Slot& sl, const Task& t) {
  Call* c = t.call;
  const Shard& sh = c->shards[t.shard];
  int rc;
  if (c->ctx->closed && !c->sync) {
    rc = BLSGPU_ERR_CLOSED;
  } else {
    try {
      std::shared_lock<std::shared_mutex> tl(d.table_mu);
      if (!table_covers(d, c, sh)) {
        rc = BLSGPU_ERR_ARGS;
      } else {
        std::vector<uint64_t> scal(std::max<uint32_t>(sh.set_end - sh.set_begin, 1));
        shard_scalars(c->b, sh, c->key, scal.data());
        rc = run_call_shard(d, sl, c->b, sh, c->job_result, c->seed, c->opt, c->max_index, c->sst[t.shard],
                            scal.data());
        c->sst[t.shard].run_calls = 1;
        c->sst[t.shard].urgent_lane = sl.urgent ? 1 : 0;
      }
    } catch (...) {
      rc = BLSGPU_DEVICE_ERROR;
    }
  }
  if (rc == BLSGPU_DEVICE_ERROR)  // a device failure rejects every job of the shard, never `false`
    for (uint32_t j = sh.job_begin; j < sh.job_end; j++) c->job_result[j] = -BLSGPU_DEVICE_ERROR;
  c->rc[t.shard] = rc;
  d.load.fetch_sub(sh.cost, std::memory_order_relaxed);
  if (c->remaining.fetch_sub(1) == 1) finish_call(c);
}

inline uint32_t task_sets(const Task& t) {
  const Shard& sh = t.call->shards[t.shard];
  return sh.set_end - sh.set_begin;
}

// A slot's dispatcher: takes the oldest queued shard of its device, merges the compatible shards queued behind it
// (up to merge_sets sets), runs them, completes their calls.  Exits when the device stops (queue drained) or when
// the slot is retired (option "slots" lowered).
void worker_loop(Device* d, Slot* sl) {
  tl_dispatcher = true;
  pthread_setname_np(pthread_self(), "blsgpu-slot");  // host-cost accounting by thread (bench.py "host")
  (void)hipSetDevice(d->id);
  for (;;) {
    std::vector<Task> parts;
    {
      std::unique_lock<std::mutex> lk(d->q_mu);
      // Run formation.  A device keeps at most pipeline_depth runs in flight (the streams are shared, so a further
      // run would only queue behind them); a free slot takes the oldest queued call and merges the compatible calls
      // queued behind it, up to merge_sets sets.  While other runs are in flight the GPU is busy anyway, so the
      // slot lingers up to merge_wait_us for more calls to merge: bursts of calls become a few chip-filling runs
      // instead of many small ones; an idle device starts at once (an isolated call pays no wait).
      d->q_cv.wait(lk, [&] {
        return d->stop || sl->retire ||
               (!d->queue.empty() && d->runs_inflight < std::max<int64_t>(1, d->queue.front().call->opt.pipeline_depth));
      });
      if (sl->retire) return;
      if (d->queue.empty()) return;  // stop requested and nothing left
      parts.push_back(d->queue.front());
      d->queue.pop_front();
      const Call* c0 = parts[0].call;
      uint32_t total = task_sets(parts[0]);
      int64_t cap = c0->opt.merge_sets;
      // balanced runs: a backlog above the cap is cut into equal runs (19 queued 16k calls at a 131,072-set cap: 6 + 6
      // + 7 calls instead of 8 + 8 + 3, so the last run of a burst is not a short one draining alone)
      if (cap > 0 && c0->opt.merge_balance) {
        int64_t backlog = total;
        for (const Task& t : d->queue) backlog += task_sets(t);
        if (backlog > cap) {
          const int64_t runs = (backlog + cap - 1) / cap;
          cap = (backlog + runs - 1) / runs;
        }
      }
      const auto t_start = std::chrono::steady_clock::now();
      const auto deadline = t_start + std::chrono::microseconds(c0->opt.merge_wait_us);
      // idle device: linger only while a burst keeps arriving -- each new call extends the wait by idle_wait_us / 4,
      // up to idle_wait_us in all, so an isolated call waits at most idle_wait_us / 4
      const auto idle_end = t_start + std::chrono::microseconds(c0->opt.idle_wait_us);
      auto idle_deadline = t_start + std::chrono::microseconds(c0->opt.idle_wait_us / 4);
      for (;;) {
        size_t took = 0;
        while (!d->queue.empty() && cap > 0 && !(c0->ctx->closed)) {
          const Task& nx = d->queue.front();
          const Call* c = nx.call;
          if ((int64_t)(total + task_sets(nx)) > cap || pk_mode(c->b) != pk_mode(c0->b) || !c->opt.same_run(c0->opt))
            break;
          total += task_sets(nx);
          parts.push_back(nx);
          d->queue.pop_front();
          took++;
        }
        const bool room = cap > 0 && (int64_t)total < cap && d->queue.empty();
        if (!room || d->stop || c0->ctx->closed) break;
        if (d->runs_inflight == 0) {
          if (c0->opt.idle_wait_us <= 0) break;
          const auto now = std::chrono::steady_clock::now();
          if (took) idle_deadline = std::min(idle_end, now + std::chrono::microseconds(c0->opt.idle_wait_us / 4));
          if (now >= idle_deadline) break;
          if (d->q_cv.wait_until(lk, idle_deadline) == std::cv_status::timeout && d->queue.empty()) break;
          continue;
        }
        if (d->q_cv.wait_until(lk, deadline) == std::cv_status::timeout && d->queue.empty()) break;
      }
      sl->alone = d->runs_inflight == 0;
      d->runs_inflight++;
      sl->in_flight = true;
    }
    tl_run_t0 = std::chrono::steady_clock::now();
    tl_merge_ms = 0;
    struct InflightGuard {  // the run leaves the in-flight count when its batch pass completes (run_shard) or here
      Device* d;
      Slot* sl;
      ~InflightGuard() { release_inflight(*d, *sl); }
    } guard{d, sl};
    if (parts.size() == 1) {
      run_task(*d, *sl, parts[0]);
      continue;
    }
    std::vector<int> rcs(parts.size(), BLSGPU_OK);
    try {
      std::shared_lock<std::shared_mutex> tl(d->table_mu);
      run_merged(*d, *sl, parts, rcs);
    } catch (...) {  // run_merged catches its own failures; this only guards the lock
      for (size_t p = 0; p < parts.size(); p++) {
        const Shard& sh = parts[p].call->shards[parts[p].shard];
        for (uint32_t j = sh.job_begin; j < sh.job_end; j++) parts[p].call->job_result[j] = -BLSGPU_DEVICE_ERROR;
        rcs[p] = BLSGPU_DEVICE_ERROR;
      }
    }
    for (size_t p = 0; p < parts.size(); p++) {
      Call* c = parts[p].call;
      c->rc[parts[p].shard] = rcs[p];
      d->load.fetch_sub(c->shards[parts[p].shard].cost, std::memory_order_relaxed);
      if (c->remaining.fetch_sub(1) == 1) finish_call(c);
    }
  }
}

// The urgent lane's dispatcher: takes the oldest urgent call and the compatible urgent calls queued behind it (up to
// urgent_max_sets sets: a burst of urgent calls becomes one run, not a queue of runs), and runs them on the lane's own
// stream pairs (run_shard: Slot::urgent) -- the reference's verifyOnMainThread verifies at once, outside the pool queue
// (multithread/index.ts:138-151).  `alone` holds for its streams, so a run takes the latency forms of an idle device:
// the speculative MSM and the pubkey branch on the idle pair, r_i sig_i beside the batch pass, cooperative fallback
// checks.  Exits when the device stops and its urgent queue is drained.
bool ensure_urgent_streams(Device* d, Slot* sl);
void urgent_loop(Device* d, Slot* sl) {
  tl_dispatcher = true;
  pthread_setname_np(pthread_self(), "blsgpu-urgent");
  (void)hipSetDevice(d->id);
  for (;;) {
    std::vector<Task> parts;
    {
      std::unique_lock<std::mutex> lk(d->q_mu);
      d->q_cv.wait(lk, [&] { return d->stop || !d->uqueue.empty(); });
      if (d->uqueue.empty()) return;  // stop requested and nothing left
      parts.push_back(d->uqueue.front());
      d->uqueue.pop_front();
      const Call* c0 = parts[0].call;
      uint32_t total = task_sets(parts[0]);
      // a burst of urgent calls (several main-thread verifications issued in one JS tick) arrives a few microseconds
      // apart: the burst lasts while each next call comes within urgent_wait_us of the previous one (at most 8 gaps'
      // worth in all), so it becomes one run instead of a run and a queue behind it
      const auto gap = std::chrono::microseconds(std::max<int64_t>(c0->opt.urgent_wait_us, 0));
      const auto linger_end = std::chrono::steady_clock::now() + 8 * gap;
      for (;;) {
        bool blocked = false;
        while (!d->uqueue.empty()) {
          const Task& nx = d->uqueue.front();
          if ((int64_t)(total + task_sets(nx)) > c0->opt.urgent_max_sets || pk_mode(nx.call->b) != pk_mode(c0->b) ||
              !nx.call->opt.same_run(c0->opt)) {
            blocked = true;
            break;
          }
          total += task_sets(nx);
          parts.push_back(nx);
          d->uqueue.pop_front();
        }
        if (blocked || gap.count() == 0 || d->stop || (int64_t)total >= c0->opt.urgent_max_sets) break;
        const auto now = std::chrono::steady_clock::now();
        if (now >= linger_end) break;
        if (!d->q_cv.wait_for(lk, std::min<std::chrono::steady_clock::duration>(gap, linger_end - now),
                              [&] { return d->stop || !d->uqueue.empty(); }))
          break;  // the gap passed with no new urgent call: the burst is over
      }
    }
    sl->alone = true;
    tl_run_t0 = std::chrono::steady_clock::now();
    tl_merge_ms = 0;
    const size_t np = parts.size();
    if (!ensure_urgent_streams(d, sl)) {  // no streams: every call of the run completes with a device error
      for (size_t p = 0; p < np; p++) {
        Call* c = parts[p].call;
        const Shard& sh = c->shards[parts[p].shard];
        for (uint32_t j = sh.job_begin; j < sh.job_end; j++) c->job_result[j] = -BLSGPU_DEVICE_ERROR;
        c->rc[parts[p].shard] = BLSGPU_DEVICE_ERROR;
        c->sst[parts[p].shard].urgent_lane = 1;
        if (c->remaining.fetch_sub(1) == 1) finish_call(c);
      }
      d->upending.fetch_sub((int)np, std::memory_order_relaxed);
      continue;
    }
    if (np == 1) {
      run_task(*d, *sl, parts[0]);  // completes the call
    } else {
      std::vector<int> rcs(np, BLSGPU_OK);
      try {
        std::shared_lock<std::shared_mutex> tl(d->table_mu);
        run_merged(*d, *sl, parts, rcs);
      } catch (...) {  // run_merged catches its own failures; this only guards the lock
        for (size_t p = 0; p < np; p++) {
          const Shard& sh = parts[p].call->shards[parts[p].shard];
          for (uint32_t j = sh.job_begin; j < sh.job_end; j++) parts[p].call->job_result[j] = -BLSGPU_DEVICE_ERROR;
          rcs[p] = BLSGPU_DEVICE_ERROR;
        }
      }
      for (size_t p = 0; p < np; p++) {
        Call* c = parts[p].call;
        c->rc[parts[p].shard] = rcs[p];
        c->sst[parts[p].shard].urgent_lane = 1;
        if (c->remaining.fetch_sub(1) == 1) finish_call(c);
      }
    }
    d->upending.fetch_sub((int)np, std::memory_order_relaxed);
  }
}

// Frees a slot whose dispatcher has exited (or never started): its buffers (stream-ordered frees on the stream the
// slot last grew them on, then that stream is drained) and events.
void free_slot(Device* d, Slot* s) {
  (void)hipSetDevice(d->id);
  hipStream_t last = s->d_in.st;
  s->release_all();
  if (last) (void)hipStreamSynchronize(last);
  for (auto& e : s->ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : {s->join_in, s->join_msg, s->join_pk, s->join_mask, s->join_gsm, s->join_dec, s->join_msm,
                       s->join_rsig, s->done})
    if (e) (void)hipEventDestroy(e);
  if (s->fb) (void)hipStreamSynchronize(s->fb), (void)hipStreamDestroy(s->fb);
  delete s;
}

// A stream on the CUs of `mask` (hipExtStreamCreateWithCUMask: its own hardware queue, normal priority), or, with no
// mask, a non-blocking stream of priority `prio`.
hipStream_t make_stream(const std::vector<uint32_t>& mask, int prio) {
  hipStream_t st = nullptr;
  if (!mask.empty())
    HIPCHK(hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()));
  else
    HIPCHK(hipStreamCreateWithPriority(&st, hipStreamNonBlocking, prio));
  return st;
}

// The device's pipeline streams and its urgent lane's (created with the first call, so "urgent_cus" set after init
// applies).  The urgent streams are CU-masked streams (hipExtStreamCreateWithCUMask), which HIP gives hardware queues
// of their own: an urgent kernel never waits in a queue behind a pipeline kernel, only for free SIMDs.  Their mask is
// every CU, or with "urgent_cus" > 0 a partition, mask bits [0, urgent_cus): the driver deals mask bits round-robin
// over the XCDs (bit i -> XCD i % 8 in SPX mode, then over each XCD's shader engines; profiles/r06_cu_probe.json), so a
// multiple of 8 bits gives every XCD the same number of partition CUs -- a workgroup is dealt to any XCD, and an XCD
// without a CU of the stream's mask would never run it.  With urgent_isolate 1 the pipeline streams (and the slots'
// fallback streams) are masked to the complement, so the partition always has free SIMDs for an urgent run.  Measured
// (profiles/r06_urgent_ab.json): that costs ~10% of C2 throughput for 8 CUs, not 3% -- the partition leaves shader
// engine 0 of every XCD with 7 of its 8 CUs, the dispatcher deals workgroups evenly over the engines, and that engine
// finishes last -- so the default is no partition.  urgent_isolate 2: plain highest-priority urgent streams (HIP deals
// them over its shared hardware queues); 3 (diagnostics): the pipeline streams masked with every CU.
void create_streams(blsgpu_ctx* ctx, Device* d) {
  HIPCHK(hipSetDevice(d->id));
  int prio_lo = 0, prio_hi = 0;
  HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
  int n_cu = 0;
  HIPCHK(hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, d->id));
  const int part = (int)std::min<int64_t>(ctx->urgent_cus, n_cu / 2) & ~7;
  d->urgent_cus = part;
  const size_t words = (size_t)(n_cu + 31) / 32;
  std::vector<uint32_t> pmask(words, 0);
  d->main_mask.clear();
  for (int i = 0; i < n_cu; i++)
    if (part == 0 || i < part) pmask[i / 32] |= 1u << (i % 32);
  if (part > 0 && ctx->urgent_isolate == 1) {
    d->main_mask.assign(words, 0);
    for (int i = part; i < n_cu; i++) d->main_mask[i / 32] |= 1u << (i % 32);
  }
  if (ctx->urgent_isolate == 3) d->main_mask.assign(words, ~0u);
  if (ctx->urgent_isolate == 2) pmask.clear();
  // The message branch (hash_to_G2 -> Miller lines -> Miller accumulation -> F reduction) is the serial chain that
  // bounds a device's throughput (~70% of the work, one in-order stream shared by the runs in flight): its stream
  // gets the device's highest priority, so its kernels take free SIMDs first and the signature / pubkey branches
  // fill the gaps its tails leave, instead of stretching the chain; so does the short tail (final
  // exponentiations -> results), which returns finished calls sooner.  (C2, interleaved A/B: 2.90M sets/s with no
  // priorities, 2.94M message stream, 2.945M message + tail; profiles/r03_ab6_stream_priority.txt.)
  // A third stream pair when the process has the hardware queues for it (GPU_MAX_HW_QUEUES >= 6): each of the
  // default three slots' runs then has its own pair, and a run never queues behind another run's tail.
  d->npairs = ctx->hw_queues >= 6 ? kMaxPairs : 2;
  for (int k = 0; k < 2 * d->npairs; k++) {
    const bool high = ctx->pipeline_prio && ((BLSGPU_STREAM_PRIO & (1 << (k & 3))) != 0 || (k >= kStreams && (k & 1)));
    d->st[k] = make_stream(d->main_mask, high ? prio_hi : prio_lo);
  }
  // The urgent streams are created when the lane takes its first call (ensure_urgent_streams): a process that never
  // verifies an urgent call holds no idle hardware queues for them (each CU-masked stream is a queue of its own, and
  // eight device contexts on one GPU -- bench.py --devices-same -- would otherwise hold 32).  BLSGPU_URGENT_EAGER=1
  // (build define) creates them here.
  d->umask = pmask;
  d->uprio = prio_hi;
#if BLSGPU_URGENT_EAGER
  for (int k = 0; k < 4; k++) d->ust[k] = make_stream(d->umask, d->uprio);
#endif
}

// The urgent lane's streams on first use (its dispatcher thread; the slot's buffers follow stream 0).  A failed
// creation leaves them null and is reported as a device error for the run.
bool ensure_urgent_streams(Device* d, Slot* sl) {
  if (d->ust[0]) return true;
  try {
    HIPCHK(hipSetDevice(d->id));
    for (int k = 0; k < 4; k++) d->ust[k] = make_stream(d->umask, d->uprio);
  } catch (HipError&) {
    for (hipStream_t& st : d->ust)
      if (st) (void)hipStreamDestroy(st), st = nullptr;
    return false;
  }
  sl->set_stream(d->ust[0]);
  return true;
}

// A slot's events: the two its dispatcher waits on (join_msg, done) block the thread in the driver when
// d->blocking_sync is set (hipEventBlockingSync) instead of spinning -- a dispatcher waits ~10-40 ms per run, and three
// spinning per device cost ~1 host core per million sets/s (round 6, bench.py "host").
void create_slot_events(Device* d, Slot* s) {
  const unsigned wait_flags = hipEventDisableTiming | (d->blocking_sync ? hipEventBlockingSync : 0u);
  for (hipEvent_t* e : {&s->join_in, &s->join_pk, &s->join_mask, &s->join_gsm, &s->join_dec, &s->join_msm, &s->join_rsig})
    HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  for (hipEvent_t* e : {&s->join_msg, &s->done}) HIPCHK(hipEventCreateWithFlags(e, wait_flags));
  for (auto& e : s->ev) HIPCHK(hipEventCreate(&e));
}

void add_slot(Device* d) {  // caller holds d->q_mu (or the device is not yet shared)
  Slot* s = new Slot();
  HIPCHK(hipSetDevice(d->id));
  try {
    s->set_stream(d->st[kSig]);
    create_slot_events(d, s);
    int prio_lo = 0, prio_hi = 0;
    HIPCHK(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
    s->fb = make_stream(d->main_mask, prio_lo);
  } catch (HipError&) {
    free_slot(d, s);
    throw;
  }
  d->slots.push_back(s);
  d->workers.emplace_back(worker_loop, d, s);
}

// Brings the device to `want` slots: new slots start their dispatcher; surplus slots are retired (their dispatcher
// finishes the run it holds, then exits) and freed.  Called with no device lock held.
void resize_slots(Device* d, int64_t want) {
  std::vector<std::thread> joins;
  std::vector<Slot*> gone;
  {
    std::lock_guard<std::mutex> lk(d->q_mu);
    while ((int64_t)d->slots.size() < want) add_slot(d);
    while ((int64_t)d->slots.size() > want) {
      Slot* s = d->slots.back();
      s->retire = true;
      gone.push_back(s);
      joins.push_back(std::move(d->workers.back()));
      d->slots.pop_back();
      d->workers.pop_back();
    }
  }
  d->q_cv.notify_all();
  // (set_option refuses "slots" on a dispatcher thread, so no thread joins itself here; a failing join leaves the
  // retired dispatcher to finish on its own and keeps its slot: detached, never destroyed while joinable)
  for (size_t k = 0; k < joins.size(); k++) {
    try {
      joins[k].join();
      free_slot(d, gone[k]);
    } catch (std::system_error&) {
      joins[k].detach();
    }
  }
}

void destroy_device(Device* d) {
  {
    std::lock_guard<std::mutex> lk(d->q_mu);
    d->stop = true;
  }
  d->q_cv.notify_all();
  for (auto& t : d->workers) t.join();
  if (d->uworker.joinable()) d->uworker.join();
  for (Slot* s : d->slots) free_slot(d, s);
  if (d->uslot) free_slot(d, d->uslot);
  (void)hipSetDevice(d->id);
  for (hipStream_t st : d->st)
    if (st) (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st);
  for (hipStream_t st : d->ust)
    if (st) (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st);
  for (hipStream_t st : d->same_st)
    if (st) (void)hipStreamSynchronize(st), (void)hipStreamDestroy(st);
  for (hipEvent_t e : d->same_ev)
    if (e) (void)hipEventDestroy(e);
  d->helper.release_all();
  d->table.release();
  if (d->table_stream) (void)hipStreamDestroy(d->table_stream);
  delete d;
}

// Hardware queues HIP gives this process per device: GPU_MAX_HW_QUEUES as HIP read it at its initialization
// (HIP's default is 4).  Read-only: the library never writes the environment.
int64_t hw_queues_of_process() {
  const char* v = getenv("GPU_MAX_HW_QUEUES");
  const long q = v ? strtol(v, nullptr, 10) : 0;
  return q > 0 ? q : 4;
}

// Default slots per device.  Slots share the device's kStreams streams, so the count no longer depends on the
// hardware queues; several slots let one run's host work (merging, packing, fallback round trips) overlap another's
// kernels.
int64_t default_slots(int64_t) { return 3; }

// Creates the devices' slots on the first call (so a "slots" value set after init is the count created).
int ensure_slots(blsgpu_ctx* ctx) {
  std::lock_guard<std::mutex> lk(ctx->slots_mu);
  if (ctx->slots_started) return BLSGPU_OK;
  try {
    for (Device* d : ctx->devs) {
      if (!d->st[0]) {
        d->blocking_sync = ctx->blocking_sync != 0;
        create_streams(ctx, d);
      }
      resize_slots(d, ctx->slots_per_device);
      if (!d->uslot) {  // the urgent lane: one slot, its own dispatcher
        Slot* u = new Slot();
        u->urgent = true;
        try {
          u->set_stream(d->ust[0]);
          create_slot_events(d, u);
        } catch (HipError&) {
          free_slot(d, u);
          throw;
        }
        d->uslot = u;  // fallback on its own signature stream (Slot::fb null)
        try {
          d->uworker = std::thread(urgent_loop, d, u);
        } catch (std::system_error&) {
          d->uslot = nullptr;
          free_slot(d, u);
          return BLSGPU_DEVICE_ERROR;
        }
      }
    }
  } catch (HipError&) {
    return BLSGPU_DEVICE_ERROR;
  }
  ctx->slots_started = true;
  return BLSGPU_OK;
}

// Routes a call (whole, or split over the least-loaded devices: route_rule) and queues the shard tasks.
int64_t shard_cost(const blsgpu_batch& b, const Shard& sh) {
  int64_t c = 256 * (int64_t)(sh.set_end - sh.set_begin);
  if (b.set_pk_first) c += b.set_pk_first[sh.set_end] - b.set_pk_first[sh.set_begin];
  return c;
}

// An urgent call (a BLSGPU_JOB_URGENT job) of <= urgent_max_sets sets goes whole to the urgent lane of the device with
// the fewest urgent calls pending (ties rotate); a larger one is routed as any call but queued at the head of each
// device's queue.  Returns true when the call was queued on an urgent lane.
bool launch_urgent(blsgpu_ctx* ctx, Call* c) {
  const blsgpu_batch& b = c->b;
  const uint32_t nd = (uint32_t)std::min<int64_t>((int64_t)ctx->devs.size(), c->opt.max_devices);
  if (!c->opt.urgent_lane || (int64_t)b.n_sets > c->opt.urgent_max_sets || nd == 0) return false;
  const uint32_t start = ctx->route_seq.fetch_add(1, std::memory_order_relaxed) % nd;
  uint32_t best = start;
  for (uint32_t k = 1; k < nd; k++) {
    const uint32_t x = (start + k) % nd;
    if (ctx->devs[x]->upending.load(std::memory_order_relaxed) < ctx->devs[best]->upending.load(std::memory_order_relaxed))
      best = x;
  }
  Device* d = ctx->devs[best];
  if (!d->uslot) return false;
  Shard sh{0, b.n_jobs, 0, b.n_sets};
  sh.dev = best;
  sh.cost = 0;
  c->shards.push_back(sh);
  c->sst.assign(1, blsgpu_stats{});
  c->rc.assign(1, BLSGPU_OK);
  c->remaining = 1;
  c->t0 = std::chrono::steady_clock::now();
  d->upending.fetch_add(1, std::memory_order_relaxed);
  {
    std::lock_guard<std::mutex> lk(d->q_mu);
    d->uqueue.push_back({c, 0});
  }
  d->q_cv.notify_all();
  return true;
}

void launch_call(blsgpu_ctx* ctx, Call* c) {
  const blsgpu_batch& b = c->b;
  bool urgent = false;
  if (b.job_flags)
    for (uint32_t j = 0; j < b.n_jobs && !urgent; j++) urgent = (b.job_flags[j] & BLSGPU_JOB_URGENT) != 0;
  if (urgent && launch_urgent(ctx, c)) return;
  const uint32_t nd_all = (uint32_t)std::min<int64_t>((int64_t)ctx->devs.size(), c->opt.max_devices);
  std::vector<int64_t> load(nd_all);
  for (uint32_t d = 0; d < nd_all; d++) load[d] = ctx->devs[d]->load.load(std::memory_order_relaxed);
  std::vector<uint32_t> devs(std::max<uint32_t>(nd_all, 1));
  const uint32_t nd = route_rule(b.n_sets, nd_all, load.data(), c->opt.route_split_sets,
                                 ctx->route_seq.fetch_add(1, std::memory_order_relaxed), devs.data());
  std::vector<uint32_t> parts(nd + 1);
  shard_rule(b.job_first_set, b.set_pk_first, b.n_jobs, nd, parts.data());
  for (uint32_t k = 0; k < nd; k++) {
    Shard sh{parts[k], parts[k + 1], b.n_jobs ? b.job_first_set[parts[k]] : 0,
             b.n_jobs ? b.job_first_set[parts[k + 1]] : 0};
    sh.dev = devs[k];
    sh.cost = shard_cost(b, sh);
    c->shards.push_back(sh);
  }
  c->sst.assign(nd, blsgpu_stats{});
  c->rc.assign(nd, BLSGPU_OK);
  c->remaining = nd;
  c->t0 = std::chrono::steady_clock::now();
  for (uint32_t k = 0; k < nd; k++) {
    Device* d = ctx->devs[c->shards[k].dev];
    d->load.fetch_add(c->shards[k].cost, std::memory_order_relaxed);
    {
      std::lock_guard<std::mutex> lk(d->q_mu);
      if (urgent)  // too large for the urgent lane: ahead of every queued call
        d->queue.push_front({c, k});
      else
        d->queue.push_back({c, k});
    }
    d->q_cv.notify_all();  // a lingering slot (merge_wait_us) must see it, not only an idle one
  }
}

}  // namespace
bool blsgpu_rt::resolve_key(uint64_t seed, batch_rand::Key& key, uint64_t& hash_key) {
  if (seed == 0) {
    if (!batch_rand::os_key(key)) return false;
    hash_key = batch_rand::hash_key(key);  // its own keystream block, not key material
  } else {
    key = batch_rand::seed_key(seed);
    hash_key = batch_rand::hash_key(key);
  }
  return true;
}
namespace {

void reject_all(const blsgpu_batch* b, int8_t* job_result, int code) {
  if (job_result)
    for (uint32_t j = 0; j < b->n_jobs; j++) job_result[j] = (int8_t)-code;
}

Options snapshot(blsgpu_ctx* ctx) {
  std::lock_guard<std::mutex> lk(ctx->opt_mu);
  return ctx->opt;
}

}  // namespace

extern "C" {

int blsgpu_init(const int* devices, int n_devices, blsgpu_ctx** out) {
  if (!out) return BLSGPU_ERR_ARGS;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return BLSGPU_ERR_NO_DEVICE;
  std::vector<int> ids;
  if (devices && n_devices > 0) {
    for (int i = 0; i < n_devices; i++) {
      if (devices[i] < 0 || devices[i] >= count) return BLSGPU_ERR_ARGS;
      ids.push_back(devices[i]);
    }
  } else {
    for (int i = 0; i < count; i++) ids.push_back(i);
  }
  blsgpu_ctx* ctx = new blsgpu_ctx();
  ctx->hw_queues = hw_queues_of_process();
  ctx->slots_per_device = default_slots(ctx->hw_queues);
  // diagnostics / tests: BLSGPU_MILLER_SEGMENTS = J forces the one-lane accumulation's step segments (run_shard);
  // unset, 0 or anything else: by run size
  if (const char* v = getenv("BLSGPU_MILLER_SEGMENTS")) {
    const long j = strtol(v, nullptr, 10);
    if (j >= 1 && j <= MILLER_MAX_SEGS) ctx->opt.miller_segments = j;
  }
  try {
    for (int id : ids) {
      Device* d = new Device();
      d->id = id;
      ctx->devs.push_back(d);
      HIPCHK(hipSetDevice(id));
      HIPCHK(hipStreamCreateWithFlags(&d->table_stream, hipStreamNonBlocking));
      // (the pipeline and urgent streams are created with the first call: create_streams)
    }
  } catch (HipError&) {
    blsgpu_destroy(ctx);
    return BLSGPU_ERR_NO_DEVICE;
  }
  *out = ctx;
  return BLSGPU_OK;
}

void blsgpu_destroy(blsgpu_ctx* ctx) {
  if (!ctx) return;
  {
    std::unique_lock<std::mutex> lk(ctx->active_mu);
    ctx->closed = true;  // queued asynchronous shards now complete with BLSGPU_ERR_CLOSED
    ctx->active_cv.wait(lk, [&] { return ctx->active == 0; });
  }
  for (Device* d : ctx->devs) destroy_device(d);
  delete ctx;
}

int blsgpu_device_count(const blsgpu_ctx* ctx) { return ctx ? (int)ctx->devs.size() : 0; }

uint32_t blsgpu_pubkeys_count(const blsgpu_ctx* ctx) {
  if (!ctx || ctx->devs.empty()) return 0;
  uint32_t n = UINT32_MAX;
  for (Device* d : ctx->devs) {
    std::shared_lock<std::shared_mutex> lk(d->table_mu);
    n = std::min(n, d->table_n);
  }
  return n;
}

int blsgpu_pubkeys_upload(blsgpu_ctx* ctx, uint32_t first_index, const uint8_t* pk96, uint32_t n) {
  if (!ctx) return BLSGPU_ERR_ARGS;
  if (n == 0) return BLSGPU_OK;
  if (!pk96) return BLSGPU_ERR_ARGS;
  if (!enter(ctx)) return BLSGPU_ERR_CLOSED;
  std::lock_guard<std::mutex> tl(ctx->table_mu);
  int result = BLSGPU_OK;
  for (Device* d : ctx->devs) {  // no gaps: an upload may only extend or overwrite the table
    std::shared_lock<std::shared_mutex> lk(d->table_mu);
    if (first_index > d->table_n) result = BLSGPU_ERR_ARGS;
  }
  // every device decodes and stores its own replica; the devices upload concurrently (one host thread each), so a
  // 2^20-key table on 8 GPUs costs one device's upload time, not eight
  auto upload_one = [&](Device* d) -> int {
    try {
      HIPCHK(hipSetDevice(d->id));
      hipStream_t ts = d->table_stream;
      const uint32_t need = first_index + n;
      uint8_t* dpk = nullptr;
      int8_t* dst = nullptr;
      uint32_t* tmp = nullptr;
      HIPCHK(hipMalloc((void**)&dpk, (size_t)n * 96));
      HIPCHK(hipMalloc((void**)&dst, n));
      HIPCHK(hipMalloc((void**)&tmp, (size_t)n * W_PKTAB * 4));
      HIPCHK(hipMemcpyAsync(dpk, pk96, (size_t)n * 96, hipMemcpyHostToDevice, ts));
      launch_pk_table_fill(dpk, n, tmp, dst, ts);
      HIPCHK(hipGetLastError());
      std::vector<int8_t> hst(n);
      HIPCHK(hipMemcpyAsync(hst.data(), dst, n, hipMemcpyDeviceToHost, ts));
      HIPCHK(hipStreamSynchronize(ts));
      int err = 0;
      for (uint32_t i = 0; i < n && !err; i++) err = hst[i];
      if (!err) {
        std::unique_lock<std::shared_mutex> lk(d->table_mu);
        if (need > d->table.cap / W_PKTAB) {
          DevBuf<uint32_t> nt;
          nt.ensure((size_t)std::max<uint32_t>(need, d->table_n + d->table_n / 2) * W_PKTAB);
          if (d->table_n)
            HIPCHK(hipMemcpyAsync(nt.p, d->table.p, (size_t)d->table_n * W_PKTAB * 4, hipMemcpyDeviceToDevice, ts));
          d->table.release();
          d->table = nt;
        }
        // (on the table stream: a null-stream copy would also wait for the CU-masked streams, which are blocking)
        HIPCHK(hipMemcpyAsync(d->table.p + (size_t)first_index * W_PKTAB, tmp, (size_t)n * W_PKTAB * 4,
                              hipMemcpyDeviceToDevice, ts));
        HIPCHK(hipStreamSynchronize(ts));
        d->table_n = std::max(d->table_n, need);
      }
      (void)hipFree(dpk);
      (void)hipFree(dst);
      (void)hipFree(tmp);
      return err;
    } catch (HipError&) {
      return BLSGPU_DEVICE_ERROR;
    } catch (std::exception&) {
      return BLSGPU_DEVICE_ERROR;
    }
  };
  if (!result) {
    std::vector<int> rc(ctx->devs.size(), 0);
    if (ctx->devs.size() == 1) {
      rc[0] = upload_one(ctx->devs[0]);
    } else {
      std::vector<std::thread> th;
      for (size_t k = 0; k < ctx->devs.size(); k++) th.emplace_back([&, k] { rc[k] = upload_one(ctx->devs[k]); });
      for (auto& t : th) t.join();
    }
    for (int r : rc)
      if (r && !result) result = r;
  }
  leave(ctx);
  return result;
}

int blsgpu_set_option(blsgpu_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return BLSGPU_ERR_ARGS;
  std::string k(key);
  if (k == "urgent_cus" || k == "urgent_isolate" || k == "blocking_sync" || k == "pipeline_prio") {
    // stream / event creation: before the first call only
    std::lock_guard<std::mutex> sk(ctx->slots_mu);
    if (ctx->slots_started) return BLSGPU_ERR_ARGS;
    if (k == "blocking_sync" || k == "pipeline_prio") {
      if (value < 0 || value > 1) return BLSGPU_ERR_ARGS;
      (k == "blocking_sync" ? ctx->blocking_sync : ctx->pipeline_prio) = value;
    } else if (k == "urgent_cus") {
      if (value < 0 || value > 128 || (value & 7)) return BLSGPU_ERR_ARGS;
      ctx->urgent_cus = value;
    } else {
      if (value < 0 || value > 3) return BLSGPU_ERR_ARGS;
      ctx->urgent_isolate = value;
    }
    return BLSGPU_OK;
  }
  if (k == "slots") {
    // not from a dispatcher thread (a done callback): retiring its own slot would join itself
    if (value < 1 || value > 64 || tl_dispatcher) return BLSGPU_ERR_ARGS;
    std::lock_guard<std::mutex> sk(ctx->slots_mu);
    ctx->slots_per_device = value;
    if (ctx->slots_started) {
      try {
        for (Device* d : ctx->devs) resize_slots(d, value);
      } catch (HipError&) {
        return BLSGPU_DEVICE_ERROR;
      }
    }
    return BLSGPU_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->opt_mu);
  if (k == "group_sets") {
    if (value < 1) return BLSGPU_ERR_ARGS;
    ctx->opt.group_sets = value;
  } else if (k == "profile") {
    ctx->opt.profile = value != 0;
  } else if (k == "max_devices") {
    if (value < 1) return BLSGPU_ERR_ARGS;
    ctx->opt.max_devices = value;
  } else if (k == "dedupe") {
    ctx->opt.dedupe = value != 0;
  } else if (k == "merge_sets") {
    if (value < 0) return BLSGPU_ERR_ARGS;
    ctx->opt.merge_sets = value;
  } else if (k == "miller_k") {
    if (value < 0 || value > 64) return BLSGPU_ERR_ARGS;
    ctx->opt.miller_k = value;
  } else if (k == "group_policy") {
    if (value < 0 || value > 1) return BLSGPU_ERR_ARGS;
    ctx->opt.group_policy = value;
  } else if (k == "merge_wait_us") {
    if (value < 0 || value > 1000000) return BLSGPU_ERR_ARGS;
    ctx->opt.merge_wait_us = value;
  } else if (k == "idle_wait_us") {
    if (value < 0 || value > 1000000) return BLSGPU_ERR_ARGS;
    ctx->opt.idle_wait_us = value;
  } else if (k == "pipeline_depth") {
    if (value < 1 || value > 64) return BLSGPU_ERR_ARGS;
    ctx->opt.pipeline_depth = value;
  } else if (k == "serial") {
    ctx->opt.serial = value != 0;
  } else if (k == "miller_lanes") {
    if (value < 0 || (value > 3 && value != 6)) return BLSGPU_ERR_ARGS;
    ctx->opt.miller_lanes = value;
  } else if (k == "msm_slice_mid") {
    if (value < 8 || value > MSM_SLICE) return BLSGPU_ERR_ARGS;
    ctx->opt.msm_slice_mid = value;
  } else if (k == "copy_stream") {
    ctx->opt.copy_stream = value != 0;
  } else if (k == "tail_on_msg") {
    ctx->opt.tail_on_msg = value != 0;
  } else if (k == "early_release") {
    ctx->opt.early_release = value != 0;
  } else if (k == "merge_balance") {
    ctx->opt.merge_balance = value != 0;
  } else if (k == "lines_lanes") {
    if (value < 1 || value > 2) return BLSGPU_ERR_ARGS;
    ctx->opt.lines_lanes = value;
  } else if (k == "msm_tree") {
    ctx->opt.msm_tree = value != 0;
  } else if (k == "coop_max") {
    if (value < 0 || value > (1 << 24)) return BLSGPU_ERR_ARGS;
    ctx->opt.coop_max = value;
  } else if (k == "coop_g2_max") {
    if (value < 0 || value > (1 << 24)) return BLSGPU_ERR_ARGS;
    ctx->opt.coop_g2_max = value;
  } else if (k == "coop_excl_max") {
    if (value < 0 || value > (1 << 24)) return BLSGPU_ERR_ARGS;
    ctx->opt.coop_excl_max = value;
  } else if (k == "rsig_spec") {
    ctx->opt.rsig_spec = value != 0;
  } else if (k == "spec_large") {
    ctx->opt.spec_large = value != 0;
  } else if (k == "spec_gsm") {
    ctx->opt.spec_gsm = value != 0;
  } else if (k == "fb_lane_min") {
    if (value < 0) return BLSGPU_ERR_ARGS;
    ctx->opt.fb_lane_min = value;
  } else if (k == "fb_force_busy") {
    ctx->opt.fb_force_busy = value != 0;
  } else if (k == "keep_f") {
    ctx->opt.keep_f = value != 0;
  } else if (k == "keep_copy") {
    ctx->opt.keep_copy = value != 0;
  } else if (k == "urgent_lane") {
    ctx->opt.urgent_lane = value != 0;
  } else if (k == "urgent_max_sets") {
    if (value < 0) return BLSGPU_ERR_ARGS;
    ctx->opt.urgent_max_sets = value;
  } else if (k == "urgent_excl") {
    ctx->opt.urgent_excl = value != 0;
  } else if (k == "group_adapt") {
    ctx->opt.group_adapt = value != 0;
  } else if (k == "urgent_wait_us") {
    if (value < 0 || value > 100000) return BLSGPU_ERR_ARGS;
    ctx->opt.urgent_wait_us = value;
  } else if (k == "fb_check6") {
    if (value < 0 || value > 2) return BLSGPU_ERR_ARGS;
    ctx->opt.fb_check6 = value;
  } else if (k == "fb_direct_min") {
    if (value < 0) return BLSGPU_ERR_ARGS;
    ctx->opt.fb_direct_min = value;
  } else if (k == "small_max") {
    if (value < 0) return BLSGPU_ERR_ARGS;
    ctx->opt.small_max = value;
  } else if (k == "miller_pairs") {
    if (value < 0 || value > 1) return BLSGPU_ERR_ARGS;
    ctx->opt.miller_pairs = value;
  } else if (k == "acc6_max") {
    if (value < 0) return BLSGPU_ERR_ARGS;
    ctx->opt.acc6_max = value;
  } else if (k == "route_split_sets") {
    if (value < 1) return BLSGPU_ERR_ARGS;
    ctx->opt.route_split_sets = value;
  } else if (k == "lane_tail_parts") {
    if (value < 0 || value > 3) return BLSGPU_ERR_ARGS;
    ctx->opt.lane_tail_parts = value;
  } else if (k == "lane_tail_min") {
    if (value < 0) return BLSGPU_ERR_ARGS;
    ctx->opt.lane_tail_min = value;
  } else if (k == "f_run_max") {
    if (value < 1 || value > 1024 || (value & (value - 1))) return BLSGPU_ERR_ARGS;
    ctx->opt.f_run_max = value;
  } else {
    return BLSGPU_ERR_ARGS;
  }
  return BLSGPU_OK;
}

int blsgpu_get_option(const blsgpu_ctx* cctx, const char* key, int64_t* value) {
  if (!cctx || !key || !value) return BLSGPU_ERR_ARGS;
  blsgpu_ctx* ctx = const_cast<blsgpu_ctx*>(cctx);
  const std::string k(key);
  if (k == "slots") {
    std::lock_guard<std::mutex> sk(ctx->slots_mu);
    if (ctx->slots_started && !ctx->devs.empty()) {
      std::lock_guard<std::mutex> lk(ctx->devs[0]->q_mu);
      *value = (int64_t)ctx->devs[0]->slots.size();
    } else {
      *value = ctx->slots_per_device;
    }
    return BLSGPU_OK;
  }
  if (k == "hw_queues") {
    *value = ctx->hw_queues;
    return BLSGPU_OK;
  }
  if (k == "blocking_sync" || k == "pipeline_prio") {
    std::lock_guard<std::mutex> sk(ctx->slots_mu);
    *value = k == "blocking_sync" ? ctx->blocking_sync : ctx->pipeline_prio;
    return BLSGPU_OK;
  }
  if (k == "urgent_cus" || k == "urgent_isolate") {
    std::lock_guard<std::mutex> sk(ctx->slots_mu);
    // once the streams exist: the partition device 0 was created with (0 when the device is too small for it)
    if (k == "urgent_cus")
      *value = ctx->slots_started && !ctx->devs.empty() ? ctx->devs[0]->urgent_cus : ctx->urgent_cus;
    else
      *value = ctx->urgent_isolate;
    return BLSGPU_OK;
  }
  if (k == "abi_version") {
    *value = BLSGPU_ABI_VERSION;
    return BLSGPU_OK;
  }
  if (k == "spurious_groups") {
    uint64_t c = 0;
    for (const Device* d : ctx->devs) c += d->spurious_groups.load(std::memory_order_relaxed);
    *value = (int64_t)c;
    return BLSGPU_OK;
  }
  std::lock_guard<std::mutex> lk(ctx->opt_mu);
  const Options& o = ctx->opt;
  if (k == "group_sets") *value = o.group_sets;
  else if (k == "profile") *value = o.profile;
  else if (k == "max_devices") *value = o.max_devices;
  else if (k == "dedupe") *value = o.dedupe;
  else if (k == "merge_sets") *value = o.merge_sets;
  else if (k == "miller_k") *value = o.miller_k;
  else if (k == "group_policy") *value = o.group_policy;
  else if (k == "merge_wait_us") *value = o.merge_wait_us;
  else if (k == "idle_wait_us") *value = o.idle_wait_us;
  else if (k == "pipeline_depth") *value = o.pipeline_depth;
  else if (k == "serial") *value = o.serial;
  else if (k == "miller_lanes") *value = o.miller_lanes;
  else if (k == "f_run_max") *value = o.f_run_max;
  else if (k == "lane_tail_min") *value = o.lane_tail_min;
  else if (k == "lane_tail_parts") *value = o.lane_tail_parts;
  else if (k == "msm_slice_mid") *value = o.msm_slice_mid;
  else if (k == "msm_tree") *value = o.msm_tree;
  else if (k == "lines_lanes") *value = o.lines_lanes;
  else if (k == "merge_balance") *value = o.merge_balance;
  else if (k == "early_release") *value = o.early_release;
  else if (k == "tail_on_msg") *value = o.tail_on_msg;
  else if (k == "copy_stream") *value = o.copy_stream;
  else if (k == "coop_max") *value = o.coop_max;
  else if (k == "coop_g2_max") *value = o.coop_g2_max;
  else if (k == "coop_excl_max") *value = o.coop_excl_max;
  else if (k == "rsig_spec") *value = o.rsig_spec;
  else if (k == "spec_large") *value = o.spec_large;
  else if (k == "spec_gsm") *value = o.spec_gsm;
  else if (k == "fb_lane_min") *value = o.fb_lane_min;
  else if (k == "route_split_sets") *value = o.route_split_sets;
  else if (k == "acc6_max") *value = o.acc6_max;
  else if (k == "miller_pairs") *value = o.miller_pairs;
  else if (k == "small_max") *value = o.small_max;
  else if (k == "fb_direct_min") *value = o.fb_direct_min;
  else if (k == "fb_check6") *value = o.fb_check6;
  else if (k == "fb_force_busy") *value = o.fb_force_busy;
  else if (k == "keep_f") *value = o.keep_f;
  else if (k == "keep_copy") *value = o.keep_copy;
  else if (k == "urgent_lane") *value = o.urgent_lane;
  else if (k == "urgent_max_sets") *value = o.urgent_max_sets;
  else if (k == "urgent_excl") *value = o.urgent_excl;
  else if (k == "urgent_wait_us") *value = o.urgent_wait_us;
  else if (k == "group_adapt") *value = o.group_adapt;
  else return BLSGPU_ERR_ARGS;
  return BLSGPU_OK;
}

int blsgpu_chunkify(uint32_t len, uint32_t min_per_chunk, uint32_t* chunk_first, uint32_t* n_chunks) {
  if (!chunk_first || !n_chunks || min_per_chunk == 0) return BLSGPU_ERR_ARGS;
  const uint32_t per = chunk_size(len, min_per_chunk);
  uint32_t c = 0;
  if (len / min_per_chunk <= 1) chunk_first[c++] = 0;  // [arr], also for an empty arr
  else
    for (uint32_t i = 0; i < len; i += per) chunk_first[c++] = i;
  chunk_first[c] = len;
  *n_chunks = c;
  return BLSGPU_OK;
}

int blsgpu_verify(blsgpu_ctx* ctx, const blsgpu_batch* b, int8_t* job_result, blsgpu_stats* stats) {
  if (!ctx) return BLSGPU_ERR_ARGS;
  int v = validate_batch(b);
  if (v) return v;
  if (b->n_jobs && !job_result) return BLSGPU_ERR_ARGS;
  if (!enter(ctx)) return BLSGPU_ERR_CLOSED;
  Call c;
  c.ctx = ctx;
  c.b = *b;
  c.job_result = job_result;
  c.stats = stats;
  if (!resolve_key(b->seed, c.key, c.seed)) {
    reject_all(b, job_result, BLSGPU_DEVICE_ERROR);
    leave(ctx);
    return BLSGPU_ERR_ENTROPY;
  }
  c.max_index = max_table_index(b);
  c.opt = snapshot(ctx);
  c.sync = true;
  if (b->n_jobs == 0) {
    if (stats) *stats = blsgpu_stats{};
    leave(ctx);
    return BLSGPU_OK;
  }
  if (int e = ensure_slots(ctx)) {
    leave(ctx);
    return e;
  }
  launch_call(ctx, &c);
  std::unique_lock<std::mutex> lk(c.m);
  c.cv.wait(lk, [&] { return c.finished; });
  return c.status;  // device errors are reported per job
}

int blsgpu_submit(blsgpu_ctx* ctx, const blsgpu_batch* b, int8_t* job_result, blsgpu_stats* stats,
                  blsgpu_done_cb done, void* user) {
  if (!ctx || !b) return BLSGPU_ERR_ARGS;
  int v = validate_batch(b);
  if (v) return v;
  if (b->n_jobs && !job_result) return BLSGPU_ERR_ARGS;
  if (!enter(ctx)) return BLSGPU_ERR_CLOSED;
  batch_rand::Key key;
  uint64_t hash_key = 0;
  if (!resolve_key(b->seed, key, hash_key)) {
    reject_all(b, job_result, BLSGPU_DEVICE_ERROR);
    leave(ctx);
    return BLSGPU_ERR_ENTROPY;
  }
  // deep-copy the inputs so the caller may reuse its buffers immediately
  Call* c = new Call();
  c->key = key;
  c->seed = hash_key;
  Owned* o = new Owned();
  c->ctx = ctx;
  c->owned = o;
  c->b = *b;
  o->jfs.assign(b->job_first_set, b->job_first_set + b->n_jobs + 1);
  c->b.job_first_set = o->jfs.data();
  if (b->job_flags) {
    o->jflags.assign(b->job_flags, b->job_flags + b->n_jobs);
    c->b.job_flags = o->jflags.data();
  }
  o->siglen.assign(b->sig_len, b->sig_len + b->n_sets);
  c->b.sig_len = o->siglen.data();
  o->sigs.assign(b->sigs, b->sigs + (size_t)b->n_sets * b->sig_stride);
  c->b.sigs = o->sigs.data();
  o->msgs.assign(b->msgs, b->msgs + (size_t)b->n_sets * 32);
  c->b.msgs = o->msgs.data();
  const uint32_t npk = b->set_pk_first ? b->set_pk_first[b->n_sets] : b->n_sets;
  if (b->set_pk_first) {
    o->pkfirst.assign(b->set_pk_first, b->set_pk_first + b->n_sets + 1);
    c->b.set_pk_first = o->pkfirst.data();
  }
  if (b->pk_bytes) {
    o->pkb.assign(b->pk_bytes, b->pk_bytes + (size_t)npk * 96);
    c->b.pk_bytes = o->pkb.data();
  } else {
    o->pkidx.assign(b->pk_index, b->pk_index + npk);
    c->b.pk_index = o->pkidx.data();
  }
  c->job_result = job_result;
  c->stats = stats;
  c->max_index = max_table_index(&c->b);
  c->opt = snapshot(ctx);
  c->done = done;
  c->user = user;
  if (b->n_jobs == 0) {
    c->shards.clear();
    finish_call(c);  // calls done(user, OK) and leaves
    return BLSGPU_OK;
  }
  if (int e = ensure_slots(ctx)) {
    delete c->owned;
    delete c;
    leave(ctx);
    return e;
  }
  launch_call(ctx, c);
  return BLSGPU_OK;
}

int blsgpu_batch_scalars(const blsgpu_batch* b, uint64_t* words) {
  if (!b || !b->job_first_set || (b->n_sets && !words)) return BLSGPU_ERR_ARGS;
  // the job structure validate_batch requires (first entry 0, non-decreasing, last == n_sets): shard_scalars writes
  // out[first set of a job] for single-set jobs, which must stay inside words[0 .. n_sets)
  if (b->n_jobs == 0 ? b->n_sets != 0 : (b->job_first_set[0] != 0 || b->job_first_set[b->n_jobs] != b->n_sets))
    return BLSGPU_ERR_ARGS;
  for (uint32_t j = 0; j < b->n_jobs; j++)
    if (b->job_first_set[j + 1] < b->job_first_set[j]) return BLSGPU_ERR_ARGS;
  batch_rand::Key key;
  uint64_t hash_key = 0;
  if (!resolve_key(b->seed, key, hash_key)) return BLSGPU_ERR_ENTROPY;
  shard_scalars(*b, Shard{0, b->n_jobs, 0, b->n_sets}, key, words);
  return BLSGPU_OK;
}

int blsgpu_debug_inject(int what, int64_t skip, int64_t count) {
  // a process-wide failure switch: armed only in processes started with BLSGPU_FAULT_INJECTION=1 (tests), read once
  static const bool enabled = [] {
    const char* v = getenv("BLSGPU_FAULT_INJECTION");
    return v && v[0] == '1' && v[1] == 0;
  }();
  if (!enabled || skip < 0 || count < 0) return BLSGPU_ERR_ARGS;
  if (what == BLSGPU_INJECT_ENTROPY) {
    batch_rand::inject_count() = 0;
    batch_rand::inject_skip() = skip;
    batch_rand::inject_count() = count;
  } else if (what == BLSGPU_INJECT_DEVICE) {
    g_fail_run_count = 0;
    g_fail_run_skip = skip;
    g_fail_run_count = count;
  } else {
    return BLSGPU_ERR_ARGS;
  }
  return BLSGPU_OK;
}

int blsgpu_route_call(uint32_t n_sets, uint32_t n_devices, const int64_t* device_load, int64_t split_sets,
                      uint32_t start, uint32_t* out_devices, uint32_t* n_out) {
  if (!n_out || n_devices == 0 || !device_load || !out_devices || split_sets < 1) return BLSGPU_ERR_ARGS;
  *n_out = route_rule(n_sets, n_devices, device_load, split_sets, start, out_devices);
  return BLSGPU_OK;
}

int blsgpu_shard_jobs(const uint32_t* job_first_set, const uint32_t* set_pk_first, uint32_t n_jobs,
                      uint32_t n_parts, uint32_t* part_first_job) {
  if (!job_first_set || !part_first_job || n_parts == 0) return BLSGPU_ERR_ARGS;
  shard_rule(job_first_set, set_pk_first, n_jobs, n_parts, part_first_job);
  return BLSGPU_OK;
}

const char* blsgpu_code_name(int code) {
  switch (code) {
    case BLSGPU_OK: return "BLST_SUCCESS";
    case BLSGPU_BAD_ENCODING: return "BLST_BAD_ENCODING";
    case BLSGPU_POINT_NOT_ON_CURVE: return "BLST_POINT_NOT_ON_CURVE";
    case BLSGPU_POINT_NOT_IN_GROUP: return "BLST_POINT_NOT_IN_GROUP";
    case BLSGPU_AGGR_TYPE_MISMATCH: return "BLST_AGGR_TYPE_MISMATCH";
    case BLSGPU_VERIFY_FAIL: return "BLST_VERIFY_FAIL";
    case BLSGPU_PK_IS_INFINITY: return "BLST_PK_IS_INFINITY";
    case BLSGPU_BAD_SCALAR: return "BLST_BAD_SCALAR";
    case BLSGPU_INVALID_SIZE: return "BLST_INVALID_SIZE";
    case BLSGPU_EMPTY_AGGREGATE: return "EMPTY_AGGREGATE_ARRAY";
    case BLSGPU_EMPTY_SET: return "Empty signature set";
    case BLSGPU_DEVICE_ERROR: return "BLSGPU_DEVICE_ERROR";
    case BLSGPU_ERR_ARGS: return "BLSGPU_ERR_ARGS";
    case BLSGPU_ERR_NO_DEVICE: return "BLSGPU_ERR_NO_DEVICE";
    case BLSGPU_ERR_CLOSED: return "QUEUE_ERROR_QUEUE_ABORTED";
    case BLSGPU_ERR_ENTROPY: return "BLSGPU_ERR_ENTROPY";
    default: return nullptr;
  }
}

}  // extern "C"
