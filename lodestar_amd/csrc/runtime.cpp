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
//
// This unit holds the contexts, devices, slots, the two dispatchers (worker_loop, urgent_loop) with the one function
// that runs and completes the parts they form (run_parts), the uploads and the ABI entry points.  The host arithmetic
// lives in headers with no HIP in them, each checked by CPU tests through a probe: what a call decides before a run
// and the packing of a merged run in call_plan.hpp, the options table in options.hpp, the plan of a run in
// run_plan.hpp (pipeline.cpp runs it); helpers.cpp holds the synchronous helper calls.
#include <pthread.h>
#include <stdio.h>
#include <sys/random.h>

#include <system_error>

#include "call_plan.hpp"  // the HIP-free side of a call: validity, sharding, routing, scalars, merged batches
#include "runtime_internal.hpp"

using namespace blsgpu_rt;

namespace {

// set on the runtime's dispatcher threads (a `slots` change from a done callback would join its own thread)
thread_local bool tl_dispatcher = false;

}  // namespace

namespace blsgpu_rt __attribute__((visibility("hidden"))) {  // (Task, in runtime_internal.hpp, points to a Call)

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

// Does the device's table hold every index the call's shard uses?  (Checked per device under its table lock: a
// call may race an upload that has reached some devices only.)
inline bool table_covers(const Device& d, const Call* c, const Shard& sh) {
  return table_covers(c->b, sh, c->max_index, d.table_n);
}

// Several queued shards (of different calls) run as ONE pipeline: their inputs are concatenated into one
// batch (call_plan.hpp MergedBatch; jobs and results stay per call), so a launch fills the chip instead of one call's
// 16k-set share -- the device-side counterpart of the pool packing queued jobs into one worker request (prepareWork,
// multithread/index.ts:386-401).  Jobs never interact, so every job's result is the one it gets alone.  A call
// that cannot run (a table index beyond the device's table) is completed with ERR_ARGS on its own and never
// joins the run; a failure of the run gives its calls DEVICE_ERROR.  rcs: the parts' status codes.
// The caller holds the device's table lock (shared).
void run_merged(Device& d, Slot& sl, const std::vector<Task>& parts, std::vector<int>& rcs) {
  const auto t_merge0 = std::chrono::steady_clock::now();
  std::vector<size_t> live;
  std::vector<CallPart> live_parts;
  uint32_t max_index = 0;
  for (size_t p = 0; p < parts.size(); p++) {
    Call* c = parts[p].call;
    const Shard& sh = c->shards[parts[p].shard];
    if (c->ctx->closed && !c->sync) {
      rcs[p] = BLSGPU_ERR_CLOSED;
    } else if (!table_covers(d, c, sh)) {
      rcs[p] = BLSGPU_ERR_ARGS;
    } else {
      live.push_back(p);
      live_parts.push_back({c->b, sh, c->key, c->job_result});
      max_index = std::max(max_index, c->max_index);
    }
  }
  if (live.empty()) return;
  int rc = BLSGPU_OK;
  blsgpu_stats st{};
  try {
    const MergedBatch m(live_parts);
    std::vector<int8_t> res(std::max<uint32_t>(m.nj, 1), 0);
    const Call* c0 = parts[live[0]].call;
    tl_merge_ms = ms_since(t_merge0);
    rc = run_call_shard(d, sl, m.b, Shard{0, m.nj, 0, m.n}, res.data(), c0->seed, c0->opt, max_index, st,
                        m.scal.data());
    if (rc == BLSGPU_OK) scatter_results(m, live_parts, res.data());
  } catch (...) {
    rc = BLSGPU_DEVICE_ERROR;
  }
  st.run_calls = (uint32_t)live.size();
  for (size_t k = 0; k < live.size(); k++) {
    const size_t p = live[k];
    blsgpu_stats& cs = parts[p].call->sst[parts[p].shard];
    if (k == 0) {
      cs = st;  // the merged run's counters (and stage times) go to its first call
    } else {
      cs = blsgpu_stats{};
      cs.run_calls = st.run_calls;
    }
    rcs[p] = rc;
  }
}

// One shard as its own run; returns its status code.  The caller holds the device's table lock (shared).
int run_task(Device& d, Slot& sl, const Task& t) {
  Call* c = t.call;
  const Shard& sh = c->shards[t.shard];
  if (c->ctx->closed && !c->sync) return BLSGPU_ERR_CLOSED;
  if (!table_covers(d, c, sh)) return BLSGPU_ERR_ARGS;
  try {
    std::vector<uint64_t> scal(std::max<uint32_t>(sh.set_end - sh.set_begin, 1));
    shard_scalars(c->b, sh, c->key, scal.data());
    const int rc = run_call_shard(d, sl, c->b, sh, c->job_result, c->seed, c->opt, c->max_index, c->sst[t.shard],
                                  scal.data());
    c->sst[t.shard].run_calls = 1;
    return rc;
  } catch (...) {
    return BLSGPU_DEVICE_ERROR;
  }
}

// a device failure rejects every job of the shard, never `false`
void reject_shard(const Task& t) {
  const Shard& sh = t.call->shards[t.shard];
  for (uint32_t j = sh.job_begin; j < sh.job_end; j++) t.call->job_result[j] = -BLSGPU_DEVICE_ERROR;
}

// Completes the parts of a run with their status codes: a device error rejects every job of the part; the call whose
// last shard this was is finished.  lane: the urgent lane's run.
void complete_parts(Device& d, const std::vector<Task>& parts, const std::vector<int>& rcs, bool lane) {
  for (size_t p = 0; p < parts.size(); p++) {
    Call* c = parts[p].call;
    if (rcs[p] == BLSGPU_DEVICE_ERROR) reject_shard(parts[p]);
    c->rc[parts[p].shard] = rcs[p];
    c->sst[parts[p].shard].urgent_lane = lane ? 1 : 0;
    d.load.fetch_sub(c->shards[parts[p].shard].cost, std::memory_order_relaxed);  // (an urgent lane's shard costs 0)
    if (c->remaining.fetch_sub(1) == 1) finish_call(c);
  }
}

// Runs the parts a dispatcher formed -- one as its own run, several as one merged run -- on its slot (sl.urgent: the
// urgent lane's) and completes their calls.
void run_parts(Device& d, Slot& sl, const std::vector<Task>& parts) {
  std::vector<int> rcs(parts.size(), BLSGPU_OK);
  try {
    std::shared_lock<std::shared_mutex> tl(d.table_mu);
    if (parts.size() == 1)
      rcs[0] = run_task(d, sl, parts[0]);
    else
      run_merged(d, sl, parts, rcs);
  } catch (...) {  // the runs catch their own failures; this only guards the lock
    rcs.assign(parts.size(), BLSGPU_DEVICE_ERROR);
  }
  complete_parts(d, parts, rcs, sl.urgent);
}

inline uint32_t task_sets(const Task& t) {
  const Shard& sh = t.call->shards[t.shard];
  return sh.set_end - sh.set_begin;
}

// A slot's dispatcher: takes the oldest queued shard of its device, merges the compatible shards queued behind it
// (up to merge_sets sets), runs them, completes their calls.  Exits when the device stops (queue drained) or when
// the slot is retired (option `slots` lowered).
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
    // the run leaves the in-flight count when its batch pass completes (pipeline.cpp wait_batch_pass) or here
    struct InflightGuard {
      Device* d;
      Slot* sl;
      ~InflightGuard() { release_inflight(*d, *sl); }
    } guard{d, sl};
    run_parts(*d, *sl, parts);
  }
}

// The urgent lane's dispatcher: takes the oldest urgent call and the compatible urgent calls queued behind it (up to
// urgent_max_sets sets: a burst of urgent calls becomes one run, not a queue of runs), and runs them on the lane's own
// stream pairs (pipeline.cpp pick_streams: Slot::urgent) -- the reference's verifyOnMainThread verifies at once,
// outside the pool queue (multithread/index.ts:138-151).  `alone` holds for its streams, so a run takes the latency forms of an idle device:
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
    if (!ensure_urgent_streams(d, sl))  // no streams: every call of the run completes with a device error
      complete_parts(*d, parts, std::vector<int>(parts.size(), BLSGPU_DEVICE_ERROR), true);
    else
      run_parts(*d, *sl, parts);
    d->upending.fetch_sub((int)parts.size(), std::memory_order_relaxed);
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

// The device's pipeline streams and its urgent lane's (created with the first call, so `urgent_cus` set after init
// applies).  The urgent streams are CU-masked streams (hipExtStreamCreateWithCUMask), which HIP gives hardware queues
// of their own: an urgent kernel never waits in a queue behind a pipeline kernel, only for free SIMDs.  Their mask is
// every CU, or with `urgent_cus` > 0 a partition, mask bits [0, urgent_cus): the driver deals mask bits round-robin
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
  // (set_option refuses `slots` on a dispatcher thread, so no thread joins itself here; a failing join leaves the
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
  d->cm_first.release();
  d->cm_members.release();
  d->cm_sums.release();
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

// Creates the devices' slots on the first call (so a `slots` value set after init is the count created).
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

// Routes a call (whole, or split over the least-loaded devices: call_plan.hpp route_rule) and queues the shard tasks.
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
  // diagnostics / tests: BLSGPU_MILLER_SEGMENTS = J forces the one-lane accumulation's step segments (run_plan.hpp
  // plan_run); unset, 0 or anything else: by run size
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

}  // extern "C"

namespace {

// How one encoding fills table rows: `elem` bytes per key, and the launcher that decodes n keys at `src` (device) into
// n rows at `rows` and a status byte per key (an all-zero row for a rejected key); `validate` is passed on to it.
struct TableFill {
  uint32_t elem;
  void (*launch)(const uint8_t* src, uint32_t n, uint32_t* rows, int8_t* status, bool validate, hipStream_t s);
  bool validate;
};
void fill_from96(const uint8_t* src, uint32_t n, uint32_t* rows, int8_t* status, bool, hipStream_t s) {
  launch_pk_table_fill(src, n, rows, status, s);
}

// a device allocation of one upload, freed however the upload ends
struct UploadTemp {
  void* p = nullptr;
  ~UploadTemp() {
    if (p) (void)hipFree(p);
  }
};

// The scaffold of both table uploads (n > 0, keys non-null): entries [first_index, first_index + n) of every device's
// replica from keys[fill.elem k].  The call's value is the code of the lowest-index rejected key (nothing is written
// then), BLSGPU_ERR_ARGS for a first_index beyond the table, BLSGPU_ERR_CLOSED / BLSGPU_DEVICE_ERROR.  Once the keys
// were decoded, status (nullable, [n]) holds every key's code and *first_bad (nullable) the lowest rejected index or
// 0xffffffff: the decode is the same on every device, device 0's is reported.
int table_upload(blsgpu_ctx* ctx, uint32_t first_index, const uint8_t* keys, uint32_t n, const TableFill& fill,
                 int8_t* status, uint32_t* first_bad) {
  if (!enter(ctx)) return BLSGPU_ERR_CLOSED;
  std::lock_guard<std::mutex> tl(ctx->table_mu);
  int result = BLSGPU_OK;
  for (Device* d : ctx->devs) {  // no gaps: an upload may only extend or overwrite the table
    std::shared_lock<std::shared_mutex> lk(d->table_mu);
    if (first_index > d->table_n) result = BLSGPU_ERR_ARGS;
  }
  // every device decodes and stores its own replica; the devices upload concurrently (one host thread each), so a
  // 2^20-key table on 8 GPUs costs one device's upload time, not eight
  // (report: this device's statuses are the call's -- device 0)
  auto upload_one = [&](Device* d, bool report) -> int {
    try {
      HIPCHK(hipSetDevice(d->id));
      hipStream_t ts = d->table_stream;
      const uint32_t need = first_index + n;
      UploadTemp t_pk, t_st, t_rows;
      HIPCHK(hipMalloc(&t_pk.p, (size_t)n * fill.elem));
      HIPCHK(hipMalloc(&t_st.p, n));
      HIPCHK(hipMalloc(&t_rows.p, (size_t)n * W_PKTAB * 4));
      uint8_t* dpk = static_cast<uint8_t*>(t_pk.p);
      int8_t* dst = static_cast<int8_t*>(t_st.p);
      uint32_t* tmp = static_cast<uint32_t*>(t_rows.p);
      HIPCHK(hipMemcpyAsync(dpk, keys, (size_t)n * fill.elem, hipMemcpyHostToDevice, ts));
      fill.launch(dpk, n, tmp, dst, fill.validate, ts);
      HIPCHK(hipGetLastError());
      std::vector<int8_t> hst(n);
      HIPCHK(hipMemcpyAsync(hst.data(), dst, n, hipMemcpyDeviceToHost, ts));
      HIPCHK(hipStreamSynchronize(ts));
      int err = 0;
      uint32_t bad = 0xffffffffu;
      for (uint32_t i = 0; i < n && !err; i++)
        if (hst[i]) err = hst[i], bad = i;
      if (report) {
        if (status) memcpy(status, hst.data(), n);
        if (first_bad) *first_bad = bad;
      }
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
        // rows were overwritten: the stored committee sums (helpers.cpp) may no longer be their members' sums
        if (first_index < d->table_n) d->cm_n = 0, d->cm_first_host.clear();
        d->table_n = std::max(d->table_n, need);
      }
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
      rc[0] = upload_one(ctx->devs[0], true);
    } else {
      std::vector<std::thread> th;
      for (size_t k = 0; k < ctx->devs.size(); k++)
        th.emplace_back([&, k] { rc[k] = upload_one(ctx->devs[k], k == 0); });
      for (auto& t : th) t.join();
    }
    for (int r : rc)
      if (r && !result) result = r;
  }
  leave(ctx);
  return result;
}

}  // namespace

extern "C" {

int blsgpu_pubkeys_upload(blsgpu_ctx* ctx, uint32_t first_index, const uint8_t* pk96, uint32_t n) {
  if (!ctx) return BLSGPU_ERR_ARGS;
  if (n == 0) return BLSGPU_OK;
  if (!pk96) return BLSGPU_ERR_ARGS;
  return table_upload(ctx, first_index, pk96, n, TableFill{96, fill_from96, false}, nullptr, nullptr);
}

int blsgpu_pubkeys_upload_compressed(blsgpu_ctx* ctx, uint32_t first_index, const uint8_t* pk48, uint32_t n,
                                     uint32_t flags, int8_t* status, uint32_t* first_bad) {
  if (!ctx || (flags & ~BLSGPU_PK_VALIDATE)) return BLSGPU_ERR_ARGS;
  if (n == 0) return BLSGPU_OK;
  if (!pk48 || (uint64_t)first_index + n > 0xffffffffull) return BLSGPU_ERR_ARGS;
  const TableFill fill{48, launch_pk_table_fill48, (flags & BLSGPU_PK_VALIDATE) != 0};
  return table_upload(ctx, first_index, pk48, n, fill, status, first_bad);
}

// The options of the table (options.hpp kOptionRows) are stored in ctx->opt under opt_mu; the keys that live on the
// context itself (CtxKey) are handled here by name.
int blsgpu_set_option(blsgpu_ctx* ctx, const char* key, int64_t value) {
  if (!ctx || !key) return BLSGPU_ERR_ARGS;
  const CtxKey k = ctx_key(key);
  if (k == CtxKey::slots) {
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
  if (k != CtxKey::none) {
    // stream / event creation: before the first call only
    std::lock_guard<std::mutex> sk(ctx->slots_mu);
    if (ctx->slots_started) return BLSGPU_ERR_ARGS;
    switch (k) {
      case CtxKey::blocking_sync:
      case CtxKey::pipeline_prio:
        if (value < 0 || value > 1) return BLSGPU_ERR_ARGS;
        (k == CtxKey::blocking_sync ? ctx->blocking_sync : ctx->pipeline_prio) = value;
        return BLSGPU_OK;
      case CtxKey::urgent_cus:
        if (value < 0 || value > 128 || (value & 7)) return BLSGPU_ERR_ARGS;
        ctx->urgent_cus = value;
        return BLSGPU_OK;
      case CtxKey::urgent_isolate:
        if (value < 0 || value > 3) return BLSGPU_ERR_ARGS;
        ctx->urgent_isolate = value;
        return BLSGPU_OK;
      default:  // the read-only keys
        return BLSGPU_ERR_ARGS;
    }
  }
  const OptionRow* row = find_option(key, true);
  if (!row) return BLSGPU_ERR_ARGS;
  std::lock_guard<std::mutex> lk(ctx->opt_mu);
  return store_option(ctx->opt, *row, value) ? BLSGPU_OK : BLSGPU_ERR_ARGS;
}

int blsgpu_get_option(const blsgpu_ctx* cctx, const char* key, int64_t* value) {
  if (!cctx || !key || !value) return BLSGPU_ERR_ARGS;
  blsgpu_ctx* ctx = const_cast<blsgpu_ctx*>(cctx);
  const CtxKey k = ctx_key(key);
  if (k == CtxKey::none) {
    const OptionRow* row = find_option(key, true);
    if (!row) return BLSGPU_ERR_ARGS;
    std::lock_guard<std::mutex> lk(ctx->opt_mu);
    *value = ctx->opt.*row->member;
    return BLSGPU_OK;
  }
  if (k == CtxKey::hw_queues) {
    *value = ctx->hw_queues;
  } else if (k == CtxKey::abi_version) {
    *value = BLSGPU_ABI_VERSION;
  } else if (k == CtxKey::spurious_groups) {
    uint64_t c = 0;
    for (const Device* d : ctx->devs) c += d->spurious_groups.load(std::memory_order_relaxed);
    *value = (int64_t)c;
  } else {
    std::lock_guard<std::mutex> sk(ctx->slots_mu);
    const bool started = ctx->slots_started && !ctx->devs.empty();
    if (k == CtxKey::slots) {
      if (started) {
        std::lock_guard<std::mutex> lk(ctx->devs[0]->q_mu);
        *value = (int64_t)ctx->devs[0]->slots.size();
      } else {
        *value = ctx->slots_per_device;
      }
    } else if (k == CtxKey::urgent_cus) {
      // once the streams exist: the partition device 0 was created with (0 when the device is too small for it)
      *value = started ? ctx->devs[0]->urgent_cus : ctx->urgent_cus;
    } else {
      *value = k == CtxKey::urgent_isolate ? ctx->urgent_isolate
               : k == CtxKey::blocking_sync ? ctx->blocking_sync
                                            : ctx->pipeline_prio;
    }
  }
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
