// Host types the translation units of the runtime share: runtime.cpp (contexts, devices, slots, dispatchers, uploads,
// the ABI; the call side's arithmetic is call_plan.hpp, the options table options.hpp),
// pipeline.cpp (one pipeline run: run_call_shard) and helpers.cpp (the synchronous helper calls).  Nothing here is
// part of the C ABI (include/blsgpu.h): the namespace is hidden, so none of it reaches the library's dynamic symbol
// table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <shared_mutex>
#include <thread>
#include <vector>

#include "../../include/blsgpu.h"
#include "batch_rand.hpp"
#include "kernels.h"
#include "run_plan.hpp"  // Options (options.hpp), Shard, pk_mode, MsgIndex, al256 and the plan of a pipeline run: the
                         // HIP-free side

namespace blsgpu_rt __attribute__((visibility("hidden"))) {

struct HipError {
  hipError_t e;
};
#define HIPCHK(x)                             \
  do {                                        \
    hipError_t _e = (x);                      \
    if (_e != hipSuccess) throw HipError{_e}; \
  } while (0)

// g_grow_mu and tl_async_grow (below) are C++17 inline variables: DevBuf, defined in this header, needs them, and an
// inline variable is ONE object in the library (one per thread for the thread-local) however many translation units
// include the header.  In an anonymous namespace, or static, each unit would get its own: two copies of g_grow_mu
// would undo what it is for, growth of stream-ordered buffers serialized across all threads.  So are
// the state runtime.cpp sets and pipeline.cpp reads (below); tl_dispatcher is used by runtime.cpp alone and is defined
// there.
// Device-failure injection (blsgpu_debug_inject, tests only): the next `count` pipeline runs after `skip` more fail as
// if a HIP call had failed once their batch pass completed.
inline std::atomic<int64_t> g_fail_run_skip{0}, g_fail_run_count{0};
// per dispatcher thread: when the slot picked its run, and the milliseconds it spent merging calls into it (st.host_ms,
// BLSGPU_HOST_TRACE)
inline thread_local std::chrono::steady_clock::time_point tl_run_t0;
inline thread_local double tl_merge_ms = 0;
// Device buffer that only grows.  A slot's buffers grow stream-ordered (hipFreeAsync / hipMallocAsync on the
// slot's stream): a plain hipFree waits for the whole device, so a merged run larger than any before would stall
// every other slot's work (seen as 1.4-2.5 s call latencies in the bench's tail).  Growth doubles.
// growths of stream-ordered slot buffers by this thread (pipeline.cpp enqueue_batch_pass: an input copy may leave the
// run's stream only when no buffer of the run was (re)allocated in that stream's order)
inline thread_local uint64_t tl_async_grow = 0;
// Diagnostics (BLSGPU_POISON=1 in the environment): every (re)allocated device buffer is filled with 0xA5 bytes before
// first use, so a kernel that reads memory no kernel of its run wrote fails every time instead of only when the
// allocator hands it memory another run left with different contents.
inline bool poison_buffers() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_POISON");
    return v && v[0] == '1';
  }();
  return on;
}
// Diagnostics (BLSGPU_SYNC_GROW=1): buffer growth with a whole-device synchronisation and plain hipFree / hipMalloc
// instead of stream-ordered hipFreeAsync / hipMallocAsync.
inline bool sync_grow() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_SYNC_GROW");
    return v && v[0] == '1';
  }();
  return on;
}
// Every growth and release of a stream-ordered slot buffer holds this lock: the dispatcher threads of a device's slots
// (and of every device) grow their buffers at the same moments -- a fresh process's first runs, and whenever the run
// shapes change -- and the stream-ordered pool is then entered from several threads at once.  Growth is rare (buffers
// only double), so the lock costs nothing measurable.  BLSGPU_GROW_UNLOCKED=1 (diagnostics) leaves it out.
inline std::mutex g_grow_mu;
inline bool grow_unlocked() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_GROW_UNLOCKED");
    return v && v[0] == '1';
  }();
  return on;
}
// Diagnostics (BLSGPU_FB_VERIFY=1): every fallback of small jobs is re-computed and compared (pipeline.cpp
// verify_fallback)
inline bool fb_verify() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_FB_VERIFY");
    return v && v[0] == '1';
  }();
  return on;
}
inline bool grow_free() {
  static const bool on = [] {
    const char* v = getenv("BLSGPU_GROW_FREE");
    return v && v[0] == '1';
  }();
  return on;
}
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  hipStream_t st = nullptr;  // set for slot buffers
  std::vector<T*> retired;   // outgrown stream-ordered blocks, freed with the buffer (ensure)
  void ensure(size_t n) {
    if (n <= cap) return;
    std::unique_lock<std::mutex> lk(g_grow_mu, std::defer_lock);
    if (!grow_unlocked()) lk.lock();
    const size_t c = std::max<size_t>(n, cap * 2);
    if (st && sync_grow()) {
      HIPCHK(hipDeviceSynchronize());
      if (p) HIPCHK(hipFree(p));
      p = nullptr;
      HIPCHK(hipMalloc((void**)&p, c * sizeof(T)));
      if (poison_buffers()) HIPCHK(hipMemset(p, 0xA5, c * sizeof(T)));
      HIPCHK(hipDeviceSynchronize());
      tl_async_grow++;
    } else if (st) {
      // the outgrown block is kept until the buffer is released instead of going back to the stream-ordered pool at
      // once (BLSGPU_GROW_FREE=1: freed at once, as before): with the adaptive group sizes, whose buffer shapes change
      // over a fresh process's first runs, the kept per-set Miller values (run_plan.hpp Forms::keep_f) were found
      // overwritten in ~6% of fresh C5 processes.  Growth doubles, so the kept blocks add up to less
      // than the buffer.
      if (p && grow_free()) HIPCHK(hipFreeAsync(p, st));
      else if (p) retired.push_back(p);
      p = nullptr;
      HIPCHK(hipMallocAsync((void**)&p, c * sizeof(T), st));
      if (poison_buffers()) HIPCHK(hipMemsetAsync(p, 0xA5, c * sizeof(T), st));
      tl_async_grow++;
    } else {
      if (p) HIPCHK(hipFree(p));
      p = nullptr;
      HIPCHK(hipMalloc((void**)&p, c * sizeof(T)));
      if (poison_buffers()) {  // the fill is on the null stream: complete it before any stream uses the buffer
        HIPCHK(hipMemset(p, 0xA5, c * sizeof(T)));
        HIPCHK(hipStreamSynchronize(nullptr));
      }
    }
    cap = c;
  }
  void release() {
    std::unique_lock<std::mutex> lk(g_grow_mu, std::defer_lock);
    if (!grow_unlocked()) lk.lock();
    if (p) (void)(st ? hipFreeAsync(p, st) : hipFree(p));
    for (T* q : retired) (void)(st ? hipFreeAsync(q, st) : hipFree(q));
    retired.clear();
    p = nullptr;
    cap = 0;
  }
};

template <class T>
struct HostBuf {  // pinned staging
  T* p = nullptr;
  size_t cap = 0;
  void ensure(size_t n) {
    if (n <= cap) return;
    std::unique_lock<std::mutex> lk(g_grow_mu, std::defer_lock);
    if (!grow_unlocked()) lk.lock();
    if (p) HIPCHK(hipHostFree(p));
    p = nullptr;
    size_t c = std::max<size_t>(n, cap * 2);
    HIPCHK(hipHostMalloc((void**)&p, c * sizeof(T), hipHostMallocDefault));
    if (poison_buffers()) memset(p, 0x5A, c * sizeof(T));
    cap = c;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
};

constexpr int kStages = 8;
static_assert(kMillerLineWords == (size_t)MILLER_STEPS * W_LINE, "run_plan.hpp");

// One runtime slot: a dispatcher's staging and work buffers and its events.  The pipeline streams belong to the device
// (Device::st) and are shared by its slots; each slot adds its own fallback stream (Slot::fb).  Under HIP's default of
// 4 hardware queues a process's streams share queues (HIP deals streams over its queues), so a fallback stream may
// share a queue with a pipeline stream; CU-masked streams (urgent partition, create_streams) get queues of their own.
struct Slot {
  hipEvent_t join_in = nullptr, join_msg = nullptr, join_pk = nullptr, join_mask = nullptr, join_gsm = nullptr,
             join_dec = nullptr, join_msm = nullptr, join_rsig = nullptr, done = nullptr;  // no timing
  hipEvent_t ev[2 * (kStages + 2)] = {};  // profile: (start, end) per stage; pairs kStages, kStages + 1 = the
                                          // Miller lines, the groups' MillerLoop(-g1, S) (parts of stages 5, 7)
  // d_in / h_in: every per-call input packed into one arena (one H2D transfer); d_res / h_res: job errors +
  // group verdicts (one D2H transfer).
  DevBuf<uint8_t> d_in, d_res, d_bytes, d_ok, d_fbflags;
  DevBuf<uint32_t> d_work, d_lines, d_S, d_F, d_G, d_list, d_msmB, d_msmW, d_fb;
  DevBuf<uint32_t> d_fkeep;  // the batch pass's per-set Miller values, kept for the fallback (run_plan.hpp Forms::keep_f)
  DevBuf<uint32_t> d_fseg;   // step segments: the (segment, group) heads of the F tree before their fold (k_f_fold)
  DevBuf<uint32_t> d_parts;  // helper slot: what a split same-message call adds (helper_layout.hpp AwrParts)
  HostBuf<uint8_t> h_in, h_res, h_ok;
  HostBuf<uint32_t> h_list;
  // The slot's own stream for the fallback of its runs (lowest priority).  A failed group's checks used to run on the
  // run's signature stream, shared by every run of that stream pair: under load (C5, 1% invalid) a 3,424-check launch
  // held that stream 33-46 ms and the next runs' decodes and MSMs queued behind it (r05 trace).
  hipStream_t fb = nullptr;
  bool retire = false;     // set under the device queue lock: the dispatcher exits instead of taking work
  bool in_flight = false;  // the slot's run counts in Device::runs_inflight
  bool alone = false;      // no other run was in flight when the slot took its run
  bool urgent = false;     // the device's urgent-lane slot (BLSGPU_JOB_URGENT calls): its own streams (Device::ust)

  // the stream buffer growth is ordered on (hipFreeAsync / hipMallocAsync); the slot's previous work is complete
  // whenever it grows a buffer (its dispatcher waits for each run), so only this ordering matters
  void set_stream(hipStream_t st) {
    for (auto* b : {&d_in, &d_res, &d_bytes, &d_ok, &d_fbflags}) b->st = st;
    for (auto* b : {&d_work, &d_lines, &d_S, &d_F, &d_G, &d_list, &d_msmB, &d_msmW, &d_fb, &d_fkeep, &d_fseg, &d_parts}) b->st = st;
  }
  void release_all() {
    d_in.release(); d_res.release(); d_bytes.release(); d_ok.release(); d_fbflags.release();
    d_work.release(); d_lines.release(); d_S.release(); d_F.release(); d_list.release();
    d_msmB.release(); d_msmW.release(); d_fb.release(); d_G.release(); d_fkeep.release(); d_fseg.release(); d_parts.release();
    h_in.release(); h_res.release(); h_ok.release(); h_list.release();
  }
};

struct Call;
struct Task {
  Call* call;
  uint32_t shard;
};

// The device's pipeline streams, shared by its slots: one per branch of a run's DAG (pipeline.cpp
// enqueue_batch_pass).  Runs of different
// slots queue behind each other per branch, so the chip always has the next run's work while one run's tail drains.
enum { kSig = 0, kMsg = 1, kPk = 2, kTail = 3, kStreams = 4, kMaxPairs = 3 };
// streams created with the device's highest priority (bit k = stream k); see blsgpu_init
#ifndef BLSGPU_STREAM_PRIO
#define BLSGPU_STREAM_PRIO ((1 << kMsg) | (1 << kTail))
#endif
// Stream pairs (default): consecutive runs alternate between two (signature, message) stream pairs -- run parity p
// uses st[2p] for its signature, pubkey and tail branches and st[2p + 1] (high priority) for its message branch --
// so the message chains of the two runs in flight (pipeline_depth 2) overlap instead of queueing behind each other on
// one message stream, the serial chain that bounded throughput.  0: one stream per branch, shared by all runs.
#ifndef BLSGPU_STREAM_PAIRS
#define BLSGPU_STREAM_PAIRS 1
#endif


struct Device {
  int id = 0;
  hipStream_t table_stream = nullptr;  // uploads and the synchronous helpers (debug, aggregate, ...)
  hipStream_t st[2 * kMaxPairs] = {};
  int npairs = 2;  // stream pairs in use: 3 when the process has >= 6 hardware queues (a pair per slot)
  std::mutex enq_mu;  // one run's batch (or fallback) launches are enqueued without another slot's in between
  std::mutex helper_mu;
  Slot helper;  // buffers of the synchronous helpers (on table_stream)
  // blsgpu_verify_same_message (under helper_mu): the streams of its key-sum and message branches and the events that
  // join them into table_stream, created by the first such call
  hipStream_t same_st[2] = {};
  hipEvent_t same_ev[3] = {};
  // pubkey table (AoS, W_PKTAB words per key): verification holds it shared, uploads exclusive
  std::shared_mutex table_mu;
  DevBuf<uint32_t> table;
  uint32_t table_n = 0;
  // committee store (used on device 0; blsgpu_committees_upload, helpers.cpp), under table_mu like the table: committee
  // c is cm_members[cm_first[c] .. cm_first[c + 1]) and cm_sums holds its members' sum (kernels.h CommitteeStore).
  // cm_first_host mirrors cm_first ([cm_n + 1], or empty).  A table upload that overwrites rows empties it.
  DevBuf<uint32_t> cm_first, cm_members, cm_sums;
  std::vector<uint32_t> cm_first_host;
  uint32_t cm_n = 0;
  // slots, each served by one dispatcher thread taking tasks from this device's queue
  std::mutex q_mu;
  std::condition_variable q_cv;
  std::deque<Task> queue;
  bool stop = false;
  std::vector<Slot*> slots;
  std::vector<std::thread> workers;
  int runs_inflight = 0;  // under q_mu: runs taken by a slot whose batch pass has not completed
  std::atomic<uint32_t> run_seq{0};  // run counter: the stream pair of a run (BLSGPU_STREAM_PAIRS)
  std::atomic<int64_t> load{0};  // cost (sets + pubkeys / 256, x256) of the shards queued or running here (routing)
  // Urgent lane (BLSGPU_JOB_URGENT, the reference's verifyOnMainThread): one slot with its own dispatcher and two stream
  // pairs, taking urgent calls from uqueue (under q_mu) one at a time.  It never counts in runs_inflight and never takes
  // enq_mu, so an urgent call waits for no throughput run on the host; on the device its streams either run on a
  // reserved CU partition that the pipeline streams are masked off (`urgent_cus` > 0) or at the highest priority.
  hipStream_t ust[4] = {};         // the urgent lane's streams, created by its dispatcher before its first run
  std::vector<uint32_t> umask;      // their CU mask (empty: plain streams of priority uprio)
  int uprio = 0;
  std::deque<Task> uqueue;
  Slot* uslot = nullptr;
  std::thread uworker;
  std::atomic<int> upending{0};  // urgent calls queued or running here (routing of urgent calls)
  // batch groups whose equation failed although every job of theirs verified on its own in the fallback -- zero unless a
  // kernel computed a group's equation wrong (read-only option `spurious_groups`; each one is also logged)
  std::atomic<uint64_t> spurious_groups{0};
  int urgent_cus = 0;            // CUs of the partition the streams were created with (0 = none)
  std::vector<uint32_t> main_mask;  // CU mask of the pipeline and fallback streams (empty = all CUs, priorities)
  bool blocking_sync = true;        // the dispatchers' wait events block instead of spinning (create_slot_events)
  std::mutex fail_mu;
  double fail_rate = 0;  // EWMA over this device's runs of the fraction of invalid sets (group_adapt)
};

inline double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// The call's scalar key and message-index hash key from its seed (batch_rand.hpp): seed 0 = 256 bits of OS
// entropy, else the comparison-run key of the seed.  false = no entropy: the call must fail (never a constant).
bool resolve_key(uint64_t seed, batch_rand::Key& key, uint64_t& hash_key);  // runtime.cpp

// pipeline.cpp: one shard of a call (or a merged batch) as one pipeline run on a slot, under the call's group policy
// (writes job_result[job_begin .. job_end)); and the run's leaving the device's in-flight count (once)
int run_call_shard(Device& d, Slot& sl, const blsgpu_batch& b, const Shard& sh, int8_t* job_result, uint64_t seed,
                   const Options& opt, uint32_t max_index, blsgpu_stats& st, const uint64_t* scal_words);
void release_inflight(Device& d, Slot& sl);

}  // namespace blsgpu_rt

struct blsgpu_ctx {
  std::vector<blsgpu_rt::Device*> devs;
  std::atomic<bool> closed{false};
  std::mutex active_mu;  // calls in progress (sync and async): destroy waits for zero
  std::condition_variable active_cv;
  int active = 0;
  std::mutex table_mu;  // serializes uploads
  std::mutex opt_mu;
  blsgpu_rt::Options opt;
  int64_t slots_per_device = 2;  // set at init from the hardware queues (default_slots)
  int64_t hw_queues = 4;
  std::mutex slots_mu;  // slot creation / resizing
  bool slots_started = false;
  std::atomic<uint32_t> route_seq{0};  // rotating tie-break of route_rule
  // urgent lane partition (set before the first call: the streams are created with it): CUs per device reserved for
  // the urgent streams, a multiple of 8; with urgent_isolate the pipeline streams are masked off them
  int64_t urgent_cus = 0;
  int64_t urgent_isolate = 1;  // (no effect without a partition)
  int64_t blocking_sync = 1;   // dispatchers block on their runs' completion events instead of spinning
  int64_t pipeline_prio = 1;   // the pipeline's message and tail streams take the device's highest priority
};

namespace blsgpu_rt __attribute__((visibility("hidden"))) {
inline bool enter(blsgpu_ctx* ctx) {  // register a call in progress unless the context is closing
  std::lock_guard<std::mutex> lk(ctx->active_mu);
  if (ctx->closed) return false;
  ctx->active++;
  return true;
}
inline void leave(blsgpu_ctx* ctx) {
  {
    std::lock_guard<std::mutex> lk(ctx->active_mu);
    ctx->active--;
  }
  ctx->active_cv.notify_all();
}
}  // namespace blsgpu_rt
