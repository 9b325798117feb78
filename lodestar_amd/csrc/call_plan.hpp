// Host plan of a call (runtime.cpp): everything a call decides before a pipeline run, as plain arithmetic on the batch's
// arrays -- the batch's validity, its largest table index, the sharding and routing rules, a shard's cost and batch
// scalars -- and the packing of several calls' shards into the one batch of a merged run (MergedBatch), with the way
// back for the results.  No HIP here: tests/native/call_plan_probe.cpp includes this header alone and
// tests/test_call_plan.py checks what the arrays mean.
#pragma once
#include <pthread.h>

#include <system_error>
#include <thread>

#include "batch_rand.hpp"
#include "run_plan.hpp"

namespace blsgpu_rt __attribute__((visibility("hidden"))) {

// ---- contiguous cost-balanced sharding (the rule lodestar_amd/shard.py restates) ------------------------
// cost of a job = its sets + 1/256 per aggregated pubkey; part k ends at the largest job boundary whose
// prefix cost is <= total (k+1)/n_parts; the last part takes the rest.
inline void shard_rule(const uint32_t* jfs, const uint32_t* spf, uint32_t n_jobs, uint32_t n_parts, uint32_t* out) {
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
inline uint32_t route_rule(uint32_t n_sets, uint32_t n_dev, const int64_t* load, int64_t split_sets, uint32_t start,
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

// routing cost of a shard, x256 (Device::load): its sets + 1/256 per pubkey
inline int64_t shard_cost(const blsgpu_batch& b, const Shard& sh) {
  int64_t c = 256 * (int64_t)(sh.set_end - sh.set_begin);
  if (b.set_pk_first) c += b.set_pk_first[sh.set_end] - b.set_pk_first[sh.set_begin];
  return c;
}

inline uint32_t max_table_index(const blsgpu_batch* b) {
  uint32_t m = 0;
  if (!b->pk_bytes && b->n_sets)
    for (uint32_t k = 0; k < b->set_pk_first[b->n_sets]; k++) m = std::max(m, b->pk_index[k]);
  return m;
}

inline int validate_batch(const blsgpu_batch* b) {
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

// Batch scalar words of a shard (shard-relative): single-set non-batchable jobs use r = 1 (word 0, CoreVerify,
// maybeBatch.ts:34-38), every other set i the call's keystream word i (batch_rand.hpp).
inline void shard_scalars(const blsgpu_batch& b, const Shard& sh, const batch_rand::Key& key, uint64_t* out) {
  if (sh.set_end > sh.set_begin) batch_rand::words(key, sh.set_begin, sh.set_end - sh.set_begin, out);
  for (uint32_t j = sh.job_begin; j < sh.job_end; j++) {
    const uint32_t a = b.job_first_set[j], e = b.job_first_set[j + 1];
    const bool batchable = b.job_flags && (b.job_flags[j] & 1u);
    if (!batchable && e - a == 1) out[a - sh.set_begin] = 0;
  }
}

// Does a table of table_n keys hold every index the call's shard uses?  max_index: the call's max_table_index.  (A
// shard with no sets, or with no keys, uses none.)
inline bool table_covers(const blsgpu_batch& b, const Shard& sh, uint32_t max_index, uint32_t table_n) {
  if (b.pk_bytes || !b.set_pk_first || sh.set_end == sh.set_begin) return true;
  if (b.set_pk_first[sh.set_end] == b.set_pk_first[sh.set_begin]) return true;
  return max_index < table_n;
}

// ---- merged runs: several calls' shards as one batch ---------------------------------------------------------------
// One call's part of a merged run: its batch, its shard, its scalar key, and where its job results go (the call's
// array: the shard's jobs are job_result[job_begin .. job_end)).
struct CallPart {
  const blsgpu_batch& b;
  const Shard& sh;
  const batch_rand::Key& key;
  int8_t* job_result;
};

// The parts' inputs concatenated into one batch `b` (jobs and sets in part order, every prefix array re-based), the
// batch scalar words of every part under its own key at the call's own set indices (shard_scalars), and the parts'
// offsets.  The parts share a pubkey mode (the first part's).  Signatures go out at sig_w = 96 bytes, or 192 as soon
// as any set of any part carries a 192-byte one; a signature of another length than 96 or 192 leaves its row zero.
struct MergedBatch {
  uint32_t n = 0, nj = 0, npk = 0, sig_w = 96;
  int mode = 0;
  std::vector<uint32_t> set_off, job_off, key_off;  // per part: where its sets, jobs and keys start
  std::vector<uint32_t> jfs, siglen, spf, pki;
  std::vector<uint8_t> flags, pkb, msgs, sigs;
  std::vector<uint64_t> scal;
  blsgpu_batch b{};  // points into the vectors

  // Parts of >= thread_min_sets sets pack on their own threads (a small part packs faster than a thread starts), the
  // first part and the others on the calling thread: the batch scalars (ChaCha20, ~0.4 ms per 16k-set call) and the
  // copies of a 131k-set run took ~2.5 ms on one thread.
  explicit MergedBatch(const std::vector<CallPart>& parts, uint32_t thread_min_sets = 4096) {
    if (parts.empty()) return;
    mode = pk_mode(parts[0].b);
    // the parts' offsets (sets, jobs, pubkeys) first, then every part packs into its own ranges
    for (const CallPart& p : parts) {
      set_off.push_back(n);
      job_off.push_back(nj);
      key_off.push_back(npk);
      n += p.sh.set_end - p.sh.set_begin;
      nj += p.sh.job_end - p.sh.job_begin;
      if (p.b.set_pk_first) npk += p.b.set_pk_first[p.sh.set_end] - p.b.set_pk_first[p.sh.set_begin];
      for (uint32_t i = p.sh.set_begin; i < p.sh.set_end && sig_w == 96; i++)
        if (p.b.sig_len[i] == 192) sig_w = 192;
    }
    using U32 = std::vector<uint32_t>;
    using U8 = std::vector<uint8_t>;
    jfs = U32(nj + 1), siglen = U32(n), spf = U32(mode == 1 ? 1 : n + 1), pki = U32(mode == 0 ? npk : 0);
    flags = U8(nj), pkb = U8(mode == 1 ? (size_t)n * 96 : mode == 2 ? (size_t)npk * 96 : 0);
    msgs = U8((size_t)n * 32), sigs = U8((size_t)n * sig_w, 0);
    scal = std::vector<uint64_t>(std::max<uint32_t>(n, 1));
    jfs[0] = 0;
    spf[0] = 0;
    {
      struct Joiner {  // joins the started threads on every exit, so none is destroyed while joinable
        std::vector<std::thread> th;
        ~Joiner() {
          for (auto& x : th)
            if (x.joinable()) x.join();
        }
      } j;
      std::vector<uint8_t> inline_pack(parts.size(), 0);
      for (size_t q = 0; q < parts.size(); q++) {
        inline_pack[q] = q == 0 || parts[q].sh.set_end - parts[q].sh.set_begin < thread_min_sets;
        if (inline_pack[q]) continue;
        try {
          j.th.emplace_back([this, &parts, q] {
            pthread_setname_np(pthread_self(), "blsgpu-pack");
            pack(parts[q], q);
          });
        } catch (std::system_error&) {  // no thread: this part packs on the current one
          inline_pack[q] = 1;
        }
      }
      for (size_t q = 0; q < parts.size(); q++)
        if (inline_pack[q]) pack(parts[q], q);
    }
    b.n_sets = n;
    b.n_jobs = nj;
    b.job_first_set = jfs.data();
    b.job_flags = flags.data();
    b.pk_bytes = mode ? pkb.data() : nullptr;
    b.set_pk_first = mode == 1 ? nullptr : spf.data();
    b.pk_index = mode == 0 ? pki.data() : nullptr;
    b.msgs = msgs.data();
    b.sigs = sigs.data();
    b.sig_len = siglen.data();
    b.sig_stride = sig_w;
  }
  MergedBatch(const MergedBatch&) = delete;  // (b points into this object's vectors)
  MergedBatch& operator=(const MergedBatch&) = delete;

 private:
  void pack(const CallPart& p, size_t q) {
    const Shard& sh = p.sh;
    const blsgpu_batch& c = p.b;
    const uint32_t so = set_off[q], jo = job_off[q], ko = key_off[q], ns = sh.set_end - sh.set_begin;
    shard_scalars(c, sh, p.key, scal.data() + so);
    for (uint32_t j = sh.job_begin; j < sh.job_end; j++) {
      jfs[jo + (j - sh.job_begin) + 1] = so + c.job_first_set[j + 1] - sh.set_begin;
      flags[jo + (j - sh.job_begin)] = c.job_flags ? c.job_flags[j] : 0;
    }
    if (!ns) return;  // (nothing more to copy, and a call without sets may leave its set arrays null)
    memcpy(siglen.data() + so, c.sig_len + sh.set_begin, (size_t)ns * 4);
    if (c.sig_stride == sig_w) {
      memcpy(sigs.data() + (size_t)so * sig_w, c.sigs + (size_t)sh.set_begin * sig_w, (size_t)ns * sig_w);
    } else {
      for (uint32_t i = sh.set_begin; i < sh.set_end; i++) {
        const uint32_t len = c.sig_len[i];
        if (len == 96 || len == 192)
          memcpy(sigs.data() + (size_t)(so + i - sh.set_begin) * sig_w, c.sigs + (size_t)i * c.sig_stride, len);
      }
    }
    memcpy(msgs.data() + (size_t)so * 32, c.msgs + (size_t)sh.set_begin * 32, (size_t)ns * 32);
    if (mode == 1) {
      memcpy(pkb.data() + (size_t)so * 96, c.pk_bytes + (size_t)sh.set_begin * 96, (size_t)ns * 96);
    } else {
      const uint32_t k0 = c.set_pk_first[sh.set_begin], k1 = c.set_pk_first[sh.set_end];
      for (uint32_t i = sh.set_begin; i < sh.set_end; i++)
        spf[so + (i - sh.set_begin) + 1] = ko + c.set_pk_first[i + 1] - k0;
      if (mode == 0)
        memcpy(pki.data() + ko, c.pk_index + k0, (size_t)(k1 - k0) * 4);
      else
        memcpy(pkb.data() + (size_t)ko * 96, c.pk_bytes + (size_t)k0 * 96, (size_t)(k1 - k0) * 96);
    }
  }
};

// The merged run's per-job results (m.nj of them, in part order) back into the parts' own job ranges.
inline void scatter_results(const MergedBatch& m, const std::vector<CallPart>& parts, const int8_t* res) {
  for (size_t q = 0; q < parts.size(); q++) {
    const Shard& sh = parts[q].sh;
    if (sh.job_end > sh.job_begin)
      memcpy(parts[q].job_result + sh.job_begin, res + m.job_off[q], sh.job_end - sh.job_begin);
  }
}

}  // namespace blsgpu_rt
