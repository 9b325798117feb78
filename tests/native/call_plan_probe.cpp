// Host probe of lodestar_amd/csrc/call_plan.hpp (tests/test_call_plan.py): flat C functions that take calls as
// blsgpu_batch structs, pack shards of them into the batch of a merged run and hand the merged arrays back by name,
// scatter a run's results, and expose the call-side rules (validate_batch, max_table_index, table_covers,
// shard_scalars).  With -DCALL_PLAN_PROBE_MAIN it is a program that walks the tests' shapes (for a sanitizer build on
// the host).
#include "../../lodestar_amd/csrc/call_plan.hpp"

#include <deque>
#include <string>

using namespace blsgpu_rt;

namespace {

// The parts of a merged run and, once packed, its batch.  (Deques: CallPart holds references.)
struct Handle {
  std::deque<blsgpu_batch> batches;
  std::deque<Shard> shards;
  std::deque<batch_rand::Key> keys;
  std::vector<CallPart> parts;
  MergedBatch* m = nullptr;
  ~Handle() { delete m; }
};

Shard shard_of(const blsgpu_batch& b, uint32_t job_begin, uint32_t job_end) {
  return Shard{job_begin, job_end, b.job_first_set[job_begin], b.job_first_set[job_end]};
}

}  // namespace

extern "C" {

void* cp_new() { return new Handle(); }
void cp_free(void* h) { delete static_cast<Handle*>(h); }

// A part: jobs [job_begin, job_end) of the call *b (its arrays stay the caller's), scalars keyed by b->seed, results
// into job_result (the call's array, b->n_jobs long).
void cp_add(void* hv, const blsgpu_batch* b, uint32_t job_begin, uint32_t job_end, int8_t* job_result) {
  Handle* h = static_cast<Handle*>(hv);
  h->batches.push_back(*b);
  h->shards.push_back(shard_of(*b, job_begin, job_end));
  h->keys.push_back(batch_rand::seed_key(b->seed));
  h->parts.push_back({h->batches.back(), h->shards.back(), h->keys.back(), job_result});
}

// thread_min_sets: parts of at least this many sets pack on their own threads (the runtime: 4,096)
void cp_pack(void* hv, uint32_t thread_min_sets) {
  Handle* h = static_cast<Handle*>(hv);
  delete h->m;
  h->m = new MergedBatch(h->parts, thread_min_sets);
}

// An array of the merged run by name, as bytes, read through the merged blsgpu_batch's own pointers (the scalar words
// and the parts' offsets from the MergedBatch).  Returns its length in bytes; UINT32_MAX: no such name;
// UINT32_MAX - 1: the batch's pointer is null.
uint32_t cp_bytes(void* hv, const char* name, uint8_t* out, uint32_t cap) {
  const MergedBatch& m = *static_cast<Handle*>(hv)->m;
  const blsgpu_batch& b = m.b;
  const std::string k(name);
  const void* p = nullptr;
  size_t len = 0;
  const uint32_t npk = b.set_pk_first ? b.set_pk_first[b.n_sets] : b.n_sets;
  if (k == "job_first_set") p = b.job_first_set, len = ((size_t)b.n_jobs + 1) * 4;
  else if (k == "job_flags") p = b.job_flags, len = b.n_jobs;
  else if (k == "sig_len") p = b.sig_len, len = (size_t)b.n_sets * 4;
  else if (k == "sigs") p = b.sigs, len = (size_t)b.n_sets * b.sig_stride;
  else if (k == "msgs") p = b.msgs, len = (size_t)b.n_sets * 32;
  else if (k == "set_pk_first") p = b.set_pk_first, len = ((size_t)b.n_sets + 1) * 4;
  else if (k == "pk_index") p = b.pk_index, len = (size_t)npk * 4;
  else if (k == "pk_bytes") p = b.pk_bytes, len = (size_t)npk * 96;
  else if (k == "scal") p = m.scal.data(), len = (size_t)m.n * 8;
  else if (k == "set_off") p = m.set_off.data(), len = m.set_off.size() * 4;
  else if (k == "job_off") p = m.job_off.data(), len = m.job_off.size() * 4;
  else if (k == "key_off") p = m.key_off.data(), len = m.key_off.size() * 4;
  else return UINT32_MAX;
  if (!p) return UINT32_MAX - 1;
  if (len) memcpy(out, p, std::min<size_t>(len, cap));
  return (uint32_t)len;
}
int64_t cp_num(void* hv, const char* name) {
  const MergedBatch& m = *static_cast<Handle*>(hv)->m;
  const std::string k(name);
  if (k == "n_sets") return m.b.n_sets;
  if (k == "n_jobs") return m.b.n_jobs;
  if (k == "sig_stride") return m.b.sig_stride;
  if (k == "mode") return pk_mode(m.b);
  if (k == "n") return m.n;
  if (k == "nj") return m.nj;
  if (k == "npk") return m.npk;
  return -1;
}

// res: the merged run's per-job results (nj of them)
void cp_scatter(void* hv, const int8_t* res) {
  Handle* h = static_cast<Handle*>(hv);
  scatter_results(*h->m, h->parts, res);
}

int cp_validate(const blsgpu_batch* b) { return validate_batch(b); }
uint32_t cp_max_table_index(const blsgpu_batch* b) { return max_table_index(b); }
int cp_table_covers(const blsgpu_batch* b, uint32_t job_begin, uint32_t job_end, uint32_t max_index, uint32_t table_n) {
  return table_covers(*b, shard_of(*b, job_begin, job_end), max_index, table_n);
}
// out: one word per set of jobs [job_begin, job_end)
void cp_shard_scalars(const blsgpu_batch* b, uint32_t job_begin, uint32_t job_end, uint64_t* out) {
  shard_scalars(*b, shard_of(*b, job_begin, job_end), batch_rand::seed_key(b->seed), out);
}
int64_t cp_shard_cost(const blsgpu_batch* b, uint32_t job_begin, uint32_t job_end) {
  return shard_cost(*b, shard_of(*b, job_begin, job_end));
}
}

#ifdef CALL_PLAN_PROBE_MAIN
#include <stdio.h>
// A call: jobs of the given set counts (the third not batchable), set i with 1 + i % 3 keys (one in mode 1), its
// signature 96 or 192 bytes long (or neither) in rows of `stride` bytes.
struct CallShape {
  std::vector<uint32_t> jfs{0}, sig_len, spf{0}, pki;
  std::vector<uint8_t> flags, msgs, sigs, pkb;
  std::vector<int8_t> result;
  blsgpu_batch b{};
  CallShape(const std::vector<uint32_t>& counts, int mode, uint32_t stride, uint64_t seed) {
    for (uint32_t c : counts) jfs.push_back(jfs.back() + c), flags.push_back(flags.size() == 2 ? 0 : 1);
    const uint32_t n = jfs.back();
    for (uint32_t i = 0; i < n; i++) {
      sig_len.push_back(stride >= 192 && i % 2 ? 192 : stride == 200 && i % 5 == 0 ? 100 : 96);
      spf.push_back(spf.back() + (mode == 1 ? 1 : i % 3));
    }
    const uint32_t npk = mode == 1 ? n : spf.back();
    msgs.assign((size_t)n * 32 + 1, 3), sigs.assign((size_t)n * stride + 1, 5), pkb.assign((size_t)npk * 96 + 1, 7);
    pki.assign(npk + 1, 11);
    result.assign(counts.size() + 1, 99);
    b.n_sets = n, b.n_jobs = (uint32_t)counts.size(), b.job_first_set = jfs.data(), b.job_flags = flags.data();
    b.pk_bytes = mode ? pkb.data() : nullptr, b.set_pk_first = mode == 1 ? nullptr : spf.data();
    b.pk_index = mode == 0 ? pki.data() : nullptr, b.msgs = msgs.data(), b.sigs = sigs.data();
    b.sig_len = sig_len.data(), b.sig_stride = stride, b.seed = seed;
  }
};

int main() {
  uint64_t sum = 0;
  int runs = 0;
  std::vector<uint8_t> out(1 << 22);
  const char* names[] = {"job_first_set", "job_flags", "sig_len", "sigs", "msgs", "set_pk_first", "pk_index",
                         "pk_bytes", "scal", "set_off", "job_off", "key_off"};
  for (int mode : {0, 1, 2})
    for (uint32_t stride : {96u, 192u, 200u})
      for (uint32_t big : {0u, 4096u}) {
        CallShape a({2, 0, 1, 2}, mode, stride, 1), b({1}, mode, 96, 2), c({0, 3, 0, 4, 0}, mode, stride, 3);
        CallShape d({3, 2, 0, 1}, mode, 192, 4), e({big, 1}, mode, stride, 5);
        if (cp_validate(&a.b) || cp_validate(&b.b) || cp_validate(&c.b) || cp_validate(&d.b) || cp_validate(&e.b)) return 1;
        void* h = cp_new();
        cp_add(h, &a.b, 0, 4, a.result.data());
        cp_add(h, &b.b, 0, 1, b.result.data());
        cp_add(h, &c.b, 0, 5, c.result.data());
        cp_add(h, &d.b, 1, 3, d.result.data());  // a middle shard
        if (big) cp_add(h, &e.b, 0, 2, e.result.data());
        cp_add(h, &a.b, 1, 2, a.result.data());  // a shard with no sets
        for (uint32_t thread_min : {4096u, UINT32_MAX}) {
          cp_pack(h, thread_min);
          for (const char* nm : names) {
            const uint32_t len = cp_bytes(h, nm, out.data(), (uint32_t)out.size());
            if (len < UINT32_MAX - 1)
              for (uint32_t i = 0; i < len; i++) sum += out[i];
          }
          std::vector<int8_t> res((size_t)cp_num(h, "nj") + 1, 1);
          cp_scatter(h, res.data());
          sum += cp_max_table_index(&a.b) + cp_table_covers(&a.b, 0, 4, 11, 12) + cp_table_covers(&a.b, 1, 2, 11, 0);
          sum += (uint64_t)cp_shard_cost(&d.b, 1, 3);
          runs++;
        }
        cp_free(h);
      }
  {  // no parts, and refused batches
    void* h = cp_new();
    cp_pack(h, 4096);
    sum += (uint64_t)cp_num(h, "n");
    cp_free(h);
    CallShape a({2, 1}, 0, 96, 1);
    a.b.sig_stride = 95;
    sum += cp_validate(&a.b) + cp_validate(nullptr);
  }
  printf("%d merged runs, checksum %llu\n", runs, (unsigned long long)sum);
  return 0;
}
#endif
