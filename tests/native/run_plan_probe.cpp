// Host probe of lodestar_amd/csrc/run_plan.hpp (tests/test_run_plan.py, tests/test_gpu_run_plan.py): flat C functions
// that take a batch's arrays and option values, build the plan of one pipeline run (or its F tree, verdict sorting,
// fallback lists, pool groups) and hand every vector and number back by name.
// With -DRUN_PLAN_PROBE_MAIN it is a program that walks the tests' shapes (for a sanitizer build on the host).
#include "../../lodestar_amd/csrc/run_plan.hpp"

#include <map>
#include <string>

using namespace blsgpu_rt;

namespace {

// What a probe call computed: vectors and numbers by name (rp_vec, rp_num)
struct Handle {
  std::map<std::string, std::vector<uint32_t>> vec;
  std::map<std::string, double> num;
  RunPlan plan;  // rp_plan handles: what rp_classify, rp_fallback and rp_next_fail_rate read
};

void put_ftree(Handle& h, const FTree& t) {
  h.vec["f_rng"] = t.f_rng, h.vec["ftree"] = t.ftree, h.vec["f_level_end"] = t.f_level_end;
  h.num["n_fruns"] = t.n_fruns, h.num["f_k"] = t.f_k, h.num["n_franges"] = t.n_franges;
}

constexpr int kRows = sizeof kOptionRows / sizeof kOptionRows[0];

}  // namespace

extern "C" {

void* rp_options_new() { return new Options(); }
// any row of the options table by name (options.hpp), the raw value with no range check
int rp_option(void* o, const char* key, int64_t v) {
  const OptionRow* r = find_option(key, false);
  if (r) static_cast<Options*>(o)->*r->member = v;
  return r ? 0 : -1;
}
// as blsgpu_set_option stores it: -1 = refused (no such ABI key, or the value is out of range), nothing changed
int rp_option_checked(void* o, const char* key, int64_t v) {
  const OptionRow* r = find_option(key, true);
  return r && store_option(*static_cast<Options*>(o), *r, v) ? 0 : -1;
}
int rp_option_get(const void* o, const char* key, int64_t* v) {
  const OptionRow* r = find_option(key, false);
  if (r) *v = static_cast<const Options*>(o)->*r->member;
  return r ? 0 : -1;
}
int rp_options_same_run(const void* a, const void* b) {
  return static_cast<const Options*>(a)->same_run(*static_cast<const Options*>(b));
}
void rp_options_free(void* o) { delete static_cast<Options*>(o); }
// the table's rows, i = 0, 1, ...: the key (null past the last row), whether it is an ABI key, whether it takes part
// in same_run, its default
const char* rp_option_key(int i) { return i >= 0 && i < kRows ? kOptionRows[i].key : nullptr; }
int rp_option_abi(int i) { return kOptionRows[i].abi; }
int rp_option_same_run(int i) { return kOptionRows[i].run; }
int64_t rp_option_default(int i) { return Options().*kOptionRows[i].member; }
// the keys outside the table, space-separated: those that live on the context (read_only 0), the read-only ones (1)
const char* rp_extra_keys(int read_only) {
  static std::string out[2];
  std::string& s = out[read_only != 0];
  s.clear();
  for (int i = read_only ? kCtxKeysSettable : 0; i < (read_only ? (int)CtxKey::none : kCtxKeysSettable); i++)
    s += std::string(s.empty() ? "" : " ") + kCtxKeys[i];
  return s.c_str();
}

uint32_t rp_vec(void* h, const char* name, uint32_t* out, uint32_t cap) {
  const auto& m = static_cast<Handle*>(h)->vec;
  const auto it = m.find(name);
  if (it == m.end()) return UINT32_MAX;
  for (size_t i = 0; i < it->second.size() && i < cap; i++) out[i] = it->second[i];
  return (uint32_t)it->second.size();
}
int rp_num(void* h, const char* name, double* out) {
  const auto& m = static_cast<Handle*>(h)->num;
  const auto it = m.find(name);
  if (it == m.end()) return -1;
  *out = it->second;
  return 0;
}
void rp_free(void* h) { delete static_cast<Handle*>(h); }

// The plan of jobs [job_begin, job_end) of a batch.  pk_mode: 0 table, 1 one key per set, 2 bytes aggregate (the key
// arrays themselves are never read by the plan: any non-null pointer stands for them).  pool: n_pool (first, end,
// batchable) triples, or null.  The caller keeps job_first_set alive as long as the handle.
void* rp_plan(const uint32_t* job_first_set, const uint8_t* job_flags, uint32_t job_begin, uint32_t job_end,
              const uint8_t* msgs, const uint32_t* sig_len, const uint32_t* set_pk_first, int pk_mode, const void* opt,
              int urgent, int alone, double fail_rate, uint64_t seed, const uint32_t* pool, uint32_t n_pool) {
  static const uint8_t some_keys[1] = {0};
  static const uint32_t some_index[1] = {0};
  blsgpu_batch b{};
  b.n_jobs = job_end, b.n_sets = job_first_set[job_end];
  b.job_first_set = job_first_set, b.job_flags = job_flags, b.msgs = msgs, b.sig_len = sig_len;
  b.pk_bytes = pk_mode ? some_keys : nullptr;
  b.set_pk_first = pk_mode == 1 ? nullptr : set_pk_first;
  b.pk_index = pk_mode == 0 ? some_index : nullptr;
  const Shard sh{job_begin, job_end, job_first_set[job_begin], job_first_set[job_end]};
  RunEnv env;
  env.urgent = urgent != 0, env.alone = alone != 0, env.fail_rate = fail_rate;
  std::vector<GroupPlanEntry> groups;
  for (uint32_t g = 0; g < n_pool; g++) groups.push_back({pool[3 * g], pool[3 * g + 1], pool[3 * g + 2] != 0});
  Handle* h = new Handle();
  h->plan = plan_run(b, sh, *static_cast<const Options*>(opt), env, seed, pool ? &groups : nullptr);
  const RunPlan& p = h->plan;
  auto& v = h->vec;
  auto& x = h->num;
  for (const auto& g : p.group_jobs) v["group_jobs"].push_back(g.first), v["group_jobs"].push_back(g.second);
  v["group_batchable"].assign(p.group_batchable.begin(), p.group_batchable.end());
  v["msg_idx"] = p.msg_idx, v["uniq"] = p.uniq, v["unit_of_set"] = p.unit_of_set, v["unit_msg"] = p.unit_msg;
  v["unit_first"] = p.unit_first, v["unit_sets"] = p.unit_sets, v["g_unit_first"] = p.g_unit_first;
  v["chunk_first"] = p.chunk_first, v["chunk_items"] = p.chunk_items, v["g_chunks"] = p.g_chunks;
  v["slices"] = p.slices, v["range_slices"] = p.range_slices, v["agg_sets"] = p.agg_sets;
  v["seg_first"].assign(p.segments.first, p.segments.first + p.segments.n + 1);
  put_ftree(*h, p.ft);
  x["n"] = p.n, x["nj"] = p.nj, x["stride"] = p.stride, x["ng0"] = p.ng0, x["n_umsg"] = p.n_umsg, x["nm"] = p.nm;
  x["merged"] = p.merged, x["n_units"] = p.n_units, x["n_items"] = p.n_items, x["n_chunks"] = p.n_chunks;
  x["n_slices"] = p.n_slices, x["sig_w"] = p.sig_w, x["npk"] = p.npk, x["pk_base"] = p.pk_base;
  const Forms& f = p.f;
  x["coop"] = f.coop, x["coop_g2"] = f.coop_g2, x["excl"] = f.excl, x["small"] = f.small, x["spec"] = f.spec;
  x["rsig_spec"] = f.rsig_spec, x["keep_f"] = f.keep_f, x["lane_tail"] = f.lane_tail, x["interleave"] = f.interleave;
  x["seg_plan"] = f.seg_plan, x["mk"] = f.mk, x["mk_whole"] = f.mk_whole, x["segs"] = f.segs;
  x["slice_len"] = f.slice_len, x["msm_tree"] = f.msm_tree;
  const InArena& a = p.in;
  const size_t in[] = {a.scal, a.jobs, a.sigs, a.siglen, a.umsg, a.midx, a.ranges, a.franges, a.ufirst, a.usets,
                       a.umsgi, a.cfirst, a.citems, a.agg, a.slices, a.rslices, a.ftree, a.pk_first, a.pk_keys,
                       a.bytes};
  const char* in_names[] = {"scal", "jobs", "sigs", "siglen", "umsg", "midx", "ranges", "franges", "ufirst", "usets",
                            "umsgi", "cfirst", "citems", "agg", "slices", "rslices", "ftree", "pk_first", "pk_keys",
                            "bytes"};
  for (size_t i = 0; i < sizeof in / sizeof in[0]; i++) x[std::string("in.") + in_names[i]] = (double)in[i];
  x["by.flags"] = p.by.flags, x["by.mflags"] = p.by.mflags, x["by.unit_ok"] = p.by.unit_ok;
  x["by.status"] = p.by.status, x["by.include"] = p.by.include, x["by.spec"] = p.by.spec, x["by.total"] = p.by.total;
  x["res.job_err"] = p.res.job_err, x["res.ok"] = p.res.ok, x["res.bytes"] = p.res.bytes;
  x["res.max_ranges"] = p.res.max_ranges;
  const WorkArena& w = p.work;
  const size_t wk[] = {w.sig_aff, w.pk_jac, w.pk_aff, w.f_chunk, w.scal_tab, w.unit_p, w.inv_buf, w.inv_buf_pk, w.h_aff,
                       w.h_jac, w.h_norm, w.h_prep, w.h_q, w.words};
  const char* wk_names[] = {"sig_aff", "pk_jac", "pk_aff", "f_chunk", "scal_tab", "unit_p", "inv_buf", "inv_buf_pk",
                            "h_aff", "h_jac", "h_norm", "h_prep", "h_q", "words"};
  for (size_t i = 0; i < sizeof wk / sizeof wk[0]; i++) x[std::string("work.") + wk_names[i]] = (double)wk[i];
  x["S_words"] = p.S_words(), x["F_words"] = p.F_words(), x["G_words"] = p.G_words();
  x["msmB_words"] = p.msmB_words(), x["msmW_words"] = p.msmW_words(), x["lines_words"] = p.lines_words();
  x["fkeep_words"] = p.fkeep_words(), x["fseg_words"] = p.fseg_words(), x["fb_words"] = p.fb_words();
  return h;
}

void* rp_ftree(const uint32_t* g_chunks, uint32_t ng, uint32_t n_chunks, uint32_t segs, int64_t f_run_max) {
  Handle* h = new Handle();
  put_ftree(*h, plan_f_tree(g_chunks, ng, n_chunks, segs, f_run_max));
  return h;
}

// job_err: nj codes; group_ok: ng0 verdicts.  The handle has jr, retry, failed_g, batch_retries and
// batch_sigs_success; jr goes out biased by 256 (the vectors are unsigned, an error code e is -e in jr).
void* rp_classify(void* plan, const int8_t* job_err, const uint8_t* group_ok, int spec) {
  const Classified c = classify_groups(static_cast<Handle*>(plan)->plan, job_err, group_ok, spec != 0);
  Handle* h = new Handle();
  for (int r : c.jr) h->vec["jr"].push_back((uint32_t)(r + 256));
  h->vec["retry"] = c.retry, h->vec["failed_g"] = c.failed_g;
  h->num["batch_retries"] = c.batch_retries, h->num["batch_sigs_success"] = c.batch_sigs_success;
  return h;
}

double rp_next_fail_rate(void* plan, const int32_t* jr, double rate) {
  const RunPlan& p = static_cast<Handle*>(plan)->plan;
  return next_fail_rate(p, std::vector<int>(jr, jr + p.nj), rate);
}

void* rp_fallback(void* plan, const uint32_t* retry, uint32_t nr, const void* opt, int alone) {
  const FallbackPlan fp = plan_fallback(static_cast<Handle*>(plan)->plan, std::vector<uint32_t>(retry, retry + nr),
                                        *static_cast<const Options*>(opt), alone != 0);
  Handle* h = new Handle();
  auto& v = h->vec;
  auto& x = h->num;
  v["rr"] = fp.rr, v["rf"] = fp.rf, v["rfirst"] = fp.rfirst, v["ritems"] = fp.ritems, v["rsl"] = fp.rsl;
  v["rrs"] = fp.rrs, v["rset"] = fp.rset, v["subr"] = fp.subr;
  x["nr"] = fp.nr, x["small_jobs"] = fp.small_jobs, x["busy"] = fp.busy, x["direct"] = fp.direct, x["nsub"] = fp.nsub;
  x["nc"] = fp.nc, x["nrs"] = fp.nrs, x["o_rf"] = fp.o_rf, x["o_rfirst"] = fp.o_rfirst, x["o_ritems"] = fp.o_ritems;
  x["o_rsl"] = fp.o_rsl, x["o_rrs"] = fp.o_rrs, x["o_rset"] = fp.o_rset, x["o_sub"] = fp.o_sub, x["o_sel"] = fp.o_sel;
  x["words"] = fp.words, x["kFbSub"] = kFbSub, x["kFbLaneMin"] = kFbLaneMin, x["kFbDirectMax"] = kFbDirectMax;
  x["lane_checks_nr"] = fp.lane_checks(nr);
  return h;
}

// subs: (call, a, e, batchable) per sub-job; groups: (first, end, batchable) per group
void* rp_pool(const uint32_t* job_first_set, const uint8_t* job_flags, uint32_t job_begin, uint32_t job_end) {
  const PoolPlan pp = plan_pool_groups(job_first_set, job_flags, job_begin, job_end);
  Handle* h = new Handle();
  for (const PoolSub& s : pp.subs)
    for (uint32_t w : {s.call, s.a, s.e, (uint32_t)s.batchable}) h->vec["subs"].push_back(w);
  h->vec["order"] = pp.order;
  for (const GroupPlanEntry& g : pp.groups)
    for (uint32_t w : {g.first, g.end, (uint32_t)g.batchable}) h->vec["groups"].push_back(w);
  return h;
}

uint32_t rp_chunk_size(uint32_t len, uint32_t min_per_chunk) { return chunk_size(len, min_per_chunk); }
uint32_t rp_adapt_group_sets(double f, int64_t group_sets, double sets_per_job) {
  return adapt_group_sets(f, group_sets, sets_per_job);
}
uint32_t rp_miller_k_auto(uint32_t n_items) { return miller_k_auto(n_items); }
}

#ifdef RUN_PLAN_PROBE_MAIN
#include <stdio.h>
// A batch: jobs of the given set counts (the third not batchable), message of set i = its index modulo `distinct`.
struct Shape {
  std::vector<uint32_t> jfs{0}, sig_len, spf{0};
  std::vector<uint8_t> flags, msgs;
  Shape(const std::vector<uint32_t>& counts, uint32_t distinct, uint32_t keys_per_set = 1) {
    for (uint32_t c : counts) jfs.push_back(jfs.back() + c), flags.push_back(flags.size() == 2 ? 0 : 1);
    const uint32_t n = jfs.back();
    sig_len.assign(n, 96);
    msgs.assign((size_t)n * 32 + 32, 0);
    for (uint32_t i = 0; i < n; i++) {
      const uint32_t m = i % std::max(distinct, 1u);
      memcpy(&msgs[(size_t)i * 32], &m, 4);
      spf.push_back(spf.back() + keys_per_set);
    }
  }
  void* plan(const Options& o, int mode, bool alone, const uint32_t* pool = nullptr, uint32_t n_pool = 0) {
    return rp_plan(jfs.data(), flags.data(), 0, (uint32_t)flags.size(), msgs.data(), sig_len.data(), spf.data(), mode,
                   &o, 0, alone, 0.01, 7, pool, n_pool);
  }
};

int main() {
  double sum = 0, x = 0;
  int plans = 0;
  auto take = [&](void* h, const char* name) {
    if (rp_num(h, name, &x) == 0) sum += x;
  };
  const std::vector<std::vector<uint32_t>> counts = {
      {2, 0, 1, 3, 1, 2, 1}, {1}, {0, 0, 0}, {2000, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, std::vector<uint32_t>(40, 1)};
  for (const auto& cs : counts)
    for (uint32_t distinct : {1u, 3u, 1u << 20})
      for (int64_t gs : {1, 4, 1024})
        for (int64_t mk : {0, 1, 2, 4})
          for (int mode : {0, 1, 2}) {
            Options o;
            o.group_sets = gs, o.miller_k = mk, o.dedupe = distinct != 1 || gs != 4, o.group_adapt = mode == 1;
            o.miller_segments = mk == 4 ? 2 : 0, o.keep_f = mode != 2;
            Shape s(cs, distinct, mode == 1 ? 1 : 2);
            void* h = s.plan(o, mode, mk == 0);
            plans++;
            take(h, "in.bytes"), take(h, "work.words"), take(h, "n_chunks"), take(h, "f_k");
            // every job clean, every group failed: all non-empty jobs are retried
            Handle* hp = static_cast<Handle*>(h);
            std::vector<int8_t> err(hp->plan.nj, 0);
            std::vector<uint8_t> ok(hp->plan.ng0 + 1, 0);
            void* c = rp_classify(h, err.data(), ok.data(), mode == 0);
            const std::vector<uint32_t> retry = static_cast<Handle*>(c)->vec["retry"];
            std::vector<int32_t> jr(hp->plan.nj + 1, 0);
            if (hp->plan.ng0) sum += rp_next_fail_rate(h, jr.data(), 0.25);
            void* f = rp_fallback(h, retry.data(), (uint32_t)retry.size(), &o, mode == 2);
            take(f, "words"), take(f, "nsub");
            rp_free(f), rp_free(c), rp_free(h);
          }
  {  // a pool-policy list with a group of only empty jobs
    Options o;
    Shape s({2, 0, 1, 3, 1, 2, 1}, 3);
    const uint32_t pool[] = {0, 1, 1, 1, 2, 1, 2, 5, 1, 5, 7, 0};
    void* h = s.plan(o, 1, false, pool, 4);
    take(h, "ng0");
    rp_free(h), plans++;
  }
  for (int64_t f_run_max : {16, 32})
    for (uint32_t segs : {1u, 2u}) {  // the F tree across its 16,384-slot threshold
      const uint32_t lens[] = {9000, 1, 0, 7001, 37, 400};
      std::vector<uint32_t> gc;
      uint32_t at = 0;
      for (uint32_t l : lens) gc.push_back(at), gc.push_back(at += l);
      void* h = rp_ftree(gc.data(), 6, at, segs, f_run_max);
      take(h, "f_k"), take(h, "n_fruns");
      rp_free(h), plans++;
    }
  for (uint32_t nr : {31u, 32u, 33u, 641u}) {  // the fallback's sub-groups
    Options o;
    o.small_max = nr == 641 ? 4096 : 0;
    Shape s(std::vector<uint32_t>(nr, 1), 1u << 20);
    void* h = s.plan(o, 1, true);
    std::vector<uint32_t> retry(nr);
    for (uint32_t q = 0; q < nr; q++) retry[q] = q;
    void* f = rp_fallback(h, retry.data(), nr, &o, 1);
    take(f, "nsub"), take(f, "words");
    rp_free(f), rp_free(h), plans++;
  }
  {
    const uint32_t jfs[] = {0, 0, 1, 128, 256, 385, 685};
    const uint8_t flags[] = {1, 1, 0, 1, 1, 0};
    void* h = rp_pool(jfs, flags, 0, 6);
    uint32_t out[4];
    sum += rp_vec(h, "order", out, 4) + rp_chunk_size(300, 128) + rp_adapt_group_sets(0.01, 1024, 2.0);
    rp_free(h), plans++;
  }
  printf("%d plans, checksum %.0f\n", plans, sum);
  return 0;
}
#endif
