// Host probe of lodestar_amd/csrc/same_plan.hpp and of the message dedupe the helper calls take from run_plan.hpp
// (tests/test_same_plan.py): HIP-free headers alone.  With -DSAME_PLAN_PROBE_MAIN it is a program that walks a few
// shapes (for a sanitizer build on the host).
#include "../../lodestar_amd/csrc/aggverify_plan.hpp"
#include "../../lodestar_amd/csrc/run_plan.hpp"
#include "../../lodestar_amd/csrc/same_plan.hpp"

namespace sp = same_plan;

extern "C" {

uint32_t probe_form(uint32_t n_items, uint32_t flags) { return sp::form(n_items, flags); }
uint32_t probe_blocks(uint32_t n_groups, uint32_t flags) { return sp::blocks(n_groups, flags); }
// kCoopMax, kBlockGroups, the five stats.form bits, aggverify_plan's threshold
void probe_constants(uint32_t* out) {
  const uint32_t c[] = {sp::kCoopMax,    sp::kBlockGroups, sp::kFormGroupLane,   sp::kFormRetryLane,
                        sp::kFormBlocks, sp::kFormDescent, sp::kFormDescentLane, aggverify_plan::kCoopMax};
  for (size_t i = 0; i < sizeof c / sizeof c[0]; i++) out[i] = c[i];
}
// which 0: the same-message calls' key for a call's hash key, 1: blsgpu_aggregate_verify's constant
uint64_t probe_msg_key(int which, uint64_t hash_key) { return which ? aggverify_plan::kMsgKey : sp::msg_key(hash_key); }

// listed has room for n_groups entries; returns how many were written
uint32_t probe_descent_list(uint32_t n_groups, uint32_t n_blocks, const uint8_t* any, const uint8_t* ok,
                            const uint8_t* include, uint32_t* listed) {
  const std::vector<uint32_t> l = sp::descent_list(n_groups, n_blocks, any, ok, include);
  for (size_t i = 0; i < l.size(); i++) listed[i] = l[i];
  return (uint32_t)l.size();
}

// sets and msg have room for group_first[n_groups] entries; counts = (groups_accepted, groups_retried); returns the
// number of listed sets
uint32_t probe_retry_list(const uint32_t* group_first, uint32_t n_groups, const int8_t* group_result,
                          const uint32_t* group_msg, uint32_t* sets, uint32_t* msg, uint32_t* counts) {
  const sp::Retry r = sp::retry_list(group_first, n_groups, group_result, group_msg);
  for (size_t i = 0; i < r.sets.size(); i++) sets[i] = r.sets[i], msg[i] = r.msg[i];
  counts[0] = r.groups_accepted, counts[1] = r.groups_retried;
  return r.sets.size() == r.msg.size() ? (uint32_t)r.sets.size() : 0xFFFFFFFFu;
}

// idx has room for n entries, uniq for n, packed for 32 n bytes (what unique_messages returns, whose indices must be
// dedupe_messages' own); returns the number of unique messages
uint32_t probe_dedupe(const uint8_t* msgs, uint32_t n, uint64_t key, uint32_t* idx, uint32_t* uniq, uint8_t* packed) {
  std::vector<uint32_t> i, u, i2;
  blsgpu_rt::dedupe_messages(msgs, n, key, i, u);
  const std::vector<uint8_t> p = blsgpu_rt::unique_messages(msgs, n, key, i2);
  if (i2 != i || p.size() != u.size() * 32) return 0xFFFFFFFFu;
  for (uint32_t k = 0; k < n; k++) idx[k] = i[k];
  for (size_t k = 0; k < u.size(); k++) uniq[k] = u[k];
  if (!p.empty()) memcpy(packed, p.data(), p.size());
  return (uint32_t)u.size();
}
}

#ifdef SAME_PLAN_PROBE_MAIN
#include <stdio.h>
int main() {
  uint64_t sum = 0;
  for (uint32_t G : {1u, 2u, 1024u, 1025u, 2050u, 4096u}) {
    const uint32_t NB = probe_blocks(G, BLSGPU_SAME_BLOCK_CHECK);
    std::vector<uint8_t> any(NB), ok(NB), inc(G);
    std::vector<uint32_t> listed(G);
    for (uint32_t pattern = 0; pattern < 6; pattern++) {
      for (uint32_t b = 0; b < NB; b++) any[b] = pattern != 4, ok[b] = (pattern + b) % 2;
      for (uint32_t g = 0; g < G; g++)
        inc[g] = pattern == 0 ? 1 : pattern == 1 ? 0 : pattern == 2 ? g % 1024 == 0 : pattern == 3 ? g % 7 == 0 : g % 2;
      sum += probe_descent_list(G, NB, any.data(), ok.data(), inc.data(), listed.data());
      sum += probe_form(G, pattern & 1) + probe_blocks(G, pattern);
    }
  }
  for (const std::vector<uint32_t>& sizes : {std::vector<uint32_t>{0, 3, 1, 0, 2}, {0, 0}, {1}, {5, 0, 0, 300}}) {
    const uint32_t G = (uint32_t)sizes.size();
    std::vector<uint32_t> gf(G + 1, 0), gmsg(G);
    for (uint32_t g = 0; g < G; g++) gf[g + 1] = gf[g] + sizes[g], gmsg[g] = g / 2;
    std::vector<uint32_t> sets(gf[G] + 1), msg(gf[G] + 1);
    uint32_t counts[2];
    for (int8_t v : {(int8_t)1, (int8_t)0, (int8_t)-3}) {
      std::vector<int8_t> res(G, v);
      if (G > 1) res[1] = 1;
      sum += probe_retry_list(gf.data(), G, res.data(), gmsg.data(), sets.data(), msg.data(), counts);
      sum += counts[0] + 3 * counts[1];
    }
  }
  for (uint32_t n : {0u, 1u, 15u, 16u, 17u, 40u, 1000u}) {
    std::vector<uint8_t> msgs((size_t)n * 32 + 1);
    for (uint32_t i = 0; i < n; i++) memset(msgs.data() + (size_t)i * 32, (int)(i * i % 11), 32);
    std::vector<uint32_t> idx(n + 1), uniq(n + 1);
    std::vector<uint8_t> packed((size_t)n * 32 + 1);
    for (int which : {0, 1})
      sum += probe_dedupe(msgs.data(), n, probe_msg_key(which, 12345), idx.data(), uniq.data(), packed.data());
  }
  printf("checksum %llu\n", (unsigned long long)sum);
  return 0;
}
#endif
