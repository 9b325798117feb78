// TEST HARNESS ONLY: host probe of lodestar_amd/csrc/committee_plan.hpp (the host decisions of the committee store and
// of blsgpu_aggregate_pubkeys_bits) and of hl::AggPubkeysBits (helper_layout.hpp), for tests/test_committee_bits_host.py.
// Neither header needs HIP.
#include <string.h>

#include "../../lodestar_amd/csrc/committee_plan.hpp"
#include "../../lodestar_amd/csrc/helper_layout.hpp"

namespace cmp = committee_plan;
namespace hl = helper_layout;

extern "C" {
uint32_t probe_mode(uint32_t size, uint32_t present, uint32_t flags) { return cmp::mode(size, present, flags); }
uint32_t probe_lanes(uint32_t n_sets, uint64_t n_items) { return cmp::lanes(n_sets, n_items); }
uint32_t probe_popcount(const uint8_t* s, uint64_t n_bytes, uint64_t pos, uint32_t count) {
  return cmp::popcount_range(s, n_bytes, pos, count);
}
int probe_check_upload(uint32_t first_committee, uint32_t n, const uint32_t* committee_first, const uint32_t* members,
                       uint32_t count, uint32_t table_n) {
  return cmp::check_upload(first_committee, n, committee_first, members, count, table_n);
}
int probe_check_call(uint32_t n_sets, const void* ssf, const void* seg, const void* sbf, const void* bits, uint32_t flags,
                     const void* out, uint32_t out_len, const void* status) {
  return cmp::check_call(n_sets, ssf, seg, sbf, bits, flags, out, out_len, status);
}
// The plan of one call.  counts[8]: segments, segments_complemented, keys_present, keys_added, keys_subtracted, lanes,
// n_items, bits_bytes; seg_desc[n_segs] and present_first[n_sets + 1] as the device receives them.  Returns the code.
int probe_plan(uint32_t n_sets, const uint32_t* ssf, const uint32_t* seg, const uint32_t* sbf, const uint8_t* bits,
               uint32_t flags, const uint32_t* committee_first, uint32_t n_committees, uint64_t* counts,
               uint32_t* seg_desc, uint32_t* present_first) {
  cmp::Plan p;
  const int rc = cmp::make_plan(n_sets, ssf, seg, sbf, bits, flags, committee_first, n_committees, p);
  if (rc) return rc;
  const cmp::Counts& c = p.counts;
  const uint64_t v[8] = {c.segments,        c.segments_complemented, c.keys_present, c.keys_added,
                         c.keys_subtracted, c.lanes,                 p.n_items,      p.bits_bytes};
  memcpy(counts, v, sizeof v);
  if (p.n_segs) memcpy(seg_desc, p.seg_desc.data(), (size_t)p.n_segs * 4);
  memcpy(present_first, p.present_first.data(), ((size_t)n_sets + 1) * 4);
  return 0;
}
// every field of hl::AggPubkeysBits, in declaration order; returns the field count
int probe_agg_pubkeys_bits(uint64_t n, uint64_t n_segs, uint64_t bits_bytes, uint64_t out_len, uint64_t* out) {
  const hl::AggPubkeysBits l(n, n_segs, bits_bytes, out_len);
  static_assert(sizeof l % sizeof(size_t) == 0 && sizeof(size_t) == sizeof(uint64_t), "size_t fields only");
  memcpy(out, &l, sizeof l);
  return (int)(sizeof l / sizeof(uint64_t));
}
}
