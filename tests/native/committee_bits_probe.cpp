// TEST HARNESS ONLY: host build of the per-set core of blsgpu_aggregate_pubkeys_bits (lodestar_amd/csrc/
// committee_bits.hpp, the text k_pk_bits runs per lane) with the host plan (committee_plan.hpp) in front of it, for
// tests/test_committee_bits_host.py: the table, the committees and their stored sums live in host arrays, the L lanes
// of a set run one after another and are added up as the kernel's butterfly adds them, and the sum is encoded as
// k_pk_serialize encodes it.  With -DCOMMITTEE_BITS_PROBE_MAIN it is a program that reads 96-byte keys from a file
// and runs a fixed set of committees and bit patterns over them once (for a sanitizer build on the host).
#include <string.h>

#include <vector>

#include "../../lodestar_amd/csrc/committee_bits.hpp"
#include "../../lodestar_amd/csrc/committee_plan.hpp"
#include "../../lodestar_amd/csrc/pk_row.hpp"

namespace cmp = committee_plan;

static_assert(COMMITTEE_COMPLEMENT == cmp::kComplement && COMMITTEE_SUM_WORDS == PK_ROW_WORDS, "one descriptor, one row");

namespace {
struct Store {
  std::vector<uint32_t> table;  // PK_ROW_WORDS per key
  std::vector<uint32_t> sums;   // COMMITTEE_SUM_WORDS per committee
  const uint32_t* committee_first;
  const uint32_t* members;
};
bool ld_row(const uint32_t* row, g1a& q) {
  for (int l = 0; l < BLS_NL; l++) q.x.l[l] = row[l], q.y.l[l] = row[BLS_NL + l];
  return row[2 * BLS_NL] != COMMITTEE_SUM_IS_IDENTITY;
}
// the table from 96-byte keys (trusted, as blsgpu_pubkeys_upload) and every committee's stored row
int build(const uint8_t* pk96, uint32_t n_keys, uint32_t n_committees, const uint32_t* committee_first,
          const uint32_t* members, Store& st) {
  st.table.assign((size_t)n_keys * PK_ROW_WORDS, 0);
  for (uint32_t k = 0; k < n_keys; k++) {
    g1a a;
    bool inf = false;
    if (pk_decode96(pk96 + 96 * (size_t)k, a, inf) != BLS_OK || inf) return 1;
    for (int l = 0; l < BLS_NL; l++) st.table[(size_t)k * PK_ROW_WORDS + l] = a.x.l[l], st.table[(size_t)k * PK_ROW_WORDS + BLS_NL + l] = a.y.l[l];
  }
  st.sums.assign((size_t)n_committees * COMMITTEE_SUM_WORDS, 0);
  for (uint32_t c = 0; c < n_committees; c++) {
    g1j acc = jac_infinity<fp>();
    for (uint32_t k = committee_first[c]; k < committee_first[c + 1]; k++) {
      g1a q;
      ld_row(&st.table[(size_t)members[k] * PK_ROW_WORDS], q);
      acc = jac_add_aff(acc, q);
    }
    g1a a;
    uint32_t* row = &st.sums[(size_t)c * COMMITTEE_SUM_WORDS];
    if (jac_to_aff(acc, a))
      for (int l = 0; l < BLS_NL; l++) row[l] = a.x.l[l], row[BLS_NL + l] = a.y.l[l];
    else
      row[2 * BLS_NL] = COMMITTEE_SUM_IS_IDENTITY;
  }
  st.committee_first = committee_first;
  st.members = members;
  return 0;
}
}  // namespace

// One set on L lanes: segments seg_committee[0 .. n_segs) over the bit string `bits`, against a table of n_keys
// 96-byte keys and n_committees committees.  out[out_len] and the value are what blsgpu_aggregate_pubkeys_bits answers
// for the set (status 0 / EMPTY_AGGREGATE); complemented (nullable) receives the segments taken by complement.
// -1: the keys do not decode; -100: the plan refuses the call.
extern "C" int probe_committee_bits(const uint8_t* pk96, uint32_t n_keys, uint32_t n_committees,
                                    const uint32_t* committee_first, const uint32_t* members, uint32_t n_segs,
                                    const uint32_t* seg_committee, const uint8_t* bits, uint32_t n_bytes, uint32_t flags,
                                    uint32_t L, uint32_t out_len, uint8_t* out, uint32_t* complemented) {
  Store st;
  if (build(pk96, n_keys, n_committees, committee_first, members, st)) return -1;
  const uint32_t ssf[2] = {0, n_segs}, sbf[2] = {0, n_bytes};
  cmp::Plan p;
  if (cmp::make_plan(1, ssf, seg_committee, sbf, bits, flags, committee_first, n_committees, p)) return -100;
  if (complemented) *complemented = p.counts.segments_complemented;
  CommitteeBitsSet cs{p.seg_desc.data(), n_segs, bits, n_bytes, committee_first, members};
  std::vector<g1j> lane(L);
  for (uint32_t t = 0; t < L; t++)
    lane[t] = committee_bits_lane_sum(cs, t, L, [&](bool stored, uint32_t i, g1a& q) {
      return ld_row(stored ? &st.sums[(size_t)i * COMMITTEE_SUM_WORDS] : &st.table[(size_t)i * PK_ROW_WORDS], q);
    });
  for (uint32_t m = L / 2; m >= 1; m >>= 1)  // the butterfly's levels, as lane 0 sees them
    for (uint32_t t = 0; t < m; t++) lane[t] = jac_add(lane[t], lane[t + m]);
  memset(out, 0, out_len);
  if (p.present_first[1] == 0) return BLS_EMPTY_AGGREGATE;
  g1a a;
  if (!jac_to_aff(lane[0], a))
    out[0] = out_len == 48 ? 0xc0 : 0x40;
  else
    pk_point_to_bytes(a, out_len, out);
  return BLS_OK;
}

#ifdef COMMITTEE_BITS_PROBE_MAIN
#include <stdio.h>
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> keys;
  uint8_t buf[96];
  while (fread(buf, 1, 96, f) == 96) keys.insert(keys.end(), buf, buf + 96);
  fclose(f);
  const uint32_t n_keys = (uint32_t)(keys.size() / 96);
  if (n_keys < 70) return 2;
  // committees of 1, 2, 7, 8, 9, 33, 65 members (keys reused across them), a two-segment set over the last two
  const uint32_t sizes[] = {1, 2, 7, 8, 9, 33, 65};
  std::vector<uint32_t> first{0}, members;
  for (uint32_t s : sizes) {
    for (uint32_t k = 0; k < s; k++) members.push_back((k * 7 + s) % n_keys);
    first.push_back((uint32_t)members.size());
  }
  const uint32_t nc = (uint32_t)(sizeof sizes / sizeof sizes[0]);
  uint32_t sets = 0, complemented = 0, equal = 0;
  for (uint32_t c = 0; c < nc; c++)
    for (uint32_t pattern = 0; pattern < 4; pattern++) {
      const uint32_t two = c + 1 < nc && pattern == 3;
      const uint32_t seg[2] = {c, c + 1};
      const uint32_t n_bits = sizes[c] + (two ? sizes[c + 1] : 0), n_bytes = (n_bits + 7) / 8;
      std::vector<uint8_t> bits(n_bytes, 0);
      for (uint32_t i = 0; i < n_bits; i++) {
        const bool on = pattern == 0 ? true : pattern == 1 ? i != 0 : pattern == 2 ? i % 2 == 0 : i % 5 != 3;
        if (on) bits[i / 8] |= (uint8_t)(1u << (i % 8));
      }
      uint8_t a[96], b[96];
      uint32_t comp = 0, none = 0;
      const int ra = probe_committee_bits(keys.data(), n_keys, nc, first.data(), members.data(), two ? 2 : 1, seg,
                                          bits.data(), n_bytes, 0, 8, 96, a, &comp);
      const int rb = probe_committee_bits(keys.data(), n_keys, nc, first.data(), members.data(), two ? 2 : 1, seg,
                                          bits.data(), n_bytes, cmp::kNoComplement, 64, 96, b, &none);
      if (ra < 0 || rb < 0 || none != 0) return 1;
      sets++, complemented += comp, equal += ra == rb && memcmp(a, b, 96) == 0;
    }
  printf("%u sets, %u segments complemented, %u equal under the flag\n", sets, complemented, equal);
  return equal == sets ? 0 : 1;
}
#endif
