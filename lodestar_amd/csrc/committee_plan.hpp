// Host decisions of the committee store and of blsgpu_aggregate_pubkeys_bits (helpers.cpp): what an upload
// and a bits call are refused for, every segment's popcount and mode (sum the participants, or subtract the absent from
// the committee's stored sum), what the kernel will gather, and the lanes a set gets.  No HIP here:
// tests/native/committee_plan_probe.cpp includes this header alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace committee_plan {

constexpr uint32_t kMaxSets = 1u << 20, kMaxSegments = 1u << 22;
constexpr uint32_t kMaxUploadMembers = 1u << 20;   // members per upload call
constexpr uint32_t kMaxCommittees = 1u << 30;      // ids stay clear of kComplement
constexpr uint64_t kMaxCallBits = 1ull << 31;      // bits per call over all sets: every count of the call fits 32 bits
constexpr uint32_t kNoComplement = 1u;             // BLSGPU_BITS_NO_COMPLEMENT
constexpr uint32_t kComplement = 0x80000000u;      // in a segment's descriptor: taken by complement
constexpr int kOk = 0, kErrArgs = 100;             // BLSGPU_OK, BLSGPU_ERR_ARGS

// A segment of `size` members of which `present` participate: 1 = by complement (the stored sum minus the absent keys,
// absent + 1 additions) iff that is fewer additions than the `present` of summing the participants, else 0.
inline uint32_t mode(uint32_t size, uint32_t present, uint32_t flags) {
  if ((flags & kNoComplement) || present > size) return 0;
  return (uint64_t)(size - present) + 1 < present ? 1 : 0;
}

// Lanes per set of a call of n_sets sets whose kernel gathers n_items points in all (table rows and stored sums): the
// count rule of launch_pk_aggregate -- a wave per set while that leaves SIMDs idle, else the fewest lanes of 32, 16, 8
// that still give every SIMD a wave -- capped by the fewest lanes of 8, 16, 32, 64 that cover the mean items of a set (a
// lane without an item only lengthens the butterfly).  Non-increasing in n_sets for a given n_items.
inline uint32_t lanes(uint32_t n_sets, uint64_t n_items) {
  if (n_sets == 0) return 8;
  const uint64_t n = n_sets, chip = 1024 * 64;
  const uint32_t by_count = n * 64 <= chip ? 64 : n * 32 <= 2 * chip ? 32 : n * 16 <= 2 * chip ? 16 : 8;
  const uint64_t mean = (n_items + n - 1) / n;
  const uint32_t by_size = mean <= 8 ? 8 : mean <= 16 ? 16 : mean <= 32 ? 32 : 64;
  return by_count < by_size ? by_count : by_size;
}

// bits [pos, pos + 32) of the SSZ bit string s of n_bytes bytes (bit i = s[i / 8] >> (i % 8) & 1); bits past its end are 0
inline uint32_t word_at(const uint8_t* s, size_t n_bytes, uint64_t pos) {
  const size_t b = (size_t)(pos >> 3);
  uint64_t v = 0;
  for (size_t k = 0; k < 5 && b + k < n_bytes; k++) v |= (uint64_t)s[b + k] << (8 * k);
  return (uint32_t)(v >> (pos & 7));
}
// set bits among bits [pos, pos + count) of s
inline uint32_t popcount_range(const uint8_t* s, size_t n_bytes, uint64_t pos, uint32_t count) {
  uint32_t c = 0;
  for (uint32_t k = 0; k < count; k += 32) {
    uint32_t w = word_at(s, n_bytes, pos + k);
    if (count - k < 32) w &= (1u << (count - k)) - 1u;
    c += (uint32_t)__builtin_popcount(w);
  }
  return c;
}

// blsgpu_committees_upload: kOk, or kErrArgs with nothing to store.  `count` committees are stored, the table holds
// table_n keys.  (A null ctx is the caller's.)
inline int check_upload(uint32_t first_committee, uint32_t n, const uint32_t* committee_first, const uint32_t* members,
                        uint32_t count, uint32_t table_n) {
  if (first_committee > count) return kErrArgs;
  if (n == 0) return kOk;
  if (!committee_first || !members || (uint64_t)first_committee + n > kMaxCommittees) return kErrArgs;
  if (committee_first[0] != 0) return kErrArgs;
  for (uint32_t c = 0; c < n; c++)
    if (committee_first[c + 1] <= committee_first[c]) return kErrArgs;  // empty, or decreasing
  const uint32_t total = committee_first[n];
  if (total > kMaxUploadMembers) return kErrArgs;
  for (uint32_t k = 0; k < total; k++)
    if (members[k] >= table_n) return kErrArgs;
  return kOk;
}

// What blsgpu_committee_bits_stats reports, but for device_ms
struct Counts {
  uint32_t segments = 0, segments_complemented = 0, keys_present = 0, keys_added = 0, keys_subtracted = 0, lanes = 0;
};

struct Plan {
  std::vector<uint32_t> seg_desc;       // per segment: its committee, | kComplement when it is taken by complement
  std::vector<uint32_t> present_first;  // [n_sets + 1]: running count of set bits (a set's keys, as set_pk_first counts)
  uint32_t n_segs = 0;
  size_t bits_bytes = 0;  // set_bits_first[n_sets]
  uint64_t n_items = 0;   // points the kernel gathers: keys added + keys subtracted + stored sums
  Counts counts;
};

// The pointer, length and flag checks of blsgpu_aggregate_pubkeys_bits (n_sets > 0)
inline int check_call(uint32_t n_sets, const void* set_seg_first, const void* seg_committee, const void* set_bits_first,
                      const void* bits, uint32_t flags, const void* out, uint32_t out_len, const void* status) {
  if (!set_seg_first || !seg_committee || !set_bits_first || !bits || !out || !status) return kErrArgs;
  if ((out_len != 48 && out_len != 96) || (flags & ~kNoComplement) || n_sets > kMaxSets) return kErrArgs;
  return kOk;
}

// The call's plan from its arrays (checked by check_call) and the sizes of the stored committees: committee c has
// committee_first[c + 1] - committee_first[c] members, c < n_committees.  kErrArgs: offsets not non-decreasing from 0,
// more than kMaxSegments segments or kMaxCallBits bits, a committee id >= n_committees, a set whose bit string is not
// exactly ceil(bits / 8) bytes, a non-zero padding bit.
inline int make_plan(uint32_t n_sets, const uint32_t* set_seg_first, const uint32_t* seg_committee,
                     const uint32_t* set_bits_first, const uint8_t* bits, uint32_t flags,
                     const uint32_t* committee_first, uint32_t n_committees, Plan& p) {
  if (set_seg_first[0] != 0 || set_bits_first[0] != 0) return kErrArgs;
  for (uint32_t s = 0; s < n_sets; s++)
    if (set_seg_first[s + 1] < set_seg_first[s] || set_bits_first[s + 1] < set_bits_first[s]) return kErrArgs;
  p.n_segs = set_seg_first[n_sets];
  p.bits_bytes = set_bits_first[n_sets];
  if (p.n_segs > kMaxSegments || (uint64_t)p.bits_bytes * 8 > kMaxCallBits) return kErrArgs;
  for (uint32_t k = 0; k < p.n_segs; k++)
    if (seg_committee[k] >= n_committees) return kErrArgs;
  p.seg_desc.resize(p.n_segs);
  p.present_first.assign((size_t)n_sets + 1, 0);
  Counts c;
  c.segments = p.n_segs;
  uint64_t complemented_sums = 0;
  for (uint32_t s = 0; s < n_sets; s++) {
    const uint8_t* str = bits + set_bits_first[s];
    const size_t n_bytes = set_bits_first[s + 1] - set_bits_first[s];
    uint64_t pos = 0;
    uint32_t present_set = 0;
    for (uint32_t k = set_seg_first[s]; k < set_seg_first[s + 1]; k++) {
      const uint32_t id = seg_committee[k], size = committee_first[id + 1] - committee_first[id];
      if (pos + size > (uint64_t)n_bytes * 8) return kErrArgs;  // the string is too short
      const uint32_t present = popcount_range(str, n_bytes, pos, size);
      const uint32_t m = mode(size, present, flags);
      p.seg_desc[k] = id | (m ? kComplement : 0);
      if (m)
        c.segments_complemented++, c.keys_subtracted += size - present, complemented_sums++;
      else
        c.keys_added += present;
      present_set += present;
      pos += size;
    }
    if ((pos + 7) / 8 != n_bytes) return kErrArgs;  // the string is too long
    if (pos & 7)                                    // padding bits of the last byte
      if (str[n_bytes - 1] >> (pos & 7)) return kErrArgs;
    c.keys_present += present_set;
    p.present_first[s + 1] = c.keys_present;
  }
  p.n_items = (uint64_t)c.keys_added + c.keys_subtracted + complemented_sums;
  c.lanes = lanes(n_sets, p.n_items);
  p.counts = c;
  return kOk;
}

}  // namespace committee_plan
