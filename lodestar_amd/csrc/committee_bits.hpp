// One set of blsgpu_aggregate_pubkeys_bits: the share of the set's aggregated key that lane t of the
// set's L lanes sums, read from the participation bits themselves.  The text k_pk_bits (k_committee.hip) runs per lane,
// and tests/native/committee_bits_probe.cpp compiles for the host with the table and the stored sums in host arrays.
#pragma once
#include "ops.hpp"

// A stored committee sum is a row shaped like a pubkey-table row (pk_row.hpp): the Montgomery limbs of the affine x and
// y, then four pad words of which the first is COMMITTEE_SUM_IS_IDENTITY when the members' keys add up to the identity
// (x and y are then zero).
#define COMMITTEE_SUM_WORDS 32
#define COMMITTEE_SUM_IS_IDENTITY 1u
static_assert(2 * BLS_NL + 4 == COMMITTEE_SUM_WORDS, "x limbs | y limbs | flag word | three pad words");
// in a segment's descriptor (committee_plan.hpp kComplement): the segment is taken by complement
#define COMMITTEE_COMPLEMENT 0x80000000u

struct CommitteeBitsSet {
  const uint32_t* seg_desc;  // the set's segments: committee id, | COMMITTEE_COMPLEMENT
  uint32_t n_segs;
  const uint8_t* bits;  // the set's bit string: one bit per member of each segment's committee, in segment order
  uint32_t n_bytes;
  const uint32_t* committee_first;  // the store: committee c is members[committee_first[c] .. committee_first[c + 1])
  const uint32_t* members;          // table indices
};

// bits [pos, pos + 32) of the SSZ bit string s (bit i = s[i / 8] >> (i % 8) & 1); bits past its n_bytes bytes are 0
BLS_INL uint32_t committee_bits_word(const uint8_t* s, uint32_t n_bytes, uint32_t pos) {
  const uint32_t b = pos >> 3;
  uint64_t v = 0;
#pragma unroll
  for (uint32_t k = 0; k < 5; k++)
    if (b + k < n_bytes) v |= (uint64_t)s[b + k] << (8 * k);
  return (uint32_t)(v >> (pos & 7));
}

// Lane t of L.  The lanes stride over the 32-bit words of every segment's bits.  A direct segment adds the key of each
// set bit.  A complement segment subtracts the key of each clear bit (the word inverted, the key's y negated), and one
// lane of the set, k mod L for the set's k-th segment, adds the committee's stored sum as one more point of its walk.
// The lanes' values add up to the sum of the participants' keys.  point(stored, i, q): table row i, or with `stored`
// the sum of committee i, as the affine q; false when that sum is the identity.  Every addition goes through the
// complete jac_add_aff: equal points, opposite points and the identity all occur (a committee may repeat a key, an
// absent key may equal the stored sum).
template <class Point>
BLS_INL g1j committee_bits_lane_sum(const CommitteeBitsSet& a, uint32_t t, uint32_t L, Point point) {
  g1j acc = jac_infinity<fp>();
  uint32_t pos = 0;  // the segment's first bit in the set's string
  for (uint32_t k = 0; k < a.n_segs; k++) {
    const uint32_t d = a.seg_desc[k], id = d & ~COMMITTEE_COMPLEMENT;
    const bool complement = (d & COMMITTEE_COMPLEMENT) != 0;
    const uint32_t m0 = a.committee_first[id], size = a.committee_first[id + 1] - m0;
    bool sum_due = complement && k % L == t;
    uint32_t w = 32 * t, base = 0, v = 0;  // v: the bits still to walk of the word that starts at bit `base`
    for (;;) {
      while (v == 0 && w < size) {
        v = committee_bits_word(a.bits, a.n_bytes, pos + w);
        if (complement) v = ~v;
        if (size - w < 32) v &= (1u << (size - w)) - 1u;  // the segment's tail: the next segment's bits, or padding
        base = w;
        w += 32 * L;
      }
      g1a q;
      if (v) {
        const uint32_t i = (uint32_t)__builtin_ctz(v);
        v &= v - 1;
        point(false, a.members[m0 + base + i], q);
        if (complement) q.y = fp_neg(q.y);
      } else if (sum_due) {
        sum_due = false;
        if (!point(true, id, q)) continue;
      } else {
        break;
      }
      acc = jac_add_aff(acc, q);
    }
    pos += size;
  }
  return acc;
}
