// Rows of the trusted pubkey table (kernels.h W_PKTAB, k_common.hpp ld_pktab) built from and turned back into the ZCash
// encodings: the text k_pk_table_fill48 and k_pk_table_read (k_pk.hip) run per lane, and tests/native/pk_ingest_probe.cpp
// compiles for the host.  A row is PK_ROW_WORDS words: the Montgomery limbs of x, those of y, four zero pad words.
#pragma once
#include "ops.hpp"

#define PK_ROW_WORDS 32
static_assert(2 * BLS_NL + 4 == PK_ROW_WORDS, "x limbs | y limbs | four pad words");

// 48 compressed bytes -> status and row.  Checked in this order: BAD_ENCODING, POINT_NOT_ON_CURVE, PK_IS_INFINITY and,
// with `validate` (KeyValidate: the key is untrusted), POINT_NOT_IN_GROUP -- the rules of pk_decode48 / pk_key_validate.
// Without it an on-curve point outside G1 is stored, as the 96-byte upload stores one (pubkeyCache.ts:56-77 skips the
// subgroup check for keys already in the state).  A rejected key leaves an all-zero row.  `validate` is a template
// argument so that the trusted form holds no [z^2]P chain.
template <bool validate>
BLS_HDNI int pk_row_from48(const uint8_t* b, uint32_t* row) {
  g1a a;
  bool inf = false;
  int st = pk_decode48(b, a, inf);
  if (st == BLS_OK && inf) st = BLS_PK_IS_INFINITY;
  if (validate) {
    if (st == BLS_OK && !g1_in_subgroup(a)) st = BLS_POINT_NOT_IN_GROUP;
  }
  const bool ok = st == BLS_OK;
#pragma unroll
  for (int l = 0; l < BLS_NL; l++) {
    row[l] = ok ? a.x.l[l] : 0;
    row[BLS_NL + l] = ok ? a.y.l[l] : 0;
  }
#pragma unroll
  for (int l = 2 * BLS_NL; l < PK_ROW_WORDS; l++) row[l] = 0;
  return st;
}

// an affine table point -> 96 bytes (big-endian x || y) or 48 (compressed)
BLS_HD void pk_point_to_bytes(const g1a& a, uint32_t out_len, uint8_t* out) {
  if (out_len == 48)
    g1a_compress(a, out);
  else
    g1a_to_be96(a, out);
}

// row -> 96 / 48 bytes
BLS_HD void pk_row_to_bytes(const uint32_t* row, uint32_t out_len, uint8_t* out) {
  g1a a;
#pragma unroll
  for (int l = 0; l < BLS_NL; l++) {
    a.x.l[l] = row[l];
    a.y.l[l] = row[BLS_NL + l];
  }
  pk_point_to_bytes(a, out_len, out);
}
