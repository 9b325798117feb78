// TEST HARNESS ONLY: host build of the pubkey-table row builder (lodestar_amd/csrc/pk_row.hpp, the text
// k_pk_table_fill48 and k_pk_table_read run per lane) and of hl::PubkeysRead (helper_layout.hpp), for
// tests/test_pubkeys_compressed_host.py.  With -DPK_INGEST_PROBE_MAIN it is a program that reads 48-byte keys from a file
// and runs both modes over them once (for a sanitizer build on the host).
#include <string.h>

#include "../../lodestar_amd/csrc/helper_layout.hpp"
#include "../../lodestar_amd/csrc/pk_row.hpp"

namespace hl = helper_layout;

// n keys at pk48[48 k] -> status[k], rows[PK_ROW_WORDS k] (words), out96[96 k] and out48[48 k] (both from the row).
// Returns the words per row.
extern "C" int probe_pk_ingest(const uint8_t* pk48, uint32_t n, int validate, int8_t* status, uint32_t* rows,
                               uint8_t* out96, uint8_t* out48) {
  for (uint32_t k = 0; k < n; k++) {
    uint32_t* row = rows + (size_t)k * PK_ROW_WORDS;
    const int st = validate ? pk_row_from48<true>(pk48 + 48 * (size_t)k, row)
                            : pk_row_from48<false>(pk48 + 48 * (size_t)k, row);
    status[k] = (int8_t)st;
    pk_row_to_bytes(row, 96, out96 + 96 * (size_t)k);
    pk_row_to_bytes(row, 48, out48 + 48 * (size_t)k);
  }
  return PK_ROW_WORDS;
}

// every field of hl::PubkeysRead, in declaration order; returns the field count
extern "C" int probe_pubkeys_read(uint64_t n, uint64_t out_len, uint64_t* out) {
  const hl::PubkeysRead l(n, out_len);
  static_assert(sizeof l % sizeof(size_t) == 0 && sizeof(size_t) == sizeof(uint64_t), "size_t fields only");
  memcpy(out, &l, sizeof l);
  return (int)(sizeof l / sizeof(uint64_t));
}

#ifdef PK_INGEST_PROBE_MAIN
#include <stdio.h>

#include <vector>
int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint8_t> keys;
  uint8_t buf[48];
  while (fread(buf, 1, 48, f) == 48) keys.insert(keys.end(), buf, buf + 48);
  fclose(f);
  const uint32_t n = (uint32_t)(keys.size() / 48);
  std::vector<int8_t> st(n);
  std::vector<uint32_t> rows((size_t)n * PK_ROW_WORDS);
  std::vector<uint8_t> o96((size_t)n * 96), o48((size_t)n * 48);
  for (int validate = 0; validate < 2; validate++) {
    probe_pk_ingest(keys.data(), n, validate, st.data(), rows.data(), o96.data(), o48.data());
    uint32_t accepted = 0;
    for (uint32_t k = 0; k < n; k++) accepted += st[k] == 0;
    printf("validate %d: %u of %u keys accepted\n", validate, accepted, n);
  }
  uint64_t fields[4];
  printf("%d layout fields\n", probe_pubkeys_read(n, 96, fields));
  return 0;
}
#endif
