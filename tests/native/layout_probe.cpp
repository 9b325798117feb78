// Host probe of lodestar_amd/csrc/helper_layout.hpp (tests/test_helper_layout.py): per helper call one function that
// writes the call's layout -- every field of its struct, in declaration order -- to out[] and returns the field count.
// With -DLAYOUT_PROBE_MAIN it is a program that walks the test's shapes (for a sanitizer build on the host).
#include "../../lodestar_amd/csrc/helper_layout.hpp"

#include <string.h>

namespace hl = helper_layout;

template <class L>
static int put(const L& l, uint64_t* out) {
  static_assert(sizeof(L) % sizeof(size_t) == 0 && sizeof(size_t) == sizeof(uint64_t), "size_t fields only");
  memcpy(out, &l, sizeof l);
  return (int)(sizeof l / sizeof(uint64_t));
}

extern "C" {
int probe_agg_pubkeys(uint64_t n, uint64_t npk, int bytes, uint64_t out_len, uint64_t* out) {
  return put(hl::AggPubkeys(n, npk, bytes != 0, out_len), out);
}
int probe_agg_sigs(uint64_t G, uint64_t n, uint64_t stride, uint64_t out_len, uint64_t* out) {
  return put(hl::AggSigs(G, n, stride, out_len), out);
}
int probe_awr(uint64_t G, uint64_t n, uint64_t stride, int bytes, uint64_t out_pk_len, uint64_t out_sig_len,
              uint64_t lanes, uint64_t* out) {
  return put(hl::Awr(G, n, stride, bytes != 0, out_pk_len, out_sig_len, lanes), out);
}
int probe_same(uint64_t G, uint64_t n, uint64_t U, uint64_t stride, int bytes, uint64_t lanes, uint64_t* out) {
  return put(hl::Same(G, n, U, stride, bytes != 0, lanes), out);
}
int probe_same_retry(uint64_t nr, uint64_t* out) { return put(hl::SameRetry(nr), out); }
int probe_key_validate(uint64_t n, uint64_t stride, uint64_t* out) { return put(hl::KeyValidate(n, stride), out); }
int probe_signing_roots(uint64_t n, uint64_t object_stride, uint64_t domain_stride, uint64_t* out) {
  return put(hl::SigningRoots(n, object_stride, domain_stride), out);
}
}

#ifdef LAYOUT_PROBE_MAIN
#include <initializer_list>
#include <stdio.h>
int main() {
  const uint64_t shapes[][2] = {{1, 0}, {1, 1}, {3, 5}, {4, 8}, {257, 300}};
  uint64_t out[64], sum = 0;
  int fields = 0;
  for (auto& sh : shapes)
    for (uint64_t stride : {96, 192})
      for (int bytes : {0, 1})
        for (uint64_t big : {0, 1}) {
          const uint64_t G = sh[0], n = sh[1];
          fields += probe_agg_pubkeys(G, n, bytes, big ? 96 : 48, out);
          fields += probe_agg_sigs(G, n, stride, big ? 192 : 96, out);
          fields += probe_awr(G, n, stride, bytes, big ? 96 : 48, big ? 192 : 96, 2 * G, out);
          fields += probe_same(G, n, big ? G : 1, stride, bytes, 2 * G, out);
          fields += probe_same_retry(n, out);
          fields += probe_key_validate(n, big ? 96 : 48, out);
          fields += probe_signing_roots(n, big ? 128 : 32, big ? 32 : 0, out);
          sum += out[0] + out[3];
        }
  printf("%d fields, checksum %llu\n", fields, (unsigned long long)sum);
  return 0;
}
#endif
