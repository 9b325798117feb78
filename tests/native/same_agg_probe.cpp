// Host probe of hl::SameAgg (lodestar_amd/csrc/helper_layout.hpp; tests/test_same_message_agg_host.py): writes every
// field of the struct, in declaration order, to out[] and returns the field count.  With -DSAME_AGG_PROBE_MAIN it is a
// program that walks a few shapes (for a sanitizer build on the host).
#include "../../lodestar_amd/csrc/helper_layout.hpp"

#include <string.h>

namespace hl = helper_layout;

extern "C" int probe_same_agg(uint64_t G, uint64_t n, uint64_t out_len, uint64_t* out) {
  const hl::SameAgg l(G, n, out_len);
  static_assert(sizeof l % sizeof(size_t) == 0 && sizeof(size_t) == sizeof(uint64_t), "size_t fields only");
  memcpy(out, &l, sizeof l);
  return (int)(sizeof l / sizeof(uint64_t));
}

#ifdef SAME_AGG_PROBE_MAIN
#include <initializer_list>
#include <stdio.h>
int main() {
  uint64_t out[16], sum = 0;
  int fields = 0;
  for (uint64_t G : {0, 1, 2, 63, 1024, 1025, 1 << 20})
    for (uint64_t n : {0, 1, 255, 256, 257, 16384, 1 << 20})
      for (uint64_t out_len : {96, 192}) {
        fields += probe_same_agg(G, n, out_len, out);
        sum += out[4];
      }
  printf("%d fields, checksum %llu\n", fields, (unsigned long long)sum);
  return 0;
}
#endif
