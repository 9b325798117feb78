// Host probe of hl::SameBlocks (lodestar_amd/csrc/helper_layout.hpp; tests/test_same_message_blocks_host.py): writes
// every field of the struct, in declaration order, to out[] and returns the field count.  With -DSAME_BLOCKS_PROBE_MAIN
// it is a program that walks a few shapes (for a sanitizer build on the host).
#include "../../lodestar_amd/csrc/helper_layout.hpp"

#include <string.h>

namespace hl = helper_layout;

extern "C" int probe_same_blocks(uint64_t nb, uint64_t width, uint64_t nl, uint64_t* out) {
  const hl::SameBlocks l(nb, width, nl);
  static_assert(sizeof l % sizeof(size_t) == 0 && sizeof(size_t) == sizeof(uint64_t), "size_t fields only");
  memcpy(out, &l, sizeof l);
  return (int)(sizeof l / sizeof(uint64_t));
}

#ifdef SAME_BLOCKS_PROBE_MAIN
#include <initializer_list>
#include <stdio.h>
int main() {
  uint64_t out[64], sum = 0;
  int fields = 0;
  for (uint64_t nb : {0, 1, 2, 3, 1024})
    for (uint64_t width : {1, 2, 64, 512})
      for (uint64_t nl : {0, 2, 513, 1024, 1 << 20}) {
        fields += probe_same_blocks(nb, width, nl, out);
        sum += out[5] + out[13];
      }
  printf("%d fields, checksum %llu\n", fields, (unsigned long long)sum);
  return 0;
}
#endif
