// Host known-answer program for the dropout counter hash: includes the real csrc/common.h (its hash
// functions are __host__ __device__) and prints what the kernels compute, for tests/test_dropmask_cpu.py
// to compare with oracle/dropmask.py.  Built host-only:
//   hipcc -x hip --offload-host-only -I unified_video_action_amd/csrc tests/host/drop_hash_main.cpp
//
// usage: drop_hash_main [p seed idx0 count]...      (seed / idx0 decimal or 0x..., any number of groups)
// per group:  "P <p> <seed> <thresh> <scale bits> <key>"  then one line "K <idx0> <count> <0/1 string>"
// of dropout_keep(seed, idx0 + i, thresh).  Without arguments a built-in list runs.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "common.h"

struct Case {
  float p;
  unsigned long long seed, idx0;
  long count;
};

static void run(const Case& c) {
  uint32_t th;
  float sc;
  uva_drop_params(c.p, &th, &sc);
  uint32_t sbits;
  memcpy(&sbits, &sc, 4);
  printf("P %.9g %llu %u %u %u\n", (double)c.p, c.seed, th, sbits, drop_key(c.seed));
  std::string bits((size_t)c.count, '0');
  for (long i = 0; i < c.count; ++i)
    if (dropout_keep(c.seed, c.idx0 + (unsigned long long)i, th)) bits[(size_t)i] = '1';
  printf("K %llu %ld %s\n", c.idx0, c.count, bits.c_str());
}

int main(int argc, char** argv) {
  std::vector<Case> cases;
  if (argc > 1) {
    if ((argc - 1) % 4 != 0) {
      fprintf(stderr, "usage: %s [p seed idx0 count]...\n", argv[0]);
      return 2;
    }
    for (int i = 1; i < argc; i += 4)
      cases.push_back({strtof(argv[i], nullptr), strtoull(argv[i + 1], nullptr, 0), strtoull(argv[i + 2], nullptr, 0),
                       strtol(argv[i + 3], nullptr, 0)});
  } else {
    cases = {{0.1f, 1234ull, 0ull, 64}, {0.5f, 0xABCDEF0123456789ull, (1ull << 33) - 32, 64}};
  }
  for (const Case& c : cases) run(c);
  return 0;
}
