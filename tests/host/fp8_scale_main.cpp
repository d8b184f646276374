// Host known-answer program for the fp8 attention tile exponent: includes the real csrc/fp8_scale.h
// (fp8_tile_exp is __host__ __device__) and prints what attn_quant_fp8_kernel computes, for
// tests/test_fp8_scale_cpu.py to compare with an integer restatement.  Built host-only:
//   hipcc -x hip --offload-host-only -I unified_video_action_amd/csrc tests/host/fp8_scale_main.cpp
//
// usage: fp8_scale_main [fp32 bit pattern, decimal or 0x...]...
// per argument one line "<bits> <e>".  Without arguments: every bf16 bit pattern 0x0000 .. 0x7FFF as the
// upper half of the fp32 word (0, the positive denormals and normals, +Inf, the NaNs).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "fp8_scale.h"

static void run(uint32_t bits) {
  float a;
  memcpy(&a, &bits, 4);
  printf("%u %d\n", bits, fp8_tile_exp(a));
}

int main(int argc, char** argv) {
  if (argc > 1) {
    for (int i = 1; i < argc; ++i) run((uint32_t)strtoul(argv[i], nullptr, 0));
    return 0;
  }
  for (uint32_t h = 0; h <= 0x7FFFu; ++h) run(h << 16);
  return 0;
}
