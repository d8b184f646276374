// The per-tile power-of-two scale of the fp8 (OCP e4m3) attention operands (attention_fp8.hip): one
// __host__ __device__ function, so tests/host/fp8_scale_main.cpp runs the kernel's own code on the CPU
// over every bf16 amax (tests/test_fp8_scale_cpu.py).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define A8_EXP_MIN (-126)
#define A8_EXP_MAX 126

// smallest e with amax * 2^-e <= 448, clamped to [-126, 126]; amax >= 0 (a maximum of |x|).
// frexpf's amax = f * 2^x, f in [0.5, 1), read off the bits (no loop, no log2f, the same on host and
// device whatever the fp32 denormal mode): 448 = 0.875 * 2^9, so e = x - 9 if f <= 0.875, else x - 8.
//   amax = 0           -> 0
//   fp32 denormal amax -> x <= -126, e <= -134: the lower clamp
//   Inf / NaN          -> the upper clamp: the elements come out as whatever the e4m3 conversion gives
// Inside the clamp 2^e, 2^-e and the e8m0 code 127 + e are all normal.
__host__ __device__ __forceinline__ int fp8_tile_exp(float amax) {
  const uint32_t u = __builtin_bit_cast(uint32_t, amax) & 0x7FFFFFFFu;
  if (u == 0u) return 0;
  const int E = (int)(u >> 23);
  if (E == 255) return A8_EXP_MAX;
  if (E == 0) return A8_EXP_MIN;
  // normal: 1.m * 2^(E - 127) = f * 2^(E - 126) with f = 1.m / 2; f <= 0.875 <=> m <= 0.75
  const int e = (E - 126) - ((u & 0x7FFFFFu) <= 0x600000u ? 9 : 8);
  return e < A8_EXP_MIN ? A8_EXP_MIN : (e > A8_EXP_MAX ? A8_EXP_MAX : e);
}
