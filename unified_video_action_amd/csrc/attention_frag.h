// Device helpers shared by the fused attention kernels (attention.hip, attention_hd.hip,
// attention_fp8.hip): the MFMA fragment reads of a 64-row bf16 LDS tile, the packed bf16 convert and
// the pi-order pack, the 16x16x32 MFMA, exp2, the keep-bit mask, the quad max and the position of a
// key / query inside a dropout mask word.  All are __forceinline__: one copy here, no code of its own.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// A / B operand of one 32-deep step ks: 8 consecutive bf16 of row row0 + (lane & 15).
// STRIDE = the tile's row stride in bf16 elements.  A linear stride keeps every fragment address
// base + immediate.
template <int STRIDE>
__device__ __forceinline__ bf16x8 row_frag(const bf16* lds, int row0, int ks) {
  const int l = threadIdx.x & 63;
  return *(const bf16x8*)(lds + (row0 + (l & 15)) * STRIDE + ks * 32 + 8 * (l >> 4));
}

// the transposed operand (16 columns from col0, k over rows) by two ds_read_b64_tr_b16: the row bases
// rowA / rowB choose which 16-row tiles form the two halves of the 32-deep step (the pi order of
// pack_pi on the other operand)
template <int STRIDE>
__device__ __forceinline__ bf16x8 tr_frag(const bf16* lds, int rowA, int rowB, int col0) {
  const int l = threadIdx.x & 63, g = l >> 4, q = (l >> 2) & 3, p = l & 3;
  const bf16* a0 = lds + (rowA + 4 * g + q) * STRIDE + col0 + 4 * p;
  const bf16* a1 = lds + (rowB + 4 * g + q) * STRIDE + col0 + 4 * p;
  s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, a0));
  s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, a1));
  s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// two f32 -> one dword of two bf16 (RNE, as the (bf16) cast): one v_cvt_pk_bf16_f32 per pair.  Plain
// casts of individually masked values compiled to one cvt per element + a v_perm per pair.
// (a vector conversion, not inline asm: the result feeds MFMAs, whose operand hazards hipcc only
// tracks for instructions it emitted itself)
__device__ __forceinline__ uint32_t cvt_pk_bf16(float lo, float hi) {
  return __builtin_bit_cast(uint32_t, __builtin_convertvector((f32x2){lo, hi}, bf16x2));
}
// two MFMA outputs (16-row tiles A and B) -> the 32-deep B operand in the pi order
__device__ __forceinline__ bf16x8 pack_pi(const f32x4& a, const f32x4& b) {
  const u32x4 u = {cvt_pk_bf16(a[0], a[1]), cvt_pk_bf16(a[2], a[3]), cvt_pk_bf16(b[0], b[1]), cvt_pk_bf16(b[2], b[3])};
  return __builtin_bit_cast(bf16x8, u);
}

__device__ __forceinline__ f32x4 mfma16(const bf16x8& a, const bf16x8& b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }
// keep-bit b of a mask word as an all-ones / all-zeros 32-bit mask.  (A v_bfe_i32 in inline asm
// saves hipcc's v_and + v_cmp + v_cndmask lowering but measured slower in the head_dim-64 dK/dV loop:
// the asm statements constrain its scheduling.)
__device__ __forceinline__ float keep_bit(float v, uint32_t w, int b) {
  return __int_as_float(__float_as_int(v) & __builtin_amdgcn_sbfe(w, b, 1));
}
// max over lanes l, l^16, l^32, l^48 by v_permlane16/32_swap (VALU) instead of two ds_bpermute.
// Builtins only: an inline-asm producer is invisible to hipcc's permlane / trans / MFMA hazard
// wait-state insertion (an asm v_max feeding the second swap read a stale register).
__device__ __forceinline__ float quad_max(float v) {
  auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
// position of element k (0..63) of a 64-wide tile inside an MQ / MK word (an involution)
__host__ __device__ constexpr int mask_pos(int k) { return ((k >> 2) & 3) * 16 + (k >> 4) * 4 + (k & 3); }
