// CLIP text tower (ViT-B/32 text side: width 512, 8 heads of 64, causal, QuickGELU) -- the four kernels the
// tower needs beside the library's LayerNorm and GEMMs (reference: utils/language_model.py:7-33 ->
// transformers CLIPTextTransformer; called from policy/unified_video_action_policy.py:241-252, 366-378).
// Forward only: the tower is frozen.  Every kernel is one small workgroup per unit of work (a token row, a
// (batch, head) pair, a batch row): no cross-workgroup communication, no atomics, no inline assembly.
#include "attention_frag.h"

// ---- token + position embedding ---------------------------------------------------------------------
// x[b L + t][:] = tok[clamp(ids[b][t], 0, vocab - 1)][:] + pos[t][:]   (fp32, one rounding)
// The clamp keeps a corrupt id inside the table: such an id reads a wrong row, never out of bounds.
__device__ __forceinline__ long long load_id(const void* ids, int i64, long long i) {
  return i64 ? ((const long long*)ids)[i] : (long long)((const int*)ids)[i];
}

__global__ __launch_bounds__(128) void clip_embed_kernel(const void* __restrict__ ids, int i64,
                                                         const float* __restrict__ tok, const float* __restrict__ pos,
                                                         float* __restrict__ x, int L, int D, int vocab) {
  const long long row = blockIdx.x;
  const int t = (int)(row % L);
  long long id = load_id(ids, i64, row);
  id = id < 0 ? 0 : (id > vocab - 1 ? vocab - 1 : id);
  const float* a = tok + id * D;
  const float* p = pos + (long long)t * D;
  float* o = x + row * D;
  for (int c = threadIdx.x * 4; c < D; c += 128 * 4) {
    const f32x4 u = *(const f32x4*)(a + c), v = *(const f32x4*)(p + c);
    *(f32x4*)(o + c) = u + v;
  }
}

// ---- pooling: the row at the first maximum of ids[b][:] ----------------------------------------------
// (CLIPTextTransformer: argmax over the ids = the EOT token, the largest id of the vocabulary)
__global__ __launch_bounds__(64) void clip_pool_kernel(const void* __restrict__ ids, int i64,
                                                       const float* __restrict__ x, float* __restrict__ out,
                                                       int* __restrict__ index, int L, int D) {
  const int b = blockIdx.x, l = threadIdx.x;
  long long best = INT64_MIN;
  int at = 0x7fffffff;
  for (int j = l; j < L; j += 64) {
    const long long v = load_id(ids, i64, (long long)b * L + j);
    if (v > best) {  // strict: a lane keeps the first of its equal values
      best = v;
      at = j;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long ob = __shfl_xor(best, o, 64);
    const int oa = __shfl_xor(at, o, 64);
    if (ob > best || (ob == best && oa < at)) {
      best = ob;
      at = oa;
    }
  }
  if (at >= L) at = 0;  // only when every id is INT64_MIN: stay inside the row
  if (index != nullptr && l == 0) index[b] = at;
  const float* src = x + ((long long)b * L + at) * D;
  float* dst = out + (long long)b * D;
  for (int c = l * 4; c < D; c += 64 * 4) *(f32x4*)(dst + c) = *(const f32x4*)(src + c);
}

// ---- QuickGELU: y = x * sigmoid(1.702 x) --------------------------------------------------------------
// sigmoid as rcp(1 + exp2(k x)), k = -1.702 log2(e) folded into one constant (one product rounding)
__device__ __forceinline__ float quick_gelu(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-2.4554669595930157f * x));
}

template <typename T>
__global__ __launch_bounds__(256) void quick_gelu_kernel(const T* __restrict__ x, T* __restrict__ y, long long n) {
  constexpr int V = 8;
  const long long nv = n / V;
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += stride) {
    __attribute__((aligned(16))) T a[V], r[V];
    if constexpr (sizeof(T) == 2) {
      *(bf16x8*)a = *(const bf16x8*)(x + i * V);
    } else {
      *(f32x4*)a = *(const f32x4*)(x + i * V);
      *(f32x4*)(a + 4) = *(const f32x4*)(x + i * V + 4);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) r[k] = from_f32<T>(quick_gelu(to_f32(a[k])));
    if constexpr (sizeof(T) == 2) {
      *(bf16x8*)(y + i * V) = *(const bf16x8*)r;
    } else {
      *(f32x4*)(y + i * V) = *(const f32x4*)r;
      *(f32x4*)(y + i * V + 4) = *(const f32x4*)(r + 4);
    }
  }
  // scalar tail (n % 8 elements), first block only
  if (blockIdx.x == 0) {
    const long long i = nv * V + threadIdx.x;
    if (i < n) y[i] = from_f32<T>(quick_gelu(to_f32(x[i])));
  }
}

// ---- causal self-attention with a key mask, head_dim 64, 1 <= L <= 77 ----------------------------------
// qkv [B L][3][H][64] (the qkv GEMM's output), out [B L][H 64].  P = softmax(scale Q K^T + causal + keymask):
// key j serves query i iff j <= i and keep[b][j] != 0 (keep == NULL: every key kept).  A masked or padded key
// gets the score CLIP_NEG (a large finite negative: no inf - inf anywhere) and its probability is set to
// exactly 0.  The host requires keep[b][0] != 0 (position 0 is BOS), so every query row has key 0; a row
// without any key (a device-side mask that breaks the rule) stores zeros, not NaN.
#define CLIP_NEG (-1.0e30f)
#define CLIP_LMAX 77

__device__ __forceinline__ int load_keep(const void* keep, int i64, int b, int L, int j) {
  if (j >= L) return 0;
  if (keep == nullptr) return 1;
  return load_id(keep, i64, (long long)b * L + j) != 0;
}

// bf16: one workgroup of 4 waves per (batch, head).  Q / K / V rows are staged once in LDS, zero-padded to
// NK * 32 rows (the MFMA tile: 16 queries, 32-deep key steps); wave w takes the 16-query tiles w, w + 4.
// Lane view after the score MFMAs (S^T = K Q^T, as csrc/attention.hip): key = kt * 16 + 4 g + r, query =
// qt * 16 + li -- a query's keys sit in the 4 lanes li + 16 g.  P^T in the pi order (pack_pi) is the B
// operand of O^T = V^T P^T, V^T read by the transposed LDS read (tr_frag).  Every lane of a wave runs every
// LDS read (the transposed read needs the full wave); only the final stores are predicated on q < L.
template <int NK>
__global__ __launch_bounds__(256) void clip_attn_bf16_kernel(const bf16* __restrict__ qkv, const void* __restrict__ keep,
                                                             int keep_i64, bf16* __restrict__ out, int L, int H,
                                                             float c) {
  constexpr int LD = 80, ROWS = NK * 32, NKT = NK * 2;
  __shared__ __attribute__((aligned(16))) bf16 sQ[ROWS * LD];
  __shared__ __attribute__((aligned(16))) bf16 sK[ROWS * LD];
  __shared__ __attribute__((aligned(16))) bf16 sV[ROWS * LD];
  __shared__ int sKeep[ROWS];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const long long ld = 3LL * H * 64;
  const bf16* base = qkv + (long long)b * L * ld + h * 64;
  for (int i = threadIdx.x; i < ROWS * 8; i += 256) {
    const int row = i >> 3, col = (i & 7) * 8;
    bf16x8 q = {}, k = {}, v = {};
    if (row < L) {
      const bf16* p = base + (long long)row * ld + col;
      q = *(const bf16x8*)p;
      k = *(const bf16x8*)(p + H * 64);
      v = *(const bf16x8*)(p + 2 * H * 64);
    }
    *(bf16x8*)(sQ + row * LD + col) = q;
    *(bf16x8*)(sK + row * LD + col) = k;
    *(bf16x8*)(sV + row * LD + col) = v;
  }
  for (int j = threadIdx.x; j < ROWS; j += 256) sKeep[j] = load_keep(keep, keep_i64, b, L, j);
  __syncthreads();

  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63, g = l >> 4, li = l & 15;
  const int nqt = (L + 15) / 16;
  const long long ldo = (long long)H * 64;
  for (int qt = w; qt < nqt; qt += 4) {  // wave-uniform
    const int q = qt * 16 + li;
    const bf16x8 qf0 = row_frag<LD>(sQ, qt * 16, 0), qf1 = row_frag<LD>(sQ, qt * 16, 1);
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      s[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
      s[kt] = mfma16(row_frag<LD>(sK, kt * 16, 0), qf0, s[kt]);
      s[kt] = mfma16(row_frag<LD>(sK, kt * 16, 1), qf1, s[kt]);
    }
    bool ok[NKT][4];
    float m = CLIP_NEG;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = kt * 16 + 4 * g + r;
        ok[kt][r] = key <= q && sKeep[key] != 0;
        s[kt][r] = ok[kt][r] ? s[kt][r] * c : CLIP_NEG;
        m = fmaxf(m, s[kt][r]);
      }
    m = quad_max(m);
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = ok[kt][r] ? exp2_fast(s[kt][r] - m) : 0.f;
        sum += p;
        s[kt][r] = p;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < NK; ++ks) {
      const bf16x8 pf = pack_pi(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) o[dt] = mfma16(tr_frag<LD>(sV, 32 * ks, 32 * ks + 16, dt * 16), pf, o[dt]);
    }
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;
    if (q < L) {
      bf16* orow = out + ((long long)b * L + q) * ldo + h * 64;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const bf16x4 v = {(bf16)(o[dt][0] * inv), (bf16)(o[dt][1] * inv), (bf16)(o[dt][2] * inv),
                          (bf16)(o[dt][3] * inv)};
        *(bf16x4*)(orow + dt * 16 + 4 * g) = v;
      }
    }
  }
}

// fp32 (the parity route; the role _attn_mat_fwd plays for the Block): plain VALU dot products on fp32 qkv.
// One workgroup of 4 waves per (batch, head); wave w takes queries w, w + 4, ...  Scores: lane = key (two
// keys per lane cover L <= 77 < 128), four partial sums over d; softmax over the wave; output: lane = d.
__global__ __launch_bounds__(256) void clip_attn_f32_kernel(const float* __restrict__ qkv, const void* __restrict__ keep,
                                                            int keep_i64, float* __restrict__ out, int L, int H,
                                                            float scale) {
  constexpr int LDK = 65;  // odd stride: lanes on consecutive keys read distinct banks
  __shared__ float sQ[CLIP_LMAX * 64];
  __shared__ float sK[CLIP_LMAX * LDK];
  __shared__ float sV[CLIP_LMAX * 64];
  __shared__ float sP[4][128];
  __shared__ int sKeep[128];
  const int b = blockIdx.x / H, h = blockIdx.x % H;
  const long long ld = 3LL * H * 64;
  const float* base = qkv + (long long)b * L * ld + h * 64;
  for (int i = threadIdx.x; i < L * 64; i += 256) {
    const int row = i >> 6, col = i & 63;
    const float* p = base + (long long)row * ld + col;
    sQ[row * 64 + col] = p[0];
    sK[row * LDK + col] = p[H * 64];
    sV[row * 64 + col] = p[2 * H * 64];
  }
  if (threadIdx.x < 128) sKeep[threadIdx.x] = load_keep(keep, keep_i64, b, L, threadIdx.x);
  __syncthreads();
  const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), l = threadIdx.x & 63;
  const long long ldo = (long long)H * 64;
  for (int q = w; q < L; q += 4) {  // wave-uniform
    float sc[2];
    bool ok[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int key = l + 64 * t;
      ok[t] = key <= q && sKeep[key] != 0;  // key <= q < L
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
      if (ok[t]) {
        const float* kr = sK + key * LDK;
        const float* qr = sQ + q * 64;
        for (int d = 0; d < 64; d += 4) {
          a0 = fmaf(qr[d], kr[d], a0);
          a1 = fmaf(qr[d + 1], kr[d + 1], a1);
          a2 = fmaf(qr[d + 2], kr[d + 2], a2);
          a3 = fmaf(qr[d + 3], kr[d + 3], a3);
        }
      }
      sc[t] = ok[t] ? ((a0 + a1) + (a2 + a3)) * scale : CLIP_NEG;
    }
    const float m = wave_max(fmaxf(sc[0], sc[1]));
    float p[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) p[t] = ok[t] ? __expf(sc[t] - m) : 0.f;
    const float sum = wave_sum(p[0] + p[1]);
    const float inv = sum > 0.f ? 1.0f / sum : 0.f;
    sP[w][l] = p[0] * inv;
    sP[w][l + 64] = p[1] * inv;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    float acc = 0.f;
    for (int j = 0; j <= q; ++j) acc = fmaf(sP[w][j], sV[j * 64 + l], acc);
    out[((long long)b * L + q) * ldo + h * 64 + l] = acc;
    __builtin_amdgcn_wave_barrier();
  }
}

extern "C" {

int uva_clip_embed(const void* ids, int ids_i64, const float* tok_emb, const float* pos_emb, float* x, int B, int L,
                   int D, int vocab, hipStream_t stream) {
  if (B < 1 || L < 1 || D < 4 || D % 4 || vocab < 1) return (int)hipErrorInvalidValue;
  if (((uintptr_t)tok_emb | (uintptr_t)pos_emb | (uintptr_t)x) & 15) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_embed_kernel, dim3(B * L), dim3(128), 0, stream, ids, ids_i64, tok_emb, pos_emb, x, L, D,
                     vocab);
  UVA_LAUNCH_CHECK();
  return 0;
}

int uva_clip_pool(const void* ids, int ids_i64, const float* x, float* out, int* index, int B, int L, int D,
                  hipStream_t stream) {
  if (B < 1 || L < 1 || D < 4 || D % 4) return (int)hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)out) & 15) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_pool_kernel, dim3(B), dim3(64), 0, stream, ids, ids_i64, x, out, index, L, D);
  UVA_LAUNCH_CHECK();
  return 0;
}

int uva_quick_gelu(int dtype, const void* x, void* y, long long n, hipStream_t stream) {
  if (n < 1) return (int)hipErrorInvalidValue;
  if (((uintptr_t)x | (uintptr_t)y) & 15) return (int)hipErrorInvalidValue;
  long long blocks = (n / 8 + 255) / 256;
  blocks = blocks < 1 ? 1 : (blocks > 2048 ? 2048 : blocks);
  if (dtype == UVA_DT_BF16)
    hipLaunchKernelGGL(quick_gelu_kernel<bf16>, dim3((int)blocks), dim3(256), 0, stream, (const bf16*)x, (bf16*)y, n);
  else if (dtype == UVA_DT_F32)
    hipLaunchKernelGGL(quick_gelu_kernel<float>, dim3((int)blocks), dim3(256), 0, stream, (const float*)x, (float*)y,
                       n);
  else
    return (int)hipErrorInvalidValue;
  UVA_LAUNCH_CHECK();
  return 0;
}

int uva_clip_attn(int dtype, const void* qkv, const void* key_mask, int mask_i64, void* out, int B, int L, int H,
                  float scale, hipStream_t stream) {
  if (B < 1 || H < 1 || L < 1 || L > CLIP_LMAX) return (int)hipErrorInvalidValue;
  if (((uintptr_t)qkv | (uintptr_t)out) & 15) return (int)hipErrorInvalidValue;
  const dim3 grid(B * H), block(256);
  if (dtype == UVA_DT_BF16) {
    const float c = scale * 1.4426950408889634f;
    const bf16* q = (const bf16*)qkv;
    bf16* o = (bf16*)out;
    if (L <= 32)
      hipLaunchKernelGGL(clip_attn_bf16_kernel<1>, grid, block, 0, stream, q, key_mask, mask_i64, o, L, H, c);
    else if (L <= 64)
      hipLaunchKernelGGL(clip_attn_bf16_kernel<2>, grid, block, 0, stream, q, key_mask, mask_i64, o, L, H, c);
    else
      hipLaunchKernelGGL(clip_attn_bf16_kernel<3>, grid, block, 0, stream, q, key_mask, mask_i64, o, L, H, c);
  } else if (dtype == UVA_DT_F32) {
    hipLaunchKernelGGL(clip_attn_f32_kernel, grid, block, 0, stream, (const float*)qkv, key_mask, mask_i64,
                       (float*)out, L, H, scale);
  } else {
    return (int)hipErrorInvalidValue;
  }
  UVA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
