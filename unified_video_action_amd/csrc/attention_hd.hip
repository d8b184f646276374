// Fused multi-head attention at head_dim 80 and 128 (non-causal, bf16 in/out, fp32 online softmax)
// for the mar_huge (D 1280, 16 heads) and mar_tiny / mar_small (D 768, 6 heads) presets of
// mar_con_unified.py:201-249 (timm Attention = SDPA with dropout_p = attn_drop while training).
// The design is attention.hip's (head_dim 64) with the head width as a template parameter, on the
// device helpers both files share (attention_frag.h); nothing here is tuned:
//   * S^T = K Q^T with the query on the lane, P^T packed in the pi order as the B operand of
//     O^T = V^T P^T (v_mfma_f32_16x16x32_bf16, V through ds_read_b64_tr_b16), lazy rescale;
//   * Q/K/V read straight from the qkv GEMM output [B, N, 3, H, HD], O written as [B, N, H, HD],
//     lse2 [B, H, N] in the log2 domain;
//   * dropout from the uva_attn_dropmask bit planes (MQ / MK, mask_pos layout) unchanged: the keep
//     decision of (b, h, q, key) does not depend on the head width;
//   * backward in two recompute kernels without atomics (bitwise reproducible): the dQ pass forms
//     D' = rowsum(dO O) / dsc into Dvec, the dK / dV pass reads it, dsc multiplies dQ / dK / dV once at
//     the stores; the qkv bias gradient comes from per-(batch, 128-row block) partials of the values
//     as stored + uva_colsum_final_launch.
//
// head_dim 80 = 2.5 of the 32-deep MFMA steps: the reduction dimension of Q K^T and dO V^T is padded
// to 96 with zeros.  The register operands (Q, dO, K, V rows held by a wave) load columns >= 80 as
// zeros, and the staging of every LDS tile writes columns 80..95 as zeros on each tile (never what
// the LDS held: a stale NaN times zero is a NaN).  No global load touches a column >= 80 of a head
// (for V of the last head in the last row that would be past the allocation).  A head's 80 columns
// are 160 B, so every 16-B load stays aligned.  The products over keys / queries (P V, dS K, dS^T Q,
// Pd^T dO) only read the 5 real 16-column output tiles.
//
// LDS row stride (bf16 elements): 112 at head_dim 80 (224-B rows, 96 used), 144 at head_dim 128
// (288-B rows).  Under gfx950's LDS lane groups (ds_read_b128 in 4 x 16 lanes {0-3,12-15,20-27}, ...;
// ds_read_b64_tr_b16 in 2 x 32; bank = dword mod 64) every row-fragment and transposed-fragment read
// of a 64-row tile is conflict-free at a stride of 16 mod 32 elements and costs a second LDS cycle
// per lane group at 96 / 104 / 120 and 136 / 152 / 160 (the model of tools/lds_swizzle_check.py with
// these widths; 128 is 8-way).
//
// Budgets.  Forward: 256 threads (4 waves x 32 queries), K and V tiles double-buffered = 56 KB
// (hd 80) / 72 KB (hd 128) of LDS per workgroup, __launch_bounds__(256, 2): 256 VGPRs, two
// workgroups per CU (two waves per SIMD, <= 144 KB of the 160 KB).  Backward: 512 threads (8 waves
// x 16 rows of the 128-row block), __launch_bounds__(512): 256 VGPRs, one workgroup per CU (two waves
// per SIMD): at 32 rows per wave the dK / dV kernel's accumulators (2 x 16 x HD / 64 registers), its
// K / V rows and the S / dP tiles do not fit 256 registers at head_dim 128.
#include "attention_frag.h"

namespace {

template <int HD> struct HdCfg;
template <> struct HdCfg<80> { static constexpr int KS = 3, DT = 5, LD = 112; };
template <> struct HdCfg<128> { static constexpr int KS = 4, DT = 8, LD = 144; };

// 8 columns ks*32 + 8g .. of one row of a head, zeros where the row is out of range or the columns are
// the padding of the reduction dimension (never a global read past the head's HD columns)
template <int HD>
__device__ __forceinline__ bf16x8 load_row8(const bf16* rowp, int ks, int g, bool ok) {
  const int c = ks * 32 + 8 * g;
  return (ok && c < HD) ? *(const bf16x8*)(rowp + c) : (bf16x8){};
}

// 64 rows x HD columns of a strided bf16 matrix -> 64 x (32 KS) LDS image (stride LD), the padding
// columns as zeros.  Tiles are always full (N % 64 == 0 is an ABI precondition).
template <int HD, int NT>
struct Stage {
  static constexpr int CPR = HdCfg<HD>::KS * 4;        // 16-B chunks per LDS row
  static constexpr int TOTAL = 64 * CPR;
  static constexpr int NI = (TOTAL + NT - 1) / NT;
  bf16x8 r[NI];
  __device__ __forceinline__ void load(const bf16* __restrict__ g, long long ld, int row0) {
    const bf16* base = g + (long long)row0 * ld;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int id = (int)threadIdx.x + i * NT, row = id / CPR, c = (id % CPR) * 8;
      r[i] = (id < TOTAL && c < HD) ? *(const bf16x8*)(base + (long long)row * ld + c) : (bf16x8){};
    }
  }
  __device__ __forceinline__ void store(bf16* lds) const {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int id = (int)threadIdx.x + i * NT, row = id / CPR, c = (id % CPR) * 8;
      if (id < TOTAL) *(bf16x8*)(lds + row * HdCfg<HD>::LD + c) = r[i];
    }
  }
};

// =====================================================================================
// forward: block = 4 waves x 32 queries, sweeps all 64-key tiles
//   lane view: q = qt*16 + li, key = kt*16 + 4g + r
// =====================================================================================
template <int HD, bool DROP>
__global__ __launch_bounds__(256, 2) void attn_hd_fwd_kernel(const bf16* __restrict__ qkv, bf16* __restrict__ out,
                                                             float* __restrict__ lse2,
                                                             const uint64_t* __restrict__ MQ, int N, int H, float c,
                                                             float dsc) {
  using C = HdCfg<HD>;
  constexpr int KS = C::KS, DT = C::DT, LD = C::LD, TILE = 64 * LD;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // > 64 KB at head_dim 128: dynamic
  bf16(*sK)[TILE] = (bf16(*)[TILE])smem;
  bf16(*sV)[TILE] = sK + 2;
  int bx, bh;
  xcd_grid2(bx, bh);
  const int b = bh / H, h = bh % H;
  const long long ld = 3LL * H * HD;
  const bf16* Qg = qkv + (long long)b * N * ld + h * HD;
  const bf16* Kg = Qg + H * HD;
  const bf16* Vg = Qg + 2 * H * HD;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, li = l & 15;
  const int q0 = bx * 128 + w * 32;
  const int nkv = N / 64;
  const uint16_t* mq = DROP ? (const uint16_t*)(MQ + (long long)bh * nkv * N) : nullptr;  // [kv][q][4 x u16]

  bf16x8 qf[2][KS];
  uint32_t mw[2], mwn[2];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    const int row = q0 + qt * 16 + li;
    const bool ok = row < N;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) qf[qt][ks] = load_row8<HD>(Qg + (long long)(ok ? row : 0) * ld, ks, g, ok);
    mw[qt] = (DROP && ok) ? mq[(long long)row * 4 + g] : 0u;
    mwn[qt] = 0u;
  }
  float m[2] = {-INFINITY, -INFINITY}, rs[2] = {0.f, 0.f};
  f32x4 o[2][DT];
#pragma unroll
  for (int qt = 0; qt < 2; ++qt)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) o[qt][dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  Stage<HD, 256> rk, rv;
  rk.load(Kg, ld, 0);
  rv.load(Vg, ld, 0);
  rk.store(sK[0]);
  rv.store(sV[0]);
  __syncthreads();
  int cur = 0;
  for (int kv = 0; kv < nkv; ++kv) {
    const bool more = kv + 1 < nkv;
    if (more) {
      rk.load(Kg, ld, (kv + 1) * 64);
      rv.load(Vg, ld, (kv + 1) * 64);
      if (DROP) {
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) {
          const int row = q0 + qt * 16 + li;
          mwn[qt] = row < N ? mq[((long long)(kv + 1) * N + row) * 4 + g] : 0u;
        }
      }
    }
    const bf16* cK = sK[cur];
    const bf16* cV = sV[cur];
    f32x4 s[4][2];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) s[kt][qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const bf16x8 kf = row_frag<LD>(cK, kt * 16, ks);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) s[kt][qt] = mfma16(kf, qf[qt][ks], s[kt][qt]);
      }
    }
    // row max (lane: 16 keys of its query; the 4 quads of a query meet through two swaps)
    float mx[2];
    bool need = false;
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      float a = fmaxf(s[0][qt][0], s[0][qt][1]);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = (kt == 0 ? 2 : 0); r < 4; ++r) a = fmaxf(a, s[kt][qt][r]);
      a = quad_max(a);
      mx[qt] = a * c;
      need |= mx[qt] > m[qt] + 8.0f;
    }
    // lazy rescale: the reference max only moves when some row grew by more than 2^8
    if (__builtin_amdgcn_ballot_w64(need)) {
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) {
        const float mnew = fmaxf(m[qt], mx[qt]);
        const float alpha = exp2_fast(m[qt] - mnew);
        rs[qt] *= alpha;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) o[qt][dt] *= alpha;
        m[qt] = mnew;
      }
    }
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const float nm = -m[qt];
      float ps[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float p = exp2_fast(fmaf(s[kt][qt][r], c, nm));
          ps[r] += p;
          s[kt][qt][r] = DROP ? keep_bit(p, mw[qt], kt * 4 + r) : p;
        }
      rs[qt] += (ps[0] + ps[1]) + (ps[2] + ps[3]);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 pf[2];
#pragma unroll
      for (int qt = 0; qt < 2; ++qt) pf[qt] = pack_pi(s[2 * ks][qt], s[2 * ks + 1][qt]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 vf = tr_frag<LD>(cV, 32 * ks, 32 * ks + 16, dt * 16);
#pragma unroll
        for (int qt = 0; qt < 2; ++qt) o[qt][dt] = mfma16(vf, pf[qt], o[qt][dt]);
      }
    }
    if (more) {
      rk.store(sK[cur ^ 1]);
      rv.store(sV[cur ^ 1]);
      if (DROP) { mw[0] = mwn[0]; mw[1] = mwn[1]; }
    }
    __syncthreads();
    cur ^= 1;
  }
  const long long ldo = (long long)H * HD;
#pragma unroll
  for (int qt = 0; qt < 2; ++qt) {
    float lsum = rs[qt];
    lsum += __shfl_xor(lsum, 16, 64);
    lsum += __shfl_xor(lsum, 32, 64);
    const int q = q0 + qt * 16 + li;
    if (q >= N) continue;
    const float inv = dsc / lsum;
    bf16* orow = out + ((long long)b * N + q) * ldo + h * HD;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      bf16x4 v = {(bf16)(o[qt][dt][0] * inv), (bf16)(o[qt][dt][1] * inv), (bf16)(o[qt][dt][2] * inv),
                  (bf16)(o[qt][dt][3] * inv)};
      *(bf16x4*)(orow + dt * 16 + 4 * g) = v;
    }
    if (g == 0) lse2[(long long)bh * N + q] = m[qt] + __log2f(lsum);
  }
}

// =====================================================================================
// backward dQ: block = 8 waves x 16 queries, sweeps all 64-key tiles (the forward's lane view:
// q = li, key = kt*16 + 4g + r)
//   S^T = K Q^T, dP'^T = V dO'^T, dQ^T[d][q] += K^T dS^T  (dS^T packed in pi order as the B operand)
// Forms D' = dmul * rowsum(dO * O) for its queries and writes Dvec for the dK / dV kernel.
// =====================================================================================
template <int HD, bool DROP>
__global__ __launch_bounds__(512) void attn_hd_bwd_dq_kernel(const bf16* __restrict__ qkv,
                                                             const bf16* __restrict__ dOs,
                                                             const bf16* __restrict__ Os,
                                                             const float* __restrict__ lse2, float* __restrict__ Dvec,
                                                             const uint64_t* __restrict__ MQ, bf16* __restrict__ dqkv,
                                                             int N, int H, float scale, float c, float dmul,
                                                             float* __restrict__ cpart) {
  using C = HdCfg<HD>;
  constexpr int KS = C::KS, DT = C::DT, LD = C::LD, TILE = 64 * LD;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // > 64 KB at head_dim 128: dynamic
  bf16(*sK)[TILE] = (bf16(*)[TILE])smem;
  bf16(*sV)[TILE] = sK + 2;
  int bx, bh;
  xcd_grid2(bx, bh);
  const int b = bh / H, h = bh % H;
  const long long ld = 3LL * H * HD, ldo = (long long)H * HD;
  const bf16* Qg = qkv + (long long)b * N * ld + h * HD;
  const bf16* Kg = Qg + H * HD;
  const bf16* Vg = Qg + 2 * H * HD;
  const bf16* dOg = dOs + (long long)b * N * ldo + h * HD;
  const bf16* Og = Os + (long long)b * N * ldo + h * HD;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, li = l & 15;
  const int row = bx * 128 + w * 16 + li;  // this lane's query
  const bool ok = row < N;                 // wave-uniform (N % 64 == 0)
  const int rowc = ok ? row : 0;
  const int nkv = N / 64;
  const uint16_t* mq = DROP ? (const uint16_t*)(MQ + (long long)bh * nkv * N) : nullptr;  // [kv][q][4 x u16]

  bf16x8 qf[KS], of[KS];
  float dsum = 0.f;
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    qf[ks] = load_row8<HD>(Qg + (long long)rowc * ld, ks, g, ok);
    of[ks] = load_row8<HD>(dOg + (long long)rowc * ldo, ks, g, ok);
    const bf16x8 ov = load_row8<HD>(Og + (long long)rowc * ldo, ks, g, ok);
#pragma unroll
    for (int j = 0; j < 8; ++j) dsum += (float)ov[j] * (float)of[ks][j];
  }
  dsum += __shfl_xor(dsum, 16, 64);
  dsum += __shfl_xor(dsum, 32, 64);
  const float Dq = ok ? dsum * dmul : 0.f;
  if (ok && g == 0) Dvec[(long long)bh * N + row] = Dq;
  const float L = ok ? lse2[(long long)bh * N + row] : 0.f;
  uint32_t mw = (DROP && ok) ? mq[(long long)row * 4 + g] : 0u, mwn = 0u;
  f32x4 dq[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dq[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  Stage<HD, 512> rk, rv;
  rk.load(Kg, ld, 0);
  rv.load(Vg, ld, 0);
  rk.store(sK[0]);
  rv.store(sV[0]);
  __syncthreads();
  int cur = 0;
  for (int kv = 0; kv < nkv; ++kv) {
    const bool more = kv + 1 < nkv;
    if (more) {
      rk.load(Kg, ld, (kv + 1) * 64);
      rv.load(Vg, ld, (kv + 1) * 64);
      if (DROP) mwn = ok ? mq[((long long)(kv + 1) * N + row) * 4 + g] : 0u;
    }
    f32x4 s[4], dp[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) s[kt] = dp[kt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        const bf16x8 ka = row_frag<LD>(sK[cur], kt * 16, ks);
        const bf16x8 va = row_frag<LD>(sV[cur], kt * 16, ks);
        s[kt] = mfma16(ka, qf[ks], s[kt]);
        dp[kt] = mfma16(va, of[ks], dp[kt]);
      }
    // dS = P (keep dP' - D')
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = exp2_fast(fmaf(s[kt][r], c, -L));
        float dpt = dp[kt][r];
        if (DROP) dpt = keep_bit(dpt, mw, kt * 4 + r);
        s[kt][r] = p * (dpt - Dq);
      }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 sb = pack_pi(s[2 * ks], s[2 * ks + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 ka = tr_frag<LD>(sK[cur], 32 * ks, 32 * ks + 16, dt * 16);
        dq[dt] = mfma16(ka, sb, dq[dt]);
      }
    }
    if (more) {
      rk.store(sK[cur ^ 1]);
      rv.store(sV[cur ^ 1]);
      if (DROP) mw = mwn;
    }
    __syncthreads();
    cur ^= 1;
  }
  // lane holds dQ^T[d = dt*16+4g+r][q = li]
  if (cpart) {
    // the qkv bias gradient's Q columns: sums over this block's 128 queries of the values as stored
    float* red = (float*)&sK[0][0];  // [8 waves][HD] (the loop is over: the last barrier passed)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sq = ok ? (float)(bf16)(dq[dt][r] * scale) : 0.f;
        sq = row16_sum(sq);
        if (li == 0) red[w * HD + dt * 16 + 4 * g + r] = sq;
      }
    __syncthreads();
    if (threadIdx.x < HD) {
      const int t = threadIdx.x;
      float v = 0.f;
#pragma unroll
      for (int ww = 0; ww < 8; ++ww) v += red[ww * HD + t];
      const long long rowp = (long long)b * gridDim.x + bx;
      cpart[rowp * (3LL * H * HD) + h * HD + t] = v;
    }
  }
  if (ok) {
    bf16* qrow = dqkv + ((long long)b * N + row) * ld + h * HD;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      bf16x4 a = {(bf16)(dq[dt][0] * scale), (bf16)(dq[dt][1] * scale), (bf16)(dq[dt][2] * scale),
                  (bf16)(dq[dt][3] * scale)};
      *(bf16x4*)(qrow + dt * 16 + 4 * g) = a;
    }
  }
}

// =====================================================================================
// backward dK, dV: block = 8 waves x 16 keys, sweeps all 64-query tiles
//   lane view of S / dP / Pd / dS: q = qt*16 + 4g + r, key = li
//   dV^T[d][key] += dO'^T Pd ; dK^T[d][key] += Q^T dS      (k = q, permuted by pi)
// =====================================================================================
template <int HD, bool DROP>
__global__ __launch_bounds__(512) void attn_hd_bwd_dkdv_kernel(const bf16* __restrict__ qkv,
                                                               const bf16* __restrict__ dOs,
                                                               const float* __restrict__ lse2,
                                                               const float* __restrict__ Dvec,
                                                               const uint64_t* __restrict__ MK,
                                                               bf16* __restrict__ dqkv, int N, int H, float scale,
                                                               float c, float vsc, float* __restrict__ cpart) {
  using C = HdCfg<HD>;
  constexpr int KS = C::KS, DT = C::DT, LD = C::LD, TILE = 64 * LD;
  extern __shared__ __attribute__((aligned(16))) char smem[];  // > 64 KB at head_dim 128: dynamic
  bf16(*sQ)[TILE] = (bf16(*)[TILE])smem;
  bf16(*sO)[TILE] = sQ + 2;
  float(*sL)[64] = (float(*)[64])(sO + 2);
  float(*sD)[64] = sL + 2;
  int bx, bh;
  xcd_grid2(bx, bh);
  const int b = bh / H, h = bh % H;
  const long long ld = 3LL * H * HD, ldo = (long long)H * HD;
  const bf16* Qg = qkv + (long long)b * N * ld + h * HD;
  const bf16* Kg = Qg + H * HD;
  const bf16* Vg = Qg + 2 * H * HD;
  const bf16* dOg = dOs + (long long)b * N * ldo + h * HD;
  const float* Lg = lse2 + (long long)bh * N;
  const float* Dg = Dvec + (long long)bh * N;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, li = l & 15;
  const int row = bx * 128 + w * 16 + li;  // this lane's key
  const bool ok = row < N;                 // wave-uniform (N % 64 == 0)
  const int rowc = ok ? row : 0;
  const int nq = N / 64;
  const uint16_t* mk = DROP ? (const uint16_t*)(MK + (long long)bh * nq * N) : nullptr;  // [qb][key][4 x u16]

  bf16x8 kf[KS], vf[KS];
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    kf[ks] = load_row8<HD>(Kg + (long long)rowc * ld, ks, g, ok);
    vf[ks] = load_row8<HD>(Vg + (long long)rowc * ld, ks, g, ok);
  }
  uint32_t mw = (DROP && ok) ? mk[(long long)row * 4 + g] : 0u, mwn = 0u;
  f32x4 dv[DT], dk[DT];
#pragma unroll
  for (int dt = 0; dt < DT; ++dt) dv[dt] = dk[dt] = (f32x4){0.f, 0.f, 0.f, 0.f};

  Stage<HD, 512> rq, ro;
  rq.load(Qg, ld, 0);
  ro.load(dOg, ldo, 0);
  rq.store(sQ[0]);
  ro.store(sO[0]);
  if (threadIdx.x < 64) { sL[0][threadIdx.x] = Lg[threadIdx.x]; sD[0][threadIdx.x] = Dg[threadIdx.x]; }
  __syncthreads();
  int cur = 0;
  for (int qi = 0; qi < nq; ++qi) {
    const bool more = qi + 1 < nq;
    float nl = 0.f, nd = 0.f;
    if (more) {
      rq.load(Qg, ld, (qi + 1) * 64);
      ro.load(dOg, ldo, (qi + 1) * 64);
      if (threadIdx.x < 64) { nl = Lg[(qi + 1) * 64 + threadIdx.x]; nd = Dg[(qi + 1) * 64 + threadIdx.x]; }
      if (DROP) mwn = ok ? mk[((long long)(qi + 1) * N + row) * 4 + g] : 0u;
    }
    // S[q][key] = Q K^T ; dP'[q][key] = dO' V^T
    f32x4 s[4], dp[4];
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) s[qt] = dp[qt] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int qt = 0; qt < 4; ++qt) {
        const bf16x8 a = row_frag<LD>(sQ[cur], qt * 16, ks);
        const bf16x8 e = row_frag<LD>(sO[cur], qt * 16, ks);
        s[qt] = mfma16(a, kf[ks], s[qt]);
        dp[qt] = mfma16(e, vf[ks], dp[qt]);
      }
    // P = exp2(S c - L);  Pd = keep P;  dS = P (keep dP' - D') = Pd dP' - P D'      (s <- Pd, dp <- dS)
#pragma unroll
    for (int qt = 0; qt < 4; ++qt) {
      const f32x4 Lq = *(const f32x4*)&sL[cur][qt * 16 + 4 * g];
      const f32x4 Dq = *(const f32x4*)&sD[cur][qt * 16 + 4 * g];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = exp2_fast(fmaf(s[qt][r], c, -Lq[r]));
        if (DROP) {
          const float pd = keep_bit(p, mw, qt * 4 + r);
          s[qt][r] = pd;
          dp[qt][r] = fmaf(pd, dp[qt][r], -(p * Dq[r]));
        } else {
          s[qt][r] = p;
          dp[qt][r] = p * (dp[qt][r] - Dq[r]);
        }
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const bf16x8 pb = pack_pi(s[2 * ks], s[2 * ks + 1]);
      const bf16x8 sb = pack_pi(dp[2 * ks], dp[2 * ks + 1]);
#pragma unroll
      for (int dt = 0; dt < DT; ++dt) {
        const bf16x8 oa = tr_frag<LD>(sO[cur], 32 * ks, 32 * ks + 16, dt * 16);
        const bf16x8 qa = tr_frag<LD>(sQ[cur], 32 * ks, 32 * ks + 16, dt * 16);
        dv[dt] = mfma16(oa, pb, dv[dt]);
        dk[dt] = mfma16(qa, sb, dk[dt]);
      }
    }
    if (more) {
      rq.store(sQ[cur ^ 1]);
      ro.store(sO[cur ^ 1]);
      if (threadIdx.x < 64) { sL[cur ^ 1][threadIdx.x] = nl; sD[cur ^ 1][threadIdx.x] = nd; }
      if (DROP) mw = mwn;
    }
    __syncthreads();
    cur ^= 1;
  }
  // lane holds [d = dt*16+4g+r][key = li]
  if (cpart) {
    // the qkv bias gradient's K / V columns: sums over this block's 128 keys of the values as stored
    float* red = (float*)&sQ[0][0];  // [8 waves][2 HD] (the loop is over: the last barrier passed)
#pragma unroll
    for (int dt = 0; dt < DT; ++dt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sk = ok ? (float)(bf16)(dk[dt][r] * scale) : 0.f;
        float sv = ok ? (float)(bf16)(dv[dt][r] * vsc) : 0.f;
        sk = row16_sum(sk);
        sv = row16_sum(sv);
        if (li == 0) {
          red[w * 2 * HD + dt * 16 + 4 * g + r] = sk;
          red[w * 2 * HD + HD + dt * 16 + 4 * g + r] = sv;
        }
      }
    __syncthreads();
    if (threadIdx.x < 2 * HD) {
      const int t = threadIdx.x;
      float v = 0.f;
#pragma unroll
      for (int ww = 0; ww < 8; ++ww) v += red[ww * 2 * HD + t];
      const long long rowp = (long long)b * gridDim.x + bx;
      cpart[rowp * (3LL * H * HD) + (t < HD ? H * HD + t : 2 * H * HD + t - HD) + h * HD] = v;
    }
  }
  if (ok) {
    bf16* krow = dqkv + ((long long)b * N + row) * ld + H * HD + h * HD;
    bf16* vrow = krow + H * HD;
#pragma unroll
    for (int dt = 0; dt < DT; ++dt) {
      bf16x4 a = {(bf16)(dk[dt][0] * scale), (bf16)(dk[dt][1] * scale), (bf16)(dk[dt][2] * scale),
                  (bf16)(dk[dt][3] * scale)};
      bf16x4 e = {(bf16)(dv[dt][0] * vsc), (bf16)(dv[dt][1] * vsc), (bf16)(dv[dt][2] * vsc),
                  (bf16)(dv[dt][3] * vsc)};
      *(bf16x4*)(krow + dt * 16 + 4 * g) = a;
      *(bf16x4*)(vrow + dt * 16 + 4 * g) = e;
    }
  }
}

template <int HD>
int fwd_launch(const void* qkv, void* out, float* lse2, const void* mask, int B, int N, int H, float scale, bool drop,
               float ds, hipStream_t s) {
  dim3 grid((N + 127) / 128, B * H);
  const float c = scale * 1.4426950408889634f;
  constexpr int lds = 4 * 64 * HdCfg<HD>::LD * (int)sizeof(bf16);  // K and V tiles, double-buffered
  static const bool once = [] {
    (void)hipFuncSetAttribute((const void*)attn_hd_fwd_kernel<HD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute((const void*)attn_hd_fwd_kernel<HD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    return true;
  }();
  (void)once;
  if (drop)
    attn_hd_fwd_kernel<HD, true><<<grid, 256, lds, s>>>((const bf16*)qkv, (bf16*)out, lse2, (const uint64_t*)mask, N, H,
                                                      c, ds);
  else
    attn_hd_fwd_kernel<HD, false><<<grid, 256, lds, s>>>((const bf16*)qkv, (bf16*)out, lse2, nullptr, N, H, c, 1.0f);
  UVA_LAUNCH_CHECK();
  return 0;
}

template <int HD>
int bwd_launch(const void* qkv, const void* out, const void* dout, const float* lse2, const void* mask, float* Dvec,
               void* dqkv, float* cpart, int B, int N, int H, float scale, bool drop, float ds, hipStream_t s) {
  const int nt = N / 64;
  const uint64_t* MQ = (const uint64_t*)mask;
  const uint64_t* MK = drop ? MQ + (long long)B * H * N * nt : nullptr;
  dim3 grid((N + 127) / 128, B * H);
  const float c = scale * 1.4426950408889634f;
  const float sk = scale * ds;
  constexpr int lds = 4 * 64 * HdCfg<HD>::LD * (int)sizeof(bf16);  // two tile pairs, double-buffered
  constexpr int ldsk = lds + 4 * 64 * (int)sizeof(float);          // + the lse2 / D' rows of a query tile
  static const bool once = [] {
    (void)hipFuncSetAttribute((const void*)attn_hd_bwd_dq_kernel<HD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute((const void*)attn_hd_bwd_dq_kernel<HD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    (void)hipFuncSetAttribute((const void*)attn_hd_bwd_dkdv_kernel<HD, true>, hipFuncAttributeMaxDynamicSharedMemorySize, ldsk);
    (void)hipFuncSetAttribute((const void*)attn_hd_bwd_dkdv_kernel<HD, false>, hipFuncAttributeMaxDynamicSharedMemorySize, ldsk);
    return true;
  }();
  (void)once;
  // dQ first: it forms D' (= rowsum(dO O) / dsc) for its queries and writes Dvec, which dK / dV reads
  if (drop) {
    attn_hd_bwd_dq_kernel<HD, true><<<grid, 512, lds, s>>>((const bf16*)qkv, (const bf16*)dout, (const bf16*)out, lse2,
                                                         Dvec, MQ, (bf16*)dqkv, N, H, sk, c, 1.0f / ds, cpart);
    attn_hd_bwd_dkdv_kernel<HD, true><<<grid, 512, ldsk, s>>>((const bf16*)qkv, (const bf16*)dout, lse2, Dvec, MK,
                                                           (bf16*)dqkv, N, H, sk, c, ds, cpart);
  } else {
    attn_hd_bwd_dq_kernel<HD, false><<<grid, 512, lds, s>>>((const bf16*)qkv, (const bf16*)dout, (const bf16*)out, lse2,
                                                          Dvec, nullptr, (bf16*)dqkv, N, H, sk, c, 1.0f, cpart);
    attn_hd_bwd_dkdv_kernel<HD, false><<<grid, 512, ldsk, s>>>((const bf16*)qkv, (const bf16*)dout, lse2, Dvec, nullptr,
                                                            (bf16*)dqkv, N, H, sk, c, ds, cpart);
  }
  UVA_LAUNCH_CHECK();
  return 0;
}

}  // namespace

// =====================================================================================
// C ABI
// =====================================================================================
int uva_colsum_final_launch(const float* part, int nrows, int cols, float* out, int accum, hipStream_t s);

extern "C" int uva_attn_hd_supported(int head_dim) { return head_dim == 80 || head_dim == 128; }

extern "C" long long uva_attn_bwd_hd_part_floats(int B, int N, int H, int head_dim) {
  return (long long)B * ((N + 127) / 128) * 3LL * H * head_dim;
}

extern "C" int uva_attn_fwd_hd(const void* qkv, void* out, float* lse2, const void* mask, int B, int N, int H,
                               int head_dim, float scale, float drop_p, hipStream_t s) {
  if (!uva_attn_hd_supported(head_dim) || N <= 0 || N % 64 != 0 || B <= 0 || H <= 0)
    return (int)hipErrorInvalidValue;
  const bool drop = drop_p > 0.f;
  if (drop && mask == nullptr) return (int)hipErrorInvalidValue;
  uint32_t th;
  float ds;
  uva_drop_params(drop_p, &th, &ds);
  return head_dim == 80 ? fwd_launch<80>(qkv, out, lse2, mask, B, N, H, scale, drop, ds, s)
                        : fwd_launch<128>(qkv, out, lse2, mask, B, N, H, scale, drop, ds, s);
}

extern "C" int uva_attn_bwd_hd(const void* qkv, const void* out, const void* dout, const float* lse2, const void* mask,
                               float* Dvec, void* dqkv, float* dbias, int accum, float* part, int B, int N, int H,
                               int head_dim, float scale, float drop_p, hipStream_t s) {
  if (!uva_attn_hd_supported(head_dim) || N <= 0 || N % 64 != 0 || B <= 0 || H <= 0)
    return (int)hipErrorInvalidValue;
  const bool drop = drop_p > 0.f;
  if (drop && mask == nullptr) return (int)hipErrorInvalidValue;
  if (dbias && !part) return (int)hipErrorInvalidValue;
  uint32_t th;
  float ds;
  uva_drop_params(drop_p, &th, &ds);
  float* cpart = dbias ? part : nullptr;
  const int r = head_dim == 80
                    ? bwd_launch<80>(qkv, out, dout, lse2, mask, Dvec, dqkv, cpart, B, N, H, scale, drop, ds, s)
                    : bwd_launch<128>(qkv, out, dout, lse2, mask, Dvec, dqkv, cpart, B, N, H, scale, drop, ds, s);
  if (r || !dbias) return r;
  return uva_colsum_final_launch(part, B * ((N + 127) / 128), 3 * H * head_dim, dbias, accum, s);
}
