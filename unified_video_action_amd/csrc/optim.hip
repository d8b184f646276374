// Fused optimizer step over the flat fp32 parameter buffer (one pass, HBM-bound):
//   torch.optim.AdamW semantics (decoupled weight decay, bias correction; policy:343-360)
//   over one parameter group region [p, p+n) (the host launches once per group with that
//   group's lr / weight_decay -- policy:326-341 no-decay / decay groups)
//   + gradient averaging over DP ranks (grad_scale = 1/world)
//   + optional fused EMA update ema = d*ema + (1-d)*p_new (ema_model.py:57-89)
//   + optional bf16 shadow copy of the new weights for the next step's MFMA GEMMs.
// Algorithmic bytes per parameter: p rw 8 + g r 4 + m rw 8 + v rw 8 (+ ema rw 8) (+ bf16 w 2) = 28..38 B.
// Group regions start 16-B aligned (ParamStore pads them), so the body runs on float4 and
// only a < 4-element tail is scalar.
//
// Gradient norm / clip / non-finite guard (opt-in; nothing below runs unless asked for):
//   grad_sumsq_chunks  fp64 sum of squares of ranges of the flat fp32 gradient buffer, one fp64 partial
//                      per fixed GN_CHUNK-element chunk (a chunk never crosses a range), no atomics;
//   grad_sumsq_slots   one workgroup per slot sums that slot's chunk partials in a fixed order;
//   grad_guard_kernel  slot sums -> rec[4 + n_slots] = total_norm, clip_coef, skip, 0, slot norms;
//   adamw_ema_kernel<true>    the AdamW body with g * grad_scale * rec[1], a no-op on p / m / v / shadow
//                      (the EMA lerp still runs) when rec[2] != 0.
// Every product (double)g * (double)g is exact (24 x 24 significand bits), so only additions round.
// Longest chain of additions an element's square passes through, L = 83 + ceil(C / 256), C = the
// number of chunks of its slot (uva_grad_norm_chain_len):
//   in-thread      64  (16 float4 of the chunk body, x y z w in order) + 1 (a scalar head or tail element)
//   in-workgroup    6  (xor-shuffle tree over the 64 lanes) + 3 (the 4 wave sums, in wave order)
//   across chunks  ceil(C / 256) (thread t of the slot's workgroup adds chunks t, t + 256, ... in index
//                  order) + 6 + 3 (the same workgroup tree)
// uva_grad_guard then adds the n_slots slot sums in slot order (n_slots - 1 more for the total only).
// The order is a function of the range table alone: a relaunch is bit-equal.
#include "common.h"

namespace {

struct AdamArgs {
  float lr, b1, b2, eps, wd, step_size, bc2_sqrt, grad_scale, ema_decay;
};

template <bool GUARD>
__device__ __forceinline__ float adam_one(float pi, float gi, float& mi, float& vi, const AdamArgs& a, float coef) {
  gi *= a.grad_scale;
  if (GUARD) gi *= coef;  // the clip coefficient folds into the gradient scaling: no extra pass
  pi = pi * (1.0f - a.lr * a.wd);
  mi = mi + (1.0f - a.b1) * (gi - mi);  // lerp, as torch's foreach AdamW
  vi = vi * a.b2 + (1.0f - a.b2) * gi * gi;
  float denom = sqrtf(vi) / a.bc2_sqrt + a.eps;
  return pi - a.step_size * (mi / denom);
}

// The guard record (uva_grad_guard) as a kernel argument: empty in the plain step, so that kernel's
// argument layout and code stay what they were
template <bool GUARD>
struct GuardRec {};
template <>
struct GuardRec<true> {
  const float* rec;
};

// GUARD = false is the plain step; GUARD = true scales the gradient by rec[1] and skips on rec[2]
template <bool GUARD>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        float* __restrict__ ema, bf16* __restrict__ pbf, long long n,
                                                        AdamArgs a, GuardRec<GUARD> gr) {
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  float coef = 1.0f;
  if constexpr (GUARD) {
    coef = gr.rec[1];
    if (gr.rec[2] != 0.0f) {
      // skipped step: p, m, v and the shadow stay; the EMA still averages the (unchanged) weights,
      // as the reference's ema.step(model) runs every iteration whatever the optimizer did
      if (!ema) return;
      const float d = a.ema_decay, e = 1.0f - a.ema_decay;
      for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 ev = reinterpret_cast<const float4*>(ema)[i];
        const float4 pv = reinterpret_cast<const float4*>(p)[i];
        ev.x = ev.x * d + pv.x * e;
        ev.y = ev.y * d + pv.y * e;
        ev.z = ev.z * d + pv.z * e;
        ev.w = ev.w * d + pv.w * e;
        reinterpret_cast<float4*>(ema)[i] = ev;
      }
      const long long t = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x;
      if (t < n) ema[t] = ema[t] * d + p[t] * e;
      return;
    }
  }
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 pv = reinterpret_cast<const float4*>(p)[i];
    const float4 gv = reinterpret_cast<const float4*>(g)[i];
    float4 mv = reinterpret_cast<const float4*>(m)[i];
    float4 vv = reinterpret_cast<const float4*>(v)[i];
    pv.x = adam_one<GUARD>(pv.x, gv.x, mv.x, vv.x, a, coef);
    pv.y = adam_one<GUARD>(pv.y, gv.y, mv.y, vv.y, a, coef);
    pv.z = adam_one<GUARD>(pv.z, gv.z, mv.z, vv.z, a, coef);
    pv.w = adam_one<GUARD>(pv.w, gv.w, mv.w, vv.w, a, coef);
    reinterpret_cast<float4*>(p)[i] = pv;
    reinterpret_cast<float4*>(m)[i] = mv;
    reinterpret_cast<float4*>(v)[i] = vv;
    if (ema) {
      float4 ev = reinterpret_cast<const float4*>(ema)[i];
      const float d = a.ema_decay, e = 1.0f - a.ema_decay;
      ev.x = ev.x * d + pv.x * e;
      ev.y = ev.y * d + pv.y * e;
      ev.z = ev.z * d + pv.z * e;
      ev.w = ev.w * d + pv.w * e;
      reinterpret_cast<float4*>(ema)[i] = ev;
    }
    if (pbf) {
      bf16x4 b;
      b[0] = (bf16)(pv.x);
      b[1] = (bf16)(pv.y);
      b[2] = (bf16)(pv.z);
      b[3] = (bf16)(pv.w);
      reinterpret_cast<bf16x4*>(pbf)[i] = b;
    }
  }
  // scalar tail (< 4 elements)
  const long long t = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) {
    float mi = m[t], vi = v[t];
    float pi = adam_one<GUARD>(p[t], g[t], mi, vi, a, coef);
    p[t] = pi;
    m[t] = mi;
    v[t] = vi;
    if (ema) ema[t] = ema[t] * a.ema_decay + pi * (1.0f - a.ema_decay);
    if (pbf) pbf[t] = (bf16)pi;
  }
}

__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p,
                                                         long long n, float d) {
  const long long n4 = n >> 2;
  const long long stride = (long long)gridDim.x * blockDim.x;
  const float e = 1.0f - d;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    float4 ev = reinterpret_cast<const float4*>(ema)[i];
    const float4 pv = reinterpret_cast<const float4*>(p)[i];
    ev.x = ev.x * d + pv.x * e;
    ev.y = ev.y * d + pv.y * e;
    ev.z = ev.z * d + pv.z * e;
    ev.w = ev.w * d + pv.w * e;
    reinterpret_cast<float4*>(ema)[i] = ev;
  }
  const long long t = (n4 << 2) + (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t < n) ema[t] = ema[t] * d + p[t] * e;
}

inline unsigned grid_for(long long n4) {
  long long blocks = (n4 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 8192) blocks = 8192;  // 32 waves/CU resident; grid-stride beyond
  return (unsigned)blocks;
}

// ---- gradient sum of squares ------------------------------------------------------------------
constexpr int GN_THREADS = 256;
constexpr int GN_CHUNK = 16384;  // elements per chunk: 16 float4 per thread
constexpr int GN_BATCH = 8;      // float4 loads per batch of a thread (each guarded by the chunk's length)
constexpr int GN_MAX_RANGES = 64;
constexpr int GN_MAX_SLOTS = 16;

// the range table, passed by value (kernel arguments: 1.6 KB); chunk0[r] = index of range r's first
// chunk among all chunks, chunk0[n] = their number
struct GradRanges {
  long long off[GN_MAX_RANGES];
  long long len[GN_MAX_RANGES];
  int chunk0[GN_MAX_RANGES + 1];
  int slot[GN_MAX_RANGES];
  int n;
};

__device__ __forceinline__ double sq(float x) { return (double)x * (double)x; }

// sum over the workgroup in a fixed order (6 shuffle levels, then the 4 wave sums in wave order);
// the result is valid in thread 0
__device__ __forceinline__ double gn_block_sum(double acc) {
  __shared__ double wave_sum[GN_THREADS / 64];
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = acc;
  __syncthreads();
  return ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

__global__ __launch_bounds__(GN_THREADS) void grad_sumsq_chunks(const float* __restrict__ g, GradRanges R,
                                                                double* __restrict__ partial) {
  const int c = blockIdx.x;
  int r = 0;
  while (c >= R.chunk0[r + 1]) ++r;  // c < chunk0[n]: the launcher's grid
  const long long beg = R.off[r] + (long long)(c - R.chunk0[r]) * GN_CHUNK;
  long long cnt = R.off[r] + R.len[r] - beg;
  if (cnt > GN_CHUNK) cnt = GN_CHUNK;
  const float* q = g + beg;
  // scalar head up to the first 16-B boundary, float4 body, scalar tail: nothing outside [beg, beg + cnt) is read
  int head = (int)((4 - ((reinterpret_cast<uintptr_t>(q) >> 2) & 3)) & 3);
  if (head > cnt) head = (int)cnt;
  const int n4 = (int)((cnt - head) >> 2);
  const int tail = (int)(cnt - head) - (n4 << 2);
  const float4* q4 = reinterpret_cast<const float4*>(q + head);
  const int tid = threadIdx.x;
  double acc = 0.0;
#pragma unroll
  for (int b = 0; b < GN_CHUNK / 4 / GN_THREADS; b += GN_BATCH) {
    float4 x[GN_BATCH];
#pragma unroll
    for (int k = 0; k < GN_BATCH; ++k) {
      const int i = tid + (b + k) * GN_THREADS;
      x[k] = i < n4 ? q4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int k = 0; k < GN_BATCH; ++k) {
      acc += sq(x[k].x);
      acc += sq(x[k].y);
      acc += sq(x[k].z);
      acc += sq(x[k].w);
    }
  }
  if (tid < head) acc += sq(q[tid]);
  if (tid >= 4 && tid < 4 + tail) acc += sq(q[head + (n4 << 2) + (tid - 4)]);
  const double s = gn_block_sum(acc);
  if (tid == 0) partial[c] = s;
}

__global__ __launch_bounds__(GN_THREADS) void grad_sumsq_slots(const double* __restrict__ partial, GradRanges R,
                                                               double* __restrict__ slot_sumsq) {
  const int s = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  int base = 0;  // chunks of this slot before range r
  for (int r = 0; r < R.n; ++r) {
    if (R.slot[r] != s) continue;
    const int nc = R.chunk0[r + 1] - R.chunk0[r];
    for (int j = (tid - base) & (GN_THREADS - 1); j < nc; j += GN_THREADS) acc += partial[R.chunk0[r] + j];
    base += nc;
  }
  const double t = gn_block_sum(acc);
  if (tid == 0) slot_sumsq[s] = t;
}

// rec[0] total norm, rec[1] clip coefficient, rec[2] skip, rec[3] 0, rec[4 + i] norm of slot i.
// torch.nn.utils.clip_grad_norm_'s coefficient: min(1, max_norm / (total_norm + 1e-6)); with the guard
// off a non-finite norm gives what torch gives (0 for Inf, NaN for NaN: NaN > 1 is false)
__global__ void grad_guard_kernel(const double* __restrict__ slot_sumsq, int n_slots, float grad_scale, float max_norm,
                                  int skip_nonfinite, float* __restrict__ rec) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const double gs = (double)grad_scale;
  double tot = 0.0;
  for (int i = 0; i < n_slots; ++i) {
    const double v = slot_sumsq[i];
    tot += v;
    rec[4 + i] = (float)(sqrt(v) * gs);
  }
  const double tn = sqrt(tot) * gs;
  double coef = 1.0;
  if (max_norm > 0.0f) {
    coef = (double)max_norm / (tn + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  const bool finite = (tn - tn) == 0.0;
  rec[0] = (float)tn;
  rec[1] = (float)coef;
  rec[2] = (skip_nonfinite && !finite) ? 1.0f : 0.0f;
  rec[3] = 0.0f;
}

// host: validate the table and lay out the chunks; -> false on any invalid argument
inline bool gn_table(const long long* ranges, int n_ranges, int n_slots, long long n_total, GradRanges& R) {
  if (n_ranges < 0 || n_ranges > GN_MAX_RANGES || n_slots < 1 || n_slots > GN_MAX_SLOTS || n_total < 0) return false;
  if (n_ranges > 0 && !ranges) return false;
  R = GradRanges{};
  long long chunks = 0;
  for (int r = 0; r < n_ranges; ++r) {
    const long long off = ranges[3 * r], len = ranges[3 * r + 1], slot = ranges[3 * r + 2];
    if (off < 0 || len < 0 || off > n_total || len > n_total - off || slot < 0 || slot >= n_slots) return false;
    R.off[r] = off;
    R.len[r] = len;
    R.slot[r] = (int)slot;
    R.chunk0[r] = (int)chunks;
    chunks += (len + GN_CHUNK - 1) / GN_CHUNK;
    if (chunks > 0x7fffffffLL) return false;
  }
  for (int r = n_ranges; r <= GN_MAX_RANGES; ++r) R.chunk0[r] = (int)chunks;
  R.n = n_ranges;
  return true;
}

inline bool aligned16(const void* q) { return q == nullptr || (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// host side of both AdamW entry points: argument checks and the step's scalars
inline int adam_prepare(const float* p, const float* g, const float* m, const float* v, const float* ema,
                        const void* p_bf16, long long n, long long n_decay, float lr, float b1, float b2, float eps,
                        float wd, int step, float grad_scale, float ema_decay, AdamArgs& a) {
  if (!aligned16(p) || !aligned16(g) || !aligned16(m) || !aligned16(v) || !aligned16(ema) ||
      (p_bf16 && (reinterpret_cast<uintptr_t>(p_bf16) & 7)))
    return (int)hipErrorInvalidValue;  // group regions are 16-B aligned by construction
  if (n_decay != 0 && n_decay != n) return (int)hipErrorInvalidValue;  // one launch = one group
  double bc1 = 1.0 - pow((double)b1, (double)step);
  double bc2 = 1.0 - pow((double)b2, (double)step);
  a.lr = lr;
  a.b1 = b1;
  a.b2 = b2;
  a.eps = eps;
  a.wd = n_decay ? wd : 0.0f;
  a.step_size = (float)(lr / bc1);
  a.bc2_sqrt = (float)sqrt(bc2);
  a.grad_scale = grad_scale;
  a.ema_decay = ema_decay;
  return 0;
}

}  // namespace

extern "C" int uva_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16, long long n,
                             long long n_decay, float lr, float b1, float b2, float eps, float wd, int step,
                             float grad_scale, float ema_decay, hipStream_t s) {
  if (n <= 0) return 0;
  AdamArgs a;
  if (int rc = adam_prepare(p, g, m, v, ema, p_bf16, n, n_decay, lr, b1, b2, eps, wd, step, grad_scale, ema_decay, a))
    return rc;
  adamw_ema_kernel<false><<<dim3(grid_for(n >> 2)), 256, 0, s>>>(p, g, m, v, ema, (bf16*)p_bf16, n, a, GuardRec<false>{});
  UVA_LAUNCH_CHECK();
  return 0;
}

extern "C" int uva_adamw_ema_guarded(float* p, const float* g, float* m, float* v, float* ema, void* p_bf16,
                                     long long n, long long n_decay, float lr, float b1, float b2, float eps, float wd,
                                     int step, float grad_scale, float ema_decay, const float* rec, hipStream_t s) {
  if (!rec) return (int)hipErrorInvalidValue;
  if (n <= 0) return 0;
  AdamArgs a;
  if (int rc = adam_prepare(p, g, m, v, ema, p_bf16, n, n_decay, lr, b1, b2, eps, wd, step, grad_scale, ema_decay, a))
    return rc;
  adamw_ema_kernel<true><<<dim3(grid_for(n >> 2)), 256, 0, s>>>(p, g, m, v, ema, (bf16*)p_bf16, n, a,
                                                                GuardRec<true>{rec});
  UVA_LAUNCH_CHECK();
  return 0;
}

extern "C" long long uva_grad_norm_chunk_elems() { return GN_CHUNK; }

extern "C" long long uva_grad_norm_chain_len(long long n_chunks) {
  if (n_chunks < 0) n_chunks = 0;
  return 83 + (n_chunks + GN_THREADS - 1) / GN_THREADS;
}

extern "C" long long uva_grad_norm_workspace_bytes(long long n_total, int n_ranges) {
  if (n_total < 0 || n_ranges < 0 || n_ranges > GN_MAX_RANGES) return -1;
  // every range has at most len / GN_CHUNK + 1 chunks, and disjoint ranges sum to at most n_total
  return (long long)sizeof(double) * (n_total / GN_CHUNK + n_ranges + 1);
}

extern "C" int uva_grad_sumsq(const float* g, long long n_total, const long long* ranges, int n_ranges, int n_slots,
                              double* slot_sumsq, void* work, long long work_bytes, hipStream_t s) {
  GradRanges R;
  if (!gn_table(ranges, n_ranges, n_slots, n_total, R)) return (int)hipErrorInvalidValue;
  const int chunks = R.chunk0[GN_MAX_RANGES];
  if (!g || !slot_sumsq || !work || (reinterpret_cast<uintptr_t>(g) & 3) || (reinterpret_cast<uintptr_t>(work) & 7) ||
      (reinterpret_cast<uintptr_t>(slot_sumsq) & 7) || (long long)chunks * (long long)sizeof(double) > work_bytes)
    return (int)hipErrorInvalidValue;
  if (chunks > 0) {
    grad_sumsq_chunks<<<dim3((unsigned)chunks), GN_THREADS, 0, s>>>(g, R, (double*)work);
    UVA_LAUNCH_CHECK();
  }
  grad_sumsq_slots<<<dim3((unsigned)n_slots), GN_THREADS, 0, s>>>((const double*)work, R, slot_sumsq);
  UVA_LAUNCH_CHECK();
  return 0;
}

extern "C" int uva_grad_guard(const double* slot_sumsq, int n_slots, float grad_scale, float max_norm,
                              int skip_nonfinite, float* rec, hipStream_t s) {
  if (!slot_sumsq || !rec || n_slots < 1 || n_slots > GN_MAX_SLOTS) return (int)hipErrorInvalidValue;
  grad_guard_kernel<<<dim3(1), 64, 0, s>>>(slot_sumsq, n_slots, grad_scale, max_norm, skip_nonfinite, rec);
  UVA_LAUNCH_CHECK();
  return 0;
}

extern "C" int uva_ema_update(float* ema, const float* p, long long n, float decay, hipStream_t s) {
  if (n <= 0) return 0;
  if (!aligned16(ema) || !aligned16(p)) return (int)hipErrorInvalidValue;
  ema_update_kernel<<<dim3(grid_for(n >> 2)), 256, 0, s>>>(ema, p, n, decay);
  UVA_LAUNCH_CHECK();
  return 0;
}
