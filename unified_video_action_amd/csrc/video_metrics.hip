// Frame-wise video metrics of two uint8 videos (eval/video_metrics.py; the epoch-end PSNR / SSIM):
// per frame the exact sum of squared differences and the sum of the SSIM index (Wang et al. 2004: 11 x 11
// gaussian window, valid positions only, per channel) over every window position and the three channels.
//
// One workgroup per (frame, 16 x 16 tile of window positions).  Per channel: the 26 x 26 uint8 patch of each
// operand goes to LDS as doubles (exact), the horizontal pass writes the five maps (a, b, aa, ab, bb; the
// products of two bytes are exact in fp64) for 26 rows x 16 columns, the vertical pass gives each thread the
// five window moments of its position.  Both passes are chains of 11 fma in tap order, so a moment passes
// through 22 roundings.  The index is formed with contraction off, one rounding per operation, and sab by
// the operation sequence of saa and sbb: where a and b hold equal values the numerator and the denominator
// are the same number and the index is exactly 1 (tests/video_metrics_ref.py counts the roundings).
//
// Deterministic: every tile writes (ssim partial, sse partial) to its own workspace slot, a second kernel
// adds a frame's slots in a fixed order.  No atomics.  The squared differences of a pixel are counted by
// the one tile that owns it (the tile whose 16 x 16 origin block holds it; the last tile of a row / column
// also owns the 10-pixel rim), so the integer sum is exact.
#include "common.h"

namespace {

constexpr int FM_WIN = 11;
constexpr int FM_TH = 16, FM_TW = 16;            // window positions per tile
constexpr int FM_PH = FM_TH + FM_WIN - 1;        // 26: patch rows
constexpr int FM_PW = FM_TW + FM_WIN - 1;        // 26: patch columns
constexpr int FM_THREADS = FM_TH * FM_TW;        // 256: one position per thread
constexpr double FM_C1 = (0.01 * 255.0) * (0.01 * 255.0);
constexpr double FM_C2 = (0.03 * 255.0) * (0.03 * 255.0);

struct FmArgs {
  double g[FM_WIN];
  long long sa[5], sb[5];  // element strides (n, t, y, x, c)
  int T, H, W, tiles_y, tiles_x;
};

struct FmSlot {
  double ssim;
  long long sse;
};

// the index of one position from its five moments; one rounding per operation
__device__ __forceinline__ double fm_index(double mua, double mub, double eaa, double eab, double ebb) {
#pragma clang fp contract(off)
  const double maa = mua * mua;
  const double mab = mua * mub;
  const double mbb = mub * mub;
  const double saa = eaa - maa;
  const double sab = eab - mab;
  const double sbb = ebb - mbb;
  const double num = ((mab + mab) + FM_C1) * ((sab + sab) + FM_C2);
  const double den = ((maa + mbb) + FM_C1) * ((saa + sbb) + FM_C2);
  return num / den;
}

__global__ __launch_bounds__(FM_THREADS) void frame_metrics_tiles(const uint8_t* __restrict__ a,
                                                                  const uint8_t* __restrict__ b, FmArgs A,
                                                                  FmSlot* __restrict__ slots) {
  __shared__ double pa[FM_PH][FM_PW + 1];
  __shared__ double pb[FM_PH][FM_PW + 1];
  __shared__ double hm[5][FM_PH][FM_TW + 1];
  __shared__ double red[FM_THREADS];
  __shared__ unsigned long long redi[FM_THREADS];
  const int tid = threadIdx.x;
  const int tiles = A.tiles_y * A.tiles_x;
  const long long bid = blockIdx.x;
  const long long frame = bid / tiles;
  const int tile = (int)(bid - frame * tiles);
  const int ty = tile / A.tiles_x, tx = tile - ty * A.tiles_x;
  const int y0 = ty * FM_TH, x0 = tx * FM_TW;
  const long long n = frame / A.T, t = frame - n * A.T;
  const uint8_t* fa = a + n * A.sa[0] + t * A.sa[1];
  const uint8_t* fb = b + n * A.sb[0] + t * A.sb[1];
  const int own_h = (ty == A.tiles_y - 1) ? FM_PH : FM_TH;  // patch rows / columns whose pixels this tile counts
  const int own_w = (tx == A.tiles_x - 1) ? FM_PW : FM_TW;
  const int oy = tid / FM_TW, ox = tid - oy * FM_TW;
  const bool live = (y0 + oy < A.H - (FM_WIN - 1)) && (x0 + ox < A.W - (FM_WIN - 1));
  double acc = 0.0;
  unsigned long long sq = 0;
  for (int c = 0; c < 3; ++c) {
    for (int i = tid; i < FM_PH * FM_PW; i += FM_THREADS) {
      const int r = i / FM_PW, q = i - r * FM_PW;
      const int y = y0 + r, x = x0 + q;
      int va = 0, vb = 0;
      if (y < A.H && x < A.W) {
        va = fa[y * A.sa[2] + x * A.sa[3] + c * A.sa[4]];
        vb = fb[y * A.sb[2] + x * A.sb[3] + c * A.sb[4]];
        if (r < own_h && q < own_w) {
          const int d = va - vb;
          sq += (unsigned long long)(d * d);
        }
      }
      pa[r][q] = (double)va;
      pb[r][q] = (double)vb;
    }
    __syncthreads();
    for (int i = tid; i < FM_PH * FM_TW; i += FM_THREADS) {
      const int r = i / FM_TW, q = i - r * FM_TW;
      double ha = 0.0, hb = 0.0, haa = 0.0, hab = 0.0, hbb = 0.0;
#pragma unroll
      for (int k = 0; k < FM_WIN; ++k) {
        const double va = pa[r][q + k], vb = pb[r][q + k], g = A.g[k];
        ha = fma(g, va, ha);
        hb = fma(g, vb, hb);
        haa = fma(g, va * va, haa);
        hab = fma(g, va * vb, hab);
        hbb = fma(g, vb * vb, hbb);
      }
      hm[0][r][q] = ha;
      hm[1][r][q] = hb;
      hm[2][r][q] = haa;
      hm[3][r][q] = hab;
      hm[4][r][q] = hbb;
    }
    __syncthreads();
    if (live) {
      double m[5];
#pragma unroll
      for (int j = 0; j < 5; ++j) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < FM_WIN; ++k) v = fma(A.g[k], hm[j][oy + k][ox], v);
        m[j] = v;
      }
      acc += fm_index(m[0], m[1], m[2], m[3], m[4]);
    }
    // the next channel's staging writes pa / pb only, the horizontal pass that rewrites hm comes after its
    // barrier: no barrier needed here
  }
  red[tid] = acc;
  redi[tid] = sq;
  __syncthreads();
  for (int s = FM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      redi[tid] += redi[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    FmSlot o;
    o.ssim = red[0];
    o.sse = (long long)redi[0];
    slots[bid] = o;
  }
}

// one workgroup per frame: thread i adds slots i, i + 256, ... in order, then the same fixed tree
__global__ __launch_bounds__(FM_THREADS) void frame_metrics_frames(const FmSlot* __restrict__ slots, int tiles,
                                                                   long long* __restrict__ sse,
                                                                   double* __restrict__ ssim_sum) {
  __shared__ double red[FM_THREADS];
  __shared__ unsigned long long redi[FM_THREADS];
  const int tid = threadIdx.x;
  const FmSlot* f = slots + (long long)blockIdx.x * tiles;
  double acc = 0.0;
  unsigned long long sq = 0;
  for (int i = tid; i < tiles; i += FM_THREADS) {
    acc += f[i].ssim;
    sq += (unsigned long long)f[i].sse;
  }
  red[tid] = acc;
  redi[tid] = sq;
  __syncthreads();
  for (int s = FM_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) {
      red[tid] += red[tid + s];
      redi[tid] += redi[tid + s];
    }
    __syncthreads();
  }
  if (tid == 0) {
    ssim_sum[blockIdx.x] = red[0];
    sse[blockIdx.x] = (long long)redi[0];
  }
}

// host: tiles per frame and in all, or false for a refused shape
inline bool fm_tiles(long long N, long long T, long long H, long long W, int& tiles_y, int& tiles_x, long long& total) {
  if (N <= 0 || T <= 0 || H < FM_WIN || W < FM_WIN || H > 0x7fffffffLL || W > 0x7fffffffLL) return false;
  const long long ty = (H - (FM_WIN - 1) + FM_TH - 1) / FM_TH, tx = (W - (FM_WIN - 1) + FM_TW - 1) / FM_TW;
  if (N > 0x7fffffffLL / T) return false;
  const long long frames = N * T;
  if (ty * tx > 0x7fffffffLL || frames > 0x7fffffffLL / (ty * tx)) return false;
  tiles_y = (int)ty;
  tiles_x = (int)tx;
  total = frames * ty * tx;
  return true;
}

}  // namespace

extern "C" int uva_frame_metrics_tile(int* th, int* tw) {
  if (!th || !tw) return (int)hipErrorInvalidValue;
  *th = FM_TH;
  *tw = FM_TW;
  return 0;
}

extern "C" long long uva_frame_metrics_workspace_bytes(int N, int T, int H, int W) {
  int ty, tx;
  long long total;
  if (!fm_tiles(N, T, H, W, ty, tx, total)) return -1;
  return total * (long long)sizeof(FmSlot);
}

extern "C" int uva_frame_metrics(const void* a, const long long* stride_a, const void* b, const long long* stride_b,
                                 const double* window, int N, int T, int H, int W, long long* sse, double* ssim_sum,
                                 void* work, long long work_bytes, hipStream_t s) {
  FmArgs A;
  long long total;
  if (!fm_tiles(N, T, H, W, A.tiles_y, A.tiles_x, total)) return (int)hipErrorInvalidValue;
  if (!a || !b || !stride_a || !stride_b || !window || !sse || !ssim_sum || !work) return (int)hipErrorInvalidValue;
  if (work_bytes < total * (long long)sizeof(FmSlot)) return (int)hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(work) & 7) || (reinterpret_cast<uintptr_t>(sse) & 7) ||
      (reinterpret_cast<uintptr_t>(ssim_sum) & 7))
    return (int)hipErrorInvalidValue;
  for (int i = 0; i < 5; ++i) {
    if (stride_a[i] < 0 || stride_b[i] < 0) return (int)hipErrorInvalidValue;
    A.sa[i] = stride_a[i];
    A.sb[i] = stride_b[i];
  }
  for (int k = 0; k < FM_WIN; ++k) A.g[k] = window[k];
  A.T = T;
  A.H = H;
  A.W = W;
  const int tiles = A.tiles_y * A.tiles_x;
  frame_metrics_tiles<<<dim3((unsigned)total), FM_THREADS, 0, s>>>((const uint8_t*)a, (const uint8_t*)b, A,
                                                                   (FmSlot*)work);
  UVA_LAUNCH_CHECK();
  frame_metrics_frames<<<dim3((unsigned)(total / tiles)), FM_THREADS, 0, s>>>((const FmSlot*)work, tiles, sse, ssim_sum);
  UVA_LAUNCH_CHECK();
  return 0;
}
