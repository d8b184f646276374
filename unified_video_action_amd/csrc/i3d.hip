// I3D feature tower kernels (forward only): the FVD evaluation's Inception-v1 inflated to 3-D.
// Activations are channels-last [N][T][H][W][C] -- the 3-D form of the NHWC layout of conv.hip.
//  * conv3d_mfma<K333> -- bf16 implicit GEMM on v_mfma_f32_16x16x32_bf16, fp32 accumulation.  The K axis
//    is walked in 8-channel chunks (tap-major: chunk q = tap * Ci / 8 + c8), four chunks per MFMA, one
//    per 16-lane group; every lane reads its own 16 bytes of the (shifted, zero-padded) input and of
//    the [Co][kt][kh][kw][Ci] weight straight from global memory, so no column matrix exists anywhere
//    and Ci only has to be a multiple of 8.  Workgroup: 4 waves, 128 output positions x 64 output
//    channels; wave: 32 x 64 (2 x 4 accumulator tiles), next step's fragments prefetched into registers.
//    The weight is the MFMA's first operand, so a lane ends with 4 consecutive output channels of one
//    position and stores them as one vector.  K333 = the 3x3x3 / stride-1 form with compile-time taps;
//    the other instantiation takes any kernel / stride (the 7x7x7 / stride-2 stem on its 8-channel
//    padded input).
//  * conv3d_f32 -- the fp32 parity route on the VALU: a thread holds 4 positions x 4 output channels.
//  * maxpool3d, i3d_head_pool / i3d_head_mean, fvd_preprocess -- see include/uva_hip.h.
// Eval-mode BatchNorm is folded into weight and bias by the host; no kernel sees it.
#include "common.h"

#define UVA_ACT_RELU 3

extern "C" int uva_gemm(int in_dtype, int out_dtype, int ta, int tb, const void* A, const void* B, void* C, int M, int N,
                        int K, long long lda, long long ldb, long long ldc, int batch, int batch_inner, long long sAo,
                        long long sAi, long long sBo, long long sBi, long long sCo, long long sCi, const float* bias,
                        const void* residual, long long ldr, long long sRo, long long sRi, void* aux, int act,
                        float alpha, float beta, float drop_p, unsigned long long drop_seed, int res_dtype,
                        const void* gate, long long ldg, int gate_dtype, int force_generic, float* workspace,
                        long long ws_floats, hipStream_t stream);

namespace {

struct Conv3dP {
  const void* in;
  const void* w;
  void* out;
  const float* bias;
  int N, T, H, W, Ci, Co;
  int KT, KH, KW, st, sh, sw, pt, ph, pw, To, Ho, Wo;
  long long ldc, M;
  int coff, act;
};

// output position m -> (n, ot, oh, ow)
__device__ __forceinline__ void decode_pos(long long m, int To, int Ho, int Wo, int& n, int& ot, int& oh, int& ow) {
  ow = (int)(m % Wo);
  long long t = m / Wo;
  oh = (int)(t % Ho);
  t /= Ho;
  ot = (int)(t % To);
  n = (int)(t / To);
}

template <bool K333>
__global__ __launch_bounds__(256) void conv3d_mfma(Conv3dP p) {
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63, g = l >> 4, li = l & 15;
  const int KT = K333 ? 3 : p.KT, KH = K333 ? 3 : p.KH, KW = K333 ? 3 : p.KW;
  const int st = K333 ? 1 : p.st, sh = K333 ? 1 : p.sh, sw = K333 ? 1 : p.sw;
  const int NT = KT * KH * KW, C8 = p.Ci >> 3;
  const bf16* __restrict__ in = (const bf16*)p.in;
  const bf16* __restrict__ w = (const bf16*)p.w;
  const long long m0 = (long long)blockIdx.x * 128 + wv * 32;
  const int n0 = blockIdx.y * 64;

  long long abase[2];
  int it0[2], ih0[2], iw0[2];
  bool mv[2];
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const long long m = m0 + f * 16 + li;
    mv[f] = m < p.M;
    int n, ot, oh, ow;
    decode_pos(mv[f] ? m : 0, p.To, p.Ho, p.Wo, n, ot, oh, ow);
    it0[f] = ot * st - p.pt;
    ih0[f] = oh * sh - p.ph;
    iw0[f] = ow * sw - p.pw;
    abase[f] = (long long)n * p.T * p.H * p.W;
  }
  const bf16* wp[4];
  bool cv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int co = n0 + j * 16 + li;
    cv[j] = co < p.Co;
    wp[j] = w + (long long)(cv[j] ? co : 0) * NT * p.Ci;
  }
  // this lane's chunk of the current step: q = 4 step + g = tap * C8 + c8
  int c8 = g % C8, tap = g / C8;
  int kw = tap % KW, kh = (tap / KW) % KH, kt = tap / (KW * KH);
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

  auto load = [&](bf16x8(&a)[2], bf16x8(&b)[4]) {
    const bool tv = tap < NT;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const int it = it0[f] + kt, ih = ih0[f] + kh, iw = iw0[f] + kw;
      const bool ok = tv && mv[f] && (unsigned)it < (unsigned)p.T && (unsigned)ih < (unsigned)p.H &&
                      (unsigned)iw < (unsigned)p.W;
      a[f] = zero;
      if (ok) a[f] = *(const bf16x8*)(in + (abase[f] + ((long long)it * p.H + ih) * p.W + iw) * p.Ci + c8 * 8);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      b[j] = zero;
      if (tv && cv[j]) b[j] = *(const bf16x8*)(wp[j] + (long long)tap * p.Ci + c8 * 8);
    }
  };
  auto advance = [&] {
    c8 += 4;
    while (c8 >= C8) {
      c8 -= C8;
      ++tap;
      if (++kw == KW) {
        kw = 0;
        if (++kh == KH) {
          kh = 0;
          ++kt;
        }
      }
    }
  };

  f32x4 acc[2][4];
#pragma unroll
  for (int f = 0; f < 2; ++f)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[f][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int steps = (NT * C8 + 3) >> 2;
  bf16x8 a[2], b[4], an[2], bn[4];
  load(a, b);
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) {
      advance();
      load(an, bn);
    }
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[f][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j], a[f], acc[f][j], 0, 0, 0);
#pragma unroll
    for (int f = 0; f < 2; ++f) a[f] = an[f];
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = bn[j];
  }

  // lane: position li of tile f, output channels n0 + 16 j + 4 g .. + 3
  bf16* out = (bf16*)p.out;
#pragma unroll
  for (int f = 0; f < 2; ++f) {
    const long long m = m0 + f * 16 + li;
    if (!mv[f]) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int co = n0 + j * 16 + 4 * g;
      if (co >= p.Co) continue;
      bf16x4 o;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[f][j][r] + (p.bias ? p.bias[co + r] : 0.f);
        if (p.act == UVA_ACT_RELU) v = v > 0.f ? v : 0.f;
        o[r] = (bf16)v;
      }
      *(bf16x4*)(out + m * p.ldc + p.coff + co) = o;
    }
  }
}

// thread: 4 output positions (m0 + pl + 16 i) x 4 output channels; workgroup: 64 positions x 64 channels.
// Every output accumulates its taps in (kt, kh, kw, ci) order; a tap outside the input adds exact zeros.
__global__ __launch_bounds__(256) void conv3d_f32(Conv3dP p) {
  const int cg = threadIdx.x & 15, pl = threadIdx.x >> 4;
  const long long m0 = (long long)blockIdx.x * 64 + pl;
  const int co = blockIdx.y * 64 + cg * 4;
  if (co >= p.Co) return;
  const float* __restrict__ in = (const float*)p.in;
  const float* __restrict__ w = (const float*)p.w;
  long long abase[4];
  int it0[4], ih0[4], iw0[4];
  bool mv[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long m = m0 + 16 * i;
    mv[i] = m < p.M;
    int n, ot, oh, ow;
    decode_pos(mv[i] ? m : 0, p.To, p.Ho, p.Wo, n, ot, oh, ow);
    it0[i] = ot * p.st - p.pt;
    ih0[i] = oh * p.sh - p.ph;
    iw0[i] = ow * p.sw - p.pw;
    abase[i] = (long long)n * p.T * p.H * p.W;
  }
  const int NT = p.KT * p.KH * p.KW;
  const long long wrow = (long long)NT * p.Ci;
  const float* wq = w + (long long)co * wrow;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[i][r] = 0.f;
  for (int kt = 0; kt < p.KT; ++kt)
    for (int kh = 0; kh < p.KH; ++kh)
      for (int kw = 0; kw < p.KW; ++kw, wq += p.Ci) {
        const float* ip[4];
        bool ok[4];
        bool any = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int it = it0[i] + kt, ih = ih0[i] + kh, iw = iw0[i] + kw;
          ok[i] = mv[i] && (unsigned)it < (unsigned)p.T && (unsigned)ih < (unsigned)p.H && (unsigned)iw < (unsigned)p.W;
          ip[i] = in + (ok[i] ? (abase[i] + ((long long)it * p.H + ih) * p.W + iw) * p.Ci : 0);
          any |= ok[i];
        }
        if (!any) continue;
        for (int ci = 0; ci < p.Ci; ci += 4) {
          f32x4 x[4], ww[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            x[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (ok[i]) x[i] = *(const f32x4*)(ip[i] + ci);
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) ww[r] = *(const f32x4*)(wq + r * wrow + ci);
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              acc[i][r] = fmaf(x[i][0], ww[r][0], acc[i][r]);
              acc[i][r] = fmaf(x[i][1], ww[r][1], acc[i][r]);
              acc[i][r] = fmaf(x[i][2], ww[r][2], acc[i][r]);
              acc[i][r] = fmaf(x[i][3], ww[r][3], acc[i][r]);
            }
        }
      }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (!mv[i]) continue;
    f32x4 o;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v = acc[i][r] + (p.bias ? p.bias[co + r] : 0.f);
      if (p.act == UVA_ACT_RELU) v = v > 0.f ? v : 0.f;
      o[r] = v;
    }
    *(f32x4*)((float*)p.out + (m0 + 16 * i) * p.ldc + p.coff + co) = o;
  }
}

// the launcher's selection: 0 conv3d_f32, 1 conv3d_mfma<true> (3x3x3 / stride 1), 2 conv3d_mfma<false>;
// < 0: -hipError.  launch = false stops before the launch (uva_conv3d_route).
int conv3d_dispatch(int dtype, const void* in, const void* w, void* out, const float* bias, int N, int T, int H, int W,
                    int Ci, int Co, int KT, int KH, int KW, int st, int sh, int sw, int pt, int ph, int pw, int To,
                    int Ho, int Wo, long long ldc, int coff, int act, bool launch, hipStream_t stream) {
  const int bad = -(int)hipErrorInvalidValue;
  if (!in || !w || !out) return bad;
  if (dtype != UVA_DT_F32 && dtype != UVA_DT_BF16) return bad;
  if (act != 0 && act != UVA_ACT_RELU) return bad;
  if (N < 1 || T < 1 || H < 1 || W < 1 || Ci < 1 || Co < 1 || KT < 1 || KH < 1 || KW < 1 || st < 1 || sh < 1 || sw < 1 ||
      To < 1 || Ho < 1 || Wo < 1 || pt < 0 || ph < 0 || pw < 0 || coff < 0 || ldc < (long long)coff + Co)
    return bad;
  // every window starts inside the front-padded input, so a tap index never runs past 2^31
  if ((long long)(To - 1) * st - pt >= T || (long long)(Ho - 1) * sh - ph >= H || (long long)(Wo - 1) * sw - pw >= W)
    return bad;
  const long long M = (long long)N * To * Ho * Wo;
  if ((M + 63) / 64 > 0x7fffffffLL) return bad;
  if ((Co & 3) || (ldc & 3) || (coff & 3)) return bad;  // 4-channel vector stores
  if (bias && ((uintptr_t)bias & 3)) return bad;
  Conv3dP p = {in, w, out, bias, N, T, H, W, Ci, Co, KT, KH, KW, st, sh, sw, pt, ph, pw, To, Ho, Wo, ldc, M, coff, act};
  const dim3 blk(256);
  if (dtype == UVA_DT_F32) {
    if ((Ci & 3) || (((uintptr_t)in | (uintptr_t)w | (uintptr_t)out) & 15)) return bad;
    if (launch) hipLaunchKernelGGL(conv3d_f32, dim3((unsigned)((M + 63) / 64), (Co + 63) / 64), blk, 0, stream, p);
    return 0;
  }
  if ((Ci & 7) || (((uintptr_t)in | (uintptr_t)w) & 15) || ((uintptr_t)out & 7)) return bad;
  const dim3 grid((unsigned)((M + 127) / 128), (Co + 63) / 64);
  if (KT == 3 && KH == 3 && KW == 3 && st == 1 && sh == 1 && sw == 1) {
    if (launch) hipLaunchKernelGGL(conv3d_mfma<true>, grid, blk, 0, stream, p);
    return 1;
  }
  if (launch) hipLaunchKernelGGL(conv3d_mfma<false>, grid, blk, 0, stream, p);
  return 2;
}

// ---- max pool, zero padding ---------------------------------------------------------------------------
// one thread per (output position, 4 channels); a window position outside the input contributes 0
template <typename T, typename V4>
__global__ __launch_bounds__(256) void maxpool3d_k(const T* __restrict__ x, T* __restrict__ y, int N, int Ti, int H, int W,
                                                   int C, int KT, int KH, int KW, int st, int sh, int sw, int pt,
                                                   int ph, int pw, int To, int Ho, int Wo, long long total) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int C4 = C >> 2;
  const int c = (int)(i % C4) * 4;
  int n, ot, oh, ow;
  decode_pos(i / C4, To, Ho, Wo, n, ot, oh, ow);
  float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  for (int kt = 0; kt < KT; ++kt) {
    const int it = ot * st + kt - pt;
    for (int kh = 0; kh < KH; ++kh) {
      const int ih = oh * sh + kh - ph;
      for (int kw = 0; kw < KW; ++kw) {
        const int iw = ow * sw + kw - pw;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if ((unsigned)it < (unsigned)Ti && (unsigned)ih < (unsigned)H && (unsigned)iw < (unsigned)W) {
          const V4 q = *(const V4*)(x + ((((long long)n * Ti + it) * H + ih) * W + iw) * C + c);
#pragma unroll
          for (int r = 0; r < 4; ++r) v[r] = (float)q[r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) m[r] = fmaxf(m[r], v[r]);
      }
    }
  }
  V4 o;
#pragma unroll
  for (int r = 0; r < 4; ++r) o[r] = (T)m[r];
  *(V4*)(y + (i / C4) * C + c) = o;
}

// ---- head: AvgPool3d([2, 7, 7], stride 1) and the time mean ---------------------------------------------
// pooled[n][t][c] = (sum over x[n][t .. t + 1][0 .. 6][0 .. 6][c]) / 98, t < T - 1; one thread per element
template <typename T>
__global__ __launch_bounds__(256) void i3d_head_pool(const T* __restrict__ x, float* __restrict__ pooled, int N, int Tn,
                                                     int C) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= (long long)N * (Tn - 1) * C) return;
  const int c = (int)(i % C);
  const int t = (int)((i / C) % (Tn - 1)), n = (int)(i / C / (Tn - 1));
  const T* px = x + ((long long)n * Tn + t) * 49 * C + c;
  float s = 0.f;
  for (int k = 0; k < 98; ++k) s += (float)px[(long long)k * C];
  pooled[i] = s / 98.0f;
}
// out[n][k] = (sum_t lg[n][t][k]) / Tm
__global__ __launch_bounds__(256) void i3d_head_mean(const float* __restrict__ lg, float* __restrict__ out, int N, int Tm,
                                                     int K) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= N * K) return;
  const int k = i % K, n = i / K;
  float s = 0.f;
  for (int t = 0; t < Tm; ++t) s += lg[((long long)n * Tm + t) * K + k];
  out[i] = s / (float)Tm;
}

// ---- FVD preprocess -------------------------------------------------------------------------------------
// uint8 [B T][Hin][Win][3] -> [B T][S][S][Cpad]: x / 255, bilinear (align_corners = False, no antialias) to
// Hr x Wr, centre crop S x S at (h0, w0), (v - 0.5) * 2; channels 3 .. Cpad - 1 are zero.  The source
// coordinate (2 d + 1) in / (2 out) - 1/2 is kept as the integer numerator over 2 out, so the cell index
// is exact and the weight is one correctly rounded division.
__device__ __forceinline__ void src_cell(int d, int in, int out, int& i0, int& i1, float& l1) {
  const long long num = (long long)(2 * d + 1) * in - out, den = 2LL * out;
  if (num <= 0) {
    i0 = 0;
    l1 = 0.f;
  } else {
    i0 = (int)(num / den);
    l1 = (float)(num - i0 * den) / (float)den;
  }
  i1 = i0 < in - 1 ? i0 + 1 : i0;
}
template <typename T>
__global__ __launch_bounds__(256) void fvd_preprocess_k(const unsigned char* __restrict__ v, T* __restrict__ out,
                                                        long long frames, int Hin, int Win, int Hr, int Wr, int h0,
                                                        int w0, int S, int Cpad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= frames * S * S) return;
  const int x = (int)(i % S), y = (int)((i / S) % S);
  const long long fr = i / ((long long)S * S);
  int y0, y1, x0, x1;
  float ly, lx;
  src_cell(y + h0, Hin, Hr, y0, y1, ly);
  src_cell(x + w0, Win, Wr, x0, x1, lx);
  const unsigned char* pf = v + fr * Hin * Win * 3;
  T* po = out + i * Cpad;
  const float my = 1.0f - ly, mx = 1.0f - lx;
  for (int c = 0; c < 3; ++c) {
    const float a = (float)pf[((long long)y0 * Win + x0) * 3 + c] / 255.0f;
    const float b = (float)pf[((long long)y0 * Win + x1) * 3 + c] / 255.0f;
    const float cc = (float)pf[((long long)y1 * Win + x0) * 3 + c] / 255.0f;
    const float d = (float)pf[((long long)y1 * Win + x1) * 3 + c] / 255.0f;
    const float top = fmaf(lx, b, mx * a), bot = fmaf(lx, d, mx * cc);
    const float r = fmaf(ly, bot, my * top);
    po[c] = (T)((r - 0.5f) * 2.0f);
  }
  for (int c = 3; c < Cpad; ++c) po[c] = (T)0.0f;
}

// fvd.py preprocess_single: shorter side to S, ceil on the other
int fvd_resized_size(int Hin, int Win, int S, int* Hr, int* Wr) {
  if (Hin < 1 || Win < 1 || S < 1 || !Hr || !Wr) return (int)hipErrorInvalidValue;
  const double scale = (double)S / (double)(Hin < Win ? Hin : Win);
  if (Hin < Win) {
    *Hr = S;
    *Wr = (int)ceil(Win * scale);
  } else {
    *Hr = (int)ceil(Hin * scale);
    *Wr = S;
  }
  return 0;
}

}  // namespace

extern "C" {

int uva_conv3d(int dtype, const void* in, const void* w, void* out, const float* bias, int N, int T, int H, int W, int Ci,
               int Co, int KT, int KH, int KW, int st, int sh, int sw, int pt, int ph, int pw, int To, int Ho, int Wo,
               long long ldc, int coff, int act, hipStream_t stream) {
  const int r = conv3d_dispatch(dtype, in, w, out, bias, N, T, H, W, Ci, Co, KT, KH, KW, st, sh, sw, pt, ph, pw, To, Ho,
                                Wo, ldc, coff, act, true, stream);
  if (r < 0) return -r;
  UVA_LAUNCH_CHECK();
  return 0;
}

int uva_conv3d_route(int dtype, const void* in, const void* w, void* out, const float* bias, int N, int T, int H, int W,
                     int Ci, int Co, int KT, int KH, int KW, int st, int sh, int sw, int pt, int ph, int pw, int To,
                     int Ho, int Wo, long long ldc, int coff, int act) {
  return conv3d_dispatch(dtype, in, w, out, bias, N, T, H, W, Ci, Co, KT, KH, KW, st, sh, sw, pt, ph, pw, To, Ho, Wo, ldc,
                         coff, act, false, nullptr);
}

int uva_maxpool3d(int dtype, const void* in, void* out, int N, int T, int H, int W, int C, int KT, int KH, int KW, int st,
                  int sh, int sw, int pt, int ph, int pw, int To, int Ho, int Wo, hipStream_t stream) {
  if (!in || !out || (dtype != UVA_DT_F32 && dtype != UVA_DT_BF16)) return (int)hipErrorInvalidValue;
  if (N < 1 || T < 1 || H < 1 || W < 1 || C < 4 || (C & 3) || KT < 1 || KH < 1 || KW < 1 || st < 1 || sh < 1 || sw < 1 ||
      pt < 0 || ph < 0 || pw < 0 || To < 1 || Ho < 1 || Wo < 1)
    return (int)hipErrorInvalidValue;
  if ((long long)(To - 1) * st - pt >= T || (long long)(Ho - 1) * sh - ph >= H || (long long)(Wo - 1) * sw - pw >= W)
    return (int)hipErrorInvalidValue;
  const int al = dtype == UVA_DT_F32 ? 15 : 7;
  if (((uintptr_t)in | (uintptr_t)out) & al) return (int)hipErrorInvalidValue;
  const long long total = (long long)N * To * Ho * Wo * (C >> 2);
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (dtype == UVA_DT_F32)
    hipLaunchKernelGGL((maxpool3d_k<float, f32x4>), dim3((unsigned)blocks), dim3(256), 0, stream, (const float*)in,
                       (float*)out, N, T, H, W, C, KT, KH, KW, st, sh, sw, pt, ph, pw, To, Ho, Wo, total);
  else
    hipLaunchKernelGGL((maxpool3d_k<bf16, bf16x4>), dim3((unsigned)blocks), dim3(256), 0, stream, (const bf16*)in,
                       (bf16*)out, N, T, H, W, C, KT, KH, KW, st, sh, sw, pt, ph, pw, To, Ho, Wo, total);
  UVA_LAUNCH_CHECK();
  return 0;
}

long long uva_i3d_head_workspace(int N, int T, int C, int num_classes) {
  if (N < 1 || T < 2 || C < 1 || num_classes < 1) return 0;
  return (long long)N * (T - 1) * ((long long)C + num_classes);
}

int uva_i3d_head(int dtype, const void* x, const float* w, const float* bias, float* out, int N, int T, int H, int W, int C,
                 int num_classes, float* workspace, long long ws_floats, hipStream_t stream) {
  if (!x || !w || !out || !workspace || (dtype != UVA_DT_F32 && dtype != UVA_DT_BF16)) return (int)hipErrorInvalidValue;
  if (H != 7 || W != 7 || T < 2 || N < 1 || C < 1 || num_classes < 1) return (int)hipErrorInvalidValue;
  if (ws_floats < uva_i3d_head_workspace(N, T, C, num_classes)) return (int)hipErrorInvalidValue;
  const int Tm = T - 1;
  float* pooled = workspace;
  float* lg = workspace + (long long)N * Tm * C;
  const long long np = (long long)N * Tm * C;
  if (dtype == UVA_DT_F32)
    hipLaunchKernelGGL(i3d_head_pool<float>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, (const float*)x,
                       pooled, N, T, C);
  else
    hipLaunchKernelGGL(i3d_head_pool<bf16>, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, stream, (const bf16*)x,
                       pooled, N, T, C);
  UVA_LAUNCH_CHECK();
  // logits of every pooled time position: fp32 on both routes (N (T - 1) rows only)
  const int rc = uva_gemm(UVA_DT_F32, UVA_DT_F32, 0, 0, pooled, w, lg, N * Tm, num_classes, C, C, C, num_classes, 1, 1, 0,
                          0, 0, 0, 0, 0, bias, nullptr, 0, 0, 0, nullptr, 0, 1.0f, 0.0f, 0.0f, 0ULL, 0, nullptr, 0, 0, 0,
                          nullptr, 0, stream);
  if (rc) return rc;
  hipLaunchKernelGGL(i3d_head_mean, dim3((N * num_classes + 255) / 256), dim3(256), 0, stream, lg, out, N, Tm,
                     num_classes);
  UVA_LAUNCH_CHECK();
  return 0;
}

int uva_fvd_preprocess(const void* videos, int odt, void* out, int B, int T, int Hin, int Win, int S, int Cpad,
                       hipStream_t stream) {
  if (!videos || !out || (odt != UVA_DT_F32 && odt != UVA_DT_BF16)) return (int)hipErrorInvalidValue;
  if (B < 1 || T < 1 || Cpad < 3) return (int)hipErrorInvalidValue;
  int Hr, Wr;
  if (fvd_resized_size(Hin, Win, S, &Hr, &Wr)) return (int)hipErrorInvalidValue;
  if ((uintptr_t)out & (odt == UVA_DT_F32 ? 3 : 1)) return (int)hipErrorInvalidValue;
  const int h0 = (Hr - S) / 2, w0 = (Wr - S) / 2;
  const long long frames = (long long)B * T, total = frames * S * S;
  const long long blocks = (total + 255) / 256;
  if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
  if (odt == UVA_DT_F32)
    hipLaunchKernelGGL(fvd_preprocess_k<float>, dim3((unsigned)blocks), dim3(256), 0, stream,
                       (const unsigned char*)videos, (float*)out, frames, Hin, Win, Hr, Wr, h0, w0, S, Cpad);
  else
    hipLaunchKernelGGL(fvd_preprocess_k<bf16>, dim3((unsigned)blocks), dim3(256), 0, stream,
                       (const unsigned char*)videos, (bf16*)out, frames, Hin, Win, Hr, Wr, h0, w0, S, Cpad);
  UVA_LAUNCH_CHECK();
  return 0;
}

}  // extern "C"
