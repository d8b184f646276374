// What gemm_4w (gemm4.hip) and gemm_8w (gemm8w.hip) both mean by "the ring": the geometry of the 2-region
// LDS ring of K-tile images, the image format (128-B rows with the chunk XOR row & 7; k-major rows with
// ring_kswz), the per-lane LDS-DMA sources that write that format and the fragment reads that take it apart,
// the GROUP-8 tile raster, and the host side the two kernels share (CU count, the dW split-K plan, the
// operand checks, the entry points gemm.hip calls).  The two kernels keep the same k order inside a
// fragment (tests compare them bit for bit), so the format has this one definition.  The substep schedules
// and the epilogues differ on purpose and stay in their kernels.  Device helpers are __forceinline__: one
// copy here, no code of its own.
#pragma once
#include "common.h"

#include <algorithm>

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

// ---------------------------------------------------------------------------------------------
// geometry
// ---------------------------------------------------------------------------------------------
// BM x BN block tile staged by NW waves; a region holds the A [BM][64] and B [BN][64] images of one K-tile
template <int BM_, int BN_, int NW_>
struct RingCfg {
  static constexpr int BM = BM_, BN = BN_, NW = NW_;
  static constexpr int GA = BM / (8 * NW), GB = BN / (8 * NW), G = GA + GB;  // DMA instructions per wave per K-tile
  static constexpr int A_BYTES = BM * 128, REGION = (BM + BN) * 128, RING = 2 * REGION;
  static_assert(GA * 8 * NW == BM && GB * 8 * NW == BN, "DMA split");
};

// 16-B chunk swizzle of a k-major image row [64 k][W] (T = 1 operands), chosen so that the 8 rows
// {8g + q} a 32-lane group of ds_read_b64_tr_b16 touches (32 B each) fall on 8 distinct 32-B bank
// slots: 512-B rows (W = 256) all start on one bank -> XOR by 8 distinct even chunk offsets; 384-B rows
// (W = 192) alternate between two bank halves -> 4 offsets within 128 B suffice (and keep the XOR
// inside each 8-chunk group of the 24-chunk row).  gemm.hip's half images take the same two: 256-B rows
// (W = 128) as the 512-B rows, 128-B rows (W = 64) as the 384-B rows
template <int W>
__device__ __forceinline__ int ring_kswz(int k) {
  static_assert(W == 256 || W == 192 || W == 128 || W == 64, "row width");
  if constexpr (W == 256 || W == 128) return ((k & 3) << 1) | (((k >> 3) & 1) << 3);
  else return (((k >> 1) & 1) << 1) | (((k >> 3) & 1) << 2);
}

// tile t -> its origin (m0, n0): GROUP-8 raster over tm x tn tiles of BM x BN (8 row tiles share a column
// of B before the raster moves on, so neighbouring tiles share operand rows in L2)
template <int BM, int BN>
__device__ __forceinline__ void ring_tile(int t, int tm, int tn, int& m0, int& n0) {
  constexpr int GROUP = 8;
  const int group = t / (GROUP * tn), first_m = group * GROUP;
  const int gsz = min(tm - first_m, GROUP);
  m0 = (first_m + (t % (GROUP * tn)) % gsz) * BM;
  n0 = ((t % (GROUP * tn)) / gsz) * BN;
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA addressing: a wave-instruction (piece) fills 1 KB of an image, 16 B per lane, lane-linear in
// LDS, so the swizzle sits in the per-lane SOURCE offset.  The K-tile step is the SGPR soffset (128 B for
// T = 0, 64 rows of ld for T = 1).
// ---------------------------------------------------------------------------------------------
// T = 0 (K-contiguous operand): piece j covers image rows 8 j .. +7 of 128 B; lane l: row (l >> 3), LDS
// chunk (l & 7) <- global chunk (l & 7) ^ (row & 7)
__device__ __forceinline__ unsigned ring_src(int lane, int piece, int ld) {
  const int row = 8 * piece + (lane >> 3);
  return (unsigned)row * (unsigned)ld * 2u + (unsigned)(((lane & 7) ^ (row & 7)) * 16);
}
// T = 1: the k-major image [64][W] taken 1 KB per piece in byte order; lane l of piece j: byte
// j KB + 16 l -> (k, chunk), global chunk = chunk ^ kswz(k)
template <int W>
__device__ __forceinline__ unsigned ring_src_k(int lane, int piece, int ld) {
  const int b = piece * 1024 + lane * 16;
  const int k = b / (W * 2), c = (b % (W * 2)) >> 4;
  return (unsigned)k * (unsigned)ld * 2u + (unsigned)((c ^ ring_kswz<W>(k)) * 16);
}
// byte offset of an item's origin (uniform): T = 0 row r0, column kb; T = 1 row kb, column r0
template <int T>
__device__ __forceinline__ unsigned ring_origin(int r0, int kb, int ld) {
  return (unsigned)__builtin_amdgcn_readfirstlane(T ? (kb * ld + r0) * 2 : (r0 * ld + kb) * 2);
}
// DMA instruction i (A first) of wave w: K-tile kt (stepA / stepB bytes apart) into region r
template <typename G>
__device__ __forceinline__ void ring_dma(char* smem, int w, int r, int i, __amdgpu_buffer_rsrc_t rsA,
                                         __amdgpu_buffer_rsrc_t rsB, const unsigned (&offA)[G::GA],
                                         const unsigned (&offB)[G::GB], int kt, int stepA, int stepB) {
  if (i < G::GA)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rsA, (__attribute__((address_space(3))) void*)(smem + r * G::REGION + (w * G::GA + i) * 1024), 16,
        (int)offA[i < G::GA ? i : 0], __builtin_amdgcn_readfirstlane(kt * stepA), 0, 0);
  else
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rsB, (__attribute__((address_space(3))) void*)(smem + r * G::REGION + G::A_BYTES + (w * G::GB + i - G::GA) * 1024),
        16, (int)offB[i < G::GA ? 0 : i - G::GA], __builtin_amdgcn_readfirstlane(kt * stepB), 0, 0);
}

// ---------------------------------------------------------------------------------------------
// fragment reads: 16 rows (m or n) x 32 k, half h of a K-tile
// ---------------------------------------------------------------------------------------------
// T = 0: the lane's byte offset inside 16 image rows: row lrow = lane & 15 (the kernels keep it: passed in,
// a second copy of it changed their code), 16-B chunk 4 H + (lane >> 4) of a 128-B row (XOR row & 7:
// conflict-free ds_read_b128)
template <int H>
__device__ __forceinline__ int ring_lofs(int lane, int lrow) {
  return lrow * 128 + (((4 * H + (lane >> 4)) ^ (lrow & 7)) << 4);
}
// T = 1: two ds_read_b64_tr_b16 of the k-major image (rows k and k + 4 of the lane's quad, 4 columns each),
// the hardware transpose gathering the lane's 8 consecutive k (as gemm_8ph's frag8; the same k order as the
// T = 0 read)
__device__ __forceinline__ bf16x8 ring_read_tr(const char* a0, const char* a1) {
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, a0));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(s16x4, a1));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}
// the fragment of columns r0 .. r0 + 15 of the image img [64][W], addresses formed in full per fragment
// (gemm_8w forms the same addresses from a lane constant: see its frag_k)
template <int W>
__device__ __forceinline__ bf16x8 ring_frag_k(const char* img, int lane, int r0, int h) {
  const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
  const int k = h * 32 + g * 8 + q;
  const int col = r0 + 4 * p;
  const int c = col >> 3, o = (col & 7) * 2;
  return ring_read_tr(img + k * W * 2 + ((c ^ ring_kswz<W>(k)) << 4) + o,
                      img + (k + 4) * W * 2 + ((c ^ ring_kswz<W>(k + 4)) << 4) + o);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// number of compute units of the current device (persistent grids); cached per translation unit
static inline int ring_cus() {
  static int n = 0;
  if (n == 0) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
  }
  return n;
}

// dW products (A [K][M], B [K][N], both M- / N-contiguous; K = tokens) on 256 x 192 tiles: split-K plan --
// enough (tile, K-slice) items for one round of the chip, slices of whole 128-deep pairs, >= 4 K-tiles
// each.  splits = 0: not eligible (more than max_tiles tiles, or no room for the partial slabs)
struct RingSplit {
  int splits, kps, grid;
};
static inline RingSplit ring_plan_tt(int M, int N, int K, long long ws_floats, bool need_ws, long long max_tiles) {
  RingSplit p{0, 0, 0};
  if (K % 128 != 0 || K < 256 || M < 256 || N < 192) return p;
  const int cus = ring_cus();
  const long long tiles = (long long)((M + 255) / 256) * ((N + 191) / 192);
  if (tiles > max_tiles) return p;
  int splits = (int)std::max<long long>(1, (cus + tiles / 2) / tiles);
  if (splits > K / 256) splits = K / 256;
  while (splits > 1 && (long long)splits * M * N > ws_floats) --splits;
  if (splits == 1 && need_ws && (long long)M * N > ws_floats) return p;
  int kps = K;
  for (; splits > 1; --splits) {
    kps = ((K + splits - 1) / splits + 127) / 128 * 128;
    const int sp = (K + kps - 1) / kps;
    if (K - (sp - 1) * kps >= 256) {
      splits = sp;
      break;
    }
  }
  if (splits <= 1) {
    splits = 1;
    kps = K;
  }
  p.splits = splits;
  p.kps = kps;
  p.grid = (int)std::min<long long>(tiles * splits, cus);
  return p;
}

// operand checks of a dW product under plan p (direct: one slice written straight to C, else p.splits
// slabs of M x N to ws).  Every byte offset the kernels form (operand origins, lane offsets, the K-step
// soffset, the store offset) is a 32-bit int and the store descriptor's range stops at 0x7fff0000
static inline bool ring_tt_ok(const void* A, const void* B, const void* C, const void* ws, int M, int N, int K,
                              long long lda, long long ldb, long long ldc, const RingSplit& p, bool direct) {
  if (M <= 0 || N <= 0 || K <= 0 || p.splits == 0) return false;
  if (lda % 8 || ldb % 8 || ldc % 8 || M % 8 || N % 8 || lda < M || ldb < N) return false;
  if (((uintptr_t)A | (uintptr_t)B | (uintptr_t)C | (uintptr_t)ws) % 16) return false;
  if (2.0 * (double)K * (double)lda >= 2147483648.0 || 2.0 * (double)K * (double)ldb >= 2147483648.0) return false;
  if (direct ? (double)M * (double)ldc * 4.0 > (double)0x7fff0000
             : (double)p.splits * (double)M * (double)N * 4.0 > (double)0x7fff0000)
    return false;
  return direct || ws != nullptr;
}

// the ring kernels' entry points (called by gemm.hip's dispatch).  1 = launched, 0 = not eligible (the
// caller falls back), < 0 = -hipError.  _tt_: *reduce = 0 -> C holds alpha * A^T B; *reduce = s > 0 -> ws
// holds s fp32 partial slabs of M x N (ld N), the caller reduces them into C (alpha, beta).
// dry != 0 (uva_gemm_route): the same answer and *reduce, nothing launched
extern "C" int uva_gemm4_try(int out_dtype, const void* A, const void* B, void* C, int M, int N, int K, long long lda,
                             long long ldb, long long ldc, const float* bias, float alpha, hipStream_t s, int dry);
extern "C" int uva_gemm8w_try(int out_dtype, const void* A, const void* B, void* C, int M, int N, int K, long long lda,
                              long long ldb, long long ldc, const float* bias, float alpha, hipStream_t s, int dry);
extern "C" int uva_gemm4_tt_try(const void* A, const void* B, float* C, int M, int N, int K, long long lda,
                                long long ldb, long long ldc, float alpha, float beta, float* ws, long long ws_floats,
                                int* reduce, hipStream_t s, int dry);
extern "C" int uva_gemm8w_tt_try(const void* A, const void* B, float* C, int M, int N, int K, long long lda,
                                 long long ldb, long long ldc, float alpha, float beta, float* ws, long long ws_floats,
                                 int* reduce, hipStream_t s, int dry);
