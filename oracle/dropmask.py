"""The dropout counter hash of csrc/common.h, restated in plain numpy integer code.

Nothing here imports the package or calls a kernel: the tests pin this file against the real header
(tests/test_dropmask_cpu.py compiles common.h for the host) and then every kernel that drops against
this file (tests/test_dropmask_gpu.py), so the masks of a training step rest on one independent
statement of the hash instead of on HIP-vs-HIP agreement.

The hash (common.h "dropout mask"):
  key   = drop_key(seed64)                                  one 32-bit key per seed
  pair  = idx >> 1                                          one 32-bit hash per two elements
  first = lo32(pair) ^ (key + rotl32(pair >> 32, 11))       mod 2^32
  h     = the two-multiply finalizer of `first`
  u16   = h & 0xFFFF for even idx, h >> 16 for odd idx
  keep iff u16 >= thresh; kept values scale by 65536 / (65536 - thresh).
"""
import numpy as np

_M32 = np.uint64(0xFFFFFFFF)


def drop_params(p):
    """p -> (thresh, scale) as uva_drop_params: thresh = p * 65536 in float32, rounded half to even
    (lrintf), clamped to 1..65535; scale = the float32 value of 65536 / (65536 - thresh).
    p <= 0 -> (0, 1.0): no dropout."""
    p = np.float32(p)
    if not (p > 0):
        return 0, 1.0
    t = int(np.rint(np.float32(p * np.float32(65536.0))))  # np.rint: half to even
    t = min(max(t, 1), 65535)
    return t, float(np.float32(65536.0) / np.float32(65536 - t))


def drop_key(seed64):
    seed = int(seed64) & 0xFFFFFFFFFFFFFFFF
    k = (seed & 0xFFFFFFFF) ^ (((seed >> 32) * 0x9E3779B1) & 0xFFFFFFFF)
    k ^= k >> 16
    k = (k * 0x7FEB352D) & 0xFFFFFFFF
    k ^= k >> 15
    return k


def _mul32(x, c):
    """x * c mod 2^32 for uint64 arrays holding 32-bit values (the product stays below 2^64)"""
    return (x * np.uint64(c)) & _M32


def drop_hash(key, pair):
    """32-bit hash of each pair index (uint64 array) under a 32-bit key"""
    pair = np.asarray(pair, dtype=np.uint64)
    hi = pair >> np.uint64(32)
    rot = ((hi << np.uint64(11)) | (hi >> np.uint64(21))) & _M32
    x = (pair & _M32) ^ ((np.uint64(key) + rot) & _M32)
    x ^= x >> np.uint64(16)
    x = _mul32(x, 0x7FEB352D)
    x ^= x >> np.uint64(15)
    x = _mul32(x, 0x846CA68B)
    x ^= x >> np.uint64(16)
    return x


def keep(seed64, idx, thresh):
    """bool array: the keep decision of each flat element index (uint64 array)"""
    idx = np.asarray(idx, dtype=np.uint64)
    h = drop_hash(drop_key(seed64), idx >> np.uint64(1))
    odd = (idx & np.uint64(1)).astype(bool)
    u16 = np.where(odd, h >> np.uint64(16), h & np.uint64(0xFFFF))
    return u16 >= np.uint64(thresh)


# ---- layouts: the element index each consumer forms ----------------------------------------------
def keep_flat(seed64, M, N, thresh, base=0):
    """[M, N] keep mask of a contiguous row-major tensor: idx = base + row * N + col (the GEMM epilogues,
    act_drop_fwd, act_bwd / act_bwd_bias, layernorm_bwd_drop, softmax_fwd with M = rows, N = L)"""
    idx = np.uint64(base) + np.arange(M * N, dtype=np.uint64)
    return keep(seed64, idx, thresh).reshape(M, N)


def keep_attn(seed64, B, H, N, thresh):
    """[B, H, N, N] (query, key) keep mask of attention dropout: idx = ((b*H + h)*N + q)*N + key, as
    attn_mask_kernel (rowpair = ((bh*N + q)*N) >> 1, + key >> 1) and softmax_fwd_kernel (row * L + j with
    row = (b*H + h)*N + q, L = N) form it"""
    return keep_flat(seed64, B * H * N, N, thresh).reshape(B, H, N, N)


def plane_words(seed64, n, thresh):
    """uva_dropout_plane's packed layout: uint32 [ceil(n / 32)], bit i of word w = keep(element 32 w + i).
    The last word's bits past n are hashed like any other index (the kernel writes whole words)."""
    nw = (n + 31) // 32
    k = keep(seed64, np.arange(nw * 32, dtype=np.uint64), thresh).reshape(nw, 32).astype(np.uint64)
    return (k << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def mask_pos(k):
    """position of element k (0..63) of a 64-wide tile inside an MQ / MK word (attention_frag.h mask_pos)"""
    return ((k >> 2) & 3) * 16 + (k >> 4) * 4 + (k & 3)


def attn_planes(seed64, B, H, N, thresh):
    """(MQ, MK) uint64 [B*H, N/64, N] as uva_attn_dropmask lays them out (N % 64 == 0):
    MQ[bh][kv][q]    bit mask_pos(k) = keep(query q, key kv*64 + k)
    MK[bh][qb][key]  bit mask_pos(j) = keep(query qb*64 + j, key)"""
    nt = N // 64
    k = keep_attn(seed64, B, H, N, thresh).reshape(B * H, N, N).astype(np.uint64)
    sh = np.array([mask_pos(i) for i in range(64)], dtype=np.uint64)
    # [bh, q, kv, k] -> word per (bh, kv, q)
    mq = (k.reshape(B * H, N, nt, 64) << sh).sum(axis=3).transpose(0, 2, 1)
    # [bh, qb, j, key] -> word per (bh, qb, key)
    mk = (k.reshape(B * H, nt, 64, N) << sh[None, None, :, None]).sum(axis=2)
    return np.ascontiguousarray(mq), np.ascontiguousarray(mk)
