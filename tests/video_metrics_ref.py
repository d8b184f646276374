"""Float64 numpy restatement of uva_frame_metrics (csrc/video_metrics.hip; include/uva_hip.h), the inputs the GPU
tests run it on, and the comparison helper with its counted bound.  No GPU code here.

Per frame of two uint8 videos a, b [N, T, H, W, 3]:

    sse       sum over pixels and channels of (a - b)^2, an exact integer
    ssim_sum  sum over the 3 channels and the (H - 10)(W - 10) valid window positions of
              ((2 mua mub + C1)(2 sab + C2)) / ((mua^2 + mub^2 + C1)(saa + sbb + C2))
              C1 = (0.01 255)^2, C2 = (0.03 255)^2;  mua = E[a], saa = E[a a] - mua^2, sab = E[a b] - mua mub
              (population moments) under the separable 11 x 11 window g (x) g,
              g[i] = exp(-(i - 5)^2 / (2 1.5^2)) / sum  (float64; the bits ops.ssim_window() passes to the kernel).

The bound on |kernel ssim_sum - this ssim_sum| counts fp64 roundings, u = 2^-53, times the magnitudes they act
on.  Nothing in it is fitted to a measured error.  Per window position and channel, for ONE implementation:

    a window moment E[x] is two passes of 11 multiply-adds over non-negative terms (the kernel: 22 fma; numpy: a
    product and a sum per tap, still at most 11 roundings on any term per pass)     |dE| <= em E,  em = 22 u
    the products of two bytes (a a, a b, b b) are exact in float64
    maa = mua mua (mab, mbb alike): two moments and one rounding                     d_maa = (2 em + u) maa
    saa = E[a a] - maa: one rounding on operands off by em E[a a] and d_maa          d_saa = em E[aa] + d_maa + u |saa|
    N1 = (mab + mab) + C1: the doubling is exact                                     d_N1 = 2 d_mab + u N1
    N2 = (sab + sab) + C2                                                            d_N2 = 2 d_sab + u |N2|
    D1 = (maa + mbb) + C1: two roundings                                             d_D1 = d_maa + d_mbb + u (maa + mbb) + u D1
    D2 = (saa + sbb) + C2                                                            d_D2 = d_saa + d_sbb + u |saa + sbb| + u D2
    index = (N1 N2) / (D1 D2): two products and a correctly rounded division; N1, D1, D2 > 0, N2 of any sign
        d_index = |index| (d_N1 / N1 + d_D1 / D1 + d_D2 / D2 + 3 u) + N1 / (D1 D2) d_N2

and 1.001 on the total for the second-order terms.  The kernel and this restatement both round, along different
chains (fma against product-and-sum), so the comparison allows 2 d_index.  The sum of a frame: the kernel adds
3 channel values per thread, a 256-leaf tree per tile (8 levels), then per frame ceil(tiles / 256) slots per
thread and the same tree -- a chain of L = 19 + ceil(tiles / 256) additions at most; this side sums with
math.fsum (one rounding):  (L + 1) u sum |index|.

The worst cancellation is E[x x] - mu^2 near 65025 against C2 = 58.5: d_saa is about 67 u 65025 = 4.8e-10 there,
a relative 2e-11 of D2; frame_bound() asserts the condition the kernel's precision is held to, bound / (3 P) <=
1e-9 on the mean SSIM -- an fp32 chain (u = 2^-24) misses it by five orders of magnitude.
"""
import math

import numpy as np

U = 2.0 ** -53
C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2
WIN = 11
MEAN_BOUND_LIMIT = 1e-9

REGIMES = ("noise", "near", "flat255", "ramp")
DEFECTS = ("same_padding", "sample_cov", "unnormalised_window", "sigma_1", "c_swapped", "range_1", "luma", "taps_7",
           "fp32_moments", "drop_last_row", "drop_last_col", "channel_2_as_1")


def window(sigma=1.5, taps=WIN, normalise=True):
    i = np.arange(taps, dtype=np.float64) - (taps // 2)
    g = np.exp(-(i * i) / (2.0 * sigma ** 2))
    return g / g.sum() if normalise else g


def fixed_shapes():
    return [(1, 1, 11, 11), (1, 2, 11, 40), (1, 2, 40, 11), (2, 3, 12, 27)]


def tile_shapes(th, tw):
    """the shapes around the kernel's tile of window positions (th, tw)"""
    out = [(1, 1, 10 + h, 10 + w) for h in (th - 1, th, th + 1) for w in (tw - 1, tw, tw + 1)]
    return out + [(1, 1, 2 * th + 13, 3 * tw + 11)]


EVAL_SHAPE = (2, 4, 256, 256)


def make_pair(regime, shape, seed=0):
    """-> (a, b) uint8 [N, T, H, W, 3] of one data regime"""
    N, T, H, W = shape
    r = np.random.default_rng([seed, N, T, H, W, REGIMES.index(regime) if regime in REGIMES else 99])
    full = (N, T, H, W, 3)
    if regime == "noise":
        a, b = r.integers(0, 256, full), r.integers(0, 256, full)
    elif regime == "near":          # a frame against itself +-3 levels
        a = r.integers(0, 256, full)
        b = np.clip(a + r.integers(-3, 4, full), 0, 255)
    elif regime == "flat255":       # the cancellation case: E[x x] - mu^2 at 65025 against C2 = 58.5
        a = np.full(full, 255)
        b = 255 - r.integers(0, 2, full)
    elif regime == "ramp":          # a clipped ramp against the ramp + 1
        g = 2 * np.add.outer(np.arange(H), np.arange(W))[None, None, :, :, None] + \
            np.arange(3)[None, None, None, None, :] * 7 + np.arange(N * T).reshape(N, T, 1, 1, 1) * 5
        a, b = np.clip(g, 0, 255), np.clip(g + 1, 0, 255)
    else:
        raise ValueError(regime)
    return np.ascontiguousarray(a.astype(np.uint8)), np.ascontiguousarray(b.astype(np.uint8))


def filt(x, g, dtype=np.float64, same=False):
    """separable filter of x [..., H, W] in the kernel's order (along W, then along H; taps in order), every
    product and sum rounded to dtype.  valid positions, or zero-padded `same`"""
    g = np.asarray(g).astype(dtype)
    k = len(g)
    x = x.astype(dtype)
    if same:
        pad = [(0, 0)] * (x.ndim - 2) + [(k // 2, k // 2)] * 2
        x = np.pad(x, pad)
    Wo, Ho = x.shape[-1] - (k - 1), x.shape[-2] - (k - 1)
    t = np.zeros(x.shape[:-1] + (Wo,), dtype)
    for i in range(k):
        t = (t + (g[i] * x[..., i:i + Wo]).astype(dtype)).astype(dtype)
    o = np.zeros(x.shape[:-2] + (Ho, Wo), dtype)
    for i in range(k):
        o = (o + (g[i] * t[..., i:i + Ho, :]).astype(dtype)).astype(dtype)
    return o


def index_map(a, b, defect=None, with_bound=False):
    """a, b: integer-valued arrays [..., H, W] (one channel plane each) -> the SSIM index at every valid window
    position, float64 [..., H - 10, W - 10] (and its one-implementation bound d_index with with_bound)"""
    g, dtype, c1, c2, same = window(), np.float64, C1, C2, False
    if defect == "unnormalised_window":
        g = window(normalise=False)
    elif defect == "sigma_1":
        g = window(sigma=1.0)
    elif defect == "taps_7":
        g = np.concatenate([np.zeros(2), window(taps=7), np.zeros(2)])
    elif defect == "fp32_moments":
        dtype = np.float32
    elif defect == "c_swapped":
        c1, c2 = C2, C1
    elif defect == "range_1":
        c1, c2 = 0.01 ** 2, 0.03 ** 2
    elif defect == "same_padding":
        same = True
    a, b = a.astype(np.float64), b.astype(np.float64)
    mua, mub = filt(a, g, dtype, same), filt(b, g, dtype, same)
    eaa, eab, ebb = filt(a * a, g, dtype, same), filt(a * b, g, dtype, same), filt(b * b, g, dtype, same)
    maa, mab, mbb = mua * mua, mua * mub, mub * mub
    saa, sab, sbb = eaa - maa, eab - mab, ebb - mbb
    if defect == "sample_cov":
        n = float(WIN * WIN)
        saa, sab, sbb = saa * (n / (n - 1)), sab * (n / (n - 1)), sbb * (n / (n - 1))
    c1, c2 = dtype(c1), dtype(c2)
    n1, n2 = (mab + mab) + c1, (sab + sab) + c2
    d1, d2 = (maa + mbb) + c1, (saa + sbb) + c2
    idx = ((n1 * n2) / (d1 * d2)).astype(np.float64)
    if defect == "drop_last_row":
        idx = idx[..., :-1, :]
    elif defect == "drop_last_col":
        idx = idx[..., :, :-1]
    if not with_bound:
        return idx
    assert defect is None
    em = 22.0 * U
    d_maa, d_mab, d_mbb = (2 * em + U) * maa, (2 * em + U) * np.abs(mab), (2 * em + U) * mbb
    d_saa = em * eaa + d_maa + U * np.abs(saa)
    d_sab = em * eab + d_mab + U * np.abs(sab)
    d_sbb = em * ebb + d_mbb + U * np.abs(sbb)
    d_n1 = 2 * d_mab + U * n1
    d_n2 = 2 * d_sab + U * np.abs(n2)
    d_d1 = d_maa + d_mbb + U * (maa + mbb) + U * d1
    d_d2 = d_saa + d_sbb + U * np.abs(saa + sbb) + U * d2
    d_idx = np.abs(idx) * (d_n1 / n1 + d_d1 / d1 + d_d2 / d2 + 3 * U) + n1 / (d1 * d2) * d_n2
    return idx, 1.001 * d_idx


def _planes(v, defect):
    """uint8 [N, T, H, W, 3] -> float64 channel planes [N, T, C, H, W]"""
    p = np.moveaxis(v.astype(np.float64), 4, 2)
    if defect == "channel_2_as_1":
        p = p.copy()
        p[:, :, 2] = p[:, :, 1]
    elif defect == "luma":
        y = 0.299 * p[:, :, 0] + 0.587 * p[:, :, 1] + 0.114 * p[:, :, 2]
        p = np.stack([y, y, y], axis=2)
    return p


def sum_chain(H, W, tile):
    """the longest chain of additions an index passes through in the kernel's sum of a frame, + 1 for fsum here"""
    th, tw = tile
    tiles = -(-(H - 10) // th) * -(-(W - 10) // tw)
    return 19 + -(-tiles // 256) + 1


def frame_metrics(a, b, defect=None, tile=(16, 16)):
    """a, b: uint8 [N, T, H, W, 3] -> (sse int64 [N, T], ssim_sum float64 [N, T], bound float64 [N, T]): the
    restatement, and the bound on |kernel ssim_sum - ssim_sum| (None for a defect: a control has no bound)"""
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.shape[-1] == 3
    N, T, H, W, _ = a.shape
    pa, pb = _planes(a, defect), _planes(b, defect)
    d = pa - pb
    sse = np.rint((d * d).sum(axis=(2, 3, 4))).astype(np.int64)   # integers below 2^53: exact in float64
    if defect is not None:
        idx = index_map(pa, pb, defect)
        return sse, np.array([[math.fsum(idx[n, t].ravel()) for t in range(T)] for n in range(N)]), None
    idx, d_idx = index_map(pa, pb, with_bound=True)
    L = sum_chain(H, W, tile)
    ssim_sum, bound = np.empty((N, T)), np.empty((N, T))
    for n in range(N):
        for t in range(T):
            ssim_sum[n, t] = math.fsum(idx[n, t].ravel())
            bound[n, t] = 2.0 * math.fsum(d_idx[n, t].ravel()) + L * U * math.fsum(np.abs(idx[n, t]).ravel())
    assert float((bound / (3 * (H - 10) * (W - 10))).max()) <= MEAN_BOUND_LIMIT, "the bound admits a low-precision kernel"
    return sse, ssim_sum, bound


def psnr(sse, n_values):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(255.0 ** 2 * n_values / np.asarray(sse, np.float64))


def aggregate(sse, ssim_sum, H, W):
    """the log's means, restated: SSIM and PSNR over all frames and per horizon, a frame of sse == 0 at the PSNR
    of sse == 1"""
    ssim = ssim_sum / (3.0 * (H - 10) * (W - 10))
    p = psnr(np.maximum(sse, 1), 3 * H * W)
    return {"psnr": float(p.mean()), "ssim": float(ssim.mean()), "psnr_t": p.mean(axis=0).tolist(),
            "ssim_t": ssim.mean(axis=0).tolist()}


def compare(got_sse, got_ssim_sum, a, b, tile=(16, 16), ref=None):
    """the kernel's outputs (arrays [N, T]) against the restatement on a, b (uint8 [N, T, H, W, 3]; ref: a
    precomputed frame_metrics(a, b)).  sse must be equal, ssim_sum inside the counted bound.
    -> (worst |error| / bound, worst |error| of a frame's MEAN ssim); asserts both conditions"""
    sse, ssim_sum, bound = ref if ref is not None else frame_metrics(a, b, tile=tile)
    H, W = a.shape[2], a.shape[3]
    got_sse, got = np.asarray(got_sse), np.asarray(got_ssim_sum, np.float64)
    err = np.abs(got - ssim_sum)
    ratio = float((err / bound).max())
    mean_err = float((err / (3.0 * (H - 10) * (W - 10))).max())
    print(f"frame_metrics {tuple(a.shape)}: worst error / bound {ratio:.3f}, worst |mean ssim error| {mean_err:.2e} "
          f"(bound on the mean <= {float((bound / (3.0 * (H - 10) * (W - 10))).max()):.2e})")
    assert got_sse.dtype == np.int64 and np.array_equal(got_sse, sse), (got_sse, sse)
    assert np.isfinite(got).all() and ratio <= 1.0, (ratio, got, ssim_sum, bound)
    return ratio, mean_err
