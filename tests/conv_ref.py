"""Float64 reference of uva_conv2d and the comparisons of tests/test_conv_exact_gpu.py and
tests/test_conv_exact_cpu.py (the GPU tests compare kernels with it, the CPU controls feed the same
comparisons a reference output computed under one deliberate defect).

The op, NHWC, w stored [Co][ks][ks][Ci]:

    out = bias + residual + conv_{ks,stride,pads}(act(x * scale[n, c] + shift[n, c]))

with zero padding applied AFTER the activation.  The reference is ks * ks shifted float64 matmuls over an
explicitly zero-padded tensor (no convolution library call), and returns next to `out` the magnitude
S = conv(|a|, |w|) + |bias| + |residual| that every bound is stated against.

Link 1 (every route without SiLU): inputs on dyadic grids (`exact_case`) make every product and every
partial sum a multiple of 1/32 below 2^24 / 32, so an fp32 accumulation is exact in any order, split or
MFMA shape, and the stored output must equal the reference (rounded once to bf16, to nearest even, for a
bf16 output) bit for bit.  `assert_exact_regime` checks that input condition in float64.

Link 2 (SiLU prologue): z = x * scale + shift on the quarter grid, |z| <= 8, without the grid values
whose float64 silu(z) lies within 2^-14 (relative) of a bf16 rounding tie (`silu_excluded`), so the bf16
activated input is known exactly whatever the kernel's SiLU evaluation (error ~2e-6 at |z| <= 8, 30x
inside the margin); products a * w are exact in fp32 and only the accumulation and the output rounding
remain: |got - ref| <= 2^-8 |ref| + (ks^2 Ci + 8) u S per element, u = 2^-24.
"""
import torch

from edge_helpers import assert_within

U = 2.0 ** -24
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
SAME3 = (1, 1, 1, 1)   # (top, left, bottom, right): 3x3 / stride 1 / pad 1
DOWN = (0, 0, 1, 1)    # Downsample: F.pad(0, 1, 0, 1) + 3x3 / stride 2 / pad 0
NOPAD = (0, 0, 0, 0)   # 1x1


# ------------------------------------------------------------------ the reference
def activate(x, scale=None, shift=None, silu=False, store=None):
    """float64 act(x * scale[n, c] + shift[n, c]); `store` = the dtype the kernel stages the activated
    input in (bf16 for the bf16 routes: rounded once, to nearest even), None = unrounded"""
    a = x.double()
    if scale is not None:
        a = a * scale.double()[:, None, None, :] + shift.double()[:, None, None, :]
        if silu:
            a = a * torch.sigmoid(a)
        if store is not None:
            a = a.float().to(store).double()
    return a


def zero_pad(a, pads):
    pt, pl, pb, pr = pads
    n, H, W, C = a.shape
    ap = a.new_zeros(n, H + pt + pb, W + pl + pr, C)
    ap[:, pt:pt + H, pl:pl + W] = a
    return ap


def tap_slice(ap, kh, kw, stride, Ho, Wo):
    """the padded input pixels tap (kh, kw) reads, [n * Ho * Wo, Ci]"""
    return ap[:, kh:kh + (Ho - 1) * stride + 1:stride, kw:kw + (Wo - 1) * stride + 1:stride].reshape(-1, ap.shape[-1])


def conv_taps(ap, w, ks, stride):
    """sum over the ks * ks taps of (shifted padded input) @ (tap weights)^T, float64 -> [n, Ho, Wo, Co]"""
    n, Hp, Wp, _ = ap.shape
    Ho, Wo = (Hp - ks) // stride + 1, (Wp - ks) // stride + 1
    out = ap.new_zeros(n * Ho * Wo, w.shape[0])
    for kh in range(ks):
        for kw in range(ks):
            out += tap_slice(ap, kh, kw, stride, Ho, Wo) @ w[:, kh, kw, :].t()
    return out.view(n, Ho, Wo, w.shape[0])


def conv_ref(x, w, ks, stride, pads, bias=None, residual=None, scale=None, shift=None, silu=False, store=None):
    """-> (out, S, a): the float64 output, its magnitude S = conv(|a|, |w|) + |bias| + |residual|, and the
    activated input a"""
    a = activate(x, scale, shift, silu, store)
    w = w.double()
    out = conv_taps(zero_pad(a, pads), w, ks, stride)
    S = conv_taps(zero_pad(a.abs(), pads), w.abs(), ks, stride)
    if bias is not None:
        out = out + bias.double()
        S = S + bias.double().abs()
    if residual is not None:
        out = out + residual.double().view_as(out)
        S = S + residual.double().abs().view_as(out)
    return out, S, a


def tile_partials(stored, Co):
    """fp32 (sum, sum of squares) per (128-pixel tile, GroupNorm(32) group) of a stored output
    [n, Ho, Wo, Co], tiles = consecutive pixels of an image: what a right kernel emits, up to its own
    tile-to-pixel mapping (the CPU controls' stand-in for gn_part)"""
    o = stored.double().reshape(-1, 128, 32, Co // 32)
    return torch.stack((o.sum(dim=(1, 3)), (o * o).sum(dim=(1, 3))), dim=-1).float()


# ------------------------------------------------------------------ inputs
def _rand_int(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _grid_scale(g, vals, n, Ci):
    """scale[n, c] from `vals`, different between neighbouring channels and between neighbouring images"""
    k = len(vals)
    idx = torch.randint(0, k, (Ci,), generator=g)
    for c in range(1, Ci):
        if idx[c] == idx[c - 1]:
            idx[c] = (idx[c] + 1) % k
    idx = (idx[None, :] + torch.arange(n)[:, None]) % k
    return torch.tensor(vals, dtype=F64)[idx]


def _finish(case, dtype, device):
    f32_keys = ("bias", "scale", "shift")
    return {k: (None if v is None else v.to(F32 if k in f32_keys else dtype).to(device)) for k, v in case.items()}


def exact_case(seed, n, H, W, Ci, Co, ks, Ho, Wo, gn=False, residual=False, dtype=BF16, ci_used=None,
               device="cpu"):
    """link 1 inputs: x integers in [-8, 8], scale in {1/2, 1, 2, 4}, shift integers in [-4, 4], w integers in
    [-3, 3] / 16, bias multiples of 1/16 in [-4, 4], residual integers in [-8, 8]; channels >= ci_used of
    x and w zero (the 8-channel padded RGB frame)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = _rand_int(g, -8, 8, (n, H, W, Ci))
    w = _rand_int(g, -3, 3, (Co, ks, ks, Ci)) / 16
    if ci_used is not None:
        x[..., ci_used:] = 0
        w[..., ci_used:] = 0
    case = dict(x=x, w=w, bias=_rand_int(g, -64, 64, (Co,)) / 16,
                scale=_grid_scale(g, [0.5, 1.0, 2.0, 4.0], n, Ci) if gn else None,
                shift=_rand_int(g, -4, 4, (n, Ci)) if gn else None,
                res=_rand_int(g, -8, 8, (n, Ho, Wo, Co)) if residual else None)
    return _finish(case, dtype, device)


def silu_excluded(margin=2.0 ** -14):
    """the quarter-grid values z in [-8, 8] whose float64 silu(z) is within `margin` (relative) of the
    midpoint of two neighbouring bf16 numbers -> (excluded z values, smallest relative distance to a tie
    among the values kept)"""
    z = torch.arange(-32, 33, dtype=F64) / 4
    v = (z * torch.sigmoid(z)).abs()
    nz = v > 0
    ulp = torch.exp2(torch.floor(torch.log2(v[nz])) - 7)   # bf16: 8 significand bits
    q = v[nz] / ulp
    dist = ((q - torch.floor(q)) - 0.5).abs() * ulp / v[nz]
    bad = dist < margin
    return z[nz][bad], float(dist[~bad].min())


def silu_case(seed, n, H, W, Ci, Co, ks, Ho, Wo, residual=False, dtype=BF16, device="cpu"):
    """link 2 inputs: x integers in [-6, 6], scale in {1/4, 1/2, 1}, shift multiples of 1/4 in [-2, 2] (z on
    the quarter grid, |z| <= 8, exact in fp32), x resampled where z would land on an excluded grid value;
    w, bias, residual as in link 1"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    scale = _grid_scale(g, [0.25, 0.5, 1.0], n, Ci)
    shift = _rand_int(g, -8, 8, (n, Ci)) / 4
    x = _rand_int(g, -6, 6, (n, H, W, Ci))
    excl, _ = silu_excluded()
    for _ in range(64):
        bad = torch.isin(x * scale[:, None, None, :] + shift[:, None, None, :], excl)
        if not bad.any():
            break
        x[bad] = _rand_int(g, -6, 6, (int(bad.sum()),))
    case = dict(x=x, w=_rand_int(g, -3, 3, (Co, ks, ks, Ci)) / 16, bias=_rand_int(g, -64, 64, (Co,)) / 16,
                scale=scale, shift=shift, res=_rand_int(g, -8, 8, (n, Ho, Wo, Co)) if residual else None)
    return _finish(case, dtype, device)


# ------------------------------------------------------------------ input conditions
def assert_exact_regime(a, S):
    """link 1: every term is a multiple of 1/32 and every partial sum stays below 2^24 / 32 in magnitude, so
    fp32 holds each one exactly; the activated input is a bf16 number"""
    assert float(S.max()) * 32 < 2 ** 24, float(S.max())
    assert torch.equal(a * 2, torch.round(a * 2)), "activated input off the half-integer grid"
    assert torch.equal(a.float().to(BF16).double(), a), "activated input not exact in bf16"


def assert_silu_regime(x, scale, shift):
    """link 2: z on the quarter grid inside [-8, 8] and on no excluded value"""
    z = x.double() * scale.double()[:, None, None, :] + shift.double()[:, None, None, :]
    assert torch.equal(z * 4, torch.round(z * 4)) and float(z.abs().max()) <= 8
    assert torch.equal(z.float().double(), z)
    assert not torch.isin(z, silu_excluded()[0].to(z.device)).any(), "an excluded SiLU grid value remains"


# ------------------------------------------------------------------ comparisons
def expected_exact(ref, dtype):
    """the stored form of an exact-regime reference: itself in fp32, rounded once (nearest even) in bf16"""
    r32 = ref.float()
    assert torch.equal(r32.double(), ref), "reference not exact in fp32"
    return r32.to(dtype)


def assert_bit_equal(got, ref, what=""):
    """link 1: got (stored dtype, any shape with ref's element order) == the reference, bit for bit"""
    exp = expected_exact(ref, got.dtype).reshape(got.shape)
    if not torch.equal(got, exp):
        g, e = got.double().reshape(-1), exp.double().reshape(-1)
        bad = ~(g == e)   # a NaN (unwritten element) is bad
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at flat index {i}: "
                             f"got {float(g[i])!r} expected {float(e[i])!r}")


def silu_bound(ref, S, K):
    return 2.0 ** -8 * ref.abs() + (K + 8) * U * S


def assert_silu_close(got, ref, S, K, what=""):
    """link 2, bf16 output"""
    assert_within(got.reshape(ref.shape), ref, silu_bound(ref, S, K), what)


def f32_silu_bound(S, K):
    """fp32 route with SiLU: 2e-6 on the activation (DESIGN §2's fp32 activation figure) plus the accumulation"""
    return (2e-6 + (K + 8) * U) * S


def assert_partials(part, stored, n, Co, what=""):
    """part [tiles, 32, 2] fp32 = per-tile (sum, sum of squares) of the stored output [n, Ho, Wo, Co]: per
    (image, group) the float64 sum over the image's tiles against the float64 sums of the stored values,
    bound (T + 8) u sum|terms|, T = 128 Co / 32 terms per tile (each tile's fp32 sum; the tiles are added
    here in float64)"""
    p = part.double().cpu().reshape(n, -1, 32, 2).sum(dim=1)
    o = stored.double().cpu().reshape(n, -1, 32, Co // 32)
    T = 128 * Co // 32
    assert_within(p[..., 0], o.sum(dim=(1, 3)), (T + 8) * U * o.abs().sum(dim=(1, 3)), what + " partial sums")
    assert_within(p[..., 1], (o * o).sum(dim=(1, 3)), (T + 8) * U * (o * o).sum(dim=(1, 3)),
                  what + " partial sums of squares")


def old_rule(got, ref):
    """the max-norm rule of test_conv_halo_gpu.py (kept for the controls' record)"""
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-12)).item()
