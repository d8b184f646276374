"""Float64 reference of uva_gemm and the comparisons of tests/test_gemm_exact_gpu.py and
tests/test_gemm_exact_cpu.py (the GPU tests compare kernels with it, the CPU controls feed the same
comparisons a reference output computed under one deliberate defect).  No GPU code here.

The op, epi_store of csrc/gemm.hip in the kernel's own order, per batch z, row, col:

    v = alpha * (a @ b^T) + bias[col];  aux = store(v);  v = act(v)
    v = keep ? v * scale : 0            keep = oracle/dropmask.keep_flat(seed, M, N, thresh, base = z M N),
                                        flat index row * N + col (never ldc)
    v *= gate[row, col]
    v = v + r                           or v * act'(r) when act >= 16 (r = a saved pre-activation)
    v += beta * C0;  out = store(v)

`epilogue_ref` returns next to `out` the magnitude S = |alpha| (|a| @ |b|^T) + |bias|, carried through the
same steps (x scale, x |gate|, + |r| or x |act'(r)|, + |beta| |C0|), that every bound is stated against, the
exact pre-activation and the aux copy.

Link 1 (no activation): operands nonzero integers in +-1..amp (dropping any one k term moves every output),
bias / residual / C0 integers, gate in {+-1/2, +-1, +-2}, alpha in {1, 1/2, -2}, beta in {0, 1, -1/2}, dropout
p = 1/2 (scale exactly 2).  Every product and partial sum is an integer below 2^24 and every epilogue step a
multiple of `grid` (the product of the dyadic denominators in play), so fp32 holds each one exactly in any
order, split or MFMA shape: an fp32 output must equal the reference bit for bit, a bf16 output the
reference rounded once to nearest even.  `assert_exact_regime` checks S / grid < 2^24 in float64.
`amp_for` sizes the operands so that bf16 outputs have most results below 256 (integers exact: a one-unit
defect shows) and a share at or above 256 with exact rounding ties (only nearest-even gives the bits):
`assert_bf16_shares`, and `assert_bf16_shares_scaled` where the dropout scale or a gate moves the 256 mark.

Link 2 (randn operands rounded to bf16): products exact in fp32, any summation order of K terms is within
(K - 1) u sum|terms|; the alpha / bias / beta steps add at most one u each (8 covers every epilogue step):
|got - ref| <= (K + 8) u S, u = 2^-24, plus 2^-8 |ref| for a bf16 output.

Link 3 (activations, link 1 operands and alpha a power of two from 1/8 to 1/128 (`act_scaling`: the
pre-activations' standard deviation at or below 3), so the pre-activation x is exact, on the grid k / 128,
|x| <= 32).
u = 2^-24 is one fp32 rounding; v_rcp_f32 and v_exp_f32 are 1 ulp = 2 u (common.h).  First order in u:
  erf_fast(y), y = x / sqrt 2 (y carries 2 u: constant + product):
    d = fma(c, |y|, 1): the c |y| term <= 3 u (y, constant, no own rounding inside the fma), d's rounding u:
    together <= 3 u since c |y| / d < 1 -- with the rcp's 2 u: t = 1 / d within 5 u.
    p(t) = t (a1 + t (a2 + t (a3 + t (a4 + t a5)))): 4 fma + 1 product; coefficient a_i passes i + 1
    roundings counting its own: |dp| <= u (W(t) + 5 |t p'(t)|), W = sum (i + 1) |a_i| t^i.
    e = exp2(k y y): the argument carries 7 u (constant, two products, y twice), exp2 its own 2 u:
    |de| <= e u (2 + 7 y^2).   erf = fma(-p, e, 1): one more u (|erf| <= 1).
    R_erf = e (W + 5 |t p'|) + p e (2 + 7 y^2) + 1;   |erf_fast - erf| <= ERF_ABS + u R_erf,
    ERF_ABS = 1.5e-7 the stated error of Abramowitz & Stegun 7.1.26.
  gelu = (0.5 x) (1 + erf): the sum and the product one u each of |gelu|:
    |d gelu| <= 0.5 |x| (ERF_ABS + u R_erf) + 2 u |gelu|.
  gelu' = fma(x, c2 e, fma(0.5, erf, 0.5)): inner fma u Phi, c2 e carries (constant, product, de) <=
    (4 + 7 y^2) u, outer fma u |gelu'|:
    |d gelu'| <= 0.5 (ERF_ABS + u R_erf) + u Phi + |x| phi(x) (4 + 7 y^2) u + u |gelu'|.
  sigmoid_fast = rcp(1 + exp2(k x)): argument 2 u (constant, product) -> E = exp(-x) within (2 + 2 |x|) u;
    the sum one u, the rcp 2 u:  |ds| <= s u (3 + (1 - s) (2 + 2 |x|)).
  silu = x s: one more u:  |d silu| <= |silu| u (4 + (1 - s) (2 + 2 |x|)).
  silu' = s (1 + x (1 - s)): a = 1 - s: da = ds + u a;  c = 1 + x a: dc = |x| da + u |x| a + u |c|;
    |d silu'| <= |c| ds + s dc + u |s c|.
  relu, relu': exact.
Forward: |got - ref| <= scale * bound(act, x) (+ 2^-8 |ref| for bf16), 0 on a dropped element; backward
(act = 16 + kind, with
dropout): |got - ref| <= |v| bound(act', r) + u |ref| (the product v act'(r)) (+ 2^-8 |ref|).
tests/test_gemm_exact_cpu.py checks float32 numpy restatements of the four functions against float64 inside
these bounds over the whole grid.
"""
import math

import dropmask
import numpy as np
import torch

from conv_ref import assert_bit_equal, expected_exact  # noqa: F401  (link 1's comparison, shared)
from edge_helpers import assert_within

U = 2.0 ** -24
F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
NONE, GELU, SILU, RELU = 0, 1, 2, 3
ERF_ABS = 1.5e-7
XMAX, XGRID = 32.0, 128.0   # link 3's pre-activation grid: multiples of 1 / XGRID up to XMAX in magnitude
_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
_C = 0.3275911


# ------------------------------------------------------------------ the reference
def act64(kind, x):
    if kind == GELU:
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if kind == SILU:
        return x * torch.sigmoid(x)
    if kind == RELU:
        return torch.where(x > 0, x, torch.zeros_like(x))
    return x


def act_grad64(kind, x):
    if kind == GELU:
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
    if kind == SILU:
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    if kind == RELU:
        return (x > 0).double()
    return torch.ones_like(x)


def store(v, dtype):
    """float64 -> the stored dtype (through fp32, then once to nearest even) -> float64"""
    return v.float().to(dtype).double()


def product(a, b):
    """a [Z, M, K], b [Z, N, K] (logical, any dtype / device) -> float64 (a @ b^T, |a| @ |b|^T), [Z, M, N]"""
    a, b = a.double(), b.double()
    return a @ b.transpose(1, 2), a.abs() @ b.abs().transpose(1, 2)


def keep_mask(seed, Z, M, N, thresh, device="cpu", with_base=True, ld=None):
    """[Z, M, N] bool keep mask: flat index z M N + row N + col.  (The controls' defects: with_base = False
    drops the batch base, ld = a leading dimension indexes with row * ld + col.)"""
    ks = []
    for z in range(Z):
        base = z * M * N if with_base else 0
        if ld is None:
            k = dropmask.keep_flat(seed, M, N, thresh, base=base)
        else:
            k = dropmask.keep_flat(seed, M, ld, thresh, base=base)[:, :N]
        ks.append(torch.from_numpy(np.ascontiguousarray(k)))
    return torch.stack(ks).to(device)


class Ref:
    __slots__ = ("out", "S", "pre", "aux", "keep", "v")


def epilogue_ref(P, Pabs, out_dtype, alpha=1.0, bias=None, act=0, drop=None, gate=None, residual=None, beta=0.0,
                 c0=None, keep=None):
    """-> Ref: out (float64, BEFORE the store), S, pre (exact pre-activation), aux (the stored pre-activation),
    keep (mask or None), v (the value entering the residual step).  P, Pabs [Z, M, N] from product();
    bias [N]; gate [M, N]; residual, c0 [Z, M, N]; drop = (seed, thresh, scale); act = kind or 16 + kind."""
    Z, M, N = P.shape
    r = Ref()
    v = alpha * P
    S = abs(alpha) * Pabs
    if bias is not None:
        v = v + bias.double()
        S = S + bias.double().abs()
    r.pre = v
    r.aux = store(v, out_dtype)
    res_grad = act - 16 if act >= 16 else 0
    v = act64(0 if act >= 16 else act, v)
    r.keep = None
    if drop is not None:
        seed, thresh, scale = drop
        r.keep = keep_mask(seed, Z, M, N, thresh, P.device) if keep is None else keep
        v = torch.where(r.keep, v * scale, torch.zeros_like(v))
        S = S * scale
    if gate is not None:
        v = v * gate.double()
        S = S * gate.double().abs()
    r.v = v
    if residual is not None:
        if res_grad:
            g = act_grad64(res_grad, residual.double())
            v, S = v * g, S * g.abs()
        else:
            v, S = v + residual.double(), S + residual.double().abs()
    if beta != 0.0:
        v, S = v + beta * c0.double(), S + abs(beta) * c0.double().abs()
    r.out, r.S = v, S
    return r


def gemm_ref(a, b, out_dtype, **epi):
    return epilogue_ref(*product(a, b), out_dtype, **epi)


# ------------------------------------------------------------------ inputs
def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)


def ints(g, amp, shape, zero=False):
    """integers in +-1..amp (zero=True: in -amp..amp), float64"""
    if zero:
        return torch.randint(-amp, amp + 1, shape, generator=g).double()
    m = torch.randint(1, amp + 1, shape, generator=g).double()
    return m * (torch.randint(0, 2, shape, generator=g).double() * 2 - 1)


def amp_for(K, alpha=1.0):
    """the largest operand amplitude in 1..16 for which the standard deviation |alpha| sqrt(K) E[x^2] of an
    output stays at or below 128 (E[x^2] = (amp + 1)(2 amp + 1) / 6 of the uniform nonzero integers): most
    outputs below 256, the tail (>= 2 sigma) at or above it"""
    amp = 1
    for cand in range(2, 17):
        if abs(alpha) * math.sqrt(K) * (cand + 1) * (2 * cand + 1) / 6 <= 128:
            amp = cand
    return amp


def act_scaling(K):
    """link 3: (amp, alpha) -- the largest amplitude in 1..4 and power of two alpha in 1/8 .. 1/128 for which the
    pre-activations alpha * (a @ b^T) have a standard deviation of at most 3"""
    for alpha in (1 / 8, 1 / 16, 1 / 32, 1 / 64, 1 / 128):
        for amp in (4, 3, 2, 1):
            if alpha * math.sqrt(K) * (amp + 1) * (2 * amp + 1) / 6 <= 3:
                return amp, alpha
    raise ValueError(f"K = {K} is too long for link 3's grid")


def exact_operands(seed, Z, M, N, K, amp):
    """link 1: a [Z, M, K], b [Z, N, K], nonzero integers in +-1..amp"""
    g = gen(seed)
    return ints(g, amp, (Z, M, K)), ints(g, amp, (Z, N, K))


def randn_operands(seed, Z, M, N, K):
    """link 2: randn rounded to bf16"""
    g = gen(seed)
    return (torch.randn((Z, M, K), generator=g).to(BF16).double(),
            torch.randn((Z, N, K), generator=g).to(BF16).double())


def gate_values(g, shape):
    vals = torch.tensor([0.5, -0.5, 1.0, -1.0, 2.0, -2.0], dtype=F64)
    return vals[torch.randint(0, 6, shape, generator=g)]


def drop_half():
    """p = 0.5 -> (thresh, scale) with the scale exactly 2"""
    thresh, scale = dropmask.drop_params(0.5)
    assert (thresh, scale) == (32768, 2.0)
    return thresh, scale


# ------------------------------------------------------------------ input conditions
def assert_exact_regime(S, ref, grid=1.0):
    """link 1: every term and partial sum is a multiple of `grid` below 2^24 grid in magnitude"""
    assert float(S.max()) / grid < 2 ** 24, (float(S.max()), grid)
    q = ref / grid
    assert torch.equal(q, torch.round(q)), "reference off the grid"


def bf16_shares(ref):
    """-> (share of |ref| < 256, share of |ref| >= 256, number of exact bf16 rounding ties)"""
    v = ref.double().abs().reshape(-1)
    big = v >= 256
    nz = v > 0
    ulp = torch.exp2(torch.floor(torch.log2(v[nz])) - 7)
    ties = (v[nz] - v[nz].float().to(BF16).double()).abs() == ulp / 2
    return float((~big).double().mean()), float(big.double().mean()), int(ties.sum())


MOST_BELOW, BIG_SHARE, MIN_TIES = 0.75, 0.002, 1


def assert_bf16_shares(ref, what=""):
    """bf16-output link 1 cases: >= 75 % of the results below 256, >= 0.2 % at or above it, at least one
    exact rounding tie among them"""
    below, big, ties = bf16_shares(ref)
    assert below >= MOST_BELOW and big >= BIG_SHARE and ties >= MIN_TIES, (what, below, big, ties)


SCALED_EXACT = 0.5


def assert_bf16_shares_scaled(ref, what="", keep=None):
    """bf16-output link 1 cases whose value passes a power-of-two factor (the dropout scale 2, a gate of 1/2 or 2)
    before it is stored: the factor moves the 256 mark with it (2 v is a bf16 number whenever v is), so the
    shares are restated on what they stand for -- more than half of the results (of the kept ones under
    dropout) exactly representable in bf16, so a one-unit defect shows; >= 0.1 % not representable, i.e.
    rounded (half of the 0.2 % asked at or above the 256 mark: on the integer grid every second value there
    needs rounding); at least one exact rounding tie"""
    v = ref.double() if keep is None else ref.double()[keep]
    exact = float((v.float().to(BF16).double() == v).double().mean())
    ties = bf16_shares(v)[2]
    assert exact >= SCALED_EXACT and 1.0 - exact >= BIG_SHARE / 2 and ties >= MIN_TIES, (what, exact, ties)


# ------------------------------------------------------------------ link 2
def link2_bound(ref, S, K, dtype):
    b = (K + 8) * U * S
    return b + 2.0 ** -8 * ref.abs() if dtype == BF16 else b


def assert_link2(got, ref, S, K, what=""):
    assert_within(got.reshape(ref.shape), ref, link2_bound(ref, S, K, got.dtype), what)


# ------------------------------------------------------------------ link 3
def _erf_terms(y):
    """float64 pieces of erf_fast at y -> (R_erf, e)"""
    ay = y.abs()
    t = 1.0 / (1.0 + _C * ay)
    p = t * (_A[0] + t * (_A[1] + t * (_A[2] + t * (_A[3] + t * _A[4]))))
    W = sum((i + 2) * abs(_A[i]) * t ** (i + 1) for i in range(5))
    tdp = sum((i + 1) * _A[i] * t ** (i + 1) for i in range(5)).abs()
    e = torch.exp(-y * y)
    return e * (W + 5 * tdp) + p * e * (2 + 7 * y * y) + 1.0


def act_bound(kind, x, grad=False):
    """per-element bound on |kernel act(x) - float64 act(x)| (grad: act') for exact fp32 x, float64"""
    x = x.double()
    if kind == GELU:
        y = x / math.sqrt(2.0)
        erf_err = ERF_ABS + U * _erf_terms(y)
        if not grad:
            return 0.5 * x.abs() * erf_err + 2 * U * act64(GELU, x).abs()
        Phi = 0.5 * (1.0 + torch.erf(y))
        xphi = x.abs() * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return 0.5 * erf_err + U * Phi + xphi * (4 + 7 * y * y) * U + U * act_grad64(GELU, x).abs()
    if kind == SILU:
        s = torch.sigmoid(x)
        ds = s * U * (3 + (1 - s) * (2 + 2 * x.abs()))
        if not grad:
            return (x * s).abs() * U * (4 + (1 - s) * (2 + 2 * x.abs()))
        a = 1 - s
        c = 1 + x * a
        da = ds + U * a
        dc = x.abs() * da + U * x.abs() * a + U * c.abs()
        return c.abs() * ds + s * dc + U * (s * c).abs()
    return torch.zeros_like(x)


def assert_act_grid(x):
    """link 3: the pre-activation is an exact multiple of 1 / XGRID inside +-XMAX"""
    assert torch.equal(x * XGRID, torch.round(x * XGRID)) and float(x.abs().max()) <= XMAX, float(x.abs().max())


def link3_fwd_bound(kind, r, scale, dtype):
    """out = act(pre) (x the dropout scale where kept): scale * bound(act, pre) (+ bf16 rounding); 0 on a
    dropped element"""
    b = scale * act_bound(kind, r.pre)
    if r.keep is not None:
        b = b * r.keep
    return b + 2.0 ** -8 * r.out.abs() if dtype == BF16 else b


def link3_bwd_bound(kind, r, pre_saved, dtype):
    """out = v * act'(pre_saved): |v| bound(act', pre_saved) + u |out| (+ bf16 rounding)"""
    b = r.v.abs() * act_bound(kind, pre_saved, grad=True) + U * r.out.abs()
    return b + 2.0 ** -8 * r.out.abs() if dtype == BF16 else b


# float32 numpy restatements of common.h (the CPU control of the counts above); _fma rounds once
def _f(x):
    return np.float32(x)


def _fma(a, b, c):
    """a * b + c rounded once to float32 (the product of two float32 is exact in float64)"""
    a, b, c = (np.asarray(v, dtype=np.float64) for v in (a, b, c))
    return (a * b + c).astype(np.float32)


def _erf_poly32(t):
    p = _fma(_f(1.061405429), t, _f(-1.453152027))
    p = _fma(p, t, _f(1.421413741))
    p = _fma(p, t, _f(-0.284496736))
    p = _fma(p, t, _f(0.254829592))
    return (p * t).astype(np.float32)


def erf_fast32(x):
    x = x.astype(np.float32)
    ax = np.abs(x)
    t = (_f(1.0) / _fma(_f(_C), ax, _f(1.0))).astype(np.float32)
    p = _erf_poly32(t)
    e = np.exp2((_f(-1.4426950408889634) * ax * ax).astype(np.float32)).astype(np.float32)
    return np.copysign(_fma(-p, e, _f(1.0)), x).astype(np.float32)


def gelu32(x):
    x = x.astype(np.float32)
    return (_f(0.5) * x * (_f(1.0) + erf_fast32((x * _f(0.70710678118654752)).astype(np.float32)))).astype(np.float32)


def gelu_grad32(x):
    x = x.astype(np.float32)
    e = np.exp2((_f(-0.72134752044448170) * x * x).astype(np.float32)).astype(np.float32)
    ax = (np.abs(x) * _f(0.70710678118654752)).astype(np.float32)
    t = (_f(1.0) / _fma(_f(_C), ax, _f(1.0))).astype(np.float32)
    p = _erf_poly32(t)
    erf_ = np.copysign(_fma(-p, e, _f(1.0)), x).astype(np.float32)
    return _fma(x, (_f(0.39894228040143268) * e).astype(np.float32), _fma(_f(0.5), erf_, _f(0.5)))


def sigmoid32(x):
    x = x.astype(np.float32)
    return (_f(1.0) / (_f(1.0) + np.exp2((_f(-1.4426950408889634) * x).astype(np.float32)))).astype(np.float32)


def silu32(x):
    return (x.astype(np.float32) * sigmoid32(x)).astype(np.float32)


def silu_grad32(x):
    x = x.astype(np.float32)
    s = sigmoid32(x)
    return (s * (_f(1.0) + x * (_f(1.0) - s))).astype(np.float32)


def old_rule(got, ref):
    """the max-norm rule of test_kernels_gpu.py / test_gemm8_gpu.py / test_gemm4_gpu.py (the controls' record)"""
    got, ref = got.double(), ref.double()
    return ((got - ref).abs().max() / (ref.abs().max() + 1e-12)).item()
