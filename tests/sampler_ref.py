"""Float64 restatements of csrc/sampler.hip (uva_sampler_linear, one step of uva_sampler_persistent) and of
uva_p_sample_step, with the bounds of tests/test_sampler_exact_gpu.py and tests/test_sampler_exact_cpu.py (the
GPU tests compare kernels with it, the CPU controls feed the same comparisons a reference computed under one
deliberate `defect`).  No GPU code here.

The ops, in the kernels' own order:

  A tile (ln):  mean = sum(x) / K;  var = sum((x - mean)^2) / K;  rstd = rsqrt(var + eps)
                y = (x - mean) rstd;  t = y lnw + lnb (affine);  h = t (1 + scale) + shift;  a = bf16(h)
  A tile (plain): a = A (bf16)
  linear:       pre = a @ W^T + bias;  v = SiLU(pre) | pre;  v = res + gate v;  out = store(v)
  persistent step: xn = bf16(x);  h = xn Win^T + bin;  depth x { a1 = bf16(SiLU(tile_i(h) W1_i^T + b1_i));
                h = h + gate_i (a1 W2_i^T + b2_i) };  out = tile_f(h) Wf^T + bf;  x = p_sample(out, x)
  p_sample:     f = (v + 1) / 2;  lv = f max_log + (1 - f) min_log;  x0 = k0 x - k1 eps [clamped to +-1]
                mean = k2 x0 + k3 x;  x' = mean + k6 exp(lv / 2) noise k7

Every bound is stated against magnitude sums S = |a| @ |W|^T + |bias| (carried through gate and residual as in
gemm_ref), u = 2^-24.

Integer regime (bit equality).  Each x row is m +- 2^j with as many + as - (m a small integer, one j per
row): the sums of x and of (x - m)^2 are exact in fp32 in any order, mean = m, var = 4^j, and y = +-1 to
within rsqrt's last bits.  lnw, lnb, 1 + scale and shift are small integers, so h sits within 1e-5 of an integer of
magnitude <= 256, which bf16 holds: a is that integer whatever rsqrt's last bit (eps = 0).  With W on a dyadic
grid and dyadic bias / gate / residual every product and partial sum is a multiple of the grid below 2^24 grid
(`gemm_ref.assert_exact_regime`), so a no-SiLU output equals the reference bit for bit.  A SiLU output is held to
`gemm_ref.act_bound` on the exact pre-activation.  In the persistent kernel the fc1 pre-activations are integers in
100..332: 1 + exp2(-1.4427 x) rounds to 1 in fp32 from x = 18 on, so SiLU returns x itself and the fc1 output
a1 = bf16(x) is known exactly; fc2 and the residual stream then stay on the grid.  `assert_tile_regime` and
`assert_live_regime` assert what this paragraph claims.  The bf16 roundings of values that need rounding, with
exact ties, are those of the fc1 output (`gemm_ref.assert_bf16_shares` on the pre-activations: most below 256, a
share above it, odd ones ties), of x0 (a tie that rounds up, `ps_x0_ints`) and of x_net of uva_p_sample_step; the A
tile holds integers <= 256 by construction (a tie there could fall either way with rsqrt's last bit) and every
bf16 output of uva_sampler_linear passes SiLU first.  Across steps (`ps_case("steps")`) only column 0 of x feeds
input_proj and the final layer's output column 0 is 0, so x[:, 0] stays a power of two (times -2, -1, 2 per step)
and every step's h0 is in the regime; the other columns observe each step's eps and variance halves.

randn regime (per-element bound).  The kernel forms h in fp32, so near a bf16 rounding boundary it may round
the other way than float64.  `ln_tile` encloses the kernel's fp32 h per element, counted from its operations:
  sum of x:  every value passes at most Dm additions (2 inside a lane's float4, K / 256 across a lane's float4s,
             6 butterfly levels; the persistent kernel: 2 + 4 + 6 = 12): |mean^ - mean| <= Dm u mean|x| =: dr
             (the division by K is a power of two; 0 when the row sums exactly, `exact_sum_rows`)
  d = x - mean^:  one rounding; with an input enclosure ex on x: |d^ - d| <= ex + dr + mean(ex) + u |d|
  var:       a shift of the mean by dr adds exactly dr^2 (sum d = 0); the subtraction, the square and Dv additions
             (the persistent kernel: 16 in the lane + 6 = 22) are (3 + Dv) u relative; an input perturbation of
             root mean square q moves var by at most 2 sqrt(var) q + q^2
  rstd:      the sum var + eps one u, rsqrtf 1 ulp = 2 u:  relative 0.5 rel(var + eps) + 2 u
  y, t, h:   one rounding per product / sum (an FMA contraction only removes some)
An element whose enclosure [h - eh, h + eh] holds a bf16 rounding boundary is *ambiguous*: the kernel's a may be
either neighbour (lo, hi).  An output's bound is (K + 8) u S plus, over its ambiguous a only, |w| (hi - lo), through
SiLU (|SiLU'| <= 1.1) and the gate, plus the output rounding as in `gemm_ref.link2_bound`.  In the persistent kernel
the rule applies again at the fc1 output (its enclosure includes what the first allowance can move), at bf16(x_t),
and the enclosure of h travels from block to block and from step to step.  There (K + 8) u S of a K = 1024
product is about half a bf16 ulp of the fc1 output: 90 % of it is ambiguous, one live block's hx bound is 4-6 % of
max|hx| and a second block's is beyond the values themselves.  `forced_block` / `forced_final`
therefore restate the last block and the final layer from what the kernel itself left in the exchange buffers
(its own input rows, its own fc1 output): first-level bounds again.
"""
import math

import numpy as np
import torch

from edge_helpers import assert_within  # noqa: F401
from gemm_ref import BF16, F32, F64, SILU, U, act64, act_bound, assert_bf16_shares, gate_values, gen, ints, store

W_PS, DEPTH = 1024, 6
PS_DEPTHS = (12, 22)
SILU_LIP = 1.1     # max |SiLU'| = 1.0998
SILU_ID = 24.0     # from here on the kernel's SiLU returns x itself (1 + exp2(-1.4427 x) == 1 from x = 18)
AMBIG_CAP = 0.02   # randn cases: at most this share of A elements ambiguous


def ln_depths(K):
    d = 2 + K // 256 + 6
    return d, d


def trunc_bf16(v):
    """float64 -> bf16 by truncation (the controls' defect)"""
    b = v.float().contiguous().view(torch.int32) & -65536
    return b.view(torch.float32).double()


def rb(v, defect=None):
    return trunc_bf16(v) if defect == "trunc" else store(v, BF16)


def exact_sum_rows(x):
    """[R, 1] bool: the row's values are multiples of one power of two g with sum|x| / g < 2^24, so fp32 adds them
    exactly in any order"""
    q = x.double().numpy() * 2.0 ** 40
    qi = np.abs(q).astype(np.int64)
    ok = (qi.astype(np.float64) == np.abs(q)).all(1) & (np.abs(q).max(1) < 2.0 ** 62)
    orr = np.bitwise_or.reduce(qi, axis=1)
    g = np.maximum(orr & -orr, 1)
    ok &= np.abs(q).sum(1) / g < 2.0 ** 24
    return torch.from_numpy(ok).view(-1, 1)


class Tile:
    __slots__ = ("h", "a", "lo", "hi", "amb", "eh")


def ln_tile(x, lnw, lnb, shift, scale, eps, depths, ex=None, defect=None):
    """x [R, K] float64 (fp32 values), lnw / lnb [K] or None, shift / scale [R, K] -> Tile (float64)"""
    R, K = x.shape
    Dm, Dv = depths
    mean = x.mean(1, keepdim=True)
    d = x - mean
    var = (d * d).mean(1, keepdim=True)
    if defect == "onepass":  # fp32 E[x^2] - mean^2
        xf = x.float()
        var = ((xf * xf).mean(1, keepdim=True) - xf.mean(1, keepdim=True) ** 2).double().clamp_min(0)
    if defect == "var_km1":
        var = var * K / (K - 1)
    e0 = 0.0 if defect == "no_eps" else float(np.float32(eps))
    rstd = 1.0 / torch.sqrt(var + e0)
    y = d * rstd
    if lnw is not None:
        t = y * lnw + (0.0 if defect == "no_lnb" else lnb)
    else:
        t = y
    sh, sc = (scale, shift) if defect == "swap_mod" else (shift, scale)
    m1 = sc if defect == "scale_no1" else 1.0 + sc
    h = t * m1 + sh
    # the enclosure of the kernel's fp32 h
    ein = torch.zeros_like(x) if ex is None else ex
    dr = torch.where(exact_sum_rows(x), torch.zeros_like(mean), Dm * U * x.abs().mean(1, keepdim=True))
    ed = ein + dr + ein.mean(1, keepdim=True) + U * d.abs()
    q = torch.sqrt((ein * ein).mean(1, keepdim=True))
    dvar = 2 * torch.sqrt(var) * q + q * q + dr * dr + (3 + Dv) * U * (var + dr * dr + q * q) * 1.01
    rel = ((dvar + 2 * U * (var + e0)) / (var + e0)).clamp_max(0.5)
    rel_r = 0.5 * rel / (1 - rel) + 2 * U
    ey = rstd * ed * (1 + rel_r) + y.abs() * (rel_r + U)
    et = ey if lnw is None else lnw.abs() * ey + U * (y * lnw).abs() + U * t.abs()
    eh = m1.abs() * et + 2 * U * (t * m1).abs() + U * h.abs()
    eh = eh * 1.001 + 2 * U * h.abs()  # second-order terms; the float64 -> fp32 -> bf16 double rounding below
    r = Tile()
    r.h, r.eh = h, eh
    r.a = rb(h, "trunc" if defect == "trunc_a" else None)
    r.lo, r.hi = store(h - eh, BF16), store(h + eh, BF16)
    r.amb = r.lo != r.hi
    return r


def plain_tile(a):
    r = Tile()
    r.h = r.a = r.lo = r.hi = a
    r.amb = torch.zeros_like(a, dtype=torch.bool)
    r.eh = torch.zeros_like(a)
    return r


def enclosed_tile(v, ev, defect=None):
    """bf16 of a value known to within ev (the fc1 output, x_t)"""
    r = Tile()
    r.h, r.eh = v, ev
    r.a = rb(v, defect)
    g = torch.where(ev > 0, ev + 2 * U * v.abs(), torch.zeros_like(v))  # ev = 0: an exact fp32 value, rounded once
    r.lo, r.hi = store(v - g, BF16), store(v + g, BF16)
    r.amb = r.lo != r.hi
    return r


class Lin:
    __slots__ = ("pre", "out", "S", "acc", "allow", "err")


def linear(tile, W, bias=None, act=0, gate=None, res=None, eres=None, kslice=None):
    """out = epi(a @ W^T + bias) in float64 BEFORE the store.  err: per-element bound on |kernel fp32 value - out|
    = (K + 8) u S + allowance (through SiLU and the gate).  kslice = ("skip" | "dup", lo, hi): the controls'
    defect of one wave's K slice."""
    a, K = tile.a, tile.a.shape[1]
    r = Lin()
    P, Pabs = a @ W.t(), a.abs() @ W.abs().t()
    if kslice is not None:
        kind, k0, k1 = kslice
        part = a[:, k0:k1] @ W[:, k0:k1].t()
        P = P - part if kind == "skip" else P + part
    r.allow = (tile.hi - tile.lo) @ W.abs().t()
    r.pre = P if bias is None else P + bias
    S = Pabs if bias is None else Pabs + bias.abs()
    r.acc = (K + 8) * U * S  # the accumulation term (8 covers every epilogue step of the no-SiLU forms)
    if gate is not None:
        S = gate.abs() * S + res.abs()
        r.out = res + gate * r.pre
        # the product's and the bias's roundings sit in the 8; the last sum rounds once more on |out| <= S
        r.err = gate.abs() * (r.acc + r.allow) + U * S + (0.0 if eres is None else eres)
    elif act:
        r.out = act64(SILU, r.pre)
        r.err = SILU_LIP * (r.acc + r.allow) + act_bound(SILU, r.pre)
    else:
        r.out, r.err = r.pre, r.acc + r.allow
    r.S = S
    return r


def out_bound(lin, dtype):
    return lin.err + 2.0 ** -8 * lin.out.abs() if dtype == BF16 else lin.err


def assert_tile_regime(tile, limit=256):
    """integer regime: the reference's A tile equals its unrounded value to 1e-5, an integer of magnitude <= 256,
    and nothing is ambiguous"""
    assert float((tile.a - tile.h).abs().max()) <= 1e-5
    assert torch.equal(tile.a, torch.round(tile.a)) and 1 <= float(tile.a.abs().min()) <= float(tile.a.abs().max()) <= limit
    assert not bool(tile.amb.any())


def ambiguity(tile, lin):
    """-> (share of ambiguous A elements, mean allowance / mean (K + 8) u S)"""
    return float(tile.amb.double().mean()), float(lin.allow.mean() / lin.acc.mean().clamp_min(1e-300))


def assert_randn_conditions(tile, lin, what=""):
    share, ratio = ambiguity(tile, lin)
    assert share <= AMBIG_CAP and ratio < 1.0, (what, share, ratio)
    return share, ratio


# ------------------------------------------------------------------ p_sample
def p_sample(eps_, v, x, noise, kc, clip, e_eps=0.0, e_v=0.0, ex=0.0, defect=None):
    """kc: 8 floats (fp32 values).  -> (x', bound): expf 1 ulp = 2 u, every product / sum one u."""
    k = [float(np.float32(c)) for c in kc]
    f = v / 2 if defect == "f_no1" else (v + 1.0) / 2
    ef = 0.5 * e_v + U * f.abs()
    lv = f * k[5] + (1 - f) * k[4]
    m = (f * k[5]).abs() + ((1 - f) * k[4]).abs()
    elv = (abs(k[5]) + abs(k[4])) * ef + U * abs(k[4]) * (1 - f).abs() + 3 * U * m
    x0 = k[0] * x - k[1] * eps_
    ex0 = abs(k[0]) * ex + abs(k[1]) * e_eps + 3 * U * ((k[0] * x).abs() + (k[1] * eps_).abs())
    if clip and defect != "clip_mean":
        x0 = x0.clamp(-1, 1)
    mean = k[2] * x0 + k[3] * x
    if clip and defect == "clip_mean":
        mean = mean.clamp(-1, 1)
    em = abs(k[2]) * ex0 + abs(k[3]) * ex + 3 * U * ((k[2] * x0).abs() + (k[3] * x).abs())
    E = torch.exp(0.5 * lv)
    eE = E * (torch.expm1(0.5 * elv) + 2 * U)
    c = k[6] * noise * k[7]
    term = c * E
    et = c.abs() * eE + 3 * U * term.abs()
    xn = mean + term
    return xn, (em + et + U * xn.abs()) * 1.001


# ------------------------------------------------------------------ one persistent step
class Step:
    __slots__ = ("xn", "h0", "eh0", "hx", "ehx", "ha", "eha", "tiles", "lins", "out", "eout", "x", "ex")


def ps_abs(pack):
    return {k: pack[k].abs() for k in ("w1", "w2", "win", "wf")}


def ps_step(x, ex, pack, modk, kc, noisek, clip, eps, defect=None, stale=None, exact=False):
    """one reverse step of uva_sampler_persistent.  x [R, C] float64 (fp32 values) known to within ex; pack:
    float64 dict (w1 / w2 [depth, W, W], b1 / b2 / lnw / lnb [depth, W], win [W, C], bin [W], wf [2C, W], bfin [2C]);
    modk [R, ncol] float64 (bf16 values).  hx[i] / ha[i]: the exchange buffers' rows after block i.
    defect = (name, block) plants one of the controls' defects; stale = (block, workgroup, rows): that workgroup's 16
    columns of the block's INPUT rows come from `rows` (the previous step's).  exact: the integer regime, where
    input_proj and the final layer carry no error (asserted on the reference by the tests)."""
    name, dblk = defect if defect is not None else (None, -1)
    W = W_PS
    C = x.shape[1]
    s = Step()
    tx = enclosed_tile(x, ex, "trunc" if name == "trunc_x" else None)
    s.xn = tx.a
    li = linear(tx, pack["win"], pack["bin"])
    li.err = li.allow + (0.0 if exact else (C + 1) * U * li.S)  # C FMAs
    h, eh = li.out, li.err
    s.h0, s.eh0 = h, eh
    s.hx, s.ehx, s.ha, s.eha, s.tiles, s.lins = [], [], [], [], [], []
    for b in range(DEPTH):
        if stale is not None and stale[0] == b:
            h = h.clone()
            h[:, 16 * stale[1]:16 * stale[1] + 16] = stale[2][:, 16 * stale[1]:16 * stale[1] + 16]
        mb = b - 1 if (name == "mod_prev" and b == dblk) else b
        m = modk[:, 3 * W * mb:3 * W * mb + 3 * W]
        t1 = ln_tile(h, pack["lnw"][b], pack["lnb"][b], m[:, :W], m[:, W:2 * W], eps, PS_DEPTHS, ex=eh)
        l1 = linear(t1, pack["w1"][b], pack["b1"][b], act=SILU)
        ta = enclosed_tile(l1.out, l1.err, "trunc" if (name == "trunc_fc1" and b == dblk) else None)
        w2 = pack["w2"][b - 1] if (name == "w2_prev" and b == dblk) else pack["w2"][b]
        l2 = linear(ta, w2, pack["b2"][b], gate=m[:, 2 * W:], res=h, eres=eh)
        h, eh = l2.out, l2.err
        s.hx.append(h); s.ehx.append(eh); s.ha.append(ta.a); s.eha.append(l1.err)
        s.tiles.append((t1, ta)); s.lins.append((l1, l2))
    mf = modk[:, 3 * W * DEPTH:3 * W * DEPTH + 2 * W]
    tf = ln_tile(h, None, None, mf[:, :W], mf[:, W:], eps, PS_DEPTHS, ex=eh)
    lf = linear(tf, pack["wf"], pack["bfin"])
    out = lf.out
    if name == "drop_tile2":
        out = out.clone()
        out[:, 16:] = 0
    s.tiles.append((tf, None)); s.lins.append((lf, None))
    s.out, s.eout = out, (torch.zeros_like(out) if exact else lf.err)
    pd = name if name in ("f_no1", "clip_mean") else None
    s.x, s.ex = p_sample(out[:, :C], out[:, C:], x, noisek, kc, clip, s.eout[:, :C], s.eout[:, C:], ex, pd)
    return s


def ps_chain(x0, pack, mod, coef, noise, clip, eps, defect=None, stale_at=None, exact=False):
    """S chained steps -> list of Step.  defect = ("coef_prev", k): step k uses coef[k - 1]; stale_at = (k, block,
    workgroup): the stale-slice control."""
    x, ex, steps = x0, torch.zeros_like(x0), []
    for k in range(mod.shape[0]):
        kc = coef[k - 1] if (defect is not None and defect[0] == "coef_prev" and defect[1] == k) else coef[k]
        stale = None
        if stale_at is not None and stale_at[0] == k:
            b = stale_at[1]
            prev = steps[k - 1].hx[b - 1] if b > 0 else steps[k - 1].h0
            stale = (b, stale_at[2], prev)
        st = ps_step(x, ex, pack, mod[k], kc.tolist(), noise[k], clip, eps,
                     defect if defect is not None and defect[0] != "coef_prev" else None, stale, exact)
        steps.append(st)
        x, ex = store(st.x, F32), st.ex + U * st.x.abs()
    return steps


# ------------------------------------------------------------------ inputs
def balanced_signs(g, R, K):
    s = torch.ones(R, K, dtype=F64)
    s[:, K // 2:] = -1
    return torch.stack([s[r][torch.randperm(K, generator=g)] for r in range(R)])


def int_rows(g, R, K, jmax=3):
    """rows m +- 2^j, balanced: mean m and variance 4^j exact"""
    m = torch.randint(-3, 4, (R, 1), generator=g).double()
    j = torch.randint(0, jmax + 1, (R, 1), generator=g).double()
    return m + balanced_signs(g, R, K) * torch.exp2(j)


def away(v, k):
    """nonzero v moved k further from 0"""
    return v + k * torch.sign(v)


def int_ln_params(g, R, K, width=None):
    """integer lnw (+-2..3), lnb (-1..1) and a bf16 table [R, width] whose first 3 K columns are shift (+-17..24) |
    scale (1 + scale in +-1..4) | gate (dyadic).  t = +-lnw + lnb is in +-1..4, t (1 + scale) in +-1..16 and h in
    +-1..40: never 0 (the kernel's h at an exact 0 would be rsqrt's last bits, not 0)"""
    width = 3 * K if width is None else width
    tbl = ints(g, 7, (R, width), zero=True)
    tbl[:, :K] = away(ints(g, 8, (R, K)), 16)
    tbl[:, K:2 * K] = ints(g, 4, (R, K)) - 1
    tbl[:, 2 * K:3 * K] = gate_values(g, (R, K))
    return away(ints(g, 2, (K,)), 1), ints(g, 1, (K,), zero=True), tbl


def randn_ln_inputs(g, R, K, width=None):
    """the data of test_sampler_linear_kernel_variants: x = 3 randn + 0.5, table 0.5 randn (bf16), lnw in 0.5..1.5,
    lnb 0.1 randn"""
    width = 3 * K if width is None else width
    x = (torch.randn(R, K, generator=g) * 3 + 0.5).double()
    tbl = (torch.randn(R, width, generator=g) * 0.5).to(BF16).double()
    lnw = (torch.rand(K, generator=g) + 0.5).double()
    lnb = (torch.randn(K, generator=g) * 0.1).double()
    return x, lnw, lnb, tbl


def ln_edge_rows(x):
    """rows 0..2 of a randn x: a large common offset (mean 1e3, spread 1), a constant row, one spike"""
    x = x.clone()
    x[0] = (1e3 + (x[0] - 0.5) / 3).float().double()
    x[1] = 2.5
    x[2, x.shape[1] // 3] = 300.0
    return x


def randn_w(g, N, K):
    return (torch.randn(N, K, generator=g) / 32).to(BF16).double()


def sparse_w(g, N, K, per=16, amp=1):
    """[N, K] with `per` nonzero integers (+-1..amp) per row, one in every K / per chunk: every K slice of every
    column carries weight"""
    w = torch.zeros(N, K, dtype=F64)
    ch = K // per
    pos = torch.randint(0, ch, (N, per), generator=g) + torch.arange(per) * ch
    w.scatter_(1, pos, ints(g, amp, (N, per)))
    return w


def ps_mod_ints(g, S, R, live=None, gate_zero=False):
    """integer-regime modulation table [S, R, 20 W]: per block shift (+-7..8) | scale (1 + scale in +-1..2) | gate
    (dyadic; 0 for every block but `live` when given, 0 everywhere with gate_zero), final shift | scale"""
    W = W_PS
    mod = torch.zeros(S, R, (3 * DEPTH + 2) * W, dtype=F64)
    for b in range(DEPTH + 1):
        o = 3 * W * b
        mod[:, :, o:o + W] = away(ints(g, 2, (S, R, W)), 6)
        mod[:, :, o + W:o + 2 * W] = ints(g, 2, (S, R, W)) - 1
        if b < DEPTH and not gate_zero and (live is None or live == b):
            mod[:, :, o + 2 * W:o + 3 * W] = gate_values(g, (S, R, W))
    return mod


def ps_pack_ints(g, C, wf_scale=1.0, b1=216.0, col0=False):
    """integer-regime weights: every block its own sparse w1 (8 per row) / w2 (16 per row), lnw +-2, lnb -1..1 (t in
    +-1..3, h in +-1..14, never 0), b1 = 216 + (-4..4) (the fc1 pre-activations stay in 216 +- (4 + 8 * 14) = 100..332
    where SiLU is the identity; those above 256 need bf16 rounding, the odd ones are exact ties), b2 integers;
    col0: only x's column 0 feeds input_proj and the final layer's output column 0 is 0 (the multi-step cases:
    x[:, 0] stays a power of two from step to step); win = sigma (x) g (one balanced
    sign pattern times per-column integers g_c, g_0 = 1), bin = a constant integer row offset; wf sparse."""
    W = W_PS
    p = {}
    p["w1"] = torch.stack([sparse_w(g, W, W, per=8) for _ in range(DEPTH)])
    p["w2"] = torch.stack([sparse_w(g, W, W) for _ in range(DEPTH)])
    p["b1"] = b1 + ints(g, 4, (DEPTH, W), zero=True)
    p["b2"] = ints(g, 4, (DEPTH, W), zero=True)
    p["lnw"] = 2 * ints(g, 1, (DEPTH, W))
    p["lnb"] = ints(g, 1, (DEPTH, W), zero=True)
    gc = ints(g, 2, (C,))
    gc[0] = 1.0
    if C >= 3:
        gc[2] = gc[1]
    if col0:
        gc[1:] = 0.0
    p["win"] = balanced_signs(g, 1, W).view(W, 1) * gc.view(1, C)
    p["bin"] = torch.full((W,), 2.0, dtype=F64)
    p["wf"] = sparse_w(g, 2 * C, W, per=16, amp=2) * wf_scale
    p["bfin"] = ints(g, 4, (2 * C,), zero=True) * wf_scale
    if col0:
        p["wf"][0] = 0.0
        p["bfin"][0] = 0.0
    p["gc"] = gc
    return p


def ps_x0_ints(g, R, C, gc):
    """x0 rows with sum_c bf16(x0)[r, c] g_c = 2^j_r: h0 rows are 2 +- 2^j_r.  From C = 3 on columns 1 and 2 (one g)
    hold 259/256, an exact bf16 tie that rounds up to 260/256, and -260/256: they cancel only after a
    round-to-nearest-even of x0"""
    t = ints(g, 2, (R, C), zero=True)
    if C >= 3:
        t[:, 1], t[:, 2] = 259.0 / 256, -260.0 / 256
    t[:, 0] = 1.0 - (store(t[:, 1:], BF16) * gc[1:]).sum(1)
    j = torch.randint(0, 3, (R, 1), generator=g).double()
    return t * torch.exp2(j)


def ps_pack_randn(g, C):
    W = W_PS
    p = {}
    p["w1"] = (torch.randn(DEPTH, W, W, generator=g) / 32).to(BF16).double()
    p["w2"] = (torch.randn(DEPTH, W, W, generator=g) / 32).to(BF16).double()
    p["b1"] = (torch.randn(DEPTH, W, generator=g) * 0.1).double()
    p["b2"] = (torch.randn(DEPTH, W, generator=g) * 0.1).double()
    p["lnw"] = (torch.rand(DEPTH, W, generator=g) + 0.5).double()
    p["lnb"] = (torch.randn(DEPTH, W, generator=g) * 0.1).double()
    p["win"] = (torch.randn(W, C, generator=g) / math.sqrt(C)).to(BF16).double()
    p["bin"] = (torch.randn(W, generator=g) * 0.1).double()
    p["wf"] = (torch.randn(2 * C, W, generator=g) / 32).to(BF16).double()
    p["bfin"] = (torch.randn(2 * C, generator=g) * 0.1).double()
    return p


def ps_mod_randn(g, S, R, live=None, gate_zero=False):
    W = W_PS
    mod = (torch.randn(S, R, (3 * DEPTH + 2) * W, generator=g) * 0.5).to(BF16).double()
    for b in range(DEPTH):
        if gate_zero or (live is not None and live != b):
            mod[:, :, 3 * W * b + 2 * W:3 * W * b + 3 * W] = 0
    return mod


def ps_coef_randn(g, S):
    """per-step schedule rows of plausible size, all different"""
    c = torch.empty(S, 8)
    for k in range(S):
        c[k] = torch.tensor([1.3 - 0.1 * k, 0.7 - 0.1 * k, 0.4 + 0.05 * k, 0.55 - 0.05 * k, -6.0 + k, -3.5 + 0.5 * k,
                             1.0, 0.95])
    return c.float().double()


# ------------------------------------------------------------------ uva_sampler_linear cases
VARIANTS = ("ln_silu", "ln_f32", "ln_f32_noaffine", "gate", "plain_silu")
OUT_DTYPE = {"ln_silu": BF16, "ln_f32": F32, "ln_f32_noaffine": F32, "gate": F32, "plain_silu": BF16}
# (R, N, K, route): both routes at every K; R in {1, 16, 31, 32, 33}; N in {1, 16, 17, 20, 64, 65} and the one
# N = 1024 narrow grid; both sides of the route boundary at N = 512; a partial last 64-column block on the wide route
LINEAR_CASES = [
    (1, 1, 256, "narrow"), (16, 16, 512, "narrow"), (31, 17, 1024, "narrow"), (32, 20, 256, "narrow"),
    (33, 64, 512, "narrow"), (16, 65, 1024, "narrow"), (16, 1024, 1024, "narrow"), (224, 512, 256, "narrow"),
    (225, 512, 256, "wide"), (225, 449, 1024, "wide"), (993, 65, 512, "wide"),
]
PAD_A, PAD_RES = 8, 3


class Case:
    pass


def linear_case(regime, variant, R, N, K, seed=0, edges=False, defect=None):
    """the operands (float64, logical values; the tests lay them out with padded strides) and the reference of one
    uva_sampler_linear call.  defect: a tile defect of ln_tile, ("skip" | "dup", wave) of a narrow wave's K slice, or
    "gate_stride"."""
    from gemm_ref import act_scaling, amp_for
    g = gen(1000 * seed + R * 7 + N * 3 + K + VARIANTS.index(variant))
    c = Case()
    c.regime, c.variant, c.R, c.N, c.K = regime, variant, R, N, K
    c.ln = variant.startswith("ln")
    c.act = SILU if variant.endswith("silu") else 0
    c.dtype = OUT_DTYPE[variant]
    c.width = 2 * K + max(N, K) + 8
    c.eps = 0.0 if regime == "int" else 1e-6
    c.lnw = c.lnb = c.res = c.gate = None
    c.grid = 1.0
    if regime == "int":
        lnw, lnb, c.tbl = int_ln_params(g, R, K, c.width)
        if c.ln:
            c.A = int_rows(g, R, K)
            if variant != "ln_f32_noaffine":
                c.lnw, c.lnb = lnw, lnb
            c.W = ints(g, 2, (N, K)) * 2.0 ** -8 if c.act else ints(g, 4, (N, K))
            c.bias = ints(g, 4, (N,), zero=True) * (2.0 ** -2 if c.act else 1.0)
        elif c.act:
            amp, alpha = act_scaling(K)
            c.A, c.W = ints(g, amp, (R, K)), ints(g, amp, (N, K)) * alpha
            c.bias = ints(g, 4, (N,), zero=True) * 0.25
        else:
            amp = amp_for(K)
            c.A, c.W = ints(g, amp, (R, K)), ints(g, amp, (N, K))
            c.bias = ints(g, 8, (N,), zero=True)
            c.res = ints(g, 64, (R, N), zero=True) * 0.25
            c.grid = 0.25
    else:
        x, lnw, lnb, c.tbl = randn_ln_inputs(g, R, K, c.width)
        c.W = randn_w(g, N, K)
        c.bias = (torch.randn(N, generator=g) * 0.1).double()
        if c.ln:
            c.A = ln_edge_rows(x) if edges else x
            if variant != "ln_f32_noaffine":
                c.lnw, c.lnb = lnw, lnb
        else:
            c.A = torch.randn(R, K, generator=g).to(BF16).double()
            if not c.act:
                c.res = (torch.randn(R, N, generator=g) * 3 + 0.5).double()
    c.shift, c.scale = c.tbl[:, :K], c.tbl[:, K:2 * K]
    if variant == "gate":
        c.gate = c.tbl[:, 2 * K:2 * K + N]
        if defect == "gate_stride":  # the gate read with the residual's leading dimension
            flat = torch.cat([c.tbl.reshape(-1), torch.zeros(R * (N + PAD_RES))])
            idx = 2 * K + torch.arange(R).view(R, 1) * (N + PAD_RES) + torch.arange(N).view(1, N)
            c.gate = flat[idx]
    tdef = defect if isinstance(defect, str) and defect != "gate_stride" else None
    c.tile = (ln_tile(c.A, c.lnw, c.lnb, c.shift, c.scale, c.eps, ln_depths(K), defect=tdef) if c.ln
              else plain_tile(c.A))
    ks = None
    if isinstance(defect, tuple):
        ks = (defect[0], defect[1] * K // 8, (defect[1] + 1) * K // 8)
    c.lin = linear(c.tile, c.W, c.bias, act=c.act, gate=c.gate, res=c.res, kslice=ks)
    c.bound = out_bound(c.lin, c.dtype)
    return c


def check_linear(got, c, what=""):
    """the comparison of one uva_sampler_linear output (a host tensor in the stored dtype) with the reference `c`
    (computed WITHOUT defect): integer regime no-SiLU bit equality, else the per-element bound"""
    from conv_ref import assert_bit_equal
    if c.regime == "int" and not c.act:
        assert_bit_equal(got, c.lin.out, what)
    elif c.regime == "int":
        b = act_bound(SILU, c.lin.pre) + 2.0 ** -8 * c.lin.out.abs()
        assert_within(got, c.lin.out, b, what)
    else:
        assert_within(got, c.lin.out, c.bound, what)


def assert_linear_regime(c):
    """the conditions on the reference alone"""
    from gemm_ref import assert_exact_regime
    if c.regime == "int":
        if c.ln:
            assert_tile_regime(c.tile)
        if c.act:
            assert float(c.lin.pre.abs().max()) <= 32 and torch.equal(c.lin.pre.float().double(), c.lin.pre)
            o = c.lin.out
            assert float((store(o, BF16) != o).double().mean()) >= 0.9  # nearly every stored value needs rounding
        else:
            assert_exact_regime(c.lin.S, c.lin.out, c.grid)
        return None
    if c.ln:
        return assert_randn_conditions(c.tile, c.lin, (c.variant, c.R, c.N, c.K))
    return 0.0, 0.0


# ------------------------------------------------------------------ uva_sampler_persistent cases
_PACKS = {}
KC_EPS = [0.0, -1.0, 1.0, 0.0, -3.0, -1.0, 0.0, 1.0]   # x' = the eps half of the final layer's output
KC_CLIP = [0.5, -1.0, 2.0, 0.25, -3.0, -1.0, 0.0, 1.0]  # x' = 2 clamp(x / 2 + eps) + x / 4, all dyadic
KC_VAR = [0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1.0, 1.0]      # x' = exp((v + 1) / 2) noise


def ps_pack(regime, C, col0=False):
    if (regime, C, col0) not in _PACKS:
        g = gen(77 + C)
        _PACKS[(regime, C, col0)] = (ps_pack_ints(g, C, wf_scale=0.125, col0=col0) if regime == "int"
                                     else ps_pack_randn(g, C))
    return _PACKS[(regime, C, col0)]


# multi-step integer regime: dyadic (k0, k1, k2, k3) with k2 k0 + k3 = -2, -1, 2 (x[:, 0] changes sign and size from
# step to step), (min_log, max_log) and a temperature of their own per step
KC_STEPS = [[1.0, 0.5, -1.0, -1.0, 0.0, 2.0, 1.0, 1.0], [2.0, -1.0, -0.5, 0.0, -1.0, 1.0, 1.0, 0.5],
            [1.0, 0.25, 1.0, 1.0, -2.0, 0.0, 1.0, 2.0]]


def ps_case(kind, R, C, regime="int", live=None, seed=0):
    """kind: "live" (block `live` alone has a nonzero gate; S = 1), "eps" / "clip" / "var" (integer regime, every gate
    0: the final layer and p_sample observed through x_out), "steps" (integer regime, S = 3, every gate 0, or block
    `live` alone), "all" (randn, S = 3, every block live)"""
    g = gen(9000 + 100 * seed + 17 * R + C + (0 if live is None else 1000 * (live + 1)))
    c = Case()
    c.kind, c.R, c.C, c.regime, c.live = kind, R, C, regime, live
    c.S = 3 if kind in ("steps", "all") else 1
    c.pack = ps_pack(regime, C, col0=kind == "steps")
    c.eps = 0.0 if regime == "int" else 1e-6
    c.clip = kind in ("clip", "all")
    modf = ps_mod_ints if regime == "int" else ps_mod_randn
    c.mod = modf(g, c.S, R, live=live, gate_zero=kind not in ("live", "all") and live is None)
    if regime == "int":
        c.x0 = ps_x0_ints(g, R, C, c.pack["gc"])
        c.noise = torch.ones(c.S, R, C, dtype=F64)
        c.coef = torch.tensor([{"var": KC_VAR, "clip": KC_CLIP}.get(kind, KC_EPS)], dtype=F64)
        if kind == "steps":
            c.coef = torch.tensor(KC_STEPS, dtype=F64)
            c.noise = ints(g, 8, (c.S, R, C), zero=True) * 0.25
            c.noise[:, :, 0] = 0.0
            c.x0 = ints(g, 8, (R, C), zero=True) * 0.25
            c.x0[:, 0] = ints(g, 1, (R,)) * torch.exp2(torch.randint(0, 3, (R,), generator=g).double())
    else:
        c.x0 = torch.randn(R, C, generator=g).double()
        c.noise = torch.randn(c.S, R, C, generator=g).double()
        c.coef = ps_coef_randn(g, c.S) if c.S > 1 else torch.tensor([KC_EPS], dtype=F64)
    return c


def ps_reference(c, defect=None, stale_at=None):
    return ps_chain(c.x0, c.pack, c.mod, c.coef, c.noise, c.clip, c.eps, defect, stale_at, exact=c.regime == "int")


def assert_live_regime(c, st):
    """integer regime of the one-live-block case: block j's tile exact, its fc1 pre-activations integers in
    SILU_ID..256 (SiLU the identity, a1 exact), h0 and the block's output on the grid 1/2"""
    j = c.live
    t1, ta = st.tiles[j]
    l1, l2 = st.lins[j]
    assert_tile_regime(t1)
    assert torch.equal(st.h0, store(st.h0, F32)) and bool(exact_sum_rows(st.h0).all())
    assert float(l1.pre.min()) >= SILU_ID and float(l1.pre.max()) <= 512 and torch.equal(l1.pre, torch.round(l1.pre))
    assert_bf16_shares(l1.pre, "fc1 output")
    assert float(l2.S.max()) * 2 < 2 ** 24 and torch.equal(l2.out * 2, torch.round(l2.out * 2))
    assert bool((c.mod[-1][:, 3 * W_PS * j + 2 * W_PS:3 * W_PS * (j + 1)] != 0).all())


def live_expected(c, st):
    """what the exchange buffers hold after the launch of a one-live-block case: (hx rows, ha rows or None).  In the
    integer regime SiLU is the identity on block j's pre-activations, so a1 is their exact value."""
    j = c.live
    if c.regime == "int":
        l1 = st.lins[j][0]
        a1 = plain_tile(store(l1.pre, BF16))
        m = c.mod[-1][:, 3 * W_PS * j:3 * W_PS * (j + 1)]
        l2 = linear(a1, c.pack["w2"][j], c.pack["b2"][j], gate=m[:, 2 * W_PS:], res=st.h0)
        return l2.out, a1.a
    return st.hx[DEPTH - 1], st.ha[DEPTH - 1]


def forced_block(c, k, hx_in, ha_got):
    """the last block of step k from what the kernel itself left in the exchange buffers: hx_in = its input rows
    (side (depth - 2) & 1, exact fp32 values), ha_got = the fc1 output it stored.  -> (l1, l2): ha is held to
    out_bound(l1, BF16), the block's output rows to l2.err (computed from the kernel's own ha: no allowance)"""
    W, b = W_PS, DEPTH - 1
    m = c.mod[k][:, 3 * W * b:3 * W * (b + 1)]
    p = c.pack
    t1 = ln_tile(hx_in, p["lnw"][b], p["lnb"][b], m[:, :W], m[:, W:2 * W], c.eps, PS_DEPTHS)
    l1 = linear(t1, p["w1"][b], p["b1"][b], act=SILU)
    l2 = linear(plain_tile(ha_got), p["w2"][b], p["b2"][b], gate=m[:, 2 * W:], res=hx_in)
    return t1, l1, l2


def forced_final(c, hx_got, x):
    """the final layer and p_sample of a one-step run from the kernel's own last residual rows -> (x', bound)"""
    W, C = W_PS, c.C
    mf = c.mod[0][:, 3 * W * DEPTH:3 * W * DEPTH + 2 * W]
    tf = ln_tile(hx_got, None, None, mf[:, :W], mf[:, W:], c.eps, PS_DEPTHS)
    lf = linear(tf, c.pack["wf"], c.pack["bfin"])
    xn, b = p_sample(lf.out[:, :C], lf.out[:, C:], x, c.noise[0], c.coef[0].tolist(), c.clip, lf.err[:, :C],
                     lf.err[:, C:])
    return tf, lf, xn, b
