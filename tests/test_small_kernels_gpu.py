"""The thin element-wise, reduction and layout kernels every training step runs (the scalar loss and the
head's upstream gradient, the gated residual, fill / cast / activation backward on strided views, the conv_fc
trunk's pool, row softmax, column sums, LayerNorm) against float64 references at the smallest shapes that
reach each of their routes: odd sizes, one row, more than one block, tails that are no multiple of the
vector width.

Every comparison is per element, |got - ref| <= rtol * |ref| + atol with atol tied to a stated quantity
(never a fraction of the tensor's maximum), on the values the kernel read (a bf16 input is rounded first,
the reference reads the rounded value).  Outputs live NaN-filled inside a larger sentinel-filled buffer:
an unwritten element fails as NaN, a write outside the output (or into the gaps of a strided view) fails the
guard check."""
import math

import pytest
import torch

from edge_helpers import BF16, DEV, F32, Guarded, assert_within, flat_out, gen

pytestmark = pytest.mark.gpu

U24, U23, U8 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -8  # fp32 half-ulp, fp32 ulp, bf16 half-ulp (relative)
DT_ID = {F32: "f32", BF16: "bf16"}


def col_slice(rows, cols, dtype, g, ld_extra=16, off=8, scale=1.0):
    """an input [rows, cols] as a column slice of a wider randn buffer (ld = cols + ld_extra); off = 8
    elements keeps the 16-byte alignment the vector routes ask for"""
    big = (scale * torch.randn(rows, cols + ld_extra, generator=g)).to(dtype).to(DEV)
    return big[:, off:off + cols]


# ---------------------------------------------------------------------------------------------------
# 5. weighted_mean, loss_grad, DiffusionLossFn
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wkind", ["none", "mask30", "onehot"])
@pytest.mark.parametrize("n", [1, 63, 1024, 1025, 70001])
def test_weighted_mean(n, wkind):
    """res[0] = sum(l w) / sum(w), res[1] = sum(w).  Bound (ceil(n / 1024) + 24) 2^-23 sum|l w| / sum(w):
    the depth of the kernel's summation (per-thread serial over n / 1024 terms, 6 shuffle levels, 16 serial
    wave partials, the division).  sum(w) of a 0/1 mask is exact in fp32 at these n."""
    from unified_video_action_amd.native import ops
    g = gen(5000 + n)
    l = torch.randn(n, generator=g).to(DEV)
    if wkind == "none":
        w, wd = None, torch.ones(n, dtype=torch.float64)
    else:
        w = torch.zeros(n)
        if wkind == "mask30":
            w[torch.rand(n, generator=g) < 0.3] = 1.0
        if wkind == "onehot" or w.sum() == 0:
            w[int(torch.randint(0, n, (1,), generator=g))] = 1.0
        wd = w.double()
        w = w.to(DEV)
    gr, res = flat_out(2, F32)
    ops.weighted_mean(l, w, res)
    gr.check()
    ld = l.double().cpu()
    wsum = wd.sum()
    ref = (ld * wd).sum() / wsum
    bound = (math.ceil(n / 1024) + 24) * U23 * (ld * wd).abs().sum() / wsum
    assert_within(res[0:1], ref.reshape(1), bound.reshape(1), "weighted mean")
    assert res[1].item() == wsum.item()


@pytest.mark.parametrize("layout", ["f32-contig", "bf16-slice"])
@pytest.mark.parametrize("masked", [False, True], ids=["w1", "mask"])
@pytest.mark.parametrize("C2", [4, 20, 32])
@pytest.mark.parametrize("rows", [1, 257])
def test_loss_grad(rows, C2, masked, layout):
    """dout[r, c] = g_up w[r] / wsum dl[r, c].  Bound 3 * 2^-24 |ref| (a product, a correctly rounded
    division, a product); a bf16 store adds 2^-8 |ref|."""
    from unified_video_action_amd.native import ops
    g = gen(5100 + rows + C2)
    dl = torch.randn(rows, C2, generator=g).to(DEV)
    w = None
    if masked:
        w = (torch.rand(rows, generator=g) < 0.5).float()
        w[0] = 1.0
        w = w.to(DEV)
    wsum = torch.tensor([float(w.sum()) if masked else float(rows)], device=DEV) * 1.37
    g_up = torch.tensor([0.37], device=DEV)
    if layout == "f32-contig":
        go = Guarded(rows, C2, F32)
    else:
        go = Guarded(rows, C2, BF16, ld=C2 + 24, off=8)
    ops.loss_grad(dl, w, wsum, g_up, go.view)
    go.check()
    wr = w.double()[:, None] if masked else 1.0
    ref = g_up.double() * wr / wsum.double() * dl.double()
    bound = 3 * U24 * ref.abs() + (U8 * ref.abs() if go.view.dtype == BF16 else 0.0)
    assert_within(go.view, ref, bound, "dout")


# the schedule tables in the order of csrc/diffusion.hip's DiffTables
TB = ("sqrt_ac", "sqrt_1mac", "coef1", "coef2", "plvc", "log_betas", "sqrt_recip_ac", "sqrt_recipm1_ac")


def diffusion_loss_f64(tables, x0, noise, t, out):
    """oracle/uva_oracle.py diffusion_training_loss in float64 (its table gather pins float32, so its dozen
    lines are restated): tables = the fp32 tables the kernel reads, cast up.  -> per-row loss [rows]"""
    tb = {k: tables[i].double().cpu()[t][:, None] for i, k in enumerate(TB)}
    C = x0.shape[1]
    x_t = tb["sqrt_ac"] * x0 + tb["sqrt_1mac"] * noise
    eps, v = out[:, :C], out[:, C:]
    eps_d = eps.detach()
    true_mean = tb["coef1"] * x0 + tb["coef2"] * x_t
    true_lv = tb["plvc"]
    frac = (v + 1) / 2
    model_lv = frac * tb["log_betas"] + (1 - frac) * tb["plvc"]
    x0_hat = tb["sqrt_recip_ac"] * x_t - tb["sqrt_recipm1_ac"] * eps_d
    model_mean = tb["coef1"] * x0_hat + tb["coef2"] * x_t
    kl = 0.5 * (-1.0 + model_lv - true_lv + torch.exp(true_lv - model_lv)
                + (true_mean - model_mean) ** 2 * torch.exp(-model_lv))
    kl = kl.mean(dim=1) / math.log(2.0)
    cdf = lambda x: 0.5 * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x.pow(3))))
    inv_std = torch.exp(-0.5 * model_lv)
    cen = x0 - model_mean
    cdf_p, cdf_m = cdf(inv_std * (cen + 1.0 / 255.0)), cdf(inv_std * (cen - 1.0 / 255.0))
    lp = torch.where(x0 < -0.999, torch.log(cdf_p.clamp(min=1e-12)),
                     torch.where(x0 > 0.999, torch.log((1.0 - cdf_m).clamp(min=1e-12)),
                                 torch.log((cdf_p - cdf_m).clamp(min=1e-12))))
    nll = -lp.mean(dim=1) / math.log(2.0)
    vb = torch.where(t == 0, nll, kl)
    return ((noise - eps) ** 2).mean(dim=1) + vb


def diffusion_case(C, odt, g):
    """rows at t = 0 whose x0 cycle through {-1, -0.9995, 0, 0.9995, 1} (both |x0| > 0.999 sub-branches of
    the decoder NLL and the middle one, in every column), rows at t = 1 and t = 999, and random t.  The eps
    half of the model output stays near the noise (a trained head): at t = 0 the NLL takes the log of a
    difference of two CDFs, which only an output near the target keeps conditioned in fp32."""
    vals = torch.tensor([-1.0, -0.9995, 0.0, 0.9995, 1.0])
    t = torch.tensor([0] * 10 + [1] * 3 + [999] * 3 + [17, 250, 500, 873])
    rows = t.numel()
    x0 = 0.5 * torch.randn(rows, C, generator=g)
    for r in range(10):
        for c in range(C):
            x0[r, c] = vals[(r + 2 * c) % 5]
    noise = torch.randn(rows, C, generator=g)
    out = torch.cat([noise + 0.3 * torch.randn(rows, C, generator=g), 0.5 * torch.randn(rows, C, generator=g)], 1)
    if odt == BF16:  # inside a wider buffer: ld_out = 2 C + 8
        wide = torch.randn(rows, 2 * C + 8, generator=g).to(BF16)
        wide[:, :2 * C] = out.to(BF16)
        out_dev = wide.to(DEV)[:, :2 * C]
    else:
        out_dev = out.to(DEV)
    return x0, noise, t, out_dev


@pytest.mark.parametrize("odt", [F32, BF16], ids=["f32", "bf16-wide"])
@pytest.mark.parametrize("C", [2, 16])
def test_diffusion_loss_edge_branches(C, odt):
    """loss rows and d(loss row)/d(out) against the float64 restatement of the oracle's
    diffusion_training_loss (gradients from autograd); the existing test's bounds: loss rtol 1e-4 / atol
    1e-5, dl rtol 1e-3 / atol 1e-6."""
    from unified_video_action_amd.model.autoregressive.diffusion import TABLE_ORDER, DiffusionSchedule
    from unified_video_action_amd.native import ops
    assert tuple(TABLE_ORDER) == TB
    sched = DiffusionSchedule(1000, DEV)
    x0, noise, t, out = diffusion_case(C, odt, gen(6000 + C))
    rows = t.numel()
    gl, lrow = flat_out(rows, F32)
    gd = Guarded(rows, 2 * C, F32)
    ops.diffusion_loss(x0.to(DEV), noise.to(DEV), t.to(DEV), out, sched.tables, lrow, gd.view)
    gl.check()
    gd.check()
    od = out.double().cpu().requires_grad_(True)
    ref = diffusion_loss_f64(sched.tables, x0.double(), noise.double(), t, od)
    ref.sum().backward()
    assert_within(lrow, ref.detach(), 1e-4 * ref.detach().abs() + 1e-5, "loss rows")
    assert_within(gd.view, od.grad, 1e-3 * od.grad.abs() + 1e-6, "dl")


@pytest.mark.parametrize("masked", [False, True], ids=["w1", "mask"])
def test_diffusion_loss_fn_backward_through_scaled_loss(masked):
    """DiffusionLossFn forward + backward of 2.5 * loss against float64 autograd of sum(w lrow) / sum(w): the
    res[1:2] hand-off from weighted_mean to loss_grad.  Bounds: the loss rows' rtol 1e-4 / atol 1e-5 on the
    weighted mean; dl's rtol 1e-3 / atol 1e-6 carried through the row factor 2.5 w / sum(w)."""
    from unified_video_action_amd.model.autoregressive.diffusion import DiffusionSchedule
    from unified_video_action_amd.model.autoregressive.diffusion_loss import DiffusionLossFn
    C = 16
    sched = DiffusionSchedule(1000, DEV)
    g = gen(6100)
    x0, noise, t, out = diffusion_case(C, F32, g)
    rows = t.numel()
    w = None
    if masked:
        w = (torch.rand(rows, generator=g) < 0.6).float()
        w[0] = w[11] = 1.0
    out = out.clone().requires_grad_(True)
    loss = DiffusionLossFn.apply(out, x0.to(DEV), noise.to(DEV), t.to(DEV), w.to(DEV) if masked else None, sched)
    (loss * 2.5).backward()
    torch.cuda.synchronize()
    od = out.detach().double().cpu().requires_grad_(True)
    wd = w.double() if masked else torch.ones(rows, dtype=torch.float64)
    ref = (wd * diffusion_loss_f64(sched.tables, x0.double(), noise.double(), t, od)).sum() / wd.sum()
    (ref * 2.5).backward()
    assert_within(loss.detach().reshape(1), ref.detach().reshape(1), (1e-4 * ref.detach().abs() + 1e-5).reshape(1),
                  "loss")
    fac = (2.5 * wd / wd.sum())[:, None]
    assert_within(out.grad, od.grad, 1e-3 * od.grad.abs() + 1e-6 * fac.expand_as(od.grad), "d loss / d out")


# ---------------------------------------------------------------------------------------------------
# 7. gate_bwd, fill, cast, act_bwd on views
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hdt,gdt", [(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("cols", [1, 100, 1024])
@pytest.mark.parametrize("rows", [1, 130])
def test_gate_bwd(rows, cols, hdt, gdt):
    """dgate = dout h, dh = dout gate with gate / dgate the last third of [rows, 3 cols] buffers (the adaLN
    trunk's call).  One product of stored values: 2^-24 |ref| for an fp32 store, 2^-8 |ref| for bf16.  The
    first two thirds of dmod keep their sentinel."""
    from unified_video_action_amd.native import ops
    g = gen(7000 + rows + cols)
    dout = torch.randn(rows, cols, generator=g).to(DEV)
    h = torch.randn(rows, cols, generator=g).to(hdt).to(DEV)
    mod = torch.randn(rows, 3 * cols, generator=g).to(gdt).to(DEV)
    gate = mod[:, 2 * cols:]
    gdh = Guarded(rows, cols, hdt)
    gdm = Guarded(rows, cols, gdt, ld=3 * cols, off=2 * cols)
    ops.gate_bwd(dout, h, gate, gdh.view, gdm.view)
    gdh.check()
    gdm.check()
    ref_g, ref_h = dout.double() * h.double(), dout.double() * gate.double()
    assert_within(gdm.view, ref_g, (U24 if gdt == F32 else U8) * ref_g.abs(), "dgate")
    assert_within(gdh.view, ref_h, (U24 if hdt == F32 else U8) * ref_h.abs(), "dh")


@pytest.mark.parametrize("n", [1, 255, 257, 2 ** 21 + 3])
def test_fill(n):
    from unified_video_action_amd.native import ops
    gf, t = flat_out(n, F32)
    ops.fill(t, 3.25)
    gf.check()
    assert (t == 3.25).all()


@pytest.mark.parametrize("sdt,ddt", [(F32, BF16), (BF16, F32)], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("rows,cols", [(7, 13), (64, 520)])
def test_cast_strided_views(rows, cols, sdt, ddt):
    """the strided cast_kernel: both sides column slices of wider buffers; exact against .to(), gaps untouched"""
    from unified_video_action_amd.native import ops
    src = col_slice(rows, cols, sdt, gen(7100 + cols), ld_extra=11, off=3)
    gd = Guarded(rows, cols, ddt, ld=cols + 5, off=2)
    ops.cast(src, gd.view)
    gd.check()
    assert torch.equal(gd.view, src.to(ddt))


@pytest.mark.parametrize("sdt,ddt", [(F32, BF16), (BF16, F32)], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("n", [91, 33283])
def test_cast_contiguous_odd_count(n, sdt, ddt):
    """contiguous with n % 8 != 0: off the 8-wide fp32 -> bf16 kernel, onto the scalar one"""
    from unified_video_action_amd.native import ops
    src = torch.randn(n, generator=gen(7200 + n)).to(sdt).to(DEV)
    gd, dst = flat_out(n, ddt)
    ops.cast(src, dst)
    gd.check()
    assert torch.equal(dst, src.to(ddt))


def act_grad_f64(act, x):
    """-> (act'(x), A(x)): the derivative and the sum of the magnitudes of its terms"""
    if act == "gelu":
        Phi = 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
        phi = torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)
        return Phi + x * phi, Phi + x.abs() * phi
    if act == "silu":
        s = torch.sigmoid(x)
        return s * (1.0 + x * (1.0 - s)), s * (1.0 + x.abs() * (1.0 - s))
    d = (x > 0).double()
    return d, d


@pytest.mark.parametrize("gdt,xdt", [(F32, F32), (BF16, F32), (BF16, BF16)], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("act", ["gelu", "silu", "relu"])
@pytest.mark.parametrize("cols", [13, 64], ids=["scalar13", "vector64"])
def test_act_bwd_accumulates_on_views(cols, act, gdt, xdt):
    """dx = dx0 + dy act'(pre) with accum onto a non-zero dx, dy and dx column slices (ld > cols), drop_p 0;
    37 rows put the vector route on two blocks.  Bound 2e-6 (|dx0| + |dy| A(pre)) for an fp32 dx, + 2^-8 |ref|
    for bf16, where A is act' with its terms taken by magnitude (GELU': Phi + |x| phi, SiLU': s (1 + |x| (1 -
    s)), ReLU': itself): GELU' and SiLU' cross zero at a negative x where their terms cancel, and an fp32
    evaluation is accurate to its terms, not to their difference.  GELU' adds 0.5 * 1.5e-7 |dy|: erf_fast's
    stated absolute error (common.h: |error| <= 1.5e-7) enters Phi = (1 + erf) / 2 as an absolute error that
    no relative bound covers in the left tail, where GELU' itself is below 1e-2.
    Measured on an MI355X (both fp32-dx GELU cases at 64 columns, 2368 elements each): against 2e-6 (|dx0| +
    |dy act'|) alone 3 and 4 elements miss, at most 5.2x (absolute error <= 4.9e-7); with only the erf_fast
    term added 2 elements of one case still miss, by 1.06x (1.19e-7 against 1.12e-7: fp32 rounding of the
    polynomial on top of the stated approximation error); under this bound the worst element is at 0.28x.
    SiLU and ReLU meet the relative form as it stands (worst 0.31x / 0.03x)."""
    from unified_video_action_amd.native import ops
    rows = 37
    g = gen(7300 + cols)
    pre = torch.randn(rows, cols, generator=g).to(gdt).to(DEV)
    dy = col_slice(rows, cols, gdt, g)
    dx0 = torch.randn(rows, cols, generator=g).to(xdt)
    gx = Guarded(rows, cols, xdt, ld=cols + 16, off=8, init=dx0.to(DEV))
    ops.act_bwd(pre, dy, gx.view, act, accum=True)
    gx.check()
    d, A = act_grad_f64(act, pre.double())
    ref = dx0.double().to(DEV) + dy.double() * d
    bound = 2e-6 * (dx0.double().to(DEV).abs() + dy.double().abs() * A)
    if act == "gelu":
        bound = bound + 0.5 * 1.5e-7 * dy.double().abs()
    if xdt == BF16:
        bound = bound + U8 * ref.abs()
    assert_within(gx.view, ref, bound, "dx")


# ---------------------------------------------------------------------------------------------------
# 8. pool4x4_cwh, pool4x4_relu_bwd
# ---------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 8), (3, 24), (5, 100)]  # n C and n 16 C are no multiple of the 256-thread block


@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("n,C", POOL_SHAPES)
def test_pool4x4_cwh(n, C, dtype):
    """AdaptiveAvgPool2d((4, 4)) of NHWC [n, 16 (w), 16 (h), C], flattened (c w h).  Bound 16 * 2^-24 of the
    4x4 block's mean |x| (a serial fp32 sum of 16 terms, an exact division by 16); bf16 adds its store."""
    from unified_video_action_amd.native import ops
    x = torch.randn(n, 16, 16, C, generator=gen(8000 + C)).to(dtype).to(DEV)
    go, out = flat_out(n * 16 * C, dtype)
    ops.pool4x4_cwh(x, out, n, C)
    go.check()
    xd = x.double().permute(0, 3, 1, 2)  # [n, C, w, h]
    ref = torch.nn.functional.adaptive_avg_pool2d(xd, (4, 4)).reshape(n, 16 * C)
    mag = torch.nn.functional.adaptive_avg_pool2d(xd.abs(), (4, 4)).reshape(n, 16 * C)
    bound = 16 * U24 * mag + (U8 * ref.abs() if dtype == BF16 else 0.0)
    assert_within(out.view(n, 16 * C), ref, bound, "pooled")


@pytest.mark.parametrize("pdt,gdt", [(F32, F32), (BF16, BF16), (BF16, F32), (F32, BF16)], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("n,C", POOL_SHAPES)
def test_pool4x4_relu_bwd(n, C, pdt, gdt):
    """dpre = (post > 0) gpool / 16, exactly (a power-of-two factor; one rounding of the fp32 product for a
    bf16 dpre); post holds exact zeros and negatives among the positives, and the `>` is strict."""
    from unified_video_action_amd.native import ops
    g = gen(8100 + C)
    post = torch.randn(n, 16, 16, C, generator=g)
    post[torch.rand(n, 16, 16, C, generator=g) < 0.15] = 0.0
    post = post.to(pdt).to(DEV)
    gpool = torch.randn(n, 16 * C, generator=g).to(gdt).to(DEV)
    gd, dpre = flat_out(n * 256 * C, pdt)
    ops.pool4x4_relu_bwd(post, gpool, dpre, n, C)
    gd.check()
    gg = (gpool.float() * 0.0625).view(n, C, 4, 4).repeat_interleave(4, dim=2).repeat_interleave(4, dim=3)
    want = torch.where(post.float() > 0, gg.permute(0, 2, 3, 1), torch.zeros((), device=DEV)).to(pdt)
    assert (post == 0).any() and (post < 0).any()
    assert torch.equal(dpre.view(n, 16, 16, C), want)


# ---------------------------------------------------------------------------------------------------
# 9. softmax, colsum, LayerNorm
# ---------------------------------------------------------------------------------------------------
def softmax_logits(rows, L, dtype, g, scale):
    S = 3 * torch.randn(rows, L, generator=g)
    if rows > 1:
        S[2, L // 3] += 40.0 / scale  # one scaled logit 40 above the rest of its row
        S[5, :] = 0.75  # a constant row
    return S.to(dtype).to(DEV)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("L", [1, 63, 100, 256])
@pytest.mark.parametrize("rows", [1, 7])
def test_softmax_fwd_bwd(rows, L, dtype):
    """forward |P - ref| <= 4e-6 ref + 1e-9 (fp32; bf16 adds 2^-8 ref); backward dS = scale P (dP - sum P dP)
    on stored P / dP: 1e-5 scale P (|dP| + sum P |dP|) (bf16 adds 2^-8 |ref|)."""
    from unified_video_action_amd.native import ops
    scale = 0.125
    g = gen(9000 + rows * 1000 + L)
    S = softmax_logits(rows, L, dtype, g, scale)
    gp = Guarded(rows, L, dtype)
    ops.softmax_fwd(S, gp.view, None, L, scale)
    gp.check()
    ref = torch.softmax(S.double() * scale, dim=-1)
    assert_within(gp.view, ref, 4e-6 * ref + 1e-9 + (U8 * ref if dtype == BF16 else 0.0), "P")
    P = ref.to(dtype)
    dP = torch.randn(rows, L, generator=g).to(dtype).to(DEV)
    gs = Guarded(rows, L, dtype)
    ops.softmax_bwd(P, dP, gs.view, L, scale)
    gs.check()
    Pd, dPd = P.double(), dP.double()
    refb = scale * Pd * (dPd - (Pd * dPd).sum(-1, keepdim=True))
    bound = 1e-5 * scale * Pd * (dPd.abs() + (Pd * dPd.abs()).sum(-1, keepdim=True))
    assert_within(gs.view, refb, bound + (U8 * refb.abs() if dtype == BF16 else 0.0), "dS")


COLSUM_ROUTES = {
    "single-kernel": (100, 301),           # fewer than 513 rows, cols % 8 != 0
    "row-partials+scalar-stage2": (1100, 301),  # three 512-row partials, cols % 4 != 0
    "row-partials+float4-stage2": (1100, 300),  # cols % 4 == 0 but % 8 != 0
    "vector-ragged-chunk": (300, 264),     # cols % 8 == 0, rows >= 256: 128-row chunks, the last of 44 rows
}


@pytest.mark.parametrize("accum", [False, True], ids=["store", "accum"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("layout", ["contig", "slice"])
@pytest.mark.parametrize("route", list(COLSUM_ROUTES))
def test_colsum_routes(route, layout, dtype, accum):
    """out[c] (+)= sum_r x[r, c]; bound (rows / 4 + 8) 2^-24 sum_r |x[r, c]| per column (the deepest route sums
    rows / 4 terms serially per thread; the randn out0 of the accumulating form is one more term far below
    the column's sum of magnitudes)."""
    from unified_video_action_amd.native import ops
    rows, cols = COLSUM_ROUTES[route]
    g = gen(9100 + rows + cols)
    x = col_slice(rows, cols, dtype, g) if layout == "slice" else torch.randn(rows, cols, generator=g).to(dtype).to(DEV)
    out0 = torch.randn(1, cols, generator=g)
    go = Guarded(1, cols, F32, init=out0.to(DEV) if accum else None)
    ops.colsum(x, go.view.view(-1), accum=accum)
    go.check()
    ref = x.double().sum(0) + (out0.double().to(DEV)[0] if accum else 0.0)
    bound = (rows / 4 + 8) * U24 * x.double().abs().sum(0)
    assert_within(go.view.view(-1), ref, bound, "column sums")


LN_D = [256, 512, 100, 1000]  # the 4-wide route with empty trailing chunks; D no multiple of 64
LN_ROWS = [1, 5, 130]         # fewer than the block's 4 waves; more than 64: two backward blocks


def ln_inputs(rows, D, g):
    """rows whose mean is about 10x their std; float64 statistics of the stored x, rounded to the fp32 the
    backward reads"""
    x = (10.0 + torch.randn(rows, D, generator=g)).to(DEV)
    xd = x.double()
    mean = xd.mean(-1)
    rstd = 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + 1e-6)
    return x, mean, rstd


def check_ln_forward(gy, gm, gr, x, mean, rstd, D, mul, add, tout):
    """y = xhat * mul + add, checked in two links that leave no gap.
    (a) the statistics the kernel stores (its mean / rstd outputs, which the backward reads) against float64:
        mean to depth * 2^-24 mean|x| (D / 64 serial terms per lane, 6 shuffle levels, the division), rstd to
        (depth + 4) * 2^-24 rstd (the same depth on the squares, halved by the square root, plus the root and
        the reciprocal);
    (b) y against the float64 normalisation of x by those stored statistics, to 2e-6 (|xhat mul| + |add|) plus
        the output's rounding.
    A row mean held in fp32 is off by up to (a)'s bound, which moves every xhat of the row by rstd * that
    whatever its size, so against float64 statistics the elements with small |xhat| carry an error their own
    magnitude does not bound (rows with mean = 10 std: 3e-7 .. 1.5e-6 absolute measured); the end-to-end
    bound is therefore (b) + |mul| rstd * (a)'s mean bound + |xhat mul| * (a)'s relative rstd bound."""
    xd = x.double()
    depth = D // 64 + 8
    mean_b = depth * U24 * xd.abs().mean(-1)
    rstd_rel = (depth + 4) * U24
    mk, rk = gm.view.view(-1).double(), gr.view.view(-1).double()
    assert_within(mk, mean, mean_b, "row mean")
    assert_within(rk, rstd, rstd_rel * rstd, "row rstd")
    rnd = U24 if tout == F32 else U8
    xk = (xd - mk[:, None]) * rk[:, None]
    refk = xk * mul + add
    assert_within(gy.view, refk, 2e-6 * ((xk * mul).abs() + add.abs()) + rnd * refk.abs(), "y from the stored statistics")
    xhat = (xd - mean[:, None]) * rstd[:, None]
    ref = xhat * mul + add
    bound = (2e-6 * ((xhat * mul).abs() + add.abs()) + rnd * ref.abs()
             + mul.abs() * (rstd * mean_b)[:, None] + (xhat * mul).abs() * rstd_rel)
    assert_within(gy.view, ref, bound, "y end to end")


@pytest.mark.parametrize("tout", [F32, BF16], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_affine_edge_shapes(D, rows, tout):
    """forward: check_ln_forward (2e-6 (|xhat w| + |b|) + the output's rounding); dx 1e-5 rstd (|g| + mean|g| + |xhat| mean|g
    xhat|) with g = dy w; dw / db (rows + 8) 2^-24 sum_r |terms|."""
    from unified_video_action_amd.native import ops
    g = gen(9200 + D + rows)
    x, mean, rstd = ln_inputs(rows, D, g)
    w = (1.0 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    b = (0.1 * torch.randn(D, generator=g)).to(DEV)
    gy = Guarded(rows, D, tout)
    gm, gr = Guarded(1, rows, F32), Guarded(1, rows, F32)
    ops.layernorm_fwd(x, w, b, gy.view, gm.view.view(-1), gr.view.view(-1))
    for q in (gy, gm, gr):
        q.check()
    check_ln_forward(gy, gm, gr, x, mean, rstd, D, w.double()[None].expand(rows, D), b.double()[None].expand(rows, D), tout)

    mean32, rstd32 = mean.float(), rstd.float()
    dy = torch.randn(rows, D, generator=g).to(DEV)
    gdx = Guarded(rows, D, F32)
    gdw, gdb = Guarded(1, D, F32), Guarded(1, D, F32)
    ops.layernorm_bwd(x, w, dy, mean32, rstd32, gdx.view, accum=False, dw=gdw.view.view(-1), db=gdb.view.view(-1),
                      accum_wb=False)
    for q in (gdx, gdw, gdb):
        q.check()
    xh = (x.double() - mean32.double()[:, None]) * rstd32.double()[:, None]
    gg = dy.double() * w.double()
    m1, m2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    rs = rstd32.double()[:, None]
    assert_within(gdx.view, rs * (gg - m1 - xh * m2),
                  1e-5 * rs * (gg.abs() + gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True)),
                  "dx")
    tw = dy.double() * xh
    assert_within(gdw.view.view(-1), tw.sum(0), (rows + 8) * U24 * tw.abs().sum(0), "dw")
    assert_within(gdb.view.view(-1), dy.double().sum(0), (rows + 8) * U24 * dy.double().abs().sum(0), "db")


@pytest.mark.parametrize("dtype", [F32, BF16], ids=lambda d: DT_ID[d])
@pytest.mark.parametrize("rows", LN_ROWS)
@pytest.mark.parametrize("D", LN_D)
def test_layernorm_modulated_edge_shapes(D, rows, dtype):
    """y = xhat (1 + scale) + shift with shift / scale the first two thirds of a [rows, 3 D] buffer: forward
    check_ln_forward (2e-6 (|xhat (1 + scale)| + |shift|) + the output's rounding); dx as the affine form with g = dy (1 +
    scale); dscale = dy xhat and dshift = dy to their stores' rounding (fp32: the product and xhat's two
    roundings, 2^-22; bf16 2^-8), the last third of dmod untouched."""
    from unified_video_action_amd.native import ops
    g = gen(9300 + D + rows)
    x, mean, rstd = ln_inputs(rows, D, g)
    mod = (0.3 * torch.randn(rows, 3 * D, generator=g)).to(dtype).to(DEV)
    shift, scale = mod[:, :D], mod[:, D:2 * D]
    gy = Guarded(rows, D, dtype)
    gm, gr = Guarded(1, rows, F32), Guarded(1, rows, F32)
    ops.layernorm_fwd(x, None, None, gy.view, gm.view.view(-1), gr.view.view(-1), scale=scale, shift=shift, ldm=3 * D)
    for q in (gy, gm, gr):
        q.check()
    check_ln_forward(gy, gm, gr, x, mean, rstd, D, 1.0 + scale.double(), shift.double(), dtype)

    mean32, rstd32 = mean.float(), rstd.float()
    dy = torch.randn(rows, D, generator=g).to(DEV)
    gdx = Guarded(rows, D, F32)
    gdm = Guarded(rows, 2 * D, dtype, ld=3 * D, off=0)
    ops.layernorm_bwd(x, None, dy, mean32, rstd32, gdx.view, accum=False, scale=scale, ldm=3 * D,
                      dscale=gdm.view[:, D:], dshift=gdm.view[:, :D])
    gdx.check()
    gdm.check()
    xh = (x.double() - mean32.double()[:, None]) * rstd32.double()[:, None]
    gg = dy.double() * (1.0 + scale.double())
    m1, m2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    rs = rstd32.double()[:, None]
    assert_within(gdx.view, rs * (gg - m1 - xh * m2),
                  1e-5 * rs * (gg.abs() + gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True)),
                  "dx")
    rnd = 2.0 ** -22 if dtype == F32 else U8
    ds_ref = dy.double() * xh
    assert_within(gdm.view[:, D:], ds_ref, rnd * ds_ref.abs(), "dscale")
    assert_within(gdm.view[:, :D], dy.double(), (0.0 if dtype == F32 else U8) * dy.double().abs(), "dshift")
