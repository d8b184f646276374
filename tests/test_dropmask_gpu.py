"""Every kernel that drops, against oracle/dropmask.py (the counter hash restated in numpy integer code and pinned
to csrc/common.h on the CPU by tests/test_dropmask_cpu.py).  No mask here is read back from another kernel.

Each case feeds inputs whose output is non-zero exactly where an element is kept (ones for the elementwise
kernels; positive operands and a positive bias for the GEMMs), then requires the kernel's keep pattern to equal
the restated one over EVERY element, and -- where the stored value is a plain product -- the kept values to equal
input * scale with the restated scale, bit for bit.

Sites: uva_dropout_plane (word tail, both clamp ends of p), act_drop_fwd, act_bwd (vectorised and scalar forms),
act_bwd_bias, the three dropout epilogues of gemm.hip (epi_store: the VALU kernel and ragged column tails;
epi_apply_row8: even and odd segment bases; gemm_8ph's residual-only ring), linear_dx_act, softmax_fwd,
softmax_bwd, the attention MQ / MK bit planes, layernorm_bwd_drop, and the three fused epilogues of gemm8w.hip in both launch
forms with the hash (DM = 1) and the keep-bit plane (DM = 2)."""
import numpy as np
import pytest
import torch

import dropmask as DM

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F32 = torch.bfloat16, torch.float32


def _rt_seed():
    """a full 64-bit seed as a training step draws it (drop_key mixes the high word)"""
    from unified_video_action_amd.runtime import _Runtime
    rt = _Runtime()
    rt.seed(77)
    rt.next_seed()
    return rt.next_seed()


SEEDS = [1234, _rt_seed()]
assert SEEDS[1] >> 32
PS = [0.1, 0.5]
sp = pytest.mark.parametrize("seed,p", [(s, p) for s in SEEDS for p in PS])


@pytest.fixture(scope="module", autouse=True)
def _lib():
    from unified_video_action_amd.native import ops  # fails loudly without the .so
    prev = ops.gemm8w_set(0, 0)
    yield
    ops.gemm8w_set(*prev)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _flat(seed, p, M, N):
    th, scale = DM.drop_params(p)
    return _t(DM.keep_flat(seed, M, N, th)), scale


def _pos(*shape, dtype=BF16, lo=0.5, hi=1.5, g=None):
    return (torch.rand(*shape, device=DEV, generator=g) * (hi - lo) + lo).to(dtype)


def _same_keep(out, keep):
    assert out.shape == keep.shape
    assert torch.isfinite(out).all()
    assert torch.equal(out != 0, keep)


# ---- uva_dropout_plane ---------------------------------------------------------------------------
@pytest.mark.parametrize("p", PS + [1e-6, 0.9999])
@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n", [70, 32 * 1000, 256 * 192 + 8])
def test_dropout_plane(n, seed, p):
    from unified_video_action_amd.native import ops
    th, _ = DM.drop_params(p)
    assert th == {0.1: 6554, 0.5: 32768, 1e-6: 1, 0.9999: 65529}[p]
    plane = ops.dropout_plane(n, p, seed, DEV)
    got = plane.cpu().numpy().view(np.uint32)
    assert np.array_equal(got, DM.plane_words(seed, n, th))


# ---- elementwise ---------------------------------------------------------------------------------
@sp
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_act_drop_fwd(dtype, seed, p):
    from unified_video_action_amd.native import ops
    n = 8 * 1237  # the kernel takes whole 8-element segments only
    keep, scale = _flat(seed, p, 1, n)
    x = torch.ones(n, device=DEV, dtype=dtype)
    y = torch.full_like(x, float("nan"))
    ops.act_drop_fwd(x, y, "none", drop_p=p, seed=seed)
    assert torch.equal(y, (keep[0].float() * scale).to(dtype))
    with pytest.raises(RuntimeError):  # no scalar tail: n % 8 != 0 is refused, not half done
        ops.act_drop_fwd(x[:70], y[:70], "none", drop_p=p, seed=seed)


@sp
@pytest.mark.parametrize("cols", [72, 70])  # 8-column vector form / scalar form
def test_act_bwd(cols, seed, p):
    from unified_video_action_amd.native import ops
    rows = 131
    keep, scale = _flat(seed, p, rows, cols)
    dy = torch.ones(rows, cols, device=DEV)
    dx = torch.full_like(dy, float("nan"))
    ops.act_bwd(None, dy, dx, "none", drop_p=p, seed=seed)
    assert torch.equal(dx, keep.float() * scale)


@sp
def test_act_bwd_bias(seed, p):
    from unified_video_action_amd.native import ops
    rows, cols = 131, 264  # two row chunks of 128, two column blocks of 256
    keep, scale = _flat(seed, p, rows, cols)
    dy = torch.ones(rows, cols, device=DEV)
    dx = torch.full_like(dy, float("nan"))
    db = torch.zeros(cols, device=DEV)
    ops.act_bwd_bias(None, dy, dx, db, "none", drop_p=p, seed=seed)
    want = keep.float() * scale
    assert torch.equal(dx, want)
    assert (db.double() - want.double().sum(0)).abs().max().item() <= 1e-5 * rows * scale
    with pytest.raises(RuntimeError):
        ops.act_bwd_bias(None, dy[:, :70].contiguous(), dx[:, :70].contiguous(), db[:70], "none", drop_p=p, seed=seed)


@sp
def test_softmax_fwd(seed, p):
    """Pd of the materialised attention: index (b*H + h)*N*N + q*N + key"""
    from unified_video_action_amd.native import ops
    B, H, N = 2, 2, 72
    th, scale = DM.drop_params(p)
    keep = _t(DM.keep_attn(seed, B, H, N, th))
    S = torch.randn(B, H, N, N, device=DEV)
    P = torch.full_like(S, float("nan"))
    Pd = torch.full_like(S, float("nan"))
    ops.softmax_fwd(S, P, Pd, N, 0.125, drop_p=p, seed=seed)
    assert (P > 0).all()
    assert torch.equal(Pd, torch.where(keep, P * scale, torch.zeros_like(P)))


@sp
def test_softmax_bwd(seed, p):
    """dS = scale * P * (dP' - sum_j P dP'), dP' = dPd * keep * dscale, with dPd = 1: the mask enters the row sum
    and each element.  dS / (scale * P) + the restated row sum recovers dP' = keep * dscale per element; values
    within fp32 rounding of the fp64 form (a row sum of L = 72 terms: L * 2^-24 of it, plus three roundings)"""
    from unified_video_action_amd.native import ops
    B, H, N = 2, 2, 72
    th, scale = DM.drop_params(p)
    keep = _t(DM.keep_attn(seed, B, H, N, th))
    P = torch.softmax(torch.randn(B, H, N, N, device=DEV), dim=-1)
    dS = torch.full_like(P, float("nan"))
    ops.softmax_bwd(P, torch.ones_like(P), dS, N, 0.125, drop_p=p, seed=seed)
    assert torch.isfinite(dS).all()
    dp = keep.double() * scale
    dot = (P.double() * dp).sum(-1, keepdim=True)
    assert torch.equal(dS.double() / (0.125 * P.double()) + dot > 0.5 * scale, keep)
    want = 0.125 * P.double() * (dp - dot)
    assert ((dS.double() - want).abs() <= (N + 3) * 2.0 ** -24 * 0.125 * P.double() * (dp + dot)).all()


@sp
def test_layernorm_bwd_drop(seed, p):
    """dy = 0 makes dx = dx_base = 1 exactly, so drop_out = bf16(keep * scale)"""
    from unified_video_action_amd.native import ops
    rows, D = 200, 768
    keep, scale = _flat(seed, p, rows, D)
    g = torch.Generator(device=DEV).manual_seed(5)
    x = torch.randn(rows, D, device=DEV, generator=g)
    w = torch.rand(D, device=DEV, generator=g) + 0.5
    dy = torch.zeros(rows, D, device=DEV, dtype=BF16)
    mean, rstd = x.mean(1), torch.rsqrt(x.var(1, unbiased=False) + 1e-6)
    base = torch.ones(rows, D, device=DEV)
    dx = torch.full_like(base, float("nan"))
    out = torch.full((rows, D), float("nan"), device=DEV, dtype=BF16)
    dw, db, dbias = (torch.zeros(D, device=DEV) for _ in range(3))
    assert ops.layernorm_bwd_drop(x, w, dy, mean, rstd, dx, dw, db, base, out, p, seed, dbias)
    assert torch.equal(dx, base)
    assert torch.equal(out, (keep.float() * scale).to(BF16))


# ---- attention bit planes ------------------------------------------------------------------------
def _planes(mask, B, N, H):
    nt = N // 64
    w = mask.view(torch.int64).cpu().numpy().view(np.uint64)
    n = B * H * nt * N
    assert w.size == 2 * n
    return w[:n].reshape(B * H, nt, N), w[n:].reshape(B * H, nt, N)


@sp
@pytest.mark.parametrize("B,N,H", [(1, 256, 2), (1, 1088, 1), (2, 128, 2)])
def test_attn_dropmask_planes(B, N, H, seed, p):
    from unified_video_action_amd.native import ops
    th, _ = DM.drop_params(p)
    mq, mk = _planes(ops.attn_dropmask(B, N, H, p, seed, DEV), B, N, H)
    wq, wk = DM.attn_planes(seed, B, H, N, th)
    assert np.array_equal(mq, wq)
    assert np.array_equal(mk, wk)
    if B > 1 and H > 1:  # the bh term of the index is live
        assert not np.array_equal(mq[B * H - 1], mq[0]) and not np.array_equal(mk[B * H - 1], mk[0])


# ---- gemm.hip epilogues --------------------------------------------------------------------------
def _linear_keep_and_scale(x, w, b, out_shape, ld, seed, p):
    """run ops.linear without and with dropout into fp32 outputs (row pitch ld): the dropped run must be
    keep ? plain * scale : 0, bit for bit -- the epilogues scale the fp32 value they would have stored.  Both runs
    carry a zero fp32 residual, so the plain one stays on the same kernel (a bias-only product would go to
    gemm_4w, which sums in another order) and v + 0 changes no bit"""
    from unified_video_action_amd.native import ops
    M, N = out_shape
    keep, scale = _flat(seed, p, M, N)
    zero = torch.zeros(M, N, device=DEV)
    outs = []
    for pp in (0.0, p):
        buf = torch.full((M, ld), float("nan"), device=DEV)
        ops.linear(x, w, buf[:, :N], bias=b, drop_p=pp, seed=seed, residual=zero)
        outs.append(buf[:, :N])
        if ld > N:
            assert buf[:, N:].isnan().all()  # nothing stored past the view
    plain, dropped = outs
    assert (plain > 0).all()
    assert torch.equal(dropped, keep.float() * (plain * scale))


@sp
def test_gemm_generic_epi_store(seed, p):
    """fp32 operands -> gemm_generic, every element through epi_store (gemm.hip)"""
    M, N, K = 70, 50, 24
    g = torch.Generator(device=DEV).manual_seed(1)
    _linear_keep_and_scale(_pos(M, K, dtype=F32, g=g), _pos(N, K, dtype=F32, g=g), _pos(N, dtype=F32, g=g), (M, N), N,
                           seed, p)


@sp
@pytest.mark.parametrize("N,ld", [(200, 200), (201, 208)])
def test_gemm_mfma_epi_apply_row8(N, ld, seed, p):
    """bf16 operands below the 8-phase kernel's shapes -> the 128 x 128 MFMA kernel's staged epilogue
    (epi_apply_row8).  N = 200: every 8-column segment starts at an even index (dropout_keep2); N = 201 in a
    208-pitch view: odd rows start at an odd index (the per-element form) and column 200 goes through epi_store"""
    from unified_video_action_amd.native import ops
    M, K = 300, 64
    assert ops.gemm_plan(M, N, K)[0] == 2
    g = torch.Generator(device=DEV).manual_seed(2)
    _linear_keep_and_scale(_pos(M, K, g=g), _pos(N, K, g=g), _pos(N, dtype=F32, g=g), (M, N), ld, seed, p)


@sp
def test_gemm_8ph_residual_ring(seed, p):
    """bias + dropout + fp32 residual at N % 384 == 0 with >= 96 tiles -> gemm_8ph's 128 x 384 tile and its
    residual-only epilogue ring (the attention proj / fc2 forward of the fp32-accumulator route)"""
    from unified_video_action_amd.native import ops
    M, N, K = 6100, 768, 128
    assert ops.gemm_plan(M, N, K) == (3, 384, 1)
    g = torch.Generator(device=DEV).manual_seed(3)
    res = torch.randn(M, N, device=DEV, generator=g)
    keep, scale = _flat(seed, p, M, N)
    x, w, b = _pos(M, K, g=g), _pos(N, K, g=g), _pos(N, dtype=F32, g=g)
    plain = torch.full_like(res, float("nan"))
    ops.linear(x, w, plain, bias=b, residual=torch.zeros_like(res))
    out = torch.full_like(res, float("nan"))
    ops.linear(x, w, out, bias=b, residual=res, drop_p=p, seed=seed)
    assert (plain > 16).all() and res.abs().max().item() < 8  # a kept element cannot equal its residual
    assert torch.equal(out == res, ~keep)
    # kept: plain * scale + res in fp32, as two roundings or one fused multiply-add
    want = torch.where(keep, plain.double() * scale + res.double(), res.double())
    assert ((out.double() - want).abs() <= 2.0 ** -22 * want.abs()).all()


@sp
def test_linear_dx_act(seed, p):
    """dx = gelu'(pre) * drop(dy @ w), index row * K + col: pre = 0 gives gelu' = 1/2 everywhere"""
    from unified_video_action_amd.native import ops
    M, N, K = 300, 64, 200
    keep, _ = _flat(seed, p, M, K)
    g = torch.Generator(device=DEV).manual_seed(4)
    dy, w = _pos(M, N, g=g), _pos(N, K, g=g)
    pre = torch.zeros(M, K, device=DEV, dtype=BF16)
    dx = torch.full((M, K), float("nan"), device=DEV, dtype=BF16)
    ops.linear_dx_act(dy, w, dx, pre, "gelu", drop_p=p, seed=seed)
    _same_keep(dx, keep)
    want = 0.5 * (dy.double() @ w.double())
    want = want * DM.drop_params(p)[1]  # one bf16 rounding of the fp32 value: 2^-8 relative (gelu'(0) to 1.5e-7)
    assert ((dx.double() - torch.where(keep, want, torch.zeros_like(want))).abs() <= 2.0 ** -8 * want).all()


# ---- gemm8w.hip fused epilogues ------------------------------------------------------------------
@pytest.fixture(params=[64, 32])
def form(request):
    """gemm_8w launch forms: 64 one 8-wave workgroup per CU, 32 two 4-wave workgroups per CU"""
    from unified_video_action_amd.native import ops
    prev = ops.gemm8w_set(-2, request.param)
    yield request.param
    ops.gemm8w_set(-2, prev[1])


@sp
@pytest.mark.parametrize("which", ["fc1", "fc2", "dgelu"])
@pytest.mark.parametrize("N,plane", [(200, False), (224, True)])  # the plane form needs N % 32 == 0
def test_gemm8w_fused_epilogues(N, plane, which, seed, p, form):
    from unified_video_action_amd.native import ops
    M, K = 300, 256
    keep, scale = _flat(seed, p, M, N)
    g = torch.Generator(device=DEV).manual_seed(6)
    pl = ops.dropout_plane(M * N, p, seed, DEV) if plane else None
    x, w = _pos(M, K, g=g), _pos(N, K, lo=0.01, hi=0.03, g=g)
    b = _pos(N, dtype=F32, g=g)
    if which == "fc1":
        pre = torch.full((M, N), float("nan"), device=DEV, dtype=BF16)
        out = torch.full_like(pre, float("nan"))
        assert ops.linear_gelu_drop(x, w, b, pre, out, drop_p=p, seed=seed, plane=pl)
        assert (pre > 0).all()
        _same_keep(out, keep)
    elif which == "fc2":
        zero = torch.zeros(M, N, device=DEV)
        plain = torch.full_like(zero, float("nan"))
        out = torch.full_like(zero, float("nan"))
        assert ops.linear_drop_res(x, w, b, zero, plain, drop_p=0.0, seed=seed)
        assert ops.linear_drop_res(x, w, b, zero, out, drop_p=p, seed=seed, plane=pl)
        assert (plain > 0).all()
        assert torch.equal(out, keep.float() * (plain * scale))  # plain = the bf16 product; one fp32 multiply
    else:
        pre = torch.zeros(M, N, device=DEV, dtype=BF16)  # gelu'(0) = 1/2
        dpre = torch.full((M, N), float("nan"), device=DEV, dtype=BF16)
        db = torch.zeros(N, device=DEV)
        assert ops.linear_dgelu_drop(x, w, pre, dpre, db, drop_p=p, seed=seed, plane=pl)
        _same_keep(dpre, keep)
