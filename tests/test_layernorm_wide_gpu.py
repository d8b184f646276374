"""LayerNorm forward / backward above D 1024 (mar_huge's 1280, and 2048, the widest the 4-wide route serves)
against float64, by the bounds tests/test_small_kernels_gpu.py applies at D 256 / 512 / 1000 (its
check_ln_forward and the dx / dw / db / dscale / dshift bounds, restated here with the wider D).

Rows 1, 5 and 67: fewer than the block's 4 waves, across them, and past the 64 rows of one backward partial
block.  Dtypes x -> y: fp32 -> fp32, fp32 -> bf16, bf16 -> bf16 (the three forms the C ABI serves), affine and
adaLN-modulated; dw / db with accum_wb off and on.  D = 1284 (above 1024, no multiple of 256) still raises."""
import pytest
import torch

from edge_helpers import BF16, DEV, F32, Guarded, assert_within, gen
from test_small_kernels_gpu import U8, U24, check_ln_forward

pytestmark = pytest.mark.gpu

WIDE_D = [1280, 2048]
WIDE_ROWS = [1, 5, 67]
COMBOS = [(F32, F32), (F32, BF16), (BF16, BF16)]
IDS = {(F32, F32): "f32-f32", (F32, BF16): "f32-bf16", (BF16, BF16): "bf16-bf16"}


def _inputs(rows, D, tin, g):
    """rows whose mean is about 10x their std, rounded to the input dtype; float64 statistics of the stored x"""
    x = (10.0 + torch.randn(rows, D, generator=g)).to(tin).to(DEV)
    xd = x.double()
    mean = xd.mean(-1)
    rstd = 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + 1e-6)
    return x, mean, rstd


def _dx_bound(rs, gg, xh):
    return 1e-5 * rs * (gg.abs() + gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True))


@pytest.mark.parametrize("accum_wb", [False, True], ids=["set", "accum"])
@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: IDS[c])
@pytest.mark.parametrize("rows", WIDE_ROWS)
@pytest.mark.parametrize("D", WIDE_D)
def test_layernorm_affine_wide(D, rows, combo, accum_wb):
    from unified_video_action_amd.native import ops
    tin, tout = combo
    g = gen(9400 + D + rows)
    x, mean, rstd = _inputs(rows, D, tin, g)
    w = (1.0 + 0.1 * torch.randn(D, generator=g)).to(DEV)
    b = (0.1 * torch.randn(D, generator=g)).to(DEV)
    gy = Guarded(rows, D, tout)
    gm, gr = Guarded(1, rows, F32), Guarded(1, rows, F32)
    ops.layernorm_fwd(x, w, b, gy.view, gm.view.view(-1), gr.view.view(-1))
    for q in (gy, gm, gr):
        q.check()
    check_ln_forward(gy, gm, gr, x, mean, rstd, D, w.double()[None].expand(rows, D), b.double()[None].expand(rows, D),
                     tout)

    mean32, rstd32 = mean.float(), rstd.float()
    dy = torch.randn(rows, D, generator=g).to(DEV)
    gdx = Guarded(rows, D, F32)
    w0 = (0.5 * torch.randn(1, D, generator=g)).to(DEV) if accum_wb else None
    b0 = (0.5 * torch.randn(1, D, generator=g)).to(DEV) if accum_wb else None
    gdw, gdb = Guarded(1, D, F32, init=w0), Guarded(1, D, F32, init=b0)
    ops.layernorm_bwd(x, w, dy, mean32, rstd32, gdx.view, accum=False, dw=gdw.view.view(-1), db=gdb.view.view(-1),
                      accum_wb=accum_wb, out_dtype=ops.dt(gy.view))
    for q in (gdx, gdw, gdb):
        q.check()
    xh = (x.double() - mean32.double()[:, None]) * rstd32.double()[:, None]
    gg = dy.double() * w.double()
    m1, m2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    rs = rstd32.double()[:, None]
    assert_within(gdx.view, rs * (gg - m1 - xh * m2), _dx_bound(rs, gg, xh), "dx")
    tw = dy.double() * xh
    base_w = w0.double().view(-1) if accum_wb else 0.0
    base_b = b0.double().view(-1) if accum_wb else 0.0
    extra_w = U24 * w0.double().abs().view(-1) if accum_wb else 0.0  # the add onto the existing gradient
    extra_b = U24 * b0.double().abs().view(-1) if accum_wb else 0.0
    assert_within(gdw.view.view(-1), tw.sum(0) + base_w, (rows + 8) * U24 * tw.abs().sum(0) + extra_w, "dw")
    assert_within(gdb.view.view(-1), dy.double().sum(0) + base_b,
                  (rows + 8) * U24 * dy.double().abs().sum(0) + extra_b, "db")


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: IDS[c])
@pytest.mark.parametrize("rows", WIDE_ROWS)
@pytest.mark.parametrize("D", WIDE_D)
def test_layernorm_modulated_wide(D, rows, combo):
    """y = xhat (1 + scale) + shift with shift / scale the first two thirds of a [rows, 3 D] buffer of the output
    dtype; dscale = dy xhat and dshift = dy to their stores' rounding, the last third of dmod untouched"""
    from unified_video_action_amd.native import ops
    tin, tout = combo
    g = gen(9500 + D + rows)
    x, mean, rstd = _inputs(rows, D, tin, g)
    mod = (0.3 * torch.randn(rows, 3 * D, generator=g)).to(tout).to(DEV)
    shift, scale = mod[:, :D], mod[:, D:2 * D]
    gy = Guarded(rows, D, tout)
    gm, gr = Guarded(1, rows, F32), Guarded(1, rows, F32)
    ops.layernorm_fwd(x, None, None, gy.view, gm.view.view(-1), gr.view.view(-1), scale=scale, shift=shift, ldm=3 * D)
    for q in (gy, gm, gr):
        q.check()
    check_ln_forward(gy, gm, gr, x, mean, rstd, D, 1.0 + scale.double(), shift.double(), tout)

    mean32, rstd32 = mean.float(), rstd.float()
    dy = torch.randn(rows, D, generator=g).to(DEV)
    gdx = Guarded(rows, D, F32)
    gdm = Guarded(rows, 2 * D, tout, ld=3 * D, off=0)
    ops.layernorm_bwd(x, None, dy, mean32, rstd32, gdx.view, accum=False, scale=scale, ldm=3 * D,
                      dscale=gdm.view[:, D:], dshift=gdm.view[:, :D])
    gdx.check()
    gdm.check()
    xh = (x.double() - mean32.double()[:, None]) * rstd32.double()[:, None]
    gg = dy.double() * (1.0 + scale.double())
    m1, m2 = gg.mean(-1, keepdim=True), (gg * xh).mean(-1, keepdim=True)
    rs = rstd32.double()[:, None]
    assert_within(gdx.view, rs * (gg - m1 - xh * m2), _dx_bound(rs, gg, xh), "dx")
    rnd = 2.0 ** -22 if tout == F32 else U8
    ds_ref = dy.double() * xh
    assert_within(gdm.view[:, D:], ds_ref, rnd * ds_ref.abs(), "dscale")
    assert_within(gdm.view[:, :D], dy.double(), (0.0 if tout == F32 else U8) * dy.double().abs(), "dshift")


def test_layernorm_width_off_the_wide_route_still_raises():
    """D = 1280 + 4: above 1024 and no multiple of 256 -> hipErrorInvalidValue before any launch (forward, backward)"""
    from unified_video_action_amd.native import ops
    D, rows = 1284, 5
    x = torch.randn(rows, D, device=DEV)
    y = torch.empty_like(x)
    m, r = torch.empty(rows, device=DEV), torch.empty(rows, device=DEV)
    with pytest.raises(RuntimeError, match="uva_layernorm_fwd"):
        ops.layernorm_fwd(x, None, None, y, m, r)
    with pytest.raises(RuntimeError, match="uva_layernorm_bwd"):
        ops.layernorm_bwd(x, None, torch.randn_like(x), m.zero_(), r.fill_(1.0), torch.empty_like(x), accum=False)
