"""Every route of uva_conv2d (csrc/conv.hip: conv3x3_halo_plain, conv3x3_halo_gn, conv3x3_gn_pt,
conv3x3s2_kernel, conv_in_kernel; csrc/gemm.hip: the TA == 2 loaders of gemm_mfma_v2, gemm_mfma_bf16,
gemm_8ph and gemm_generic) per element against the float64 reference of tests/conv_ref.py:

    out = bias + residual + conv_{ks,stride,pad}(act(x * scale[n, c] + shift[n, c]))

Link 1 (no SiLU): dyadic inputs, every partial sum exact in fp32, output torch.equal to the reference
(rounded once to bf16 for a bf16 output).  Link 2 (SiLU): quarter-grid z clear of bf16 ties, per element
2^-8 |ref| + (ks^2 Ci + 8) u S.  Outputs and partial-sum buffers are NaN-filled inside sentinel guards;
every case asserts its route by query; the raw fused GroupNorm partials are compared per (image, group)
with the sums of the stored output at (T + 8) u sum|terms|, and finalized once more in the 1e-4 form of
test_conv_halo_gpu.py.  The controls of these comparisons run on the CPU (test_conv_exact_cpu.py).
The shapes are the smallest at which each form can still go wrong (chunk counts 1 / 2 / 3, two Co blocks,
fewer tiles than workgroups, a partial last persistent round, M below one row tile)."""
import pytest
import torch

import conv_ref as R
from conv_ref import BF16, DOWN, F32, NOPAD, SAME3
from edge_helpers import DEV, Guarded, assert_within

pytestmark = pytest.mark.gpu

GEN, STAGED, DMA, PH8 = 0, 1, 2, 3   # ops.gemm_plan kernel codes


def _ops():
    from unified_video_action_amd.native import ops
    return ops


def _plan(n, Ho, Wo, Ci, Co, ks, gn=False, dtype=BF16):
    """the kernel uva_conv2d's implicit-GEMM route picks (it passes no split-K workspace)"""
    return _ops().gemm_plan(n * Ho * Wo, Co, ks * ks * Ci, ta=2, splitk=False, gn_prologue=gn, dtype=dtype)[0]


def _s2_ok(n, H, W, Ci, Co):
    from unified_video_action_amd.native.lib import lib
    return lib().query("uva_conv3x3s2_ok", n, H, W, Ci, Co) > 0


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pt_images():
    """images of 64 x 64 (32 tiles of 8 x 16 each) for ~2.5 x CUs tiles: the persistent grid is 2 x CUs
    workgroups, so its second round is partial"""
    return (5 * _cus() // 2 + 31) // 32


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def check_finalize(part, stored, n, HW, Co, seed):
    """groupnorm_finalize_tiles of the fused partials == GroupNorm(32) statistics of the stored output
    (the 1e-4 form of test_conv_halo_gpu.py)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    gamma = torch.randn(Co, generator=g).to(DEV)
    beta = torch.randn(Co, generator=g).to(DEV)
    gsc = torch.empty(n, Co, device=DEV)
    gsh = torch.empty(n, Co, device=DEV)
    _ops().groupnorm_finalize_tiles(part, n, HW, Co, gamma, beta, gsc, gsh, eps=1e-6)
    o = stored.double().reshape(n, HW, 32, Co // 32)
    mean = o.mean(dim=(1, 3))
    rstd = (o.var(dim=(1, 3), unbiased=False) + 1e-6).rsqrt()
    sc_ref = gamma.double()[None] * rstd.repeat_interleave(Co // 32, dim=1)
    sh_ref = beta.double()[None] - mean.repeat_interleave(Co // 32, dim=1) * sc_ref
    assert rel_err(gsc, sc_ref) < 1e-4
    assert rel_err(gsh, sh_ref) < 1e-4


def silu_close(got, ref, S, K):
    """link 2's assertion; prints the worst |got - ref| / bound first"""
    print(f"worst |got - ref| / bound = {float(((got.double() - ref).abs() / R.silu_bound(ref, S, K)).max()):.3f}")
    R.assert_silu_close(got, ref, S, K, "output")


def run(n, H, W, Ci, Co, ks=3, stride=1, gn=None, residual=False, part=False, dtype=BF16, force_generic=False,
        ci_used=None, seed=0):
    """one conv launch into guarded buffers + the float64 reference -> (stored output [n, Ho, Wo, Co], ref, S).
    gn: None / "affine" (GroupNorm prologue without SiLU, link 1 data) / "silu" (link 2 data).  Link 1 is
    asserted here (input regime, bit equality); the guards and the partial sums on both links."""
    ops = _ops()
    down = stride == 2
    pads = NOPAD if ks == 1 else DOWN if down else SAME3
    Ho, Wo = H // stride, W // stride
    if gn == "silu":
        c = R.silu_case(seed, n, H, W, Ci, Co, ks, Ho, Wo, residual=residual, dtype=dtype, device=DEV)
        R.assert_silu_regime(c["x"], c["scale"], c["shift"])
    else:
        c = R.exact_case(seed, n, H, W, Ci, Co, ks, Ho, Wo, gn=gn is not None, residual=residual, dtype=dtype,
                         ci_used=ci_used, device=DEV)
    ref, S, a = R.conv_ref(c["x"], c["w"], ks, stride, pads, c["bias"], c["res"], c["scale"], c["shift"],
                           silu=gn == "silu", store=BF16 if dtype == BF16 else None)
    assert ref.shape == (n, Ho, Wo, Co)
    if gn != "silu":
        R.assert_exact_regime(a, S)
    og = Guarded(n * Ho * Wo, Co, dtype)
    pg = Guarded(n * Ho * Wo // 128, 64, F32) if part else None
    pad = 0 if ks == 1 or down else 1
    ops.conv2d(c["x"], c["w"], og.view, n, H, W, Ci, Co, ks, stride, pad, pad, Ho, Wo, bias=c["bias"],
               residual=c["res"], gn_scale=c["scale"], gn_shift=c["shift"], gn_silu=gn == "silu",
               force_generic=force_generic, gn_part=pg.view if part else None)
    og.check()
    got = og.view.view(n, Ho, Wo, Co)
    if gn != "silu":
        R.assert_bit_equal(got, ref, "output")
    if part:
        pg.check()
        R.assert_partials(pg.view.view(-1, 32, 2), got, n, Co, "gn_part")
        check_finalize(pg.view.view(-1, 32, 2), got, n, Ho * Wo, Co, seed + 1)
    return got, ref, S


# ---------------------------------------------------------------- csrc/conv.hip, link 1
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("n,H,W,Ci,Co", [(2, 16, 16, 64, 128), (1, 32, 16, 192, 256), (3, 16, 32, 128, 128)])
def test_halo_plain_exact(n, H, W, Ci, Co, residual):
    """conv3x3_halo_plain: one chunk; three chunks (the halo double buffer and the weight ring end on the
    odd slot) with two Co blocks; two chunks, three images"""
    assert _ops().conv_fuses_gn(n, H, W, Ci, Co, 3, 1)
    run(n, H, W, Ci, Co, residual=residual, part=True, seed=100 + Ci + int(residual))


@pytest.mark.parametrize("n,H,W,Ci,Co,residual", [(2, 16, 16, 64, 128, False), (2, 16, 16, 64, 128, True),
                                                  (1, 16, 32, 192, 256, False), (1, 16, 32, 192, 256, True),
                                                  (2, 32, 16, 128, 128, True)])
def test_halo_gn_affine_exact(n, H, W, Ci, Co, residual):
    """conv3x3_halo_gn<false>; at Ci = Co = 128 only with a residual (without one the persistent kernel runs)"""
    assert _ops().conv_fuses_gn(n, H, W, Ci, Co, 3, 1)
    assert not (Ci == 128 and Co == 128 and not residual)
    run(n, H, W, Ci, Co, gn="affine", residual=residual, part=True, seed=200 + Ci + int(residual))


def _pt_case(case):
    return {"two_tiles": (1, 16, 16), "three_images": (3, 16, 48), "partial_round": (_pt_images(), 64, 64)}[case]


@pytest.mark.parametrize("case", ["two_tiles", "three_images", "partial_round"])
def test_gn_pt_affine_exact(case):
    """conv3x3_gn_pt<false> (Ci = Co = 128, no residual): 2 tiles (fewer than workgroups), 18 tiles over
    three images, and ~2.5 x CUs tiles (the persistent loop's partial last round)"""
    n, H, W = _pt_case(case)
    tiles = n * (H // 8) * (W // 16)
    assert _ops().conv_fuses_gn(n, H, W, 128, 128, 3, 1)
    assert (tiles > 2 * _cus()) == (case == "partial_round") and tiles % (2 * _cus()) != 0
    run(n, H, W, 128, 128, gn="affine", part=True, seed=300 + H)


@pytest.mark.parametrize("part", [False, True])
@pytest.mark.parametrize("n,H,W,Ci,Co", [(2, 16, 32, 64, 128), (1, 32, 64, 192, 256), (1, 48, 32, 128, 128)])
def test_s2_exact(n, H, W, Ci, Co, part):
    """conv3x3s2_kernel (Downsample: pad right / bottom by one, stride 2, pad 0); the padded column and row
    meet non-zero weights like every other tap"""
    assert _s2_ok(n, H, W, Ci, Co)
    run(n, H, W, Ci, Co, stride=2, part=part, seed=400 + Ci)


@pytest.mark.parametrize("n,H,W", [(3, 16, 16), (1, 48, 48), (2, 32, 48)])
def test_conv_in_exact(n, H, W):
    """conv_in_kernel (Ci 8, channels 3..7 zero in x and w): 3 tiles (less than one workgroup's 4), 9 tiles
    (a partial last workgroup), 12 tiles over two images"""
    assert not _ops().conv_fuses_gn(n, H, W, 8, 128, 3, 1) and H % 16 == 0 and W % 16 == 0
    run(n, H, W, 8, 128, part=True, ci_used=3, seed=500 + H)


# ---------------------------------------------------------------- csrc/gemm.hip conv loaders, link 1
@pytest.mark.parametrize("n,H,W,Ci,Co,ks,residual,part", [
    (2, 16, 16, 512, 512, 1, True, True),     # proj_out: 1x1 + residual + partials
    (2, 16, 16, 16, 512, 3, False, True),     # decoder.conv_in
    (2, 16, 16, 512, 32, 3, False, False),    # encoder.conv_out
    (1, 16, 16, 128, 8, 3, False, False),     # decoder.conv_out
    (1, 12, 20, 96, 256, 3, False, False),    # M = 240: no whole 128-row tile, H and W no multiples of 16
])
def test_loader_dma_exact(n, H, W, Ci, Co, ks, residual, part):
    """gemm_mfma_v2<2, 0>: the LDS-DMA conv gather"""
    assert not _ops().conv_fuses_gn(n, H, W, Ci, Co, ks, 1)
    assert _plan(n, H, W, Ci, Co, ks) == DMA
    run(n, H, W, Ci, Co, ks=ks, residual=residual, part=part, seed=600 + Ci + Co)


def test_loader_staged_gn_affine_exact():
    """gemm_mfma_bf16<2, 0>: the register-staged loader with a GroupNorm prologue, no SiLU"""
    n, H, W, Ci, Co = 1, 12, 20, 96, 256
    assert not _ops().conv_fuses_gn(n, H, W, Ci, Co, 3, 1)
    assert _plan(n, H, W, Ci, Co, 3, gn=True) == STAGED
    run(n, H, W, Ci, Co, gn="affine", seed=700)


def test_loader_8phase_exact():
    """gemm_8ph<2, 0> at the smallest image count for which the plan answers it at 64 x 64, Ci 96, Co 256"""
    H, W, Ci, Co = 64, 64, 96, 256
    n = next(i for i in range(1, 65) if _plan(i, H, W, Ci, Co, 3) == PH8)
    assert not _ops().conv_fuses_gn(n, H, W, Ci, Co, 3, 1)
    run(n, H, W, Ci, Co, part=True, seed=710)


@pytest.mark.parametrize("n,H,W,Ci,Co,stride", [(1, 16, 32, 64, 128, 2), (1, 12, 20, 12, 40, 1)])
def test_loader_generic_bf16_exact(n, H, W, Ci, Co, stride):
    """gemm_generic's scalar conv gather on bf16: force_generic at stride 2 (a shape the stride-2 halo kernel
    would take), and Ci 12 (no multiple of 8: the dispatcher's own fallback)"""
    if stride == 2:
        assert _s2_ok(n, H, W, Ci, Co)
    else:
        assert Ci % 8 != 0 and _plan(n, H, W, Ci, Co, 3) == GEN
    run(n, H, W, Ci, Co, stride=stride, force_generic=stride == 2, seed=720 + Ci)


@pytest.mark.parametrize("gn", [None, "affine"])
def test_loader_generic_f32_exact(gn):
    """fp32 in and out (gemm_generic<float, float, 2, 0>), plain and with a GroupNorm prologue without SiLU"""
    n, H, W, Ci, Co = 1, 12, 20, 24, 40
    assert _plan(n, H, W, Ci, Co, 3, gn=gn is not None, dtype=F32) == GEN
    assert not _ops().conv_fuses_gn(n, H, W, Ci, Co, 3, 1, dtype=F32)
    run(n, H, W, Ci, Co, gn=gn, dtype=F32, seed=730)


# ---------------------------------------------------------------- link 2: SiLU
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("n,H,W,Ci,Co", [(2, 16, 16, 64, 128), (1, 16, 32, 192, 256)])
def test_halo_gn_silu(n, H, W, Ci, Co, residual):
    """conv3x3_halo_gn<true>"""
    assert _ops().conv_fuses_gn(n, H, W, Ci, Co, 3, 1)
    got, ref, S = run(n, H, W, Ci, Co, gn="silu", residual=residual, part=True, seed=800 + Ci + int(residual))
    silu_close(got, ref, S, 9 * Ci)


@pytest.mark.parametrize("case", ["two_tiles", "partial_round"])
def test_gn_pt_silu(case):
    """conv3x3_gn_pt<true>"""
    n, H, W = _pt_case(case)
    tiles = n * (H // 8) * (W // 16)
    assert _ops().conv_fuses_gn(n, H, W, 128, 128, 3, 1)
    assert (tiles > 2 * _cus()) == (case == "partial_round") and tiles % (2 * _cus()) != 0
    got, ref, S = run(n, H, W, 128, 128, gn="silu", part=True, seed=810 + H)
    silu_close(got, ref, S, 9 * 128)


def test_loader_staged_gn_silu():
    """gemm_mfma_bf16<2, 0> with GroupNorm + SiLU staged in registers"""
    n, H, W, Ci, Co = 1, 12, 20, 96, 256
    assert _plan(n, H, W, Ci, Co, 3, gn=True) == STAGED
    got, ref, S = run(n, H, W, Ci, Co, gn="silu", seed=820)
    silu_close(got, ref, S, 9 * Ci)


def test_loader_generic_f32_silu():
    """fp32 generic loader with GroupNorm + SiLU: (2e-6 + (K + 8) u) S, the activation unrounded"""
    n, H, W, Ci, Co = 1, 12, 20, 24, 40
    assert _plan(n, H, W, Ci, Co, 3, gn=True, dtype=F32) == GEN
    got, ref, S = run(n, H, W, Ci, Co, gn="silu", dtype=F32, seed=830)
    bound = R.f32_silu_bound(S, 9 * Ci)
    print(f"fp32 SiLU loader: worst |got - ref| / bound = {float(((got.double() - ref).abs() / bound).max()):.3f}")
    assert_within(got, ref, bound, "output")
