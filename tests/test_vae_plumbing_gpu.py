"""The KL-VAE plumbing kernels of csrc/vae.hip against float64 references at their edge shapes:
GroupNorm statistics (every legal width class, a chunk boundary, a ragged last chunk), GroupNorm apply,
the posterior sample (NHWC moments against NCHW eps) and the frame select + bilinear resize.

Every comparison is per element, |got - ref| <= rtol * |ref| + atol with atol tied to a stated quantity
(never a fraction of the tensor's maximum), on the values the kernel read (a bf16 input is rounded first,
the reference reads the rounded value).  Outputs live NaN-filled inside a larger sentinel-filled buffer:
an unwritten element fails as NaN, a write outside the output fails the guard check."""
import pytest
import torch

from edge_helpers import BF16, DEV, F32, assert_within, flat_out, gen

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------
# 1. groupnorm_stats
# ---------------------------------------------------------------------------------------------------
# every width class of gn_partial_kernel: 256 % C == 0 (32, 64, 128, 256), C < 256 with a partial last
# lane group (96, 160, 192, 224), C > 256 (384, 512); HW: one pixel, one chunk, exactly one chunk (1024),
# one pixel past it (1025), a ragged third chunk (2500)
GN_CASES = [
    (32, 100, 3, F32), (64, 1024, 1, BF16), (96, 100, 1, F32), (96, 1025, 3, F32), (96, 2500, 1, BF16),
    (128, 2500, 1, F32), (160, 1025, 1, F32), (192, 1025, 1, BF16), (192, 2500, 3, F32), (224, 100, 1, BF16),
    (256, 1, 3, F32), (256, 1025, 1, BF16), (384, 1025, 1, F32), (512, 1, 1, BF16), (512, 100, 3, F32),
]


@pytest.mark.parametrize("C,HW,Nimg,dtype", GN_CASES, ids=lambda v: str(v).replace("torch.", ""))
def test_groupnorm_stats(C, HW, Nimg, dtype):
    """scale = gamma * rstd, shift = beta - mean * scale per (image, channel) against float64 statistics of
    the stored input; bounds of tests/test_conv_halo_gpu.py for the same quantities, per element:
    |scale - ref| <= 1e-4 |ref|, |shift - ref| <= 1e-4 (|beta| + |mean * scale_ref|)."""
    from unified_video_action_amd.native import ops
    g = gen(1000 + C * 7 + HW)
    gs = C // 32
    mu = torch.rand(Nimg, 1, 32, 1, generator=g) * 4 - 2
    sigma = torch.rand(Nimg, 1, 32, 1, generator=g) * 1.5 + 0.5
    x = (mu + sigma * torch.randn(Nimg, HW, 32, gs, generator=g)).reshape(Nimg, HW, C).to(dtype).to(DEV)
    gamma = (1.0 + 0.5 * torch.randn(C, generator=g)).to(DEV)
    beta = torch.randn(C, generator=g).to(DEV)
    eps = 1e-6
    gsc, scale = flat_out(Nimg * C, F32)
    gsh, shift = flat_out(Nimg * C, F32)
    ops.groupnorm_stats(x, Nimg, HW, C, gamma, beta, scale, shift, eps=eps)
    gsc.check()
    gsh.check()
    xd = x.double().view(Nimg, HW, 32, gs)
    mean = xd.mean(dim=(1, 3))  # [Nimg, 32]
    var = (xd - mean[:, None, :, None]).pow(2).mean(dim=(1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    mean_c, rstd_c = mean.repeat_interleave(gs, dim=1), rstd.repeat_interleave(gs, dim=1)  # [Nimg, C]
    sc_ref = gamma.double()[None] * rstd_c
    sh_ref = beta.double()[None] - mean_c * sc_ref
    assert_within(scale.view(Nimg, C), sc_ref, 1e-4 * sc_ref.abs(), "scale")
    assert_within(shift.view(Nimg, C), sh_ref, 1e-4 * (beta.double().abs()[None] + (mean_c * sc_ref).abs()), "shift")


# ---------------------------------------------------------------------------------------------------
# 2. groupnorm_apply
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("silu", [True, False], ids=["silu", "affine"])
@pytest.mark.parametrize("C,HW,Nimg", [(8, 37, 3), (8, 1, 1), (128, 37, 3), (128, 256, 1), (520, 1, 3),
                                        (520, 37, 1), (520, 256, 3)])
def test_groupnorm_apply(C, HW, Nimg, silu):
    """y = bf16(act(x * scale[n, c] + shift[n, c])) on NHWC bf16 maps.  Bound 2^-8 |ref| (the bf16 store;
    the fast exponential's relative error is far inside it) + 2^-22 (|x scale| + |shift|) (fp32 rounding of
    the product and of the sum, carried through SiLU whose slope is at most 1.1).  The images' scales
    differ by 2x and more, so an image index taken from the wrong quotient shows."""
    from unified_video_action_amd.native import ops
    g = gen(2000 + C + HW)
    x = torch.randn(Nimg, HW, C, generator=g).to(BF16).to(DEV)
    per_img = torch.tensor([1.0, 2.5, -6.0])[:Nimg, None]
    scale = (per_img * (1.0 + 0.2 * torch.randn(Nimg, C, generator=g))).to(DEV)
    shift = (per_img.flip(0) * 0.5 * torch.randn(Nimg, C, generator=g)).to(DEV)
    gy, y = flat_out(Nimg * HW * C, BF16)
    ops.groupnorm_apply(x, scale, shift, y, Nimg, HW, C, silu=silu)
    gy.check()
    prod = x.double() * scale.double()[:, None, :]
    u = prod + shift.double()[:, None, :]
    ref = u * torch.sigmoid(u) if silu else u
    bound = 2.0 ** -8 * ref.abs() + 2.0 ** -22 * (prod.abs() + shift.double().abs()[:, None, :])
    assert_within(y.view(Nimg, HW, C), ref, bound, "y")


# ---------------------------------------------------------------------------------------------------
# 3. posterior_sample
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tok_scale", [0.2325, 1.75])
@pytest.mark.parametrize("mdt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Nimg", [1, 3])
def test_posterior_sample(Nimg, mdt, tok_scale):
    """z[n, s, c] = (mean[n, s, c] + exp(0.5 clamp(logvar[n, s, c], -30, 20)) eps[n, c, s]) * scale: the
    moments are NHWC [n, 256, 32], eps is NCHW [n, 16, 16, 16] (randn: no symmetry hides the transposition).
    Bound 1e-6 (|mean| + |std eps|) scale (a few fp32 roundings and expf's 1-2 ulp)."""
    from unified_video_action_amd.native import ops
    g = gen(3000 + Nimg)
    mean = torch.randn(Nimg, 256, 16, generator=g)
    lv = torch.randn(Nimg, 256, 16, generator=g) * 3
    edge = torch.tensor([-30.0, 20.0, -30.5, -31.0, -45.0, -1000.0, 20.5, 21.0, 50.0, 1000.0, -29.5, 19.5])
    lv.view(-1)[torch.randperm(lv.numel(), generator=g)[:edge.numel() * 8]] = edge.repeat(8)
    mom = torch.cat([mean, lv], dim=2).to(mdt).to(DEV)  # [Nimg, 256, 32]
    eps = torch.randn(Nimg, 16, 16, 16, generator=g).to(DEV)
    gz, z = flat_out(Nimg * 256 * 16, F32)
    ops.posterior_sample(mom, eps, z, Nimg, scale=tok_scale)
    gz.check()
    md = mom.double()
    std = torch.exp(0.5 * md[..., 16:].clamp(-30.0, 20.0))
    e = eps.double().view(Nimg, 16, 256).transpose(1, 2)  # [n, s, c]
    ref = (md[..., :16] + std * e) * tok_scale
    bound = 1e-6 * (md[..., :16].abs() + (std * e).abs()) * tok_scale
    assert_within(z.view(Nimg, 256, 16), ref, bound, "z")


# ---------------------------------------------------------------------------------------------------
# 4. resize_select
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("odt", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Hin,Win", [(96, 128), (240, 320)])
def test_resize_select(Hin, Win, odt):
    """B = 2, T = 5, four distinct non-monotonic frames, non-square input, Cpad = 8.  Output images: every
    sample's future frames (sel[half:]) first, then the history frames (sel[:half]); each block runs over
    b then f.  Reference: float64 F.interpolate(bilinear, align_corners=False) of the selected frames, then
    x * 255 / 127.5 - 1.  Bound: the existing test's rtol 1e-5 / atol 2e-6 on the pixel in [0, 1], carried
    through the exact affine map (slope 2); a bf16 store adds 2^-8 |ref|.  Channels 3..7 are exactly zero."""
    from unified_video_action_amd.native import ops
    B, T, Cpad = 2, 5, 8
    g = gen(4000 + Hin)
    img = (0.5 + 0.25 * torch.randn(B, T, 3, Hin, Win, generator=g)).to(DEV)
    sel_l = [3, 0, 4, 1]
    sel = torch.tensor(sel_l, dtype=torch.int32, device=DEV)
    nsel, half = 4, 2
    go, out = flat_out(B * nsel * 256 * 256 * Cpad, odt)
    ops.resize_select(img, sel, out, Cpad)
    go.check()
    out = out.view(B * nsel, 256, 256, Cpad)
    order = [(b, f) for part in (sel_l[half:], sel_l[:half]) for b in range(B) for f in part]
    frames = torch.stack([img[b, f] for b, f in order]).double()  # [B nsel, 3, Hin, Win]
    pix = torch.nn.functional.interpolate(frames, size=256, mode="bilinear", align_corners=False)
    ref = (pix * 255.0 / 127.5 - 1.0).permute(0, 2, 3, 1)
    bound = 2.0 * (1e-5 * pix.abs() + 2e-6).permute(0, 2, 3, 1)
    if odt == BF16:
        bound = bound + 2.0 ** -8 * ref.abs()
    assert_within(out[..., :3], ref, bound, "pixels")
    assert not torch.isnan(out[..., 3:].float()).any()
    assert (out[..., 3:] == 0).all(), "padding channels must be exactly zero"
