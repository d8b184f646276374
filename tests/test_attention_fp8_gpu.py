"""FP8 (OCP e4m3) attention -- the "fp8_attn" precision of BASELINE config 5 (UMI-multi):

  * uva_attn_quant_fp8 rounds qkv in place exactly as torch's float8_e4m3fn cast of x * 2^-e
    (per (batch, head, q|k|v, 64-row tile) power-of-two scales, amax * 2^-e <= 448) and writes
    the fp8 Q/K rows and the key-permuted V^T (the block-scaled 32x32x64 MFMA operand order);
  * the fp8 forward vs an fp32 torch softmax attention of the SAME fp8-rounded inputs, at N = 1088
    (UMI/Libero tokens, 64-key tiles) and N = 1024 (128-key tiles), with and without dropout:
    log-sum-exp within 1e-4 (exact products of the e4m3 codes, fp32 sums), O within 2^-4 of max|O| at worst (P
    is itself rounded to e4m3 for the P.V product: <= 2^-4 relative per element, reached on rows
    that one key dominates) and within 5e-3 of it on average;
  * the backward (bf16 kernels on the rounded q/k/v with the fp8 forward's lse and O: the
    straight-through gradient) vs its fp32 restatement, 3e-2 of max|grad|, and its mean distance to
    the exact fp32 gradient of the rounded inputs <= 1e-2 of max|grad|;
  * the training step of the reduced UMI MAR (reference golden g2_mar_umi_*) under fp8_attn: loss
    within 5e-2 of the reference's fp32 loss (the bf16 path is held to 3e-2), finite gradients."""
import numpy as np
import pytest
import torch

import cases
import replay

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _qkv(B, N, H, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, N, 3, H, 64, generator=g) * 1.5
    x[:, :, 0] *= torch.linspace(0.2, 3.0, N)[None, :, None, None]  # tile-varying ranges (per-tile scales)
    return x.to(DEV, torch.bfloat16).contiguous()


def _torch_round(x):
    """reference rounding: per (b, t, h, 64-row tile) scale 2^e, e4m3 RNE cast."""
    B, N, _, H, D = x.shape
    xf = x.float().reshape(B, N // 64, 64, 3, H, D)
    amax = xf.abs().amax(dim=(2, 5), keepdim=True)
    e = torch.ceil(torch.log2(amax.clamp_min(1e-30) / 448.0))
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    e = torch.where(amax * torch.exp2(-e) > 448.0, e + 1, e)
    e = torch.where(amax * torch.exp2(-(e - 1)) <= 448.0, e - 1, e)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    e = e.clamp(-126, 126)  # csrc/fp8_scale.h: 2^e, 2^-e and the e8m0 code stay normal
    s = torch.exp2(e)
    r = (xf / s).to(torch.float8_e4m3fn).float() * s
    return r.reshape(B, N, 3, H, D).to(torch.bfloat16), s.reshape(B, N // 64, 3, H)


def _ref_attention(qkv, scale, mask_keep=None, p=0.0):
    q, k, v = (qkv[:, :, i].float().permute(0, 2, 1, 3) for i in range(3))  # [B,H,N,64]
    S = q @ k.transpose(-1, -2) * scale
    lse = torch.logsumexp(S, dim=-1)
    P = torch.softmax(S, dim=-1)
    if mask_keep is not None:
        P = P * mask_keep / (1 - p)
    return (P @ v).permute(0, 2, 1, 3), lse


@pytest.mark.parametrize("N,H", [(1088, 3), (1024, 3), (1088, 12), (1024, 12)])
def test_quant_matches_torch_e4m3_and_layouts(N, H):
    """H = 12 runs the row form of the pass (one workgroup per 64-row tile over all heads)"""
    from unified_video_action_amd.native import ops
    B = 2
    x = _qkv(B, N, H, 1)
    want, s = _torch_round(x)
    ws = ops.attn_fp8_workspace(B, N, H, DEV)
    y = x.clone()
    ops.attn_quant_fp8(y, ws, B, N, H)
    assert torch.equal(y, want), (y.float() - want.float()).abs().max()
    qk8 = ws[: 2 * B * N * H * 64].view(torch.float8_e4m3fn).float().reshape(B, N, 2, H, 64)
    sq = s[:, :, 0].repeat_interleave(64, dim=1)[:, :, None, :, None]  # [B,N,1,H,1]
    sk = s[:, :, 1].repeat_interleave(64, dim=1)[:, :, None, :, None]
    torch.testing.assert_close(qk8[:, :, 0:1] * sq, want[:, :, 0:1].float(), rtol=0, atol=0)
    torch.testing.assert_close(qk8[:, :, 1:2] * sk, want[:, :, 1:2].float(), rtol=0, atol=0)
    v8t = ws[2 * B * N * H * 64: 3 * B * N * H * 64].view(torch.float8_e4m3fn).float().reshape(B, H, 64, N)
    # key r of each 64-key tile sits at 32h + 16s + i, key = 32s + (i&3) + 8(i>>2) + 4h (the P.V operand order)
    pos = torch.tensor([(r & ~63) + 32 * ((r >> 2) & 1) + 16 * ((r & 63) >> 5) + (r & 3) + 4 * ((r & 31) >> 3)
                        for r in range(N)])
    sv = s[:, :, 2].repeat_interleave(64, dim=1)  # [B,N,H]
    vt = v8t[:, :, :, pos].permute(0, 3, 1, 2) * sv[..., None]  # [B,N,H,64]
    torch.testing.assert_close(vt, want[:, :, 2].float(), rtol=0, atol=0)
    off = (3 * B * N * H * 64 + 255) // 256 * 256
    sc = ws[off: off + 4 * B * 3 * H * (N // 64)].view(torch.float32).reshape(B, 3, H, N // 64)
    torch.testing.assert_close(sc, s.permute(0, 2, 3, 1), rtol=0, atol=0)


@pytest.mark.parametrize("N,drop", [(1088, 0.0), (1024, 0.0), (1088, 0.1), (1024, 0.1)])
def test_fp8_forward_and_backward_vs_fp32_reference(N, drop):
    from unified_video_action_amd.native import ops
    B, H = 2, 4
    scale = 64 ** -0.5
    x = _qkv(B, N, H, 2 + N)
    ws = ops.attn_fp8_workspace(B, N, H, DEV)
    ops.attn_quant_fp8(x, ws, B, N, H)  # x now holds the fp8-rounded values
    o = torch.empty(B, N, H, 64, dtype=torch.bfloat16, device=DEV)
    lse2 = torch.empty(B, H, N, device=DEV)
    mask = ops.attn_fwd_fp8(ws, o, lse2, B, N, H, scale, drop, seed=7)
    keep = None
    if drop > 0:  # the keep bits the kernels used, read back through the bf16 kernel (P = identity trick)
        ob = torch.empty_like(o)
        lb = torch.empty_like(lse2)
        ops.attn_fwd(x.view(B * N, 3 * H * 64), ob, lb, B, N, H, scale, drop, 7, mask=mask)
        torch.testing.assert_close(lb, lse2, rtol=1e-4, atol=2e-4)
        err = (o.float() - ob.float()).abs()
        print(f"\nN{N} drop: fp8 vs bf16 O max {err.max().item():.4f} mean {err.mean().item():.5f} "
              f"(max|O| {ob.float().abs().max().item():.3f})")
        assert err.max().item() <= 2 ** -4 * ob.float().abs().max().item()
        assert err.mean().item() <= 5e-3 * ob.float().abs().max().item()
        return
    ref_o, ref_lse = _ref_attention(x, scale)
    ln2 = float(np.log(2.0))
    # the codes' products are exact; the fp32 sums / exp2 / log2 of the kernel vs torch's fp32 path
    torch.testing.assert_close(lse2 * ln2, ref_lse, rtol=1e-4, atol=1e-4)
    err = (o.float() - ref_o).abs()
    print(f"\nN{N}: fp8 O vs fp32 reference max {err.max().item():.4f} mean {err.mean().item():.5f} "
          f"(max|O| {ref_o.abs().max().item():.3f})")
    assert err.max().item() <= 2 ** -4 * ref_o.abs().max().item(), err.max().item()
    assert err.mean().item() <= 5e-3 * ref_o.abs().max().item(), err.mean().item()
    # backward: the bf16 FA2 kernels on the rounded inputs with the fp8 forward's lse / O -- i.e. the
    # straight-through gradient: exact softmax P of x~, D = rowsum(dO * O_fp8).  Restated in fp32:
    dout = torch.randn(B, N, H, 64, device=DEV).to(torch.bfloat16)
    dqkv = torch.empty_like(x)
    dvec = torch.empty(B, H, N, device=DEV)
    ops.attn_bwd(x.view(B * N, 3 * H * 64), o, dout, lse2, dvec, dqkv, B, N, H, scale)
    q, k, v = (x[:, :, i].float().permute(0, 2, 1, 3) for i in range(3))
    do = dout.float().permute(0, 2, 1, 3)
    P = torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1)
    D = (do * o.float().permute(0, 2, 1, 3)).sum(-1, keepdim=True)
    dS = P * (do @ v.transpose(-1, -2) - D)
    want = torch.stack([(dS @ k) * scale, (dS.transpose(-1, -2) @ q) * scale, P.transpose(-1, -2) @ do],
                       dim=2).permute(0, 3, 2, 1, 4)  # [B,N,3,H,64]
    gerr = (dqkv.float() - want).abs()
    gmax = want.abs().max().item()
    assert gerr.max().item() <= 3e-2 * gmax, (gerr.max().item(), gmax)
    # and the distance to the exact fp32 gradient of the rounded inputs (fp8 O in D): bounded
    xr = x.float().requires_grad_(True)
    ro, _ = _ref_attention(xr, scale)
    ro.backward(dout.float())
    e = (dqkv.float() - xr.grad).abs()
    print(f"N{N}: dqkv vs STE restatement max {gerr.max().item() / gmax:.4f}, vs exact fp32 gradient "
          f"max {e.max().item() / gmax:.4f} mean {e.mean().item() / gmax:.5f} (of max|grad|)")
    assert e.mean().item() <= 1e-2 * gmax


def test_fp8_forward_timing_vs_bf16():
    """the bench shape of one layer (B=32, N=1024, H=12): fp8 forward (+ quantisation pass) next to
    the bf16 kernel -- recorded, not asserted beyond sanity."""
    from unified_video_action_amd.native import ops
    B, N, H = 32, 1024, 12
    x = _qkv(B, N, H, 3)
    ws = ops.attn_fp8_workspace(B, N, H, DEV)
    o = torch.empty(B, N, H, 64, dtype=torch.bfloat16, device=DEV)
    lse2 = torch.empty(B, H, N, device=DEV)

    def t(fn, it=20):
        fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(it):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / it
    tq = t(lambda: ops.attn_quant_fp8(x, ws, B, N, H))
    t8 = t(lambda: ops.attn_fwd_fp8(ws, o, lse2, B, N, H, 0.125))
    tb = t(lambda: ops.attn_fwd(x.view(B * N, 3 * H * 64), o, lse2, B, N, H, 0.125))
    print(f"\nattention fwd B{B} N{N} H{H}: quant {tq * 1e3:.1f} us, fp8 {t8 * 1e3:.1f} us, bf16 {tb * 1e3:.1f} us")
    assert t8 > 0 and tb > 0


def test_umi_mar_step_under_fp8_attention_tracks_reference():
    """loss-trend check on the reduced UMI MAR (N = 1088 with text tokens): reference fp32 loss vs
    this build's fp8_attn step (the bf16 path is held to 3e-2; fp8 attention to 5e-2)."""
    from functools import partial

    import torch.nn as nn
    from hashinit import hash_init_
    from unified_video_action_amd.model.autoregressive.mar_con_unified import MAR
    from unified_video_action_amd.runtime import RT
    try:
        for mode in cases.VARIANTS["umi"]["modes"]:
            g = replay.load(f"g2_mar_umi_{mode}.npz")
            losses = {}
            for prec in ("bf16", "fp8_attn"):
                RT.set_precision(prec)
                m = MAR(norm_layer=partial(nn.LayerNorm, eps=1e-6), **cases.MAR_GOLDEN, **cases.mar_kwargs("umi"))
                hash_init_(m, "mar.")
                m = m.to(DEV).train()
                inp, rng = replay.mar_case("umi", mode, device=DEV)
                prop = {k: v for k, v in inp.items() if k.startswith("robot0_")}
                loss, lv, la = m(inp["z"], inp["c"], None, inp["nactions"], inp.get("text_latents"), task_mode=mode,
                                 proprioception_input=prop, rng=rng)
                loss.backward()
                assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
                losses[prec] = loss.item()
            ref = g["loss"][0]
            assert abs(losses["bf16"] - ref) <= 3e-2 * abs(ref), (losses, ref)
            assert abs(losses["fp8_attn"] - ref) <= 5e-2 * abs(ref), (losses, ref)
            print(f"\numi {mode}: reference {ref:.5f} bf16 {losses['bf16']:.5f} fp8_attn {losses['fp8_attn']:.5f}")
    finally:
        RT.set_precision("bf16")
