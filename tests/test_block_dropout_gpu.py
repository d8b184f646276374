"""Two chained timm Blocks in train() mode (attn_drop = proj_drop = 0.1, the benchmarked configuration) through
functional.block_forward with the RT defaults (every fused route: the 8-wave GEMM's Mlp epilogues with the
counter-hash dropout, norm2's backward emitting the proj_drop backward, the second Block's norm1 backward emitting
the first Block's fc2 dropout backward) against a plain torch restatement of the Block in fp64 with autograd,
under dropout masks from oracle/dropmask.py -- no mask and no value of the reference comes from a kernel.

Measure: per-tensor relative RMS error |a - ref| / |ref| over y, dx and every parameter gradient of both Blocks
(not max over max, which a wrong mask on one site would slip under).
Bound: the project's rule (test_parity_gpu.py): max(BF16_VIDEO_FLOOR = 1.5e-2, 3 x the error of the SAME torch
Block run under bf16 autocast with the same masks), per tensor.
Control: for each of the four dropout sites, the fp64 reference with that site's mask (in both Blocks) drawn from
another seed must miss the bound in force by at least 3 x, or the test would be blind to that site.  For proj /
fc1 / fc2 the measure is y.  A wrong attention mask moves y by 0.018 only (192 keys average the mask out, and the
residual stream dilutes the branch; y - x: 0.055, too close to 3 x its bound of 0.017), so that site is held on a
tighter measure: the qkv weight gradient of each Block, which the attention branch alone feeds.

Measured on an MI355X (B 2, N 192, RT.seed(77)), relative RMS error against the fp64 Block, torch bf16 autocast /
this build: y 1.56e-3 / 1.34e-3; dx 1.58e-3 / 1.39e-3; weight gradients 4.6e-3 .. 5.4e-3 / 3.6e-3 .. 5.2e-3;
bias gradients 2.7e-3 .. 5.3e-3 / 1.6e-3 .. 4.8e-3 (this build is below the torch bf16 run on all 26 tensors).
3 x the torch bf16 error is 0.47e-2 .. 1.63e-2 (largest: 0.norm1.weight), so the bound in force lies between the
1.5e-2 floor and 1.63e-2 on every tensor.  Control, wrong-seed error / bound: attn 0.375 and 0.271 / 0.0155 and
0.0150 (qkv weight gradients); proj 0.0493, fc1 0.134, fc2 0.139 / 0.0150 (y).  proj clears 3 x 0.015 = 0.045 by a
tenth only; the figure is a mean over 295 k elements of fixed inputs (it was 0.0495 on other random inputs)."""
from functools import partial

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dropmask as DM

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1.5e-2  # test_parity_gpu.BF16_VIDEO_FLOOR (per-parameter floor of the video-class cases)
D, H, HID = 768, 12, 3072
P_DROP = 0.1
SITES = ("attn", "proj", "fc1", "fc2")
CONTROL = {"attn": ("0.attn.qkv.weight", "1.attn.qkv.weight"), "proj": ("y",), "fc1": ("y",), "fc2": ("y",)}


def _masks(seeds, B, N, dev, dtype):
    """keep * scale per site of one Block (seeds in the order attn, proj, fc1, fc2)"""
    th, scale = DM.drop_params(P_DROP)
    M = B * N
    t = lambda a: torch.from_numpy(a).to(dev).to(dtype) * scale  # noqa: E731
    return {"attn": t(DM.keep_attn(seeds[0], B, H, N, th)), "proj": t(DM.keep_flat(seeds[1], M, D, th)),
            "fc1": t(DM.keep_flat(seeds[2], M, HID, th)), "fc2": t(DM.keep_flat(seeds[3], M, D, th))}


def _drop(t, keep_scale):
    """t * keep / (1 - p), computed wide and rounded once to t's dtype (as torch's dropout does on bf16)"""
    return (t.to(keep_scale.dtype) * keep_scale).to(t.dtype)


def _ref_block(x, p, m, B, N):
    """timm Block (pre-LN, MHSA, GELU Mlp; dropout on the softmax probabilities, after proj, after GELU, after
    fc2), plain torch.  x [B*N, D]; p: parameter dict; m: keep * scale per site"""
    h = F.layer_norm(x, (D,), p["norm1.weight"], p["norm1.bias"], 1e-6)
    qkv = F.linear(h, p["attn.qkv.weight"], p["attn.qkv.bias"]).reshape(B, N, 3, H, D // H).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    a = torch.softmax((q * (D // H) ** -0.5) @ k.transpose(-2, -1), dim=-1)
    a = _drop(a, m["attn"])
    o = (a @ v).transpose(1, 2).reshape(B * N, D)
    o = F.linear(o, p["attn.proj.weight"], p["attn.proj.bias"])
    x = x + _drop(o, m["proj"])
    h = F.layer_norm(x, (D,), p["norm2.weight"], p["norm2.bias"], 1e-6)
    h = F.gelu(F.linear(h, p["mlp.fc1.weight"], p["mlp.fc1.bias"]))
    h = _drop(h, m["fc1"])
    h = F.linear(h, p["mlp.fc2.weight"], p["mlp.fc2.bias"])
    return x + _drop(h, m["fc2"])


def _ref_run(x0, gy, params, masks, B, N, dtype, backward=True):
    """both Blocks in `dtype` (fp64: as is; fp32 parameters under bf16 autocast: the torch Block in bf16)
    -> (y, dx, {name: grad})"""
    ps = [{n: t.detach().to(dtype).requires_grad_(backward) for n, t in p.items()} for p in params]
    x = x0.reshape(B * N, D).to(dtype).requires_grad_(backward)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.float32):
        y = _ref_block(_ref_block(x, ps[0], masks[0], B, N), ps[1], masks[1], B, N)
    if not backward:
        return y.detach().double(), None, None
    y.backward(gy.reshape(B * N, D).to(y.dtype))
    return (y.detach().double(), x.grad.double(),
            {f"{i}.{n}": t.grad.double() for i, p in enumerate(ps) for n, t in p.items()})


def _rel(a, ref):
    return ((a.double().reshape(ref.shape) - ref).norm() / ref.norm()).item()


def test_train_block_matches_fp64_block_under_restated_masks():
    from unified_video_action_amd.model.autoregressive import functional as Fn
    from unified_video_action_amd.model.autoregressive.mar_con_unified import Block
    from unified_video_action_amd.runtime import RT

    RT.set_precision("bf16")
    assert (RT.mlp_split_epilogue, RT.act_bwd_in_gemm, RT.ln_bwd_drop, RT.proj_8w) == (False, True, True, True)
    torch.manual_seed(0)
    blocks = []
    for _ in range(2):
        blk = Block(D, H, 4.0, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), proj_drop=P_DROP,
                    attn_drop=P_DROP).to(DEV).train()
        with torch.no_grad():
            for n, p in blk.named_parameters():
                if n.endswith("bias") or "norm" in n:
                    p.add_(torch.randn_like(p) * 0.05)  # non-trivial biases / LayerNorm affines
        blocks.append(blk)
    B, N = 2, 192  # M = 384: ragged against the 256-row tile; N % 64 == 0: flash attention
    x0 = torch.randn(B, N, D, device=DEV)
    gy = torch.randn(B, N, D, device=DEV)

    # ---- this build
    RT.begin_forward()
    RT.seed(77)
    seeds = [RT.next_seed() for _ in range(8)]  # four per Block: attn, proj, fc1, fc2
    RT.seed(77)
    for blk in blocks:  # the attention-mask prefetch would replace seeds[0] of a Block by one drawn earlier
        assert RT.take_attn_mask(id(blk), (B, N, H, float(P_DROP))) is None
    x = x0.clone().requires_grad_(True)
    y = Fn.block_forward(blocks[1], Fn.block_forward(blocks[0], x, B, N, P_DROP, P_DROP), B, N, P_DROP, P_DROP)
    ninth = RT.next_seed()
    RT.seed(77)
    assert [RT.next_seed() for _ in range(9)] == seeds + [ninth]  # the forward drew exactly these eight
    y.backward(gy)
    torch.cuda.synchronize()
    got = {"y": y.detach(), "dx": x.grad}
    got.update({f"{i}.{n}": p.grad for i, b in enumerate(blocks) for n, p in b.named_parameters()})

    # ---- the references: fp64, and the same torch Block under bf16 autocast, same masks
    params = [dict(b.named_parameters()) for b in blocks]
    masks = [_masks(seeds[4 * i:4 * i + 4], B, N, DEV, torch.float64) for i in range(2)]
    y64, dx64, g64 = _ref_run(x0, gy, params, masks, B, N, torch.float64)
    ref = {"y": y64, "dx": dx64, **g64}
    yb, dxb, gb = _ref_run(x0, gy, params, masks, B, N, torch.float32)
    refb = {"y": yb, "dx": dxb, **gb}
    assert set(ref) == set(got) and len(ref) == 2 + 2 * 12

    bound, rows, bad = {}, [], {}
    for n in ref:
        e_ref, e = _rel(refb[n], ref[n]), _rel(got[n], ref[n])
        bound[n] = max(FLOOR, 3.0 * e_ref)
        rows.append(f"{n:28s} {e_ref:.3e} {e:.3e}")
        if not e <= bound[n]:
            bad[n] = (e, e_ref)
    print("\n".join(["tensor  torch-bf16  this-build"] + rows))

    # ---- the control: a wrong mask on any one site must be far outside the bound in force
    other = [RT.next_seed() for _ in range(8)]
    wrong = [_masks(other[4 * i:4 * i + 4], B, N, DEV, torch.float64) for i in range(2)]
    for site in SITES:
        mm = [dict(masks[i], **{site: wrong[i][site]}) for i in range(2)]
        yw, dxw, gw = _ref_run(x0, gy, params, mm, B, N, torch.float64, backward=site == "attn")
        refw = {"y": yw, **(gw or {})}
        for n in CONTROL[site]:
            ew = _rel(refw[n], ref[n])
            print(f"control {site}: wrong-seed {n} error {ew:.3e} (bound {bound[n]:.3e})")
            assert ew >= 3.0 * bound[n], (site, n, ew, bound[n])
    assert not bad, bad
