"""The timm Block at the widths and head counts of the presets off the head_dim-64 route: (D 768, 6 heads:
mar_tiny / mar_small, head_dim 128) and (D 1280, 16 heads: mar_huge, head_dim 80).

1. The comparison of tests/test_block_dropout_gpu.py restated with parameters (D, H): two chained train() Blocks
   (attn_drop = proj_drop = 0.1) through functional.block_forward with the RT defaults against the plain torch
   Block in fp64 under dropout masks from oracle/dropmask.py; measure: relative RMS error per tensor over y, dx
   and every parameter gradient; bound: max(1.5e-2, 3 x the error of the same torch Block under bf16 autocast
   with the same masks).  B 1, N 128.  The fused attention route must have been taken: use_flash is true, the
   head_dim kernels were launched, and the autograd node saved no [B, H, N, N] tensor (the materialised route's
   P / Pd).  Control for the site this file is about: with the attention mask of the fp64 reference drawn from
   another seed, the qkv weight gradients (which the attention branch alone feeds) miss their bound by >= 3 x.
2. One training step of a depth-1 encoder / decoder MAR with mar_huge's width and heads, built through the
   policy's model_size lookup: forward, backward and an optimizer step in bf16 at B 2; finite loss, finite
   gradients on every parameter, parameters moved."""
from functools import partial

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import dropmask as DM

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1.5e-2  # test_parity_gpu.BF16_VIDEO_FLOOR, as tests/test_block_dropout_gpu.py
P_DROP = 0.1
PRESETS = [(768, 6), (1280, 16)]


def _masks(seeds, B, N, D, H, dev, dtype):
    """keep * scale per site of one Block (seeds in the order attn, proj, fc1, fc2)"""
    th, scale = DM.drop_params(P_DROP)
    M = B * N
    t = lambda a: torch.from_numpy(a).to(dev).to(dtype) * scale  # noqa: E731
    return {"attn": t(DM.keep_attn(seeds[0], B, H, N, th)), "proj": t(DM.keep_flat(seeds[1], M, D, th)),
            "fc1": t(DM.keep_flat(seeds[2], M, 4 * D, th)), "fc2": t(DM.keep_flat(seeds[3], M, D, th))}


def _drop(t, keep_scale):
    return (t.to(keep_scale.dtype) * keep_scale).to(t.dtype)


def _ref_block(x, p, m, B, N, D, H):
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


def _ref_run(x0, gy, params, masks, B, N, D, H, dtype):
    ps = [{n: t.detach().to(dtype).requires_grad_(True) for n, t in p.items()} for p in params]
    x = x0.reshape(B * N, D).to(dtype).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=dtype == torch.float32):
        y = _ref_block(_ref_block(x, ps[0], masks[0], B, N, D, H), ps[1], masks[1], B, N, D, H)
    y.backward(gy.reshape(B * N, D).to(y.dtype))
    out = {"y": y.detach().double(), "dx": x.grad.double()}
    out.update({f"{i}.{n}": t.grad.double() for i, p in enumerate(ps) for n, t in p.items()})
    return out


def _rel(a, ref):
    return ((a.double().reshape(ref.shape) - ref).norm() / ref.norm()).item()


def _block_node(y):
    """the BlockFn autograd node that produced y"""
    todo, seen = [y.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        if "BlockFn" in type(fn).__name__:
            return fn
        todo += [f for f, _ in fn.next_functions]
    raise AssertionError("no BlockFn node behind the Block's output")


@pytest.mark.parametrize("D,H", PRESETS, ids=[f"D{d}-H{h}" for d, h in PRESETS])
def test_train_blocks_on_the_fused_route_match_fp64(D, H, monkeypatch):
    from unified_video_action_amd.model.autoregressive import functional as Fn
    from unified_video_action_amd.model.autoregressive.mar_con_unified import Block
    from unified_video_action_amd.native import ops
    from unified_video_action_amd.runtime import RT

    RT.set_precision("bf16")
    B, N = 1, 128
    hd = D // H
    assert Fn.use_flash(N, hd)
    calls = {"fwd": 0, "bwd": 0}
    fwd, bwd = ops.attn_fwd_hd, ops.attn_bwd_hd

    def count(which, fn):
        def wrapped(*a, **kw):
            calls[which] += 1
            return fn(*a, **kw)
        return wrapped

    monkeypatch.setattr(ops, "attn_fwd_hd", count("fwd", fwd))
    monkeypatch.setattr(ops, "attn_bwd_hd", count("bwd", bwd))
    torch.manual_seed(0)
    blocks = []
    for _ in range(2):
        blk = Block(D, H, 4.0, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), proj_drop=P_DROP,
                    attn_drop=P_DROP).to(DEV).train()
        with torch.no_grad():
            for n, p in blk.named_parameters():
                if n.endswith("bias") or "norm" in n:
                    p.add_(torch.randn_like(p) * 0.05)
        blocks.append(blk)
    x0 = torch.randn(B, N, D, device=DEV)
    gy = torch.randn(B, N, D, device=DEV)

    RT.begin_forward()
    RT.seed(91)
    seeds = [RT.next_seed() for _ in range(8)]  # four per Block: attn, proj, fc1, fc2
    RT.seed(91)
    for blk in blocks:  # a prefetched mask would replace seeds[0] of a Block by one drawn earlier
        assert RT.take_attn_mask(id(blk), (B, N, H, float(P_DROP))) is None
    x = x0.clone().requires_grad_(True)
    y1 = Fn.block_forward(blocks[0], x, B, N, P_DROP, P_DROP)
    y = Fn.block_forward(blocks[1], y1, B, N, P_DROP, P_DROP)
    for out in (y1, y):
        saved = [tuple(t.shape) for t in _block_node(out).saved_tensors if t is not None]
        assert (B, H, N, N) not in saved, saved
    y.backward(gy)
    torch.cuda.synchronize()
    assert calls == {"fwd": 2, "bwd": 2}, calls
    got = {"y": y.detach(), "dx": x.grad}
    got.update({f"{i}.{n}": p.grad for i, b in enumerate(blocks) for n, p in b.named_parameters()})

    params = [dict(b.named_parameters()) for b in blocks]
    masks = [_masks(seeds[4 * i:4 * i + 4], B, N, D, H, DEV, torch.float64) for i in range(2)]
    ref = _ref_run(x0, gy, params, masks, B, N, D, H, torch.float64)
    refb = _ref_run(x0, gy, params, masks, B, N, D, H, torch.float32)
    assert set(ref) == set(got) and len(ref) == 2 + 2 * 12
    bound, rows, bad = {}, [], {}
    for n in ref:
        e_ref, e = _rel(refb[n], ref[n]), _rel(got[n], ref[n])
        bound[n] = max(FLOOR, 3.0 * e_ref)
        rows.append(f"{n:28s} {e_ref:.3e} {e:.3e}")
        if not e <= bound[n]:
            bad[n] = (e, e_ref)
    print("\n".join(["tensor  torch-bf16  this-build"] + rows))

    other = [RT.next_seed() for _ in range(8)]
    wrong = [_masks(other[4 * i:4 * i + 4], B, N, D, H, DEV, torch.float64) for i in range(2)]
    mm = [dict(masks[i], attn=wrong[i]["attn"]) for i in range(2)]
    refw = _ref_run(x0, gy, params, mm, B, N, D, H, torch.float64)
    for n in ("0.attn.qkv.weight", "1.attn.qkv.weight"):
        ew = _rel(refw[n], ref[n])
        print(f"control attn: wrong-seed {n} error {ew:.3e} (bound {bound[n]:.3e})")
        assert ew >= 3.0 * bound[n], (n, ew, bound[n])
    assert not bad, bad


def test_mar_huge_width_training_step(monkeypatch):
    """mar_huge's width (1280) and heads (16) at depth 1, registered as a model_size the way tests/golden/replay.py
    registers mar_golden and built by the policy's lookup; PushT joint inputs of the golden MAR case at B 2"""
    import cases
    import replay
    from unified_video_action_amd.model.autoregressive import mar_con_unified as pmar
    from unified_video_action_amd.native import ops
    from unified_video_action_amd.policy.unified_video_action_policy import UnifiedVideoActionPolicy
    from unified_video_action_amd.runtime import RT

    monkeypatch.setattr(pmar, "mar_huge_depth1", lambda **kw: pmar._mar(1280, 1, 16, **kw), raising=False)
    amp = dict(pretrained_model_path=None, model_size="mar_huge_depth1")
    for k in cases.POLICY_AMP_KEYS:
        amp[k] = cases.MAR_KW[k]
    amp.update(attn_dropout=P_DROP, proj_dropout=P_DROP)
    torch.manual_seed(0)
    pol = UnifiedVideoActionPolicy(
        vae_model_params=dict(autoencoder_path=None, ddconfig=dict(vae_embed_dim=16, ch_mult=[1, 1, 2, 2, 4])),
        autoregressive_model_params=amp, action_model_params=dict(predict_action=True, act_model_type="conv_fc"),
        shape_meta={"action": {"shape": [2]}}, n_action_steps=8, shift_action=True, language_emb_model=None,
        task_name="pusht", task_modes=[], normalizer_type="all", selected_training_mode=None,
        use_history_action=False, use_proprioception=False, action_mask_ratio=0.5, different_history_freq=False,
        predict_wrist_img=False, predict_proprioception=False)
    m = pol.model.to(DEV).train()
    with torch.no_grad():  # the zero-initialised output layers would leave every gradient behind them exactly zero
        for p in m.parameters():
            if p.abs().max().item() == 0:
                p.normal_(std=0.02)
    assert m.encoder_blocks[0].attn.num_heads == 16 and m.encoder_blocks[0].norm1.weight.numel() == 1280
    calls = []
    fwd = ops.attn_fwd_hd
    monkeypatch.setattr(ops, "attn_fwd_hd", lambda *a, **kw: (calls.append(a[6]), fwd(*a, **kw))[1])
    RT.set_precision("bf16")
    mode = "full_dynamic_model"
    inp, rng = replay.mar_case("pusht", mode, device=DEV)
    assert inp["z"].shape[0] == 2
    opt = torch.optim.AdamW(m.parameters(), lr=1e-4)
    for p in m.parameters():
        p.grad = torch.zeros_like(p)
    before = [p.detach().clone() for p in m.parameters()]
    RT.seed(5)
    loss, lv, la = m(inp["z"], inp["c"], None, inp["nactions"], None, task_mode=mode, rng=rng)
    loss.backward()
    torch.cuda.synchronize()
    assert calls and set(calls) == {80}, calls  # every Block took the head_dim-80 kernels
    assert torch.isfinite(loss).all(), loss
    for n, p in m.named_parameters():
        assert torch.isfinite(p.grad).all(), n
    blk = m.encoder_blocks[0]
    for p in (blk.attn.qkv.weight, blk.attn.qkv.bias, blk.norm1.weight, m.decoder_blocks[0].attn.qkv.weight):
        assert p.grad.abs().max().item() > 0
    opt.step()
    RT.bump_params()
    torch.cuda.synchronize()
    moved = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, m.parameters()))
    assert moved > 0 and all(torch.isfinite(p).all() for p in m.parameters())
