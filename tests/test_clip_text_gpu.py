"""CLIP text tower on the GPU (csrc/text_tower.hip, utils/language_model.py): every kernel per element against
the float64 restatements of tests/clip_ref.py at edge shapes, into NaN-filled guarded outputs; the whole
tower against transformers' own features recorded in tests/golden/g7_clip_text.npz (weights regenerated
by name: none are committed; transformers is not imported here); the policy taking tokens where it took
latents.  Bounds: clip_ref's docstring.  Each case prints its worst error / bound."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import clip_ref  # noqa: E402
from edge_helpers import BF16, DEV, F32, Guarded, assert_within, gen  # noqa: E402

pytestmark = pytest.mark.gpu


def _ops():
    from unified_video_action_amd.native import ops
    return ops


def _precision(name):
    from unified_video_action_amd.runtime import RT
    RT.set_precision(name)


def _worst(got, ref, bound):
    r = ((got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)).max()
    return float(r)


# ---- uva_clip_attn ------------------------------------------------------------------------------------
def _mask(kind, B, L):
    m = torch.ones(B, L, dtype=torch.int64)
    if kind == "prefix":  # per-row prefixes of different lengths (at least the BOS)
        for b in range(B):
            m[b, max(1, (L * (b + 1)) // (B + 1)):] = 0
    elif kind == "hole" and L > 2:
        m[0, L // 2] = 0
        m[B - 1, 1] = 0
    return m


@pytest.fixture(scope="module")
def attn_inputs():
    """randn Q / K / V rounded to bf16, Q and K x 2.5 (peaked rows), one draw per shape, shared by the dtypes"""
    out = {}
    for i, (B, H, L) in enumerate(ATTN_SHAPES):
        t = torch.randn(B * L, 3, H, 64, generator=gen(100 + i))
        t[:, :2] *= 2.5
        out[(B, H, L)] = t.to(BF16).float().reshape(B * L, 3 * H * 64)
    return out


ATTN_SHAPES = [(2, 8, 30), (1, 8, 77), (2, 8, 33), (2, 8, 64), (3, 2, 1), (2, 8, 16)]


@pytest.mark.parametrize("kind", ["ones", "prefix", "hole"])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("B,H,L", ATTN_SHAPES)
def test_clip_attn_per_element(attn_inputs, B, H, L, dtype, kind):
    ops = _ops()
    qkv = attn_inputs[(B, H, L)]
    mask = _mask(kind, B, L)
    ref, mag = clip_ref.attention(qkv, B, L, H, mask)
    bound = clip_ref.attn_bound(ref, mag, L, dtype == BF16)
    q = qkv.to(DEV).to(dtype).contiguous()
    md = None if kind == "ones" and L % 2 else mask.to(DEV)  # all ones: also the NULL-mask form
    g = Guarded(B * L, H * 64, dtype)
    ops.clip_attn(q, md, g.view, B, L, H)
    g.check()
    first = g.view.clone()
    print(f"clip_attn {dtype} B{B} H{H} L{L} {kind}: worst err/bound {_worst(first, ref, bound):.3f}")
    assert_within(first, ref, bound, f"clip_attn B{B} H{H} L{L} {kind}")
    if L == 1:  # a single row: out = V_0 exactly
        assert torch.equal(first.cpu().float(), qkv[:, 2 * H * 64:])
    g.view.fill_(float("nan"))
    ops.clip_attn(q, md if md is None else md.int(), g.view, B, L, H)  # second launch (int32 mask): bit-equal
    g.check()
    assert torch.equal(first.view(torch.int16 if dtype == BF16 else torch.int32),
                       g.view.view(torch.int16 if dtype == BF16 else torch.int32))


def test_clip_attn_rejects_bad_shapes():
    ops = _ops()
    q = torch.zeros(78, 3 * 64, dtype=BF16, device=DEV)
    with pytest.raises(ValueError, match="outside 1..77"):
        ops.clip_attn(q, None, torch.zeros(78, 64, dtype=BF16, device=DEV), 1, 78, 1)
    with pytest.raises(ValueError):
        ops.clip_attn(q[:30], None, torch.zeros(30, 64, dtype=F32, device=DEV), 1, 30, 1)  # mixed dtypes


# ---- uva_clip_embed / uva_clip_pool -------------------------------------------------------------------
@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
def test_clip_embed_equals_torch(idt):
    ops = _ops()
    vocab, D, B, L = 301, 512, 3, 30
    tok = torch.randn(vocab, D, generator=gen(1)).to(DEV)
    pos = torch.randn(77, D, generator=gen(2)).to(DEV)  # a position table longer than L
    ids = torch.randint(0, vocab, (B, L), generator=gen(3))
    ids[0, 0], ids[0, 1], ids[B - 1, L - 1] = 0, vocab - 1, vocab - 1
    ids = ids.to(DEV).to(idt)
    g = Guarded(B * L, D, F32)
    ops.clip_embed(ids, tok, pos, g.view)
    g.check()
    want = (tok[ids.long()] + pos[:L][None]).reshape(B * L, D)
    assert torch.equal(g.view, want)


@pytest.mark.parametrize("idt", [torch.int64, torch.int32])
@pytest.mark.parametrize("L", [30, 77, 1])
def test_clip_pool_equals_torch(idt, L):
    ops = _ops()
    B, D, EOT = 5, 512, 49407
    ids = torch.randint(1, 49000, (B, L), generator=gen(4))
    if L > 2:
        ids[0, 1:] = EOT          # EOT at 1, repeated as padding up to L - 1
        ids[1, L - 1] = EOT       # EOT at L - 1
        ids[2, 7 % L:] = EOT      # repeated maxima
        ids[3, L // 2] = ids[3, L // 2 + 1] = 48999  # a repeated maximum that is not the EOT
    ids = ids.to(DEV).to(idt)
    x = torch.randn(B * L, D, generator=gen(5)).to(DEV)
    g = Guarded(B, D, F32)
    index = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    ops.clip_pool(ids, x, g.view, index)
    g.check()
    at = ids.long().argmax(dim=1)
    if L > 2:
        assert at[:2].tolist() == [1, L - 1]
    assert torch.equal(index.long(), at)
    assert torch.equal(g.view, x.view(B, L, D)[torch.arange(B, device=DEV), at])


# ---- uva_quick_gelu -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", [8 * 40, 8 * 40 + 3, 3, 8 * 70000 + 5])
def test_quick_gelu_per_element(n, dtype):
    ops = _ops()
    x = (torch.rand(n, generator=gen(6)) * 24 - 12)
    x[0], x[n - 1], x[n // 2] = 0.0, 12.0, -12.0
    x = x.to(dtype)
    ref = clip_ref.quick_gelu(x.float())
    bound = clip_ref.quick_gelu_bound(x.float(), dtype == BF16)
    g = Guarded(1, n, dtype)
    y = g.view.view(-1)
    ops.quick_gelu(x.to(DEV), y)
    g.check()
    print(f"quick_gelu {dtype} n{n}: worst err/bound {_worst(y, ref, bound):.3f}")
    assert float(y[0]) == 0.0
    assert_within(y, ref, bound, f"quick_gelu n{n}")


# ---- the whole tower ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    g = np.load(clip_ref.GOLDEN)
    return {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}


@pytest.fixture(scope="module")
def tower():
    from unified_video_action_amd.utils.language_model import ClipTextTower
    t = ClipTextTower()
    t.load_state_dict(clip_ref.hash_state({k: tuple(v.shape) for k, v in t.state_dict().items()}))
    return t.to(DEV)


@pytest.mark.parametrize("prec", ["fp32", "bf16"])
def test_tower_vs_transformers_features(tower, golden, prec):
    """fp32: relative L2 <= 1e-4 of transformers' fp32 get_text_features; bf16: <= 3 x transformers' own
    bf16-autocast error on the same prompts (README's bf16 rule), both recorded in the golden."""
    _precision(prec)
    try:
        ids, mask = golden["ids"].to(DEV), golden["mask"].to(DEV)
        got = tower(ids, mask)
        again = tower(ids.int(), mask.int())
        assert got.shape == (4, 512) and got.dtype == F32
        assert torch.equal(got, again)
        err = clip_ref.rel_l2(got, golden["features_f32"])
        bound = 1e-4 if prec == "fp32" else 3 * float(golden["bf16_rel_l2"])
        print(f"tower {prec}: rel L2 {err:.3e}  bound {bound:.3e}")
        assert err <= bound
    finally:
        _precision("bf16")


# ---- the policy ---------------------------------------------------------------------------------------
def _tokens(B, T=32, L=30, vocab=512):
    ids = torch.randint(1, vocab - 2, (B, L), generator=gen(7))
    mask = torch.zeros(B, L, dtype=torch.int64)
    for b in range(B):
        n = 6 + 5 * b
        ids[b, 0], ids[b, n - 1:] = vocab - 2, vocab - 1
        mask[b, :n] = 1
    lang = torch.stack([ids, mask], dim=1)  # [B, 2, L]
    return lang, lang[:, None].expand(B, T, 2, L).contiguous()


def _libero_policy(path):
    import test_clip_text_cpu as cpu
    from hashinit import hash_init_
    from unified_video_action_amd.model.common.normalizer import LinearNormalizer
    cpu.write_clip_dir(path)
    pol = cpu.libero_policy(path)
    hash_init_(pol.vae_model, "vae.")
    hash_init_(pol.model, "mar.")
    pol = pol.to(DEV)
    norm = LinearNormalizer()
    norm.fit({"action": torch.tensor([[-1.0] * 10, [1.0] * 10])})
    pol.set_normalizer(norm)
    return pol


def test_policy_takes_tokens_where_it_took_latents(tmp_path):
    import cases
    _precision("bf16")
    pol = _libero_policy(str(tmp_path / "clip")).train()
    b = cases.policy_variant_batch("libero")
    B = b["action"].shape[0]
    lang, lang_bt = _tokens(B)
    lang, lang_bt = lang.to(DEV), lang_bt.to(DEV)
    latents = pol.text_model(lang[:, 0], lang[:, 1])
    assert latents.shape == (B, 512) and torch.isfinite(latents).all()
    img = torch.from_numpy(b["obs"]["agentview_rgb"]).to(DEV)
    action = torch.from_numpy(b["action"]).to(DEV)
    from unified_video_action_amd.runtime import RT
    losses = []
    for batch in ({"obs": {"agentview_rgb": img, "language": lang_bt}, "action": action},
                  {"obs": {"agentview_rgb": img}, "action": action, "language_latents": latents}):
        RT.seed(11)
        torch.manual_seed(11)
        with torch.no_grad():
            loss, _ = pol.compute_loss(batch, rng=cases.policy_variant_rng("libero", "policy_model"))
        losses.append(loss)
    assert torch.isfinite(losses[0]) and torch.equal(losses[0], losses[1])
    pol.eval()
    g = gen(8)
    obs = {"agentview_image": img[:, :16].contiguous()}
    rng = {"vae_eps": torch.randn(B * 4, 16, 16, 16, generator=g), "noise": torch.randn(B * 16, 10, generator=g).to(DEV),
           "step_noise": torch.randn(100, B * 16, 10, generator=g).to(DEV)}
    a_tok = pol.predict_action(dict(obs), language_goal=lang, rng=rng)
    a_dict = pol.predict_action(dict(obs), language_goal={"input_ids": lang[:, 0], "attention_mask": lang[:, 1]},
                                rng=rng)
    a_lat = pol.predict_action(dict(obs), language_goal=latents, rng=rng)
    assert torch.isfinite(a_tok["action_pred"]).all()
    assert torch.equal(a_tok["action_pred"], a_lat["action_pred"]) and torch.equal(a_tok["action"], a_lat["action"])
    assert torch.equal(a_dict["action_pred"], a_lat["action_pred"])
    with pytest.raises(NotImplementedError, match="tokenizer"):
        pol.predict_action(dict(obs), language_goal="put the cup on the plate", rng=rng)


def test_opcheck_clip_ops():
    from unified_video_action_amd.native import torch_ops  # noqa: F401
    utils = ("test_schema", "test_faketensor", "test_autograd_registration")
    qkv = torch.randn(2, 30, 3 * 8 * 64, device=DEV).to(BF16)
    mask = torch.ones(2, 30, dtype=torch.int64, device=DEV)
    torch.library.opcheck(torch.ops.uva.clip_attention.default, (qkv, mask, 8), test_utils=utils)
    torch.library.opcheck(torch.ops.uva.clip_attention.default, (qkv.float(), None, 8), test_utils=utils)
    torch.library.opcheck(torch.ops.uva.quick_gelu.default, (torch.randn(33, 7, device=DEV),), test_utils=utils)
    torch.library.opcheck(torch.ops.uva.quick_gelu.default, (torch.randn(16, 64, device=DEV).to(BF16),),
                          test_utils=utils)
