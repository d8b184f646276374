"""CPU side of the CLIP text tower's reference chain (no GPU, no network):

  transformers CLIPModel (fp32)  <-1e-4->  tests/clip_ref.py float64 restatement  <-1e-4->  committed golden
  (tests/golden/g7_clip_text.npz, written by tests/golden/make_clip_golden.py)

and controls in the style of test_attention_exact_cpu.py: each defect the GPU tower could have, planted in
the restatement, must miss the bound the GPU test applies (relative L2 <= 1e-4 against the golden's fp32
features -- tests/test_clip_text_gpu.py's fp32 tower case; the bf16 case's bound, 3 x the reference's own
bf16-autocast error, is looser and is reported beside it: the erf-GELU defect passes under it and is caught
per element by the quick_gelu kernel case instead).  Plus the module's interface: parameter names equal
to CLIPModel's text side, fake kernels of the two custom ops, and a policy with a tower whose optimizer groups
and flat ParamStore hold exactly what they hold without one.
"""
import json
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
import clip_ref  # noqa: E402

FP32_BOUND = 1e-4  # the project's fp32 pin (README: relative L2)


@pytest.fixture(scope="module")
def golden():
    g = np.load(clip_ref.GOLDEN)
    return {k: torch.from_numpy(np.asarray(g[k])) for k in g.files}


@pytest.fixture(scope="module")
def state():
    return clip_ref.hash_state(clip_ref.text_shapes())


@pytest.fixture(scope="module")
def restated(golden, state):
    return clip_ref.tower(state, golden["ids"], golden["mask"])


def test_golden_prompts_are_the_generated_ones(golden):
    ids, mask = clip_ref.prompts(30)
    assert torch.equal(ids, golden["ids"]) and torch.equal(mask, golden["mask"])
    assert (mask[:, 0] == 1).all() and int(ids.max()) == clip_ref.EOT
    assert ids[2, 1] == clip_ref.EOT and mask[1, 5] == 0 and mask[1, 6] == 1  # EOT at 1; the hole
    assert ids.argmax(1).tolist() == [8, 16, 1, 29]


def test_restatement_matches_golden(golden, restated):
    err = clip_ref.rel_l2(restated, golden["features_f32"])
    print(f"restatement vs golden fp32 features: rel L2 {err:.3e}")
    assert err <= FP32_BOUND
    # the bf16 yardstick is a real bf16 error, not noise
    assert 1e-3 < float(golden["bf16_rel_l2"]) < 5e-2


def test_restatement_matches_transformers(golden, restated):
    pytest.importorskip("transformers")
    import make_clip_golden
    model, names = make_clip_golden.hf_model()
    assert set(names) == set(clip_ref.text_shapes())
    with torch.no_grad():
        hf = make_clip_golden.features(model, golden["ids"], golden["mask"])
    err = clip_ref.rel_l2(restated, hf)
    print(f"restatement vs transformers fp32: rel L2 {err:.3e}")
    assert err <= FP32_BOUND
    assert clip_ref.rel_l2(hf, golden["features_f32"]) <= 1e-5  # the golden is this model's output


DEFECTS = {"no_causal_mask": dict(causal=False), "key_mask_ignored": dict(use_mask=False),
           "erf_gelu": dict(act="gelu"), "pool_last": dict(pool_at="last"), "position_shifted": dict(pos_shift=1),
           "qkv_order": dict(qkv_order=(1, 0, 2))}


@pytest.mark.parametrize("name", sorted(DEFECTS))
def test_control_defect_misses_the_gpu_bound(golden, state, name):
    bad = clip_ref.tower(state, golden["ids"], golden["mask"], **DEFECTS[name])
    ref = golden["features_f32"]
    err = clip_ref.rel_l2(bad, ref)
    rows = [clip_ref.rel_l2(bad[i], ref[i]) for i in range(4)]
    bf16_bound = 3 * float(golden["bf16_rel_l2"])
    print(f"{name}: rel L2 {err:.3e} rows {['%.2e' % r for r in rows]}  fp32 bound {FP32_BOUND:g}  "
          f"bf16 bound {bf16_bound:.3e} ({'missed' if err > bf16_bound else 'met'})")
    assert err > 10 * FP32_BOUND
    if name == "key_mask_ignored":  # only the row with a hole in its mask can tell
        assert rows[1] > 10 * FP32_BOUND and max(rows[0], rows[2], rows[3]) <= FP32_BOUND
    if name == "pool_last":  # row 3's EOT is at L - 1
        assert rows[3] <= FP32_BOUND and min(rows[:3]) > 10 * FP32_BOUND
    if name != "erf_gelu":
        assert err > bf16_bound


def test_kernel_restatements():
    """the per-kernel float64 references against plain torch on a small case"""
    g = torch.Generator().manual_seed(5)
    B, L, H = 2, 7, 2
    qkv = torch.randn(B * L, 3 * H * 64, generator=g)
    mask = torch.ones(B, L, dtype=torch.int64)
    mask[1, 3] = 0
    out, mag = clip_ref.attention(qkv, B, L, H, mask)
    t = qkv.double().view(B, L, 3, H, 64).permute(2, 0, 3, 1, 4)
    bias = torch.zeros(B, 1, L, L, dtype=torch.float64).masked_fill(~clip_ref.allowed(L, mask)[:, None], float("-inf"))
    want = torch.nn.functional.scaled_dot_product_attention(t[0], t[1], t[2], attn_mask=bias)
    assert torch.allclose(out, want.permute(0, 2, 1, 3).reshape(B * L, H * 64), atol=1e-12)
    assert (mag >= out.abs() - 1e-12).all()
    assert torch.equal(out.view(B, L, H, 64)[:, 0], t[2][:, :, 0])  # a single key: out = V_0
    ids = torch.tensor([[3, 9, 9, 1], [7, 2, 7, 7]])
    at, rows = clip_ref.pool(ids, torch.arange(8.0).view(8, 1))
    assert at.tolist() == [1, 0] and rows.view(-1).tolist() == [1.0, 4.0]
    x = torch.linspace(-12, 12, 49)
    assert torch.allclose(clip_ref.quick_gelu(x), x.double() / (1 + torch.exp(-1.702 * x.double())), atol=1e-15)


def test_tower_state_dict_names_are_the_text_side_of_clipmodel():
    transformers = pytest.importorskip("transformers")
    from unified_video_action_amd.utils.language_model import ClipTextTower
    hf = transformers.CLIPModel(transformers.CLIPConfig())
    hf_params = {k: tuple(v.shape) for k, v in hf.named_parameters()
                 if k.startswith("text_model.") or k.startswith("text_projection.")}
    tower = ClipTextTower()
    own = {k: tuple(v.shape) for k, v in tower.state_dict().items()}
    assert own == hf_params
    assert own == {k: tuple(s) for k, s in clip_ref.text_shapes().items()}
    assert not any(p.requires_grad for p in tower.parameters())
    assert not tower.train().training  # eval only


def test_tower_needs_the_gpu_library_no_torch_fallback():
    from unified_video_action_amd.utils.language_model import ClipTextTower
    tower = ClipTextTower(vocab_size=32, num_hidden_layers=1, max_position_embeddings=8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tower(torch.zeros(1, 4, dtype=torch.int64), torch.ones(1, 4, dtype=torch.int64))


def test_host_mask_must_keep_position_zero():
    from unified_video_action_amd.native import ops
    ops.clip_check_mask(torch.tensor([[1, 0, 1], [1, 1, 0]]))
    ops.clip_check_mask(None)
    with pytest.raises(ValueError, match="position 0"):
        ops.clip_check_mask(torch.tensor([[1, 1, 1], [0, 1, 1]]))


def test_fake_kernels_propagate_shapes():
    from unified_video_action_amd.native import torch_ops  # noqa: F401  (registers the ops)
    for dtype in (torch.bfloat16, torch.float32):
        qkv = torch.empty(3, 30, 3 * 8 * 64, dtype=dtype, device="meta")
        mask = torch.empty(3, 30, dtype=torch.int64, device="meta")
        out = torch.ops.uva.clip_attention(qkv, mask, 8)
        assert out.shape == (3, 30, 512) and out.dtype == dtype and out.device.type == "meta"
        assert torch.ops.uva.clip_attention(qkv, None, 8).shape == (3, 30, 512)
        x = torch.empty(90, 2048, dtype=dtype, device="meta")
        y = torch.ops.uva.quick_gelu(x)
        assert y.shape == x.shape and y.dtype == dtype
    with pytest.raises(ValueError, match="outside 1..77"):
        torch.ops.uva.clip_attention(torch.empty(1, 78, 3 * 8 * 64, device="meta"), None, 8)
    with pytest.raises(ValueError, match="3\\*heads\\*64"):
        torch.ops.uva.clip_attention(torch.empty(1, 30, 3 * 8 * 32, device="meta"), None, 8)


# ---- the policy with a tower ------------------------------------------------------------------------
SMALL = dict(vocab_size=512, hidden_size=512, intermediate_size=2048, num_hidden_layers=2, num_attention_heads=8,
             max_position_embeddings=77)


def write_clip_dir(path, dims=SMALL, projection_dim=512):
    """a local HF-layout CLIP directory: config.json (settings) + pytorch_model.bin (hash-init text side plus
    entries of the vision side that the loader must ignore)"""
    os.makedirs(path, exist_ok=True)
    with open(os.path.join(path, "config.json"), "w") as f:
        json.dump({"text_config": dict(dims, hidden_act="quick_gelu"), "projection_dim": projection_dim}, f)
    shapes = clip_ref.text_shapes(layers=dims["num_hidden_layers"], width=dims["hidden_size"],
                                  mlp=dims["intermediate_size"], vocab=dims["vocab_size"],
                                  ctx=dims["max_position_embeddings"], proj=projection_dim)
    sd = clip_ref.hash_state(shapes)
    sd["logit_scale"] = torch.tensor(2.6592)
    sd["visual_projection.weight"] = torch.zeros(4, 4)
    torch.save(sd, os.path.join(path, "pytorch_model.bin"))
    return {k: v for k, v in sd.items() if k in shapes}


def libero_policy(language_model_path=None):
    import cases
    import replay
    from unified_video_action_amd.policy.unified_video_action_policy import UnifiedVideoActionPolicy
    replay.golden_policy(normalizer=False)  # registers model_size "mar_golden"
    amp = dict(pretrained_model_path=None, model_size="mar_golden")
    for k in cases.POLICY_AMP_KEYS:
        amp[k] = cases.MAR_KW[k]
    kw = dict(cases.policy_variant_kwargs("libero"))
    if language_model_path is not None:
        kw["language_model_path"] = language_model_path
    return UnifiedVideoActionPolicy(
        vae_model_params=dict(autoencoder_path=None, ddconfig=dict(vae_embed_dim=16, ch_mult=[1, 1, 2, 2, 4])),
        autoregressive_model_params=amp, **kw)


def test_policy_tower_stays_out_of_optimizer_and_param_store(tmp_path):
    sd = write_clip_dir(str(tmp_path / "clip"))
    plain = libero_policy()
    with_tower = libero_policy(str(tmp_path / "clip"))
    assert plain.text_model is None and with_tower.text_model is not None
    tower = with_tower.text_model
    assert len(tower.text_model.encoder.layers) == 2
    for k, v in tower.state_dict().items():  # loaded by name, vision-side entries ignored
        assert torch.equal(v, sd[k]), k
    tower_ids = {id(p) for p in tower.parameters()}
    assert tower_ids and not any(p.requires_grad for p in tower.parameters())
    assert not tower_ids & {id(p) for p in with_tower.model.parameters()}
    # get_optimizer's groups (add_weight_decay over self.model) hold what they hold without a tower
    ga, gb = plain.add_weight_decay(plain.model, 0.02), with_tower.add_weight_decay(with_tower.model, 0.02)
    assert [sum(p.numel() for p in g["params"]) for g in ga] == [sum(p.numel() for p in g["params"]) for g in gb]
    assert not tower_ids & {id(p) for g in gb for p in g["params"]}
    # ... and so does the flat ParamStore behind the optimizer (built from self.model's named parameters)
    oa = plain.get_optimizer(weight_decay=0.02, learning_rate=1e-4, betas=(0.9, 0.95))
    ob = with_tower.get_optimizer(weight_decay=0.02, learning_rate=1e-4, betas=(0.9, 0.95))
    assert (ob.store.total, ob.store.n_params) == (oa.store.total, oa.store.n_params) and ob.store.n_params > 0
    assert not tower_ids & {id(p) for _, p in ob.store.order}
    assert [len(g["params"]) for g in ob.param_groups] == [len(g["params"]) for g in oa.param_groups]
    # DP: everything but the anchor is on DDP's ignore list, the tower included
    ignored = set(with_tower._ddp_params_and_buffers_to_ignore)
    assert {"text_model." + k for k in tower.state_dict()} <= ignored
    # a checkpoint written without the tower loads into the policy that has one
    with_tower.load_state_dict(plain.state_dict())
    assert with_tower.train().text_model.training is False
    # tokens are refused without a tower, exactly as before
    with pytest.raises(NotImplementedError, match="pass language_latents"):
        plain.compute_loss({"obs": {"agentview_rgb": torch.zeros(1, 32, 3, 8, 8),
                                    "language": torch.zeros(1, 32, 2, 30, dtype=torch.int64)},
                            "action": torch.zeros(1, 32, 10)})


def test_get_text_model_without_path_builds_nothing(tmp_path):
    from unified_video_action_amd.utils.language_model import get_text_model
    assert get_text_model("libero_10", "clip", None) == (None, None, 30)
    assert get_text_model("pusht", None, str(tmp_path)) == (None, None, 30)
    with pytest.raises(FileNotFoundError):
        get_text_model("libero_10", "clip", "openai/clip-vit-base-patch32")  # a hub name is never resolved
