"""CPU side of the FVD evaluation: the Fréchet distance against the reference's float64 value, the I3D tower's
state-dict layout and BatchNorm folding, the fixture's conditions, the restatements of tests/i3d_ref.py against
torch's own ops, planted defects against the comparisons the GPU tests use, and the workspace's opt-in keys."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import i3d_ref as R
from conv_ref import assert_bit_equal
from edge_helpers import assert_within
from unified_video_action_amd.fvd import fvd as FVD
from unified_video_action_amd.fvd import i3d as I3D
from unified_video_action_amd.native import ops


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.mark.parametrize("n,i", [(16, 0), (64, 1)])
def test_frechet_distance_matches_reference_float64(golden, n, i):
    a, b = R.embedding_sets()[i]
    a0, b0 = a.clone(), b.clone()
    got = float(FVD.frechet_distance(a, b))
    want = float(golden[f"fd{n}_f64"])
    assert abs(got - want) <= 1e-4 * abs(want), (got, want)
    assert torch.equal(a, a0) and torch.equal(b, b0), "frechet_distance modified its input"
    # float64 inputs are not copied by the conversion: they must survive too
    a64 = a.double()
    a64_0 = a64.clone()
    FVD.frechet_distance(a64, b)
    assert torch.equal(a64, a64_0)
    # another route to the same number (eigendecomposition instead of SVD)
    assert abs(R.frechet(a, b) - want) <= 1e-6 * abs(want)


def test_frechet_distance_of_identical_sets_is_zero():
    a, _ = R.embedding_sets()[1]
    scale = float(torch.trace(FVD.cov(a.double())))
    assert abs(float(FVD.frechet_distance(a, a.clone()))) <= 1e-6 * scale


def test_frechet_distance_needs_two_samples():
    with pytest.raises(ValueError):
        FVD.frechet_distance(torch.zeros(1, 400), torch.zeros(4, 400))


def test_fixture_conditions(golden):
    rms = {k: float(golden["ep_rms_" + k]) for k in R.RECORDED}
    spread = R.fixture_conditions(rms, golden["logits_f32"])
    assert spread >= 0.1
    assert tuple(R.clips().shape) == (2, 16, 96, 128, 3) and R.clips().dtype == torch.uint8
    assert R.resized_size(96, 128) == (224, 299)       # ceil(128 * 224 / 96 = 298.67), then a centre crop of 37
    assert 0 < float(golden["bf16_rel_l2"]) < 3e-2


def test_state_dict_names_and_shapes_equal_the_reference(golden):
    tower = I3D.InceptionI3dTower(400)
    sd = tower.state_dict()
    names = [str(n) for n in golden["names"]]
    shapes = [tuple(int(v) for v in str(s).split(",") if v) for s in golden["shapes"]]
    assert list(sd) == names
    assert [tuple(v.shape) for v in sd.values()] == shapes
    assert "Conv3d_1a_7x7.conv3d.weight" in sd and "Mixed_3b.b1b.bn.running_var" in sd and "logits.conv3d.bias" in sd
    # the hash weights load by name
    tower.load_state_dict(R.hash_state(dict(zip(names, shapes))))


def test_batchnorm_folding_against_float64():
    tower = I3D.InceptionI3dTower(400)
    names = {k: tuple(v.shape) for k, v in tower.state_dict().items() if k.startswith("Mixed_4b.b2b.")}
    sd = R.hash_state(names)
    p = "Mixed_4b.b2b."
    w, b = I3D.fold_unit(sd[p + "conv3d.weight"], None, sd[p + "bn.weight"], sd[p + "bn.bias"],
                         sd[p + "bn.running_mean"], sd[p + "bn.running_var"])
    w64, b64 = R.fold_bn(sd[p + "conv3d.weight"], None, sd[p + "bn.weight"], sd[p + "bn.bias"],
                         sd[p + "bn.running_mean"], sd[p + "bn.running_var"])
    assert tuple(w.shape) == (48, 3, 3, 3, 16) and w.is_contiguous() and w.dtype == torch.float32
    assert_within(w, w64, 4 * R.U * w64.abs() + 1e-30, "folded weight")   # sqrt, division, product: 3 roundings
    assert_within(b, b64, 6 * R.U * (b64.abs() + (sd[p + "bn.running_mean"].double() * 2).abs() + 0.1), "folded bias")
    # and against torch: conv3d -> BatchNorm3d(eval) on one input
    x = torch.randn(1, 16, 2, 5, 5, dtype=torch.float64)
    bn = torch.nn.BatchNorm3d(48, eps=1e-5).double().eval()
    bn.load_state_dict({k[len(p) + 3:]: v.double() if v.is_floating_point() else v for k, v in sd.items()
                        if k.startswith(p + "bn.")})
    with torch.no_grad():
        want = bn(F.conv3d(x, sd[p + "conv3d.weight"].double(), padding=1)).permute(0, 2, 3, 4, 1)
    got, _ = R.conv3d(x.permute(0, 2, 3, 4, 1), w64, (1, 1, 1), (1, 1, 1), (2, 5, 5), bias=b64)
    assert float((got - want).abs().max()) < 1e-12


def test_tower_operands_layout():
    tower = I3D.InceptionI3dTower(400)
    op = tower.operands()
    assert tuple(op["Conv3d_1a_7x7"]["fp32"][0].shape) == (64, 7, 7, 7, 8)
    assert float(op["Conv3d_1a_7x7"]["fp32"][0][..., 3:].abs().max()) == 0.0
    assert tuple(op["Mixed_3b.b1b"]["bf16"][0].shape) == (128, 3, 3, 3, 96)
    assert op["Mixed_3b.b1b"]["bf16"][0].dtype == torch.bfloat16
    assert tuple(op["Mixed_3b.b0"]["fp32"][0].shape) == (64, 192)
    assert tuple(op["logits"]["fp32"][0].shape) == (400, 1024)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        tower(torch.zeros(1, 16, 32, 32, 3, dtype=torch.uint8))


def test_load_i3d_pretrained_missing_path_is_loud_and_offline(tmp_path, monkeypatch):
    import socket
    import urllib.request

    def refuse(*a, **k):
        raise AssertionError("network API touched")

    monkeypatch.setattr(socket, "socket", refuse)
    monkeypatch.setattr(socket, "create_connection", refuse)
    monkeypatch.setattr(urllib.request, "urlopen", refuse)
    with pytest.raises(FileNotFoundError, match="nothing is downloaded"):
        I3D.load_i3d_pretrained(str(tmp_path / "i3d_pretrained_400.pt"), device="cpu")
    with pytest.raises(FileNotFoundError):
        I3D.load_i3d_pretrained(None, device="cpu")
    # a local file in the reference's layout loads through the code-free loader
    tower = I3D.InceptionI3dTower(400)
    shapes = {k: tuple(v.shape) for k, v in tower.state_dict().items() if k.startswith(("logits", "Conv3d_2b"))}
    sd = tower.state_dict()
    sd.update(R.hash_state(shapes))
    torch.save(sd, tmp_path / "i3d.pt")
    loaded = I3D.load_i3d_pretrained(str(tmp_path / "i3d.pt"), device="cpu", precision="bf16")
    assert loaded.precision == "bf16"
    assert torch.equal(loaded.logits.conv3d.bias, sd["logits.conv3d.bias"])


# ------------------------------------------------------------------ the restatements against torch's own ops
@pytest.mark.parametrize("size,kernel,stride", [((5, 17, 20), (7, 7, 7), (2, 2, 2)), ((2, 9, 14), (3, 3, 3), (1, 1, 1)),
                                                ((1, 7, 7), (3, 3, 3), (1, 1, 1))])
def test_conv_restatement_against_torch(size, kernel, stride):
    g = torch.Generator().manual_seed(3)
    x = torch.randn((2, *size, 8), generator=g, dtype=torch.float64)
    w = torch.randn((5, *kernel, 8), generator=g, dtype=torch.float64)
    b = torch.randn(5, generator=g, dtype=torch.float64)
    pads = R.same_pad(size, kernel, stride)
    got, S = R.conv3d(x, w, stride, tuple(p[0] for p in pads), tuple(p[2] for p in pads), bias=b, relu=True)
    xp = F.pad(x.permute(0, 4, 1, 2, 3), (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
    want = F.relu(F.conv3d(xp, w.permute(0, 4, 1, 2, 3), b, stride=stride)).permute(0, 2, 3, 4, 1)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) < 1e-10
    assert bool((S >= got.abs() - 1e-12).all())
    assert [(p[0], p[2]) for p in pads] == ops.same_pad_3d(size, kernel, stride)   # the host's own pad rule


@pytest.mark.parametrize("kernel,stride", [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)),
                                           ((2, 2, 2), (2, 2, 2))])
@pytest.mark.parametrize("size", [(4, 9, 9), (3, 14, 7), (2, 7, 7)])
def test_pool_restatement_against_torch(size, kernel, stride):
    x = -torch.rand((2, *size, 4), generator=torch.Generator().manual_seed(4), dtype=torch.float64) - 0.1
    pads = R.same_pad(size, kernel, stride)
    got = R.maxpool3d(x, kernel, stride, tuple(p[0] for p in pads), tuple(p[2] for p in pads))
    xp = F.pad(x.permute(0, 4, 1, 2, 3), (pads[2][0], pads[2][1], pads[1][0], pads[1][1], pads[0][0], pads[0][1]))
    want = F.max_pool3d(xp, kernel, stride).permute(0, 2, 3, 4, 1)
    assert torch.equal(got, want)


def test_head_and_preprocess_restatements_against_torch():
    g = torch.Generator().manual_seed(5)
    x = torch.randn((2, 3, 7, 7, 16), generator=g, dtype=torch.float64)
    w = torch.randn((6, 16), generator=g, dtype=torch.float64)
    b = torch.randn(6, generator=g, dtype=torch.float64)
    got, S = R.head(x, w, b)
    p = F.avg_pool3d(x.permute(0, 4, 1, 2, 3), (2, 7, 7), stride=1)              # [2, 16, 2, 1, 1]
    want = (F.conv3d(p, w.view(6, 16, 1, 1, 1), b).squeeze(3).squeeze(3)).mean(dim=2)
    assert float((got - want).abs().max()) < 1e-12 and bool((S >= got.abs() - 1e-12).all())
    for shape in ((1, 2, 96, 128, 3), (1, 2, 130, 100, 3)):
        v = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8)
        H, W = shape[2:4]
        Hr, Wr = R.resized_size(H, W)
        t = F.interpolate(v[0].permute(0, 3, 1, 2).double() / 255.0, size=(Hr, Wr), mode="bilinear", align_corners=False)
        h0, w0 = (Hr - 224) // 2, (Wr - 224) // 2
        want = ((t[:, :, h0:h0 + 224, w0:w0 + 224] - 0.5) * 2).permute(0, 2, 3, 1)
        assert float((R.preprocess(v)[0] - want).abs().max()) < 1e-12


# ------------------------------------------------------------------ planted defects
def test_planted_pool_padding_minus_inf_is_rejected():
    x = (-torch.rand((1, 3, 7, 7, 8), generator=torch.Generator().manual_seed(6)) - 0.1).double()
    kernel, stride = (3, 3, 3), (1, 1, 1)
    pads = R.same_pad((3, 7, 7), kernel, stride)
    front, out = tuple(p[0] for p in pads), tuple(p[2] for p in pads)
    ref = R.maxpool3d(x, kernel, stride, front, out)
    bad = R.maxpool3d(x, kernel, stride, front, out, pad_value=float("-inf"))
    with pytest.raises(AssertionError):
        assert_bit_equal(bad.float(), ref, "pool with -inf padding")
    assert_bit_equal(ref.float(), ref, "pool")


def test_planted_swapped_pads_are_rejected():
    """(5, 17, 20) under 7x7x7 / stride 2: total pads (6, 6, 5) split (3, 3), (3, 3), (2, 3); swapped (3, 2)"""
    g = torch.Generator().manual_seed(7)
    size, kernel, stride = (5, 17, 20), (7, 7, 7), (2, 2, 2)
    x = torch.randn((1, *size, 8), generator=g).double()
    w = (torch.randn((4, *kernel, 8), generator=g) / 50).double()
    pads, swapped = R.same_pad(size, kernel, stride), R.same_pad(size, kernel, stride, swap=True)
    assert [p[0] for p in pads] != [p[0] for p in swapped]
    out = tuple(p[2] for p in pads)
    ref, S = R.conv3d(x, w, stride, tuple(p[0] for p in pads), out)
    bad, _ = R.conv3d(x, w, stride, tuple(p[0] for p in swapped), out)
    with pytest.raises(AssertionError):
        assert_within(bad, ref, R.conv_bound(S, 343 * 8), "conv with swapped pads")
    # the same for the pool that takes the asymmetric split: (3, 14, 7) under (2, 2, 2) / (2, 2, 2)
    xs = torch.randn((1, 3, 14, 7, 8), generator=g).double()
    p2, s2 = R.same_pad((3, 14, 7), (2, 2, 2), (2, 2, 2)), R.same_pad((3, 14, 7), (2, 2, 2), (2, 2, 2), swap=True)
    o2 = tuple(p[2] for p in p2)
    with pytest.raises(AssertionError):
        assert_bit_equal(R.maxpool3d(xs, (2, 2, 2), (2, 2, 2), tuple(p[0] for p in s2), o2).float(),
                         R.maxpool3d(xs, (2, 2, 2), (2, 2, 2), tuple(p[0] for p in p2), o2), "pool, swapped pads")


def test_planted_biased_covariance_is_rejected(golden):
    a, b = R.embedding_sets()[0]
    want = float(golden["fd16_f64"])
    assert abs(R.frechet(a, b) - want) <= 1e-4 * abs(want)
    assert abs(R.frechet(a, b, unbiased=False) - want) > 1e-4 * abs(want)


def test_planted_rounding_uint8_conversion_is_rejected():
    from unified_video_action_amd.eval import eval as E
    x = torch.linspace(-1, 1, 4097)
    want = R.to_uint8(x)
    assert torch.equal(E.to_uint8(x), want)
    assert want.dtype == torch.uint8 and int(want[0]) == 0 and int(want[-1]) == 255
    assert not torch.equal(R.to_uint8(x, rounding=True), want)


# ------------------------------------------------------------------ the workspace's opt-in keys
def _workspace(tmp_path, extra=()):
    import cases
    import replay
    import train
    from unified_video_action_amd import config as C
    replay.golden_policy(normalizer=False)  # registers model_size "mar_golden"
    cfg = train.build_cfg(["--config-name=uva_pusht", "model.policy.autoregressive_model_params.model_size=mar_golden",
                           "model.policy.action_model_params.predict_action=true", "training.num_epochs=1",
                           "dataloader.batch_size=1", "dataloader.num_workers=0", "task.dataset.n_samples=4",
                           "training.resume=false", "training.mixed_precision=no", f"multi_run.run_dir={tmp_path}"]
                          + [f"+model.policy.autoregressive_model_params.{k}={str(v).lower() if isinstance(v, bool) else v}"
                             for k, v in cases.MAR_KW.items() if k in cases.POLICY_AMP_KEYS] + list(extra))
    return C.get_class(cfg.model._target_)(cfg)


def test_workspace_evaluates_nothing_unless_asked(tmp_path):
    """with the new keys absent the epoch-end evaluation adds no key to the epoch's log, builds no validation
    loader and loads no tower"""
    from unified_video_action_amd.runtime import RT
    try:
        ws = _workspace(tmp_path)
        assert ws.eval_plan() == (False, False)
        ws.setup(device="cpu")
        assert ws.val_dataloader is None and ws.i3d is None
        assert ws.evaluate_epoch() == {}
        ws2 = _workspace(tmp_path, ["+training.eval_action_l2=true"])
        assert ws2.eval_plan() == (False, True)
        ws3 = _workspace(tmp_path, [f"+training.i3d_pretrained_path={tmp_path}/missing.pt"])
        assert ws3.eval_plan() == (True, False)
        with pytest.raises(FileNotFoundError):
            ws3.setup(device="cpu")
    finally:
        RT.set_precision("bf16")
