"""Epoch-end evaluation (eval/eval.py) on the small golden MAR configuration with injected draws, and one
workspace epoch with both evaluations switched on."""
import json
import os
import types

import numpy as np
import pytest
import torch

import cases
import i3d_ref as R
import replay
from unified_video_action_amd.eval import eval as E
from unified_video_action_amd.fvd import fvd as FVD
from unified_video_action_amd.fvd.i3d import InceptionI3dTower

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 2


@pytest.fixture
def fp32():
    from unified_video_action_amd.runtime import RT
    RT.set_precision("fp32")
    yield
    RT.set_precision("bf16")


def _cfg(predict_action=True, debug=False):
    ns = types.SimpleNamespace
    return ns(model=ns(policy=ns(action_model_params=ns(predict_action=predict_action))), training=ns(debug=debug))


def _policy():
    return replay.golden_policy().to(DEV).eval()


def _batch(step):
    b = cases.trace_batch(step, B)
    return {"obs": {"image": torch.from_numpy(b["image"]), "agent_pos": torch.from_numpy(b["agent_pos"])},
            "action": torch.from_numpy(b["action"])}


def _dev(v):
    if isinstance(v, list):
        return [_dev(a) for a in v]
    return torch.from_numpy(v).to(DEV) if isinstance(v, np.ndarray) and v.dtype != np.int64 else v


def _eps():
    p = cases.policy_rng("full_dynamic_model", B)
    return {"vae_eps_x": p["vae_eps_x"], "vae_eps_c": p["vae_eps_c"]}


def _hash_tower():
    t = InceptionI3dTower(400)
    t.load_state_dict(R.hash_state({k: tuple(v.shape) for k, v in t.state_dict().items()}))
    return t


def test_action_l2_equals_float64_restatement(fp32):
    pol = _policy()
    rng = {k: _dev(v) for k, v in cases.sample_rng("pusht", B).items()}
    rng.update(_eps())
    loader = [_batch(0), _batch(1)]
    keep = {}
    log = E.test_action_l2(_cfg(), pol, loader, 0, None, DEV, rng=rng, keep=keep)
    assert set(log) == {"val_action_l2_distances"}
    # the same draws through sample_tokens by hand, unnormalized and measured in float64
    p = pol.normalizer["action"].params_dict
    scale, offset = p["scale"].double().cpu(), p["offset"].double().cpu()
    per_batch = []
    for batch in loader:
        batch = E.dict_apply(batch, lambda t: t.to(DEV))
        d = E.prepare_data_predict_action(None, batch, pol, DEV, rng)
        _, act = E._sample(pol, d, B, "policy_model", rng)
        assert tuple(act.shape) == (B, 16, 2)
        a = (act.double().cpu() - offset) / scale
        t = (d["trajectory"].double().cpu() - offset) / scale
        per_batch.append(torch.sqrt(((t[:, :, :9] - a[:, :, :9]) ** 2).sum(-1)).mean())
    want = float(torch.stack(per_batch).mean())
    got = log["val_action_l2_distances"]
    print(f"val_action_l2_distances {got:.6f} (float64 {want:.6f})")
    assert np.isfinite(got) and abs(got - want) <= 1e-6 * abs(want), (got, want)
    assert len(keep["pairs"]) == 2
    # debug stops after the first batch; a video-only policy logs nothing
    one = E.test_action_l2(_cfg(debug=True), pol, loader, 0, None, DEV, rng=rng)
    assert abs(one["val_action_l2_distances"] - float(per_batch[0])) <= 1e-6 * float(per_batch[0])
    assert E.test_action_l2(_cfg(), pol, loader, 0, None, DEV, name_label="ema_", rng=rng).keys() == \
        {"ema_val_action_l2_distances"}


def test_video_fvd_equals_frechet_of_the_towers_logits(fp32, tmp_path):
    pol = _policy()
    tower = _hash_tower().to(DEV)
    r = cases.video_sample_rng("pusht", num_iter=pol.sample_params["num_iter"], B=B)
    rng = {k: _dev(v) for k, v in r.items()}
    rng.update(_eps())
    loader = [_batch(0), _batch(1)]
    keep = {}
    log = E.test_video_fvd(_cfg(), pol, loader, 3, str(tmp_path), DEV, i3d=tower, rng=rng, keep=keep)
    assert set(log) == {"video_fvd"} and np.isfinite(log["video_fvd"])
    # the reference's shapes and dtypes: 4-frame halves repeated x4 to 16 frames, 256 x 256 RGB, uint8
    for k in ("real_clips", "pred_clips"):
        c = keep[k]
        assert tuple(c.shape) == (2 * B, 16, 256, 256, 3) and c.dtype == torch.uint8, (k, c.shape, c.dtype)
        assert torch.equal(c[:, 0::4], c[:, 1::4]) and torch.equal(c[:, 0::4], c[:, 3::4])
    assert not torch.equal(keep["real_clips"][:, 0], keep["real_clips"][:, 4])
    for k, f in (("real_grid", "real_3.npy"), ("pred_grid", "predicted_3.npy")):
        assert tuple(keep[k].shape) == (2 * B, 3, 8, 256, 256) and keep[k].dtype == torch.uint8
        assert np.array_equal(np.load(os.path.join(tmp_path, "vis", f)), keep[k].numpy())
    # both grids open with the same 4 history frames; the real one ends with the real clip's frames
    assert torch.equal(keep["real_grid"][:, :, :4], keep["pred_grid"][:, :, :4])
    assert torch.equal(keep["real_grid"][:, :, 4:].permute(0, 2, 3, 4, 1), keep["real_clips"][:, ::4])
    # the real frames are the truncated resize of the batch's future frames
    img = torch.cat([b["obs"]["image"] for b in loader])
    sel = [19, 23, 27, 31]
    up = torch.nn.functional.interpolate(img[:, sel].reshape(-1, 3, 96, 96).double(), size=(256, 256), mode="bilinear",
                                         align_corners=False).reshape(2 * B, 4, 3, 256, 256).permute(0, 1, 3, 4, 2)
    want = (up * 255.0 / 127.5 - 1 + 1) * 127.5
    diff = (keep["real_clips"][:, ::4].double() - want.floor()).abs()
    assert float(diff.max()) <= 1.0 and float((diff > 0).double().mean()) < 1e-3   # ties at integer values only
    # the logged number is the Fréchet distance of the tower's logits on exactly these clips
    pe, re = tower(keep["pred_clips"]).cpu(), tower(keep["real_clips"]).cpu()
    assert torch.equal(pe, keep["pred_embeddings"]) and torch.equal(re, keep["real_embeddings"])
    want = float(FVD.frechet_distance(pe, re))
    print(f"video_fvd {log['video_fvd']:.4f}")
    assert abs(log["video_fvd"] - want) <= 1e-9 * abs(want)


def test_workspace_epoch_logs_both_metrics_and_ranks_by_the_configured_key(tmp_path):
    import train
    from unified_video_action_amd import config as C
    from unified_video_action_amd.runtime import RT
    tower = _hash_tower()
    path = os.path.join(tmp_path, "i3d_pretrained_400.pt")
    torch.save(tower.state_dict(), path)
    replay.golden_policy(normalizer=False)  # registers model_size "mar_golden"
    fmt = "epoch={epoch:04d}-val_action_l2_distances={val_action_l2_distances:.3f}.ckpt"
    cfg = train.build_cfg(
        ["--config-name=uva_pusht", "model.policy.autoregressive_model_params.model_size=mar_golden",
         "model.policy.action_model_params.predict_action=true", "training.num_epochs=1", "training.max_train_steps=2",
         "training.checkpoint_every=1", "dataloader.batch_size=1", "dataloader.num_workers=0",
         "val_dataloader.batch_size=2", "val_dataloader.num_workers=0", "task.dataset.n_samples=4",
         "task.dataset.val_ratio=0.5", "training.resume=false", "training.mixed_precision=no",
         f"multi_run.run_dir={tmp_path}", "+training.eval_action_l2=true", f"+training.i3d_pretrained_path={path}",
         "checkpoint.topk.monitor_key=val_action_l2_distances", f"checkpoint.topk.format_str='{fmt}'"]
        + [f"+model.policy.autoregressive_model_params.{k}={str(v).lower() if isinstance(v, bool) else v}"
           for k, v in cases.MAR_KW.items() if k in cases.POLICY_AMP_KEYS])
    try:
        ws = C.get_class(cfg.model._target_)(cfg)
        assert ws.eval_plan() == (True, True)
        ws.run()
    finally:
        RT.set_precision("bf16")
    assert ws.i3d.precision == "fp32"
    logs = [json.loads(x) for x in open(os.path.join(tmp_path, "logs.json.txt"))]
    end = [r for r in logs if r.get("epoch_end")]
    assert len(end) == 1
    assert np.isfinite(end[0]["video_fvd"]) and np.isfinite(end[0]["val_action_l2_distances"])
    assert end[0]["val_action_l2_distances"] > 0
    names = os.listdir(os.path.join(tmp_path, "checkpoints"))
    assert any(n.startswith("epoch=0000-val_action_l2_distances=") for n in names), names
    assert not any("train_loss" in n for n in names), names
    for f in ("real_0.npy", "predicted_0.npy"):
        assert np.load(os.path.join(tmp_path, "vis", f)).dtype == np.uint8
