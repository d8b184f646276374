"""The frame-wise video metrics through the epoch-end evaluation (eval/eval.py:test_video_eval) on the small golden
MAR configuration with injected draws, and through one workspace epoch with training.eval_video_metrics."""
import json
import os
import types

import numpy as np
import pytest
import torch

import cases
import i3d_ref as I3
import replay
import video_metrics_ref as R
from unified_video_action_amd.eval import eval as E
from unified_video_action_amd.eval import video_metrics as VM
from unified_video_action_amd.fvd.i3d import InceptionI3dTower
from unified_video_action_amd.native import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
B = 2
METRIC_KEYS = {"video_psnr", "video_ssim"} | {f"video_{k}/t{t}" for k in ("psnr", "ssim") for t in (1, 2, 3, 4)}


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
    t.load_state_dict(I3.hash_state({k: tuple(v.shape) for k, v in t.state_dict().items()}))
    return t


def _rng(pol):
    r = cases.video_sample_rng("pusht", num_iter=pol.sample_params["num_iter"], B=B)
    rng = {k: _dev(v) for k, v in r.items()}
    rng.update(_eps())
    return rng


def test_metrics_entry_logs_the_restatements_aggregate(fp32, tmp_path):
    pol = _policy()
    keep = {}
    log = E.test_video_eval(_cfg(), pol, [_batch(0), _batch(1)], 3, str(tmp_path), DEV, rng=_rng(pol), keep=keep,
                            fvd=False, metrics=True)
    assert set(log) == METRIC_KEYS                                   # ten keys for h = 4, and no tower was needed
    assert "pred_embeddings" not in keep
    pred, real = keep["pred_clips"][:, ::4], keep["real_clips"][:, ::4]   # the frames before the x4 repeat
    assert tuple(pred.shape) == (2 * B, 4, 256, 256, 3) and pred.dtype == torch.uint8
    sse, ssim_sum, bound = R.frame_metrics(pred.numpy(), real.numpy(), tile=ops.frame_metrics_tile())
    want = R.aggregate(sse, ssim_sum, 256, 256)
    print(f"golden policy (hash-initialised weights: no statement about quality): video_psnr {log['video_psnr']:.4f} dB, "
          f"video_ssim {log['video_ssim']:.6f}; per horizon psnr {[round(log[f'video_psnr/t{t}'], 4) for t in (1, 2, 3, 4)]} "
          f"ssim {[round(log[f'video_ssim/t{t}'], 6) for t in (1, 2, 3, 4)]}")
    assert abs(log["video_ssim"] - want["ssim"]) <= 1e-9 and abs(log["video_psnr"] - want["psnr"]) <= 1e-7
    for t in range(4):
        assert abs(log[f"video_ssim/t{t + 1}"] - want["ssim_t"][t]) <= 1e-9
        assert abs(log[f"video_psnr/t{t + 1}"] - want["psnr_t"][t]) <= 1e-7
    # keep receives the per-frame values [n, h]
    assert tuple(keep["psnr"].shape) == (2 * B, 4) and tuple(keep["ssim"].shape) == (2 * B, 4)
    assert keep["psnr"].dtype == torch.float64 and keep["ssim"].dtype == torch.float64
    assert float((keep["ssim"] - torch.from_numpy(ssim_sum / (3.0 * 246 * 246))).abs().max()) <= 1e-9
    assert float((keep["psnr"] - torch.from_numpy(R.psnr(sse, 3 * 256 * 256))).abs().max()) <= 1e-7
    # the planar grids the evaluation saves give the same frames through channels=1
    m = VM.psnr_ssim(keep["pred_grid"][:, :, 4:].to(DEV), keep["real_grid"][:, :, 4:].to(DEV), channels=1)
    assert torch.equal(m["psnr"], keep["psnr"]) and torch.equal(m["ssim"], keep["ssim"])
    assert E.test_video_eval(_cfg(), pol, [_batch(0)], 3, None, DEV, rng=_rng(pol), fvd=False, metrics=True,
                             name_label="ema_").keys() == {"ema_" + k for k in METRIC_KEYS}


def test_perfect_prediction_logs_one_and_the_cap():
    real = torch.from_numpy(R.make_pair("noise", (2, 4, 256, 256))[0]).to(DEV)
    clip = real.repeat_interleave(4, dim=1)
    m = VM.psnr_ssim(clip.clone()[:, ::4], clip[:, ::4])
    assert bool((m["sse"] == 0).all()) and bool(torch.isinf(m["psnr"]).all()) and bool((m["ssim"] == 1.0).all())
    log = VM.log_entries(VM.aggregate(m))
    cap = 10.0 * np.log10(255.0 ** 2 * 3 * 256 * 256)
    assert log["video_ssim"] == 1.0 and abs(log["video_psnr"] - cap) <= 1e-12
    assert all(log[f"video_ssim/t{t}"] == 1.0 and abs(log[f"video_psnr/t{t}"] - cap) <= 1e-12 for t in (1, 2, 3, 4))


def test_fvd_is_bit_equal_with_metrics_on(fp32, tmp_path):
    pol = _policy()
    tower = _hash_tower().to(DEV)
    loader = [_batch(0), _batch(1)]
    off_dir, on_dir = os.path.join(tmp_path, "off"), os.path.join(tmp_path, "on")
    off = E.test_video_fvd(_cfg(), pol, loader, 3, off_dir, DEV, i3d=tower, rng=_rng(pol))
    on = E.test_video_eval(_cfg(), pol, loader, 3, on_dir, DEV, i3d=tower, rng=_rng(pol), fvd=True, metrics=True)
    assert set(off) == {"video_fvd"} and set(on) == METRIC_KEYS | {"video_fvd"}
    assert on["video_fvd"] == off["video_fvd"], (on["video_fvd"], off["video_fvd"])
    for f in ("real_3.npy", "predicted_3.npy"):
        assert np.array_equal(np.load(os.path.join(on_dir, "vis", f)), np.load(os.path.join(off_dir, "vis", f)))


def _workspace(tmp_path, extra):
    import train
    from unified_video_action_amd import config as C
    replay.golden_policy(normalizer=False)  # registers model_size "mar_golden"
    cfg = train.build_cfg(
        ["--config-name=uva_pusht", "model.policy.autoregressive_model_params.model_size=mar_golden",
         "model.policy.action_model_params.predict_action=true", "training.num_epochs=1", "training.max_train_steps=2",
         "training.checkpoint_every=1", "dataloader.batch_size=1", "dataloader.num_workers=0",
         "val_dataloader.batch_size=2", "val_dataloader.num_workers=0", "task.dataset.n_samples=4",
         "task.dataset.val_ratio=0.5", "training.resume=false", "training.mixed_precision=no",
         f"multi_run.run_dir={tmp_path}"] + extra
        + [f"+model.policy.autoregressive_model_params.{k}={str(v).lower() if isinstance(v, bool) else v}"
           for k, v in cases.MAR_KW.items() if k in cases.POLICY_AMP_KEYS])
    return C.get_class(cfg.model._target_)(cfg)


def _epoch_end(tmp_path):
    logs = [json.loads(x) for x in open(os.path.join(tmp_path, "logs.json.txt"))]
    end = [r for r in logs if r.get("epoch_end")]
    assert len(end) == 1
    return end[0]


def test_workspace_logs_the_metrics_without_i3d_weights(tmp_path):
    from unified_video_action_amd.runtime import RT
    fmt = "epoch={epoch:04d}-video_psnr={video_psnr:.3f}.ckpt"
    try:
        ws = _workspace(tmp_path, ["+training.eval_video_metrics=true", "checkpoint.topk.monitor_key=video_psnr",
                                   "checkpoint.topk.mode=max", f"checkpoint.topk.format_str='{fmt}'"])
        assert ws.eval_plan() == (False, False) and ws.eval_video_metrics()
        ws.run()
    finally:
        RT.set_precision("bf16")
    assert ws.i3d is None
    end = _epoch_end(tmp_path)
    assert METRIC_KEYS <= set(end) and "video_fvd" not in end and "val_action_l2_distances" not in end
    assert all(np.isfinite(end[k]) for k in METRIC_KEYS) and 0 < end["video_psnr"] < 100 and -1 <= end["video_ssim"] <= 1
    names = os.listdir(os.path.join(tmp_path, "checkpoints"))
    assert any(n.startswith("epoch=0000-video_psnr=") for n in names), names


def test_workspace_without_the_key_logs_what_it_always_logged(tmp_path):
    from unified_video_action_amd.runtime import RT
    try:
        ws = _workspace(tmp_path, [])
        assert ws.eval_plan() == (False, False) and not ws.eval_video_metrics()
        ws.run()
    finally:
        RT.set_precision("bf16")
    assert ws.val_dataloader is None
    assert set(_epoch_end(tmp_path)) == {"train_loss", "global_step", "epoch", "epoch_end"}
