"""Epoch-end evaluation: video FVD and action L2 on validation batches (reference: eval/eval.py:60-417, run
after every epoch by workspace/train_unified_video_action_workspace.py:342-376).

test_video_fvd   n_examples = 4 validation batches, k = min(4, B) clips each: the use_history_action frame
                 drop, prepare_data_predict_action, MAR.sample_tokens(task_mode="full_dynamic_model"), decode
                 of z / 0.2325, clamp, uint8 by truncation (`.type(torch.uint8)`), frames repeated x4 when a
                 clip has fewer than 16, I3D logits of the real and the predicted clips, Fréchet distance.
test_action_l2   every validation batch: sample_tokens(task_mode="policy_model"), both trajectories
                 unnormalized, mean L2 over the first 9 action dimensions.
Both return the reference's log keys (`video_fvd`, `val_action_l2_distances`, prefixed by name_label).
test_video_eval  the loop of test_video_fvd, serving the FVD, the frame-wise PSNR / SSIM of the predicted future
                 frames against the real ones (video_metrics.py; not in the reference) or both from one pass of
                 clip generation; test_video_fvd is test_video_eval with the metrics off.

Differences from the reference: the I3D tower is this build's HIP one (fvd/i3d.py) and is passed in (or
loaded from the LOCAL file training.i3d_pretrained_path -- nothing is downloaded); no GIF / wandb video is
written (no encoder in this build): with output_dir given, the real and predicted uint8 grids
[n, 3, T, 256, 256] go to vis/<label>real_<it>.npy and vis/<label>predicted_<it>.npy; keypoint plots
(plot_actions) are not drawn.  An optional `rng` is passed through to the frame selection, the VAE posterior
draws and sample_tokens, so tests can inject every draw.
"""
import os

import numpy as np
import torch

from ..fvd.fvd import frechet_distance, get_fvd_logits
from ..native import ops
from ..runtime import cdt
from ..utils.data_utils import get_trajectory, image_key, select_frame_indices, umi_proprioception

N_EXAMPLES = 4   # eval.py:141
LATENT_SCALE = 0.2325


def dict_apply(x, fn):
    """common/pytorch_util.py dict_apply"""
    return {k: dict_apply(v, fn) if isinstance(v, dict) else fn(v) for k, v in x.items()}


def to_uint8(x):
    """an image in [-1, 1] -> uint8 as eval.py:207-217: (1 + x) * 127.5, then `.type(torch.uint8)` (truncation)"""
    return ((1 + x) * 127.5).type(torch.uint8)


def unnormalize_future_action(policy, actions):
    """data_utils.py:169-174"""
    if policy.normalizer_type == "all":
        return policy.normalizer["action"].unnormalize(actions)
    return actions


def prepare_data_predict_action(cfg, batch, policy, device, rng=None):
    """eval.py:60-126 on this build's fused pieces (normalize, process_data with the TRAINING frame selection,
    get_vae_latent(eval=True), get_trajectory) -> dict:
      x  all selected frames [B, 3, 2h, 256, 256] fp32 in [-1, 1] (history half, then future half)
      real  the future half [B, 3, h, 256, 256];  c  the history half's latent tokens [B, h, 256, C]
      text_latents, history_trajectory, trajectory, proprioception_input"""
    rng = rng or {}
    obs = dict(batch["obs"])
    img = obs.get("image", obs.get(image_key(policy.task_name)))
    B, T = img.shape[:2]
    text_latents = None
    if policy.language_emb_model == "clip":
        if policy.text_model is not None and "language" in obs:
            language = obs.pop("language")
            text_latents = policy._encode_tokens(language[:, 0, 0].long(), language[:, 0, 1].long(), device)
        elif "language_latents" in batch:
            text_latents = batch["language_latents"]
        else:
            raise NotImplementedError("evaluation of a CLIP-conditioned policy needs language tokens (with a text "
                                      "tower) or language_latents in the batch")
    nactions = policy._normalize("action", batch["action"].float())
    if policy.normalizer_type == "all":
        for k in list(obs):
            if "image" not in k and k in policy.normalizer:
                obs[k] = policy.normalizer[k].normalize(obs[k])
    prop = {}
    T_traj = T
    if "umi" in policy.task_name:
        sel = np.arange(T)
        T_traj = T * 4
        if policy.use_proprioception:
            idx = obs["img_indices"].int().squeeze(2) if "img_indices" in obs else None
            prop = umi_proprioception(obs, idx, policy.different_history_freq)
    else:
        sel = select_frame_indices(T, different_history_freq=policy.different_history_freq,
                                   rng_choice=rng.get("history_combination"))
        if policy.use_proprioception:
            prop = policy._second_camera_prop(obs, sel, train=True, eps=rng.get("vae_eps_wrist"))
    h = len(sel) // 2
    vae = policy.vae_model
    frames = torch.empty(B * len(sel), 256, 256, vae.CIN_PAD, dtype=torch.float32, device=device)
    ops.resize_select(img.float().contiguous(), torch.as_tensor(np.asarray(sel), dtype=torch.int32, device=device),
                      frames, vae.CIN_PAD)  # future half of every sample first, then the history half
    if rng.get("vae_eps_x") is not None:
        eps = torch.cat([torch.as_tensor(rng["vae_eps_x"]), torch.as_tensor(rng["vae_eps_c"])]).to(device)
    else:
        eps = torch.randn(B * len(sel), vae.embed_dim, 16, 16, device=device)
    tokens = vae.encode_tokens(frames.to(cdt()), eps)
    c = tokens[B * h:].reshape(B, h, 256, tokens.shape[-1])
    fr = frames[..., :3].reshape(2, B, h, 256, 256, 3).permute(0, 1, 5, 2, 3, 4)  # [half, B, 3, h, 256, 256]
    history, trajectory = get_trajectory(nactions, T_traj, policy.shift_action, policy.use_history_action)
    return dict(x=torch.cat([fr[1], fr[0]], dim=2), real=fr[0], c=c, text_latents=text_latents,
                history_trajectory=history if policy.use_history_action else None, trajectory=trajectory,
                proprioception_input=prop)


def _sample(policy, d, bsz, task_mode, rng):
    sp = policy.sample_params
    return policy.model.sample_tokens(
        bsz=bsz, cond=d["c"], text_latents=d["text_latents"], num_iter=sp["num_iter"], cfg=sp["cfg"],
        cfg_schedule=sp["cfg_schedule"], temperature=sp["temperature"], history_nactions=d["history_trajectory"],
        nactions=d["trajectory"], proprioception_input=d["proprioception_input"], task_mode=task_mode,
        vae_model=policy.vae_model, rng=rng)


def _frame_drop(policy, batch):
    """eval.py:155-156: with use_history_action every OBSERVATION drops its first step (the actions were taken
    out before)"""
    if not policy.use_history_action:
        return batch
    out = dict(batch)
    out["obs"] = {k: (v[:, 1:] if torch.is_tensor(v) and v.dim() >= 2 else v) for k, v in batch["obs"].items()}
    return out


def _load_i3d(cfg, device):
    from ..fvd.i3d import load_i3d_pretrained
    return load_i3d_pretrained(cfg.training.get("i3d_pretrained_path"), device,
                               precision=cfg.training.get("fvd_precision", "fp32") or "fp32")


@torch.no_grad()
def test_video_eval(cfg, policy, loader, it, output_dir, device, name_label="", i3d=None, rng=None, keep=None,
                    n_examples=N_EXAMPLES, clips_per_batch=N_EXAMPLES, fvd=True, metrics=False):
    """One pass of clip generation that serves the FVD (fvd=True), the frame-wise metrics (metrics=True) or both.
    -> the log entries: name_label + "video_fvd" with fvd; with metrics name_label + "video_psnr", "video_ssim"
    (means over every predicted frame) and "video_psnr/t1" .. "/t{h}", "video_ssim/t1" .. "/t{h}" (means per
    prediction horizon; eval/video_metrics.aggregate, whose PSNR cap for perfect frames applies).
    The metrics compare exactly the uint8 future frames the tower sees, pred against real [k, h, 256, 256, 3],
    before the x4 repeat; they draw nothing, so with both on the FVD is the FVD with metrics off.
    keep: an optional dict that receives the uint8 clips the tower saw (real_clips / pred_clips
    [n, 16, 256, 256, 3]), the saved grids, with fvd the logits (real_embeddings / pred_embeddings) and with
    metrics the per-frame psnr / ssim [n, h].  i3d: the tower (loaded from training.i3d_pretrained_path when
    absent); not needed, and not loaded, with fvd=False."""
    if not (fvd or metrics):
        raise ValueError("test_video_eval: nothing to evaluate (fvd and metrics are both off)")
    if fvd and i3d is None:
        i3d = _load_i3d(cfg, device)
    if metrics:
        from . import video_metrics as VM
    frame_psnr, frame_ssim = [], []
    real_emb, pred_emb, reals, predictions, real_clips, pred_clips = [], [], [], [], [], []
    for n, batch in enumerate(loader):
        if n >= n_examples:
            break
        batch = dict_apply(batch, lambda t: t.to(device, non_blocking=True))
        actions = batch["action"]
        batch = _frame_drop(policy, batch)
        B = actions.shape[0]
        k = min(clips_per_batch, B)
        batch = dict_apply(batch, lambda t: t[:k])
        batch["action"] = actions[:k]
        d = prepare_data_predict_action(cfg, batch, policy, device, rng)
        z, _ = _sample(policy, d, k, "full_dynamic_model", rng)
        pred = policy.vae_model.decode(z / LATENT_SCALE).clamp(-1, 1).cpu()
        pred = to_uint8(pred.reshape(k, -1, *pred.shape[1:]).permute(0, 1, 3, 4, 2))   # b t h w c
        real = to_uint8(d["real"].permute(0, 2, 3, 4, 1).cpu())
        if metrics:
            m = VM.psnr_ssim(pred.to(device), real.to(device))
            frame_psnr.append(m["psnr"])
            frame_ssim.append(m["ssim"])
        x = to_uint8(d["x"].cpu())                                                        # b c t h w
        hist = x[:, :, :x.size(2) // 2]
        reals.append(torch.cat([hist, real.permute(0, 4, 1, 2, 3)], dim=2))
        predictions.append(torch.cat([hist, pred.permute(0, 4, 1, 2, 3)], dim=2))
        if real.shape[1] < 16:
            pred = pred.repeat_interleave(repeats=4, dim=1)
            real = real.repeat_interleave(repeats=4, dim=1)
        pred, real = pred.contiguous(), real.contiguous()
        if fvd:
            pred_emb.append(get_fvd_logits(pred, i3d).cpu())
            real_emb.append(get_fvd_logits(real, i3d).cpu())
        real_clips.append(real)
        pred_clips.append(pred)
    if not real_clips:
        raise ValueError("test_video_fvd: the validation loader is empty")
    log = {}
    if fvd:
        real_emb, pred_emb = torch.cat(real_emb), torch.cat(pred_emb)
        log[f"{name_label}video_fvd"] = float(frechet_distance(pred_emb, real_emb))
    if metrics:
        frame_psnr, frame_ssim = torch.cat(frame_psnr), torch.cat(frame_ssim)
        log.update(VM.log_entries(VM.aggregate({"psnr": frame_psnr, "ssim": frame_ssim},
                                               n_values=real_clips[0][0, 0].numel()), name_label))
    if output_dir is not None:
        os.makedirs(os.path.join(output_dir, "vis"), exist_ok=True)
        np.save(os.path.join(output_dir, "vis", f"{name_label}real_{it}.npy"), torch.cat(reals).numpy())
        np.save(os.path.join(output_dir, "vis", f"{name_label}predicted_{it}.npy"), torch.cat(predictions).numpy())
    if keep is not None:
        keep.update(real_clips=torch.cat(real_clips), pred_clips=torch.cat(pred_clips), real_grid=torch.cat(reals),
                    pred_grid=torch.cat(predictions))
        if fvd:
            keep.update(real_embeddings=real_emb, pred_embeddings=pred_emb)
        if metrics:
            keep.update(psnr=frame_psnr, ssim=frame_ssim)
    return log


def test_video_fvd(cfg, policy, loader, it, output_dir, device, name_label="", plot_actions=False, i3d=None, rng=None,
                   keep=None, n_examples=N_EXAMPLES, clips_per_batch=N_EXAMPLES):
    """-> {name_label + "video_fvd": float}.  keep: an optional dict that receives the uint8 clips the tower saw
    (real_clips / pred_clips [n, 16, 256, 256, 3]) and their logits (real_embeddings / pred_embeddings).
    n_examples batches of min(clips_per_batch, B) clips are evaluated: the reference's 4 x 4 by default
    (tools/fvd_eval.py raises both for larger evaluations).  test_video_eval with the metrics off."""
    return test_video_eval(cfg, policy, loader, it, output_dir, device, name_label=name_label, i3d=i3d, rng=rng,
                           keep=keep, n_examples=n_examples, clips_per_batch=clips_per_batch, fvd=True, metrics=False)


@torch.no_grad()
def test_action_l2(cfg, policy, loader, it, output_dir, device, text_model=None, name_label="", plot_actions=False,
                   rng=None, keep=None):
    """-> {name_label + "val_action_l2_distances": float} when the policy predicts actions, else {}.
    keep: an optional dict that receives the per-batch (predicted, target) unnormalized trajectories."""
    predict_action = bool(cfg.model.policy.action_model_params.predict_action)
    dists, pairs = [], []
    for batch in loader:
        batch = dict_apply(batch, lambda t: t.to(device, non_blocking=True))
        actions = batch["action"]
        batch = _frame_drop(policy, batch)
        batch["action"] = actions
        B = actions.shape[0]
        d = prepare_data_predict_action(cfg, batch, policy, device, rng)
        _, act_out = _sample(policy, d, B, "policy_model", rng)
        if predict_action:
            act_out = unnormalize_future_action(policy, act_out)
            trajectory = unnormalize_future_action(policy, d["trajectory"])
            l2 = torch.sqrt(torch.sum((trajectory[:, :, :9] - act_out[:, :, :9]) ** 2, dim=-1))
            dists.append(l2.mean())
            pairs.append((act_out.cpu(), trajectory.cpu()))
        if cfg.training.debug:
            break
    if keep is not None:
        keep["pairs"] = pairs
    if not predict_action:
        return {}
    if not dists:
        raise ValueError("test_action_l2: the validation loader is empty")
    return {f"{name_label}val_action_l2_distances": torch.stack(dists).mean().item()}
