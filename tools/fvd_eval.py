"""FVD and frame-wise PSNR / SSIM of a checkpoint on N validation clips, or the I3D tower's own time.

    python tools/fvd_eval.py --config-name=uva_pusht --i3d PATH [--checkpoint CKPT] [--clips 64]
                             [--precision fp32|bf16] [--metrics] [key=value ...]
    python tools/fvd_eval.py --config-name=uva_pusht --metrics --no-fvd [--checkpoint CKPT] [--clips 64] [key=value ...]
    python tools/fvd_eval.py --tower-only --clips 256 --precision bf16 [--random-i3d] [--layers]

The first form builds the workspace of train.py for the config, loads the checkpoint (latest.ckpt of the run
directory when none is given and one exists), and runs eval.test_video_fvd on the EMA policy (when
training.use_ema) over as many validation batches as N clips need -- N is not capped at the epoch-end
evaluation's 16.  One JSON line: {"video_fvd", "clips", "precision", "tower_ms", "tower_calls"}; tower_ms is the
time spent in the I3D tower (HIP events around every call).
--metrics adds the frame-wise fidelity of the predicted future frames against the real ones (eval/video_metrics.py;
no weights needed): "video_psnr", "video_ssim" (means over every frame; a perfect frame counts at the PSNR of one
wrong level) and the per-horizon lists "video_psnr_t", "video_ssim_t".  --no-fvd (with --metrics)
skips the tower, and --i3d is then not required.  Two samplers on the same clips (the validation loader is not
shuffled; AP=model.policy.autoregressive_model_params):
    python tools/fvd_eval.py --metrics --no-fvd --checkpoint CKPT +$AP.video_sampler=ddpm
    python tools/fvd_eval.py --metrics --no-fvd --checkpoint CKPT +$AP.video_sampler=ddim +$AP.num_sampling_steps=ddim10
--tower-only times the tower alone on N random uint8 clips [N, 16, 256, 256, 3] (one warm-up pass, then one
timed pass between events): {"clips", "precision", "tower_ms", "ms_per_clip"}; --layers adds the time and the
TFLOP/s of every conv3d / gemm shape from the ops trace of a further pass.
--random-i3d uses a randomly initialised tower instead of --i3d: for timing only, the FVD it gives means nothing.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


class TimedTower:
    """the tower behind HIP events: every call is timed on the current stream"""

    def __init__(self, tower):
        self.tower, self.events = tower, []

    def __call__(self, videos):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = self.tower(videos)
        b.record()
        self.events.append((a, b))
        return out

    def total_ms(self):
        torch.cuda.synchronize()
        return sum(a.elapsed_time(b) for a, b in self.events)


def build_tower(args, device):
    from unified_video_action_amd.fvd.i3d import InceptionI3dTower, load_i3d_pretrained
    if args.random_i3d:
        tower = InceptionI3dTower(400, precision=args.precision)
        for u in tower.units().values():
            torch.nn.init.normal_(u.conv3d.weight, std=(2.0 / u.conv3d.weight[0].numel()) ** 0.5)
        return tower.to(device)
    return load_i3d_pretrained(args.i3d, device, precision=args.precision)


def tower_only(args):
    from unified_video_action_amd.native import ops
    dev = torch.device("cuda")
    tower = build_tower(args, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    clips = torch.randint(0, 256, (args.clips, 16, 256, 256, 3), generator=g, dtype=torch.uint8, device=dev)
    tower(clips[:min(args.clips, tower.clips_per_batch)])  # warm-up: operands, allocator, code objects
    torch.cuda.synchronize()
    timed = TimedTower(tower)
    timed(clips)
    ms = timed.total_ms()
    out = {"clips": args.clips, "precision": args.precision, "tower_ms": round(ms, 3),
           "ms_per_clip": round(ms / args.clips, 4)}
    if args.layers:
        ops.TRACE = {}
        try:
            tower(clips[:min(args.clips, tower.clips_per_batch)])
            torch.cuda.synchronize()
            rows = []
            for tag, evs in ops.TRACE.items():
                t = sum(a.elapsed_time(b) for a, b, _, _ in evs)
                fl = sum(f for _, _, f, _ in evs)
                rows.append({"op": tag, "calls": len(evs), "ms": round(t, 4),
                             "tflops": round(fl / t / 1e9, 2) if t > 0 and fl else None})
        finally:
            ops.TRACE = None
        out["layers"] = sorted(rows, key=lambda r: -r["ms"])
    print(json.dumps(out))


def checkpoint_fvd(args, overrides):
    import train
    from unified_video_action_amd import config as C
    from unified_video_action_amd.eval import eval as E
    cfg = train.build_cfg([f"--config-name={args.config_name}"] + (["--config-dir=" + args.config_dir]
                                                                    if args.config_dir else []) + overrides)
    cfg.training.resume = args.checkpoint is None
    ws = C.get_class(cfg.model._target_)(cfg)
    ws.setup()
    if args.checkpoint is not None:
        ws.load_checkpoint(path=args.checkpoint)
    policy = ws.ema_model if cfg.training.use_ema else ws.model
    policy.eval()
    vkw = dict(cfg.val_dataloader)
    loader = torch.utils.data.DataLoader(ws.dataset.get_validation_dataset(), **vkw)
    bs = int(vkw.get("batch_size", 1))
    timed = None if args.no_fvd else TimedTower(build_tower(args, ws.device))
    log = E.test_video_eval(cfg, policy, loader, ws.epoch, args.output_dir, ws.device, i3d=timed,
                            n_examples=-(-args.clips // bs), clips_per_batch=bs, fvd=timed is not None,
                            metrics=args.metrics)
    out = {"clips": min(args.clips, len(loader.dataset))}
    if timed is not None:
        out.update({"video_fvd": log["video_fvd"], "precision": args.precision,
                    "tower_ms": round(timed.total_ms(), 3), "tower_calls": len(timed.events)})
    if args.metrics:
        out.update(metrics_json(log))
    print(json.dumps(out))


def metrics_json(log):
    """the metric log keys of eval.test_video_eval -> the JSON line's entries (per-horizon values as lists)"""
    h = sum(1 for k in log if k.startswith("video_psnr/t"))
    return {"video_psnr": log["video_psnr"], "video_ssim": log["video_ssim"],
            "video_psnr_t": [log[f"video_psnr/t{t}"] for t in range(1, h + 1)],
            "video_ssim_t": [log[f"video_ssim/t{t}"] for t in range(1, h + 1)]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config-name", default="uva_pusht")
    ap.add_argument("--config-dir", default=None)
    ap.add_argument("--i3d", default=None, help="local i3d_pretrained_400.pt (the reference's state-dict layout)")
    ap.add_argument("--random-i3d", action="store_true")
    ap.add_argument("--checkpoint", default=None)
    ap.add_argument("--clips", type=int, default=16)
    ap.add_argument("--precision", default="fp32", choices=("fp32", "bf16"))
    ap.add_argument("--output-dir", default=None, help="where the real / predicted grids go (.npy); none by default")
    ap.add_argument("--tower-only", action="store_true")
    ap.add_argument("--layers", action="store_true")
    ap.add_argument("--metrics", action="store_true", help="add the frame-wise PSNR / SSIM of the predicted frames")
    ap.add_argument("--no-fvd", action="store_true", help="with --metrics: skip the I3D tower (no --i3d needed)")
    args, overrides = ap.parse_known_args(argv)
    if args.no_fvd and (not args.metrics or args.tower_only):
        ap.error("--no-fvd goes with --metrics (and not with --tower-only): nothing would be evaluated")
    if not args.no_fvd and not args.random_i3d and not args.i3d:
        ap.error("--i3d PATH (or --random-i3d for timing) is required unless --metrics --no-fvd is given")
    if not torch.cuda.is_available():
        raise SystemExit("fvd_eval.py needs the GPU: the tower runs on libuva_hip.so kernels")
    if args.tower_only:
        tower_only(args)
    else:
        checkpoint_fvd(args, overrides)


if __name__ == "__main__":
    main()
