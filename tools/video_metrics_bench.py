"""Time of the frame-wise video metrics beside the time of generating the clips they compare, tools only.

    python tools/video_metrics_bench.py [--reps 30] [--gen-reps 7] [--config pusht_joint]

ops.frame_metrics on the epoch-end operands -- 16 clips x 4 frames x 256 x 256 x 3 uint8, predicted against real,
in one call and as the evaluation issues it (4 calls of 4 clips) -- and, in the same process, the generation of
one batch of those clips as eval/eval.py does it (sample_tokens(full_dynamic_model) on 4 clips and the VAE decode
of the tokens; the evaluation runs it 4 times).  HIP events around every call, WARM warm calls first, the median
and min .. max of the repeats.  One JSON row per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unified_video_action_amd.native import ops  # noqa: E402

DEV = "cuda"
WARM = 3


def _ms(fn):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e)


def _row(what, ts, **kw):
    return dict(what=what, ms=round(statistics.median(ts), 4), min_ms=round(min(ts), 4), max_ms=round(max(ts), 4),
                n=len(ts), **kw)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--gen-reps", type=int, default=7)
    ap.add_argument("--config", default="pusht_joint")
    a = ap.parse_args()
    print(json.dumps({"device": torch.cuda.get_device_name(0), "warm": WARM}), flush=True)

    g = torch.Generator(device=DEV).manual_seed(0)
    real = torch.randint(0, 256, (16, 4, 256, 256, 3), generator=g, dtype=torch.uint8, device=DEV)
    pred = (real.int() + torch.randint(-6, 7, real.shape, generator=g, device=DEV)).clamp(0, 255).to(torch.uint8)
    work = torch.empty(ops.frame_metrics_workspace_bytes(16, 4, 256, 256) // 8, dtype=torch.float64, device=DEV)
    sse = torch.empty(16, 4, dtype=torch.int64, device=DEV)
    ssim = torch.empty(16, 4, dtype=torch.float64, device=DEV)

    def one_call():
        ops.frame_metrics(pred, real, sse=sse, ssim_sum=ssim, work=work)

    def four_calls():
        for i in range(0, 16, 4):
            ops.frame_metrics(pred[i:i + 4], real[i:i + 4], sse=sse[i:i + 4], ssim_sum=ssim[i:i + 4], work=work)

    for what, fn in (("frame_metrics 16 clips, one call", one_call), ("frame_metrics 16 clips, 4 calls of 4", four_calls)):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        print(json.dumps(_row(what, [_ms(fn) for _ in range(a.reps)], frames=64,
                              mean_ssim=round(float(ssim.mean()) / (3 * 246 * 246), 6))), flush=True)

    from unified_video_action_amd import presets
    from unified_video_action_amd.policy.unified_video_action_policy import UnifiedVideoActionPolicy
    pol = UnifiedVideoActionPolicy(**presets.policy_kwargs(a.config, autoregressive_model_params={})).to(DEV).eval()
    presets.fit_normalizer(a.config, pol)
    K = 4
    tok = torch.randn(K, 4, 256, 16, device=DEV)  # the history half's latent tokens
    nact = torch.zeros(K, 16, pol.action_dim, device=DEV)
    sp = pol.sample_params

    @torch.no_grad()
    def generate():
        z, _ = pol.model.sample_tokens(bsz=K, cond=tok, num_iter=sp["num_iter"], cfg=sp["cfg"],
                                       cfg_schedule=sp["cfg_schedule"], temperature=sp["temperature"], nactions=nact,
                                       task_mode="full_dynamic_model", vae_model=pol.vae_model)
        return pol.vae_model.decode(z / 0.2325).clamp(-1, 1)

    for _ in range(2):
        generate()
    torch.cuda.synchronize()
    print(json.dumps(_row("generation of 4 clips (sample_tokens + VAE decode); the evaluation runs it 4 times",
                          [_ms(generate) for _ in range(a.gen_reps)], clips=K, config=a.config,
                          video_steps=pol.model.diffloss.num_sampling_steps)), flush=True)


if __name__ == "__main__":
    main()
