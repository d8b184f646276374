"""Inference latency of predict_action (PushT joint config, mar_base, full KL-VAE) and of the action sampler
alone, graph vs eager.  Run on the GPU box:
    python tools/tools_infer_bench.py [--batches 1,32] [--iters 10]
        [--act-sampler ddim --act-steps ddim10 --eta 0] [--video-sampler ddim --video-steps ddim10]
Prints one JSON line per batch size.

    python tools/tools_infer_bench.py --compare --act-sampler ddim --act-steps ddim10 [--video-clips 4]
builds the default policy (100-step ancestral sampler) and the one the flags describe in ONE process and times
them alternating, call by call (HIP events around every call, median and min .. max of --iters calls after 3 warm
calls each): predict_action, the action sampler loop alone (DiffActLoss.sample on fixed decoder rows) and, with
--video-clips K, the video generation of the epoch-end FVD evaluation (sample_tokens(full_dynamic_model) on K
clips).  Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def build(config, dev, keys):
    from unified_video_action_amd import presets
    from unified_video_action_amd.policy.unified_video_action_policy import UnifiedVideoActionPolicy
    pol = UnifiedVideoActionPolicy(**presets.policy_kwargs(config, autoregressive_model_params=keys)).to(dev).eval()
    presets.fit_normalizer(config, pol)
    return pol


def sampler_keys(a):
    keys = {}
    if a.act_sampler != "ddpm" or a.act_steps is not None:
        keys.update(act_sampler=a.act_sampler, act_ddim_eta=a.eta if a.act_sampler == "ddim" else 0.0)
    if a.act_steps is not None:
        keys["act_diff_testing_steps"] = a.act_steps
    if a.video_sampler != "ddpm":
        keys.update(video_sampler=a.video_sampler, video_ddim_eta=a.eta)
    if a.video_steps is not None:
        keys["num_sampling_steps"] = a.video_steps
    return keys


def alternate(fns, iters, warm=3):
    """fns: {name: callable}.  Every callable is warmed, then they run in turn, `iters` rounds, HIP events around
    every call -> {name: (median ms, min, max)}"""
    for f in fns.values():
        for _ in range(warm):
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(iters):
        for k, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in ms.items()}


def compare(a, dev):
    from unified_video_action_amd import presets
    keys = sampler_keys(a)
    pols = {"default": build(a.config, dev, {}), "flags": build(a.config, dev, keys)}
    pols["flags"].load_state_dict(pols["default"].state_dict())  # the same weights on both legs

    def report(what, res, n=None, **extra):
        for leg, (med, lo, hi) in res.items():
            dal = pols[leg].model.diffactloss
            print(json.dumps({"what": what, "leg": leg, "ms": round(med, 3), "min": round(lo, 3), "max": round(hi, 3),
                              "n": n or a.iters, "act_sampler": dal.act_sampler, "act_steps": dal.act_diff_testing_steps,
                              "video_sampler": pols[leg].model.diffloss.video_sampler,
                              "video_steps": pols[leg].model.diffloss.num_sampling_steps, "eta": a.eta, **extra}),
                  flush=True)

    for B in [int(x) for x in a.batches.split(",")]:
        obs = presets.synthetic_batch(a.config, B, dev, seed=B)["obs"]
        report("predict_action", alternate({k: (lambda p=p: p.predict_action(obs)) for k, p in pols.items()}, a.iters),
               batch=B)
        z = torch.randn(B, 1024, pols["default"].model.decoder_embed.weight.shape[0], device=dev)
        report("action_sampler_loop",
               alternate({k: (lambda p=p: p.model.diffactloss.sample(z, 0.95)) for k, p in pols.items()}, a.iters),
               batch=B, routes={k: ("persistent" if p.model.diffactloss._sampler._cache["persist"] else "graph")
                                for k, p in pols.items()})
    if a.video_clips:
        K = a.video_clips
        tok = torch.randn(K, 4, 256, 16, device=dev)  # the history half's latent tokens
        nact = torch.zeros(K, 16, pols["default"].action_dim, device=dev)

        def gen(p):
            sp = p.sample_params
            return p.model.sample_tokens(bsz=K, cond=tok, num_iter=sp["num_iter"], cfg=sp["cfg"],
                                         cfg_schedule=sp["cfg_schedule"], temperature=sp["temperature"],
                                         nactions=nact, task_mode="full_dynamic_model", vae_model=p.vae_model)
        n = max(3, a.iters // 4)
        report("fvd_video_generation", alternate({k: (lambda p=p: gen(p)) for k, p in pols.items()}, n, warm=2),
               n=n, clips=K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--config", default="pusht_joint")
    ap.add_argument("--act-sampler", default="ddpm", choices=["ddpm", "ddim"], help="update rule of the action head")
    ap.add_argument("--act-steps", default=None, help='act_diff_testing_steps, e.g. "ddim10" (strided) or "10" (even)')
    ap.add_argument("--eta", type=float, default=0.0, help="DDIM eta (0 = deterministic)")
    ap.add_argument("--video-sampler", default="ddpm", choices=["ddpm", "ddim"])
    ap.add_argument("--video-steps", default=None, help="num_sampling_steps of the video head")
    ap.add_argument("--compare", action="store_true", help="default policy against the flags', alternating")
    ap.add_argument("--video-clips", type=int, default=0, help="--compare: also time video generation on K clips")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.compare:
        return compare(a, dev)
    pol = build(a.config, dev, sampler_keys(a))
    dal = pol.model.diffactloss

    def timed(fn, iters):
        fn()
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / iters, (time.perf_counter() - t0) * 1e3 / iters

    for B in [int(x) for x in a.batches.split(",")]:
        obs = presets_batch(a.config, B, dev)
        ms_pred, wall_pred = timed(lambda: pol.predict_action(obs), a.iters)
        z = torch.randn(B, 1024, pol.model.decoder_embed.weight.shape[0], device=dev)
        dal._sampler = None
        ms_samp, _ = timed(lambda: dal.sample(z, 0.95), a.iters)
        dal._sampler.use_graph = False
        dal._sampler._cache = None
        ms_eager, _ = timed(lambda: dal.sample(z, 0.95), max(2, a.iters // 2))
        dal._sampler = None
        print(json.dumps({"what": "predict_action", "config": a.config, "batch": B, "ms": round(ms_pred, 3),
                          "wall_ms": round(wall_pred, 3), "actions_per_s": round(B * 16 / ms_pred * 1e3, 1),
                          "sampler_graph_ms": round(ms_samp, 3), "sampler_eager_ms": round(ms_eager, 3),
                          "steps": dal.act_diff_testing_steps, "act_sampler": dal.act_sampler,
                          "eta": dal.act_ddim_eta}), flush=True)


def presets_batch(config, B, dev):
    from unified_video_action_amd import presets
    return presets.synthetic_batch(config, B, dev, seed=B)["obs"]


if __name__ == "__main__":
    main()
