"""Attention at head_dim 128 / 80 (B 32, N 1024, p = 0.1): the fused kernels of csrc/attention_hd.hip against
the materialised fp32 route (functional._attn_mat_fwd / _attn_mat_bwd, unchanged: what every head_dim other than
64 ran before), forward and forward + backward, in one process with the two routes alternating per round; the
head_dim-64 kernels at B 32, N 1024, H 12 from the same run; and torch.cuda.max_memory_allocated of one Block
forward + backward on both routes.  HIP events around every launch sequence, warm-up launches first, the median
of the repeats.  tools only.

    python tools/attn_hd_bench.py [out.json]

Per shape: ms per layer (forward; forward + backward), the fused route's fraction of the dense bf16 peak
(4 B H N^2 hd FLOP forward, 12 B H N^2 hd forward + backward, the counts of native/ops.py, over 2.5 PFLOP/s), the
time of the keep-mask planes (uva_attn_dropmask; one launch per Block and step, generated ahead on the side stream
in training) and the Block's peak memory."""
import json
import statistics
import sys
from functools import partial

import torch

sys.path.insert(0, ".")
from unified_video_action_amd.model.autoregressive import functional as Fn  # noqa: E402
from unified_video_action_amd.native import ops  # noqa: E402
from unified_video_action_amd.runtime import RT  # noqa: E402

PEAK_BF16_TFLOPS = 2500.0  # MI355X dense bf16 MFMA (bench.py)
DEV = "cuda"
P = 0.1
SHAPES = [(32, 1024, 6, 128), (32, 1024, 16, 80)]
HD64 = (32, 1024, 12, 64)


def median_ms(fn, warm=3, reps=15):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e))
    return statistics.median(ts), min(ts), max(ts)


def fused(B, N, H, hd):
    """-> (fwd, fwd + bwd, mask) closures of the fused route: the planes are made once (as in a training step,
    where they are prefetched) and timed on their own"""
    qkv = torch.randn(B * N, 3 * H * hd, device=DEV).to(torch.bfloat16)
    do = torch.randn(B * N, H * hd, device=DEV).to(torch.bfloat16)
    o = torch.empty(B * N, H * hd, device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(B, H, N, device=DEV)
    dvec = torch.empty(B, H, N, device=DEV)
    dqkv = torch.empty_like(qkv)
    db = torch.zeros(3 * H * hd, device=DEV)
    mask = ops.attn_dropmask(B, N, H, P, 1234, DEV)
    scale = hd ** -0.5
    if hd == 64:
        f = lambda: ops.attn_fwd(qkv, o, lse, B, N, H, scale, P, 1234, mask=mask)  # noqa: E731
        b = lambda: ops.attn_bwd(qkv, o, do, lse, dvec, dqkv, B, N, H, scale, P, 1234, mask=mask,  # noqa: E731
                                 dbias=db)
    else:
        f = lambda: ops.attn_fwd_hd(qkv, o, lse, B, N, H, hd, scale, P, 1234, mask=mask)  # noqa: E731
        b = lambda: ops.attn_bwd_hd(qkv, o, do, lse, dvec, dqkv, B, N, H, hd, scale, P, 1234, mask=mask,  # noqa: E731
                                    dbias=db)
    return f, lambda: (f(), b()), lambda: ops.attn_dropmask(B, N, H, P, 1234, DEV, out=mask)


def materialised(B, N, H, hd):
    """-> (fwd, fwd + bwd) closures of the materialised route exactly as BlockFn runs it (casts included)"""
    D = H * hd
    qkv = torch.randn(B * N, 3 * D, device=DEV).to(torch.bfloat16)
    do = torch.randn(B * N, D, device=DEV).to(torch.bfloat16)
    scale = hd ** -0.5
    db = torch.zeros(3 * D, device=DEV)

    def f():
        o, Pm, Pd = Fn._attn_mat_fwd(qkv, B, N, H, scale, P, 1234)
        return Fn.as_dtype(o, torch.bfloat16), Pm, Pd

    def fb():
        _, Pm, Pd = f()
        dqkv = Fn.as_dtype(Fn._attn_mat_bwd(qkv, Pm, Pd, do, B, N, H, scale, P, 1234), torch.bfloat16)
        ops.colsum(dqkv, db)
    return f, fb


def block_peak(B, N, H, hd, flash):
    """max_memory_allocated (MiB above the resident parameters and input) of one train() Block forward + backward"""
    import torch.nn as nn
    from unified_video_action_amd.model.autoregressive.mar_con_unified import Block
    D = H * hd
    RT.flash_attention = flash
    try:
        blk = Block(D, H, 4.0, qkv_bias=True, norm_layer=partial(nn.LayerNorm, eps=1e-6), proj_drop=P,
                    attn_drop=P).to(DEV).train()
        x = torch.randn(B, N, D, device=DEV, requires_grad=True)
        g = torch.randn(B, N, D, device=DEV)
        for _ in range(2):  # the first pass allocates the persistent workspaces and weight shadows
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            RT.begin_forward()
            Fn.block_forward(blk, x, B, N, P, P).backward(g)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            x.grad = None
        return peak / 2 ** 20
    finally:
        RT.flash_attention = True


def main(out_path=None, rounds=3):
    assert torch.cuda.is_available(), "needs the GPU"
    RT.set_precision("bf16")
    res = {"device": torch.cuda.get_device_name(0), "p": P, "rounds": rounds, "shapes": []}
    for B, N, H, hd in SHAPES + [HD64]:
        row = {"B": B, "N": N, "H": H, "hd": hd}
        ff, ffb, fm = fused(B, N, H, hd)
        mat = materialised(B, N, H, hd) if hd != 64 else None
        acc = {k: [] for k in ("fused_fwd", "fused_fwdbwd", "mask", "mat_fwd", "mat_fwdbwd")}
        for _ in range(rounds):  # the two routes alternate: drift of the box hits both
            acc["fused_fwd"].append(median_ms(ff)[0])
            if mat:
                acc["mat_fwd"].append(median_ms(mat[0], warm=2, reps=7)[0])
            acc["fused_fwdbwd"].append(median_ms(ffb)[0])
            if mat:
                acc["mat_fwdbwd"].append(median_ms(mat[1], warm=2, reps=7)[0])
            acc["mask"].append(median_ms(fm)[0])
        for k, v in acc.items():
            if v:
                row[k + "_ms"] = round(statistics.median(v), 4)
                row[k + "_ms_rounds"] = [round(t, 4) for t in v]
        fl = 4.0 * B * H * N * N * hd
        row["fused_fwd_frac_peak"] = round(fl / (row["fused_fwd_ms"] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)
        row["fused_fwdbwd_frac_peak"] = round(3 * fl / (row["fused_fwdbwd_ms"] * 1e-3) / 1e12 / PEAK_BF16_TFLOPS, 4)
        del ff, ffb, fm, mat
        torch.cuda.empty_cache()
        if hd != 64:
            row["block_peak_MiB_fused"] = round(block_peak(B, N, H, hd, True), 1)
            row["block_peak_MiB_materialised"] = round(block_peak(B, N, H, hd, False), 1)
            torch.cuda.empty_cache()
        print(json.dumps(row), flush=True)
        res["shapes"].append(row)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
