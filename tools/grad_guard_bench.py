"""Cost of the gradient norm / clipping / non-finite guard (csrc/optim.hip), tools only.

    python tools/grad_guard_bench.py kernels [out.json]   the norm pass and guarded vs plain AdamW at mar_base's size
    python tools/grad_guard_bench.py step [out.json]      the training step with the guard on and off

kernels: uva_grad_sumsq + uva_grad_guard over a 1.04 GB fp32 buffer (N elements, 10 ranges at odd offsets in 5
slots), HIP events around each call, WARM warm calls, the median of REPS; GB/s against the 6.3 TB/s achievable
HBM rate.  Then uva_adamw_ema (fused EMA + bf16 shadow) against uva_adamw_ema_guarded on the same buffers,
alternating between the two call by call.
step: bench.py's step body (pusht_video, mar_base, B 32, bf16) in ONE process, alternating blocks of BLOCK steps
with max_grad_norm + skip_nonfinite + the five part norms on and with the guard off; HIP events around every
step, the median per leg.
Prints one JSON row per measurement."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unified_video_action_amd.native import ops  # noqa: E402

DEV = "cuda"
N = 260_000_000
HBM_ACHIEVABLE_GBS = 6300.0
WARM, REPS = 5, 30
BLOCK, ROUNDS = 5, 5


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


def kernels():
    rows = [{"device": torch.cuda.get_device_name(0), "elements": N, "warm": WARM, "reps": REPS}]
    g = torch.randn(N, device=DEV)
    step = N // 10
    ranges = [(i * step + (1 if i else 0), step - 1, i % 5) for i in range(10)]
    work = torch.empty(ops.grad_norm_workspace_bytes(N, len(ranges)) // 8, dtype=torch.float64, device=DEV)
    sums = torch.zeros(5, dtype=torch.float64, device=DEV)
    rec = torch.zeros(9, device=DEV)
    table = ops.range_table(ranges)

    def norm_pass():
        ops.grad_sumsq(g, ranges, 5, sums, work, table=table)
        ops.grad_guard(sums, 5, 1.0, 1.0, True, rec)

    for _ in range(WARM):
        norm_pass()
    ts = [_ms(norm_pass) for _ in range(REPS)]
    nbytes = 4 * sum(k for _, k, _ in ranges)
    gbs = nbytes / (statistics.median(ts) * 1e-3) / 1e9
    rows.append(_row("grad_sumsq + grad_guard", ts, gb_per_s=round(gbs, 1),
                     of_achievable_hbm=round(gbs / HBM_ACHIEVABLE_GBS, 3), record=[round(x, 4) for x in rec.tolist()]))

    p, m, v, ema = (torch.randn(N, device=DEV) * 0.02 for _ in range(4))
    v.abs_()
    shadow = torch.empty(N, device=DEV, dtype=torch.bfloat16)
    rec.copy_(torch.tensor([1.0, 0.5, 0.0, 0.0] + [0.0] * 5))
    args = (p, g, m, v, ema, shadow, N, 1e-4, 0.9, 0.95, 1e-8, 0.02, 10, 1.0, 0.999)
    legs = {"adamw_ema": lambda: ops.adamw_ema(*args), "adamw_ema_guarded": lambda: ops.adamw_ema_guarded(*args, rec)}
    for fn in legs.values():
        for _ in range(WARM):
            fn()
    ts = {k: [] for k in legs}
    for _ in range(REPS):
        for k, fn in legs.items():  # alternating: drift hits both alike
            ts[k].append(_ms(fn))
    for k in legs:
        rows.append(_row(k, ts[k], gb_per_s=round(38.0 * N / (statistics.median(ts[k]) * 1e-3) / 1e9, 1)))
    rec.copy_(torch.tensor([float("nan"), float("nan"), 1.0, 0.0] + [0.0] * 5))
    fn = legs["adamw_ema_guarded"]
    for _ in range(WARM):
        fn()
    rows.append(_row("adamw_ema_guarded, skipped step (EMA only)", [_ms(fn) for _ in range(REPS)]))
    return rows


def step():
    import bench
    from unified_video_action_amd import presets
    pol, opt, sched, ema = bench.build("pusht_video", "bf16", torch.device(DEV))
    batch = presets.synthetic_batch("pusht_video", 32, DEV, seed=5)
    m = pol.model
    parts = {"encoder": [m.encoder_blocks], "decoder": [m.decoder_blocks],
             "video_head": [getattr(m, "diffloss", None), getattr(m, "diffloss_wrist", None)],
             "action_head": [getattr(m, "diffactloss", None), getattr(m, "diffproploss", None)]}
    legs = {"guard off": lambda: opt.set_grad_guard(),
            "guard on": lambda: opt.set_grad_guard(max_grad_norm=1.0, skip_nonfinite=True, grad_norm_parts=parts)}
    rows = [{"device": torch.cuda.get_device_name(0), "config": "pusht_video", "batch": 32, "block": BLOCK,
             "rounds": ROUNDS, "flat_elements": opt.store.total}]
    for setup in legs.values():
        setup()
        for _ in range(WARM):
            bench.step(pol, opt, sched, ema, batch)
    torch.cuda.synchronize()
    ts = {k: [] for k in legs}
    for _ in range(ROUNDS):
        for k, setup in legs.items():
            setup()
            bench.step(pol, opt, sched, ema, batch)  # the first step after a switch is not timed
            evs = []
            for _ in range(BLOCK):
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                bench.step(pol, opt, sched, ema, batch)
                e.record()
                evs.append((s, e))
            torch.cuda.synchronize()
            ts[k] += [s.elapsed_time(e) for s, e in evs]
    for k in legs:
        rows.append(_row(f"step, {k}", ts[k]))
    rows.append({"last_grad_stats": {k: round(v, 5) for k, v in opt.grad_stats().items()},
                 "skipped_steps": opt.skipped_steps, "step_count": opt.step_count})
    return rows


def main(argv):
    assert torch.cuda.is_available(), "needs the GPU"
    what = argv[1] if len(argv) > 1 else "kernels"
    rows = {"kernels": kernels, "step": step}[what]()
    for r in rows:
        print(json.dumps(r), flush=True)
    if len(argv) > 2:
        with open(argv[2], "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main(sys.argv)
