"""CLIP text tower (utils/language_model.ClipTextTower, csrc/text_tower.hip) at the Libero step's shape,
B 32 prompts of L 30 tokens: the whole tower in bf16 and in fp32 precision, and its four own kernels at the
shapes the tower launches them with.  HIP events around windows of ITERS back-to-back calls (one call is
too short to time), warm-up first, the median window of REPS; tools only.

    python tools/clip_text_bench.py [out.json]

Prints one JSON row per measurement: ms per call (median, min, max over the windows).  The tower's share of
the Libero step is this time over the step time `bench.py --full` reports for libero10_joint at B 32."""
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from unified_video_action_amd.native import ops  # noqa: E402
from unified_video_action_amd.runtime import RT  # noqa: E402
from unified_video_action_amd.utils.language_model import ClipTextTower  # noqa: E402

DEV = "cuda"
B, L, H, D, DH = 32, 30, 8, 512, 2048
ITERS, REPS = 50, 9


def window_ms(fn, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(ITERS):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / ITERS)
    return {"ms": round(statistics.median(ts), 5), "min_ms": round(min(ts), 5), "max_ms": round(max(ts), 5)}


def main(out_path=None):
    assert torch.cuda.is_available(), "needs the GPU"
    torch.manual_seed(0)
    tower = ClipTextTower().to(DEV)
    ids = torch.randint(1, 49000, (B, L), device=DEV)
    mask = torch.zeros(B, L, dtype=torch.int64, device=DEV)
    for b in range(B):
        n = 6 + b % 20
        ids[b, n - 1:] = 49407
        mask[b, :n] = 1
    rows = [{"device": torch.cuda.get_device_name(0), "B": B, "L": L, "iters_per_window": ITERS, "windows": REPS}]
    for prec in ("bf16", "fp32"):
        RT.set_precision(prec)
        rows.append(dict(what=f"tower {prec}", **window_ms(lambda: tower(ids, mask))))
    RT.set_precision("bf16")
    M = B * L
    for dtype, name in ((torch.bfloat16, "bf16"), (torch.float32, "fp32")):
        qkv = torch.randn(M, 3 * D, device=DEV).to(dtype)
        o = torch.empty(M, D, device=DEV, dtype=dtype)
        rows.append(dict(what=f"clip_attn {name}", **window_ms(lambda: ops.clip_attn(qkv, mask, o, B, L, H))))
        a = torch.randn(M, DH, device=DEV).to(dtype)
        g = torch.empty_like(a)
        rows.append(dict(what=f"quick_gelu {name}", **window_ms(lambda: ops.quick_gelu(a, g))))
    tok = tower.text_model.embeddings.token_embedding.weight
    pos = tower.text_model.embeddings.position_embedding.weight
    x = torch.empty(M, D, device=DEV)
    pooled = torch.empty(B, D, device=DEV)
    rows.append(dict(what="clip_embed", **window_ms(lambda: ops.clip_embed(ids, tok, pos, x))))
    rows.append(dict(what="clip_pool", **window_ms(lambda: ops.clip_pool(ids, x, pooled))))
    for r in rows:
        print(json.dumps(r), flush=True)
    if out_path:
        with open(out_path, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else None)
