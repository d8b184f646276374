"""Frame-wise fidelity of predicted video against the ground-truth future: PSNR and SSIM per clip and per
prediction horizon, from the HIP kernel's per-frame sums (native.ops.frame_metrics; no weights needed).

    mse  = sse / (3 H W)                       sse: the exact integer sum of (pred - real)^2 of the frame
    psnr = 10 log10(255^2 / mse)               +inf for an identical frame
    ssim = ssim_sum / (3 (H - 10)(W - 10))     the mean SSIM index (Wang et al. 2004: 11 x 11 gaussian window of
                                               sigma 1.5, valid positions only, per channel, data range 255)
"""
import math

import torch

from ..native import ops


def psnr_from_sse(sse, n_values):
    """10 log10(255^2 n_values / sse) in float64, +inf where sse == 0.  sse: an integer (or float64) tensor"""
    sse = sse.double()
    return 10.0 * torch.log10((255.0 ** 2 * float(n_values)) / sse)


def psnr_ssim(pred, real, channels=-1):
    """pred, real: uint8 CUDA videos of one shape, [n, T, H, W, 3] or with the channels in dimension `channels`
    (any strides).  -> {"psnr", "ssim", "mse"}: float64 host tensors [n, T]; also "sse" (int64 [n, T]) and
    "n_values" (3 H W, for aggregate's PSNR cap)."""
    sse, ssim_sum = ops.frame_metrics(pred, real, channels=channels)
    shape = list(pred.shape)
    shape.pop(channels % 5)
    H, W = shape[2], shape[3]
    sse, ssim_sum = sse.cpu(), ssim_sum.cpu()
    return {"psnr": psnr_from_sse(sse, 3 * H * W), "ssim": ssim_sum / float(3 * (H - 10) * (W - 10)),
            "mse": sse.double() / float(3 * H * W), "sse": sse, "n_values": 3 * H * W}


def psnr_cap(n_values):
    """the PSNR of sse = 1 over n_values uint8 values: the largest finite PSNR two such frames can have"""
    return 10.0 * math.log10(255.0 ** 2 * float(n_values))


def aggregate(m, n_values=None):
    """m: the dict of psnr_ssim (or any {"psnr", "ssim"} of [n, T] float64 tensors).
    -> {"psnr": mean over all frames, "ssim": the same, "psnr_t": [T] means per horizon, "ssim_t": [T]} as
    python floats.  In these means ONLY, a frame with sse == 0 (psnr = +inf) counts at the PSNR of sse == 1, the
    smallest non-zero error two uint8 frames can have (psnr_cap), so that one perfect frame cannot turn a logged
    mean into inf; the per-frame values of psnr_ssim keep their +inf.  n_values: 3 H W of a frame, m["n_values"]
    when absent (needed only if a frame is perfect)."""
    psnr, ssim = m["psnr"].double(), m["ssim"].double()
    perfect = torch.isinf(psnr) & (psnr > 0)
    if bool(perfect.any()):
        n_values = m.get("n_values") if n_values is None else n_values
        if n_values is None:
            raise ValueError("aggregate: a perfect frame needs n_values = 3 H W for the PSNR cap")
        psnr = torch.where(perfect, torch.full_like(psnr, psnr_cap(n_values)), psnr)
    return {"psnr": float(psnr.mean()), "ssim": float(ssim.mean()),
            "psnr_t": [float(v) for v in psnr.mean(dim=0)], "ssim_t": [float(v) for v in ssim.mean(dim=0)]}


def log_entries(agg, name_label=""):
    """the aggregate as log keys: video_psnr, video_ssim, video_psnr/t1 .. /t{h}, video_ssim/t1 .. /t{h}"""
    out = {f"{name_label}video_psnr": agg["psnr"], f"{name_label}video_ssim": agg["ssim"]}
    for t, (p, s) in enumerate(zip(agg["psnr_t"], agg["ssim_t"]), start=1):
        out[f"{name_label}video_psnr/t{t}"] = p
        out[f"{name_label}video_ssim/t{t}"] = s
    return out
