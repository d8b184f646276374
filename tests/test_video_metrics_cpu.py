"""The frame-wise video metrics without a GPU: the float64 restatement (tests/video_metrics_ref.py) against closed
forms and an independent scipy path, the planted defects it must see on the GPU test's own inputs, the host-side
queries of the library, eval/video_metrics.aggregate and the Python-side refusals of ops.frame_metrics."""
import math

import numpy as np
import pytest
import torch

import video_metrics_ref as R
from unified_video_action_amd.eval import video_metrics as VM
from unified_video_action_amd.native import ops


def test_window_is_the_one_the_op_passes_to_the_kernel():
    g = R.window()
    assert g.dtype == np.float64 and g.shape == (11,) and np.array_equal(g, ops.ssim_window())
    assert abs(g.sum() - 1.0) <= 4 * R.U and np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - math.exp(-1.0 / 4.5)) <= 1e-15


def test_host_queries_answer_without_a_device():
    th, tw = ops.frame_metrics_tile()
    assert th >= 1 and tw >= 1
    n = ops.frame_metrics_workspace_bytes(2, 4, 256, 256)
    assert n > 0 and n % 8 == 0
    assert ops.frame_metrics_workspace_bytes(1, 1, 11, 11) > 0
    for bad in ((1, 1, 10, 11), (1, 1, 11, 10), (0, 1, 11, 11), (1, 0, 11, 11), (-1, 1, 11, 11)):
        with pytest.raises(ValueError):
            ops.frame_metrics_workspace_bytes(*bad)


@pytest.mark.parametrize("shape", R.fixed_shapes() + R.tile_shapes(16, 16)[-1:])
def test_identical_frames_are_exact(shape):
    a, _ = R.make_pair("noise", shape)
    sse, ssim_sum, bound = R.frame_metrics(a, a.copy())
    H, W = shape[2], shape[3]
    assert (sse == 0).all() and (ssim_sum == 3.0 * (H - 10) * (W - 10)).all()


@pytest.mark.parametrize("p,q", [(0, 0), (0, 255), (255, 254), (17, 200), (128, 129)])
def test_constant_frames_match_the_closed_form(p, q):
    shape = (1, 2, 14, 19)
    a, b = np.full(shape + (3,), p, np.uint8), np.full(shape + (3,), q, np.uint8)
    idx = R.index_map(np.moveaxis(a, 4, 2), np.moveaxis(b, 4, 2))
    want = (2.0 * p * q + R.C1) / (p * p + q * q + R.C1)
    # not "a few ulp" of the closed form: saa, sab, sbb are the rounding residue of moments up to 65025 (<= 67 u
    # 65025 each, the restatement's docstring) beside C2 = 58.5, a relative 3e-11 at most; the luminance factor
    # itself is within a few ulp.  (0, 255) is 917 ulp off, 1.2e-13 relative
    assert float(np.abs(idx - want).max()) <= (8 * R.U + 4 * 67 * R.U * 65025 / R.C2) * want
    sse, ssim_sum, _ = R.frame_metrics(a, b)
    assert (sse == 3 * 14 * 19 * (p - q) ** 2).all()
    if p != q:
        want_psnr = 20.0 * math.log10(255.0 / abs(p - q))
        assert float(np.abs(R.psnr(sse, 3 * 14 * 19) - want_psnr).max()) <= 1e-12
    else:
        assert np.isinf(R.psnr(sse, 3 * 14 * 19)).all()


@pytest.mark.parametrize("regime", R.REGIMES)
def test_restatement_agrees_with_scipy_convolve2d(regime):
    from scipy.signal import convolve2d
    shape = (1, 2, 23, 31)
    a, b = R.make_pair(regime, shape)
    _, ssim_sum, bound = R.frame_metrics(a, b)
    k2 = np.outer(R.window(), R.window())

    def E(x):
        return convolve2d(x, k2, mode="valid")

    for t in range(2):
        tot = 0.0
        for c in range(3):
            x, y = a[0, t, :, :, c].astype(np.float64), b[0, t, :, :, c].astype(np.float64)
            mx, my = E(x), E(y)
            sxx, syy, sxy = E(x * x) - mx * mx, E(y * y) - my * my, E(x * y) - mx * my
            m = ((2 * mx * my + R.C1) * (2 * sxy + R.C2)) / ((mx * mx + my * my + R.C1) * (sxx + syy + R.C2))
            assert m.shape == (13, 21)
            tot += float(m.sum())
        # the 2-D window is a 121-term sum per moment instead of 22: allow (121 + 22) / 44 of the two-sided bound
        assert abs(tot - ssim_sum[0, t]) <= bound[0, t] * (121 + 22) / 44.0, (regime, t, tot, ssim_sum[0, t])


def test_the_bound_stays_below_1e_minus_9_on_the_mean_in_every_regime():
    worst = 0.0
    for regime in R.REGIMES:
        for shape in R.fixed_shapes() + R.tile_shapes(16, 16):
            a, b = R.make_pair(regime, shape)
            _, _, bound = R.frame_metrics(a, b)   # asserts the limit itself
            worst = max(worst, float((bound / (3.0 * (shape[2] - 10) * (shape[3] - 10))).max()))
    print(f"largest bound on a frame's mean SSIM {worst:.2e}")
    assert worst <= R.MEAN_BOUND_LIMIT


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_planted_defect_falls_outside_the_bound_on_the_gpu_tests_inputs(defect):
    """every control must be seen -- ssim_sum outside the counted bound, or another sse -- by the GPU test's own
    small inputs (every regime on every fixed and tile-edge shape), else those inputs could not see such a kernel"""
    seen, total = 0, 0
    for regime in R.REGIMES:
        for shape in R.fixed_shapes() + R.tile_shapes(16, 16):
            if defect in ("drop_last_row", "drop_last_col") and (shape[2] == 11 or shape[3] == 11):
                continue   # one row / column of windows: the control leaves nothing to sum
            a, b = R.make_pair(regime, shape)
            sse, ssim_sum, bound = R.frame_metrics(a, b)
            dsse, dsum, _ = R.frame_metrics(a, b, defect=defect)
            total += 1
            seen += int(bool((np.abs(dsum - ssim_sum) > bound).any()) or not np.array_equal(dsse, sse))
    print(f"{defect}: seen by {seen} of {total} inputs")
    assert seen >= 1
    # the data-independent controls must show on every input with noise in it
    if defect not in ("luma", "channel_2_as_1", "same_padding"):
        a, b = R.make_pair("noise", (2, 3, 12, 27))
        _, ssim_sum, bound = R.frame_metrics(a, b)
        assert (np.abs(R.frame_metrics(a, b, defect=defect)[1] - ssim_sum) > bound).all()


def test_aggregate_means_and_the_perfect_frame_rule():
    H, W = 12, 15
    sse = torch.tensor([[0, 10, 40], [5, 0, 90]], dtype=torch.int64)
    ssim = torch.tensor([[1.0, 0.9, 0.5], [0.95, 1.0, 0.25]], dtype=torch.float64)
    psnr = VM.psnr_from_sse(sse, 3 * H * W)
    assert torch.isinf(psnr[0, 0]) and torch.isinf(psnr[1, 1]) and torch.isfinite(psnr[0, 1])
    agg = VM.aggregate({"psnr": psnr, "ssim": ssim, "n_values": 3 * H * W})
    cap = 10.0 * math.log10(255.0 ** 2 * 3 * H * W)
    assert VM.psnr_cap(3 * H * W) == cap
    want = R.psnr(np.maximum(sse.numpy(), 1), 3 * H * W)
    assert want[0, 0] == pytest.approx(cap, abs=1e-12) and (want[sse.numpy() > 0] < cap).all()
    assert agg["psnr"] == pytest.approx(want.mean(), abs=1e-12) and math.isfinite(agg["psnr"])
    assert agg["psnr_t"] == pytest.approx(want.mean(axis=0).tolist(), abs=1e-12)
    assert agg["ssim"] == pytest.approx(float(ssim.mean()), abs=1e-15)
    assert agg["ssim_t"] == pytest.approx(ssim.mean(dim=0).tolist(), abs=1e-15)
    ref = R.aggregate(sse.numpy(), ssim.numpy() * 3.0 * (H - 10) * (W - 10), H, W)
    assert ref["psnr"] == pytest.approx(agg["psnr"], abs=1e-12) and ref["ssim_t"] == pytest.approx(agg["ssim_t"], abs=1e-15)
    # the per-frame values keep their inf, and a cap without the frame size is refused, not guessed
    with pytest.raises(ValueError):
        VM.aggregate({"psnr": psnr, "ssim": ssim})
    log = VM.log_entries(agg, "ema_")
    assert set(log) == {"ema_video_psnr", "ema_video_ssim"} | {f"ema_video_{k}/t{t}" for k in ("psnr", "ssim")
                                                               for t in (1, 2, 3)}
    assert log["ema_video_psnr/t3"] == agg["psnr_t"][2]


def test_python_side_refusals():
    a = torch.zeros(1, 2, 12, 12, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8"):
        ops.frame_metrics(a.float(), a.float())
    with pytest.raises(ValueError, match="uint8"):
        ops.frame_metrics(a, a.to(torch.int8))
    with pytest.raises(ValueError, match="differ in shape"):
        ops.frame_metrics(a, torch.zeros(1, 2, 12, 13, 3, dtype=torch.uint8))
    with pytest.raises(ValueError, match="channels"):
        ops.frame_metrics(torch.zeros(1, 2, 12, 12, 4, dtype=torch.uint8), torch.zeros(1, 2, 12, 12, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="channels"):
        ops.frame_metrics(a, a, channels=1)            # dimension 1 holds T = 2
    with pytest.raises(ValueError, match="5-D"):
        ops.frame_metrics(a[0], a[0])
    with pytest.raises(ValueError, match="11 x 11"):
        ops.frame_metrics(a[:, :, :10], a[:, :, :10])
    with pytest.raises(ValueError, match="no CPU path"):   # valid host tensors: refused, never computed on the host
        ops.frame_metrics(a, a)
