"""uva_frame_metrics on the GPU against the float64 restatement (tests/video_metrics_ref.py): sse equal, ssim_sum
inside the counted fp64 bound, on shapes at the edges of the kernel's tile, in every data regime, through every
layout the evaluation holds, inside guarded outputs and workspace, relaunched, and refused."""
import ctypes

import numpy as np
import pytest
import torch

import video_metrics_ref as R
from unified_video_action_amd.native import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = ops.frame_metrics_tile()   # pure host
WORST = {"ratio": 0.0, "mean_err": 0.0}
_REF = {}


def _case(regime, shape):
    """(a, b, restatement) of one input, computed once and shared (never modified)"""
    key = (regime, shape)
    if key not in _REF:
        a, b = R.make_pair(regime, shape)
        _REF[key] = (a, b, R.frame_metrics(a, b, tile=TILE))
    return _REF[key]


def _check(sse, ssim_sum, a, b, ref):
    ratio, mean_err = R.compare(sse.cpu().numpy(), ssim_sum.cpu().numpy(), a, b, tile=TILE, ref=ref)
    WORST["ratio"], WORST["mean_err"] = max(WORST["ratio"], ratio), max(WORST["mean_err"], mean_err)


def _dev(v):
    return torch.from_numpy(v).to(DEV)


def _inside(v, fill, seed=0):
    """the values of v [N, T, H, W, 3] as an interior view of a larger buffer filled with `fill` (255 or random)"""
    N, T, H, W, C = v.shape
    shape = (N + 1, T + 2, H + 3, W + 5, C + 1)
    if fill == "random":
        g = torch.Generator().manual_seed(seed)
        big = torch.randint(0, 256, shape, generator=g, dtype=torch.uint8).to(DEV)
    else:
        big = torch.full(shape, fill, dtype=torch.uint8, device=DEV)
    view = big[1:, 1:T + 1, 2:H + 2, 3:W + 3, 1:]
    view.copy_(v)
    return view


SMALL = R.fixed_shapes() + R.tile_shapes(*TILE)


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("shape", SMALL + [R.EVAL_SHAPE], ids=lambda s: "x".join(map(str, s)))
def test_frame_metrics_against_the_restatement(shape, regime):
    a, b, ref = _case(regime, shape)
    sse, ssim_sum = ops.frame_metrics(_dev(a), _dev(b))
    assert sse.dtype == torch.int64 and ssim_sum.dtype == torch.float64 and tuple(sse.shape) == shape[:2]
    _check(sse, ssim_sum, a, b, ref)


@pytest.mark.parametrize("p,q", [(0, 0), (0, 255), (255, 254), (17, 200), (128, 129)])
def test_constant_frames_match_the_closed_form(p, q):
    th, tw = TILE
    shape = (1, 2, th + 13, tw + 12)
    a = torch.full(shape + (3,), p, dtype=torch.uint8, device=DEV)
    b = torch.full(shape + (3,), q, dtype=torch.uint8, device=DEV)
    sse, ssim_sum = ops.frame_metrics(a, b)
    P = (shape[2] - 10) * (shape[3] - 10)
    want = (2.0 * p * q + R.C1) / (p * p + q * q + R.C1)
    assert (sse.cpu() == 3 * shape[2] * shape[3] * (p - q) ** 2).all()
    # the variances are rounding residue of moments up to 65025 (<= 67 u 65025 each) over C2; the sum adds
    # sum_chain roundings (tests/video_metrics_ref.py)
    tol = 8 * R.U + 4 * 67 * R.U * 65025 / R.C2 + R.sum_chain(shape[2], shape[3], TILE) * R.U
    err = float((ssim_sum.cpu() / (3.0 * P) - want).abs().max())
    print(f"constants {p} / {q}: index {want:.12f}, |mean - closed form| {err:.2e} (allowed {tol * abs(want):.2e})")
    assert err <= tol * abs(want)
    _check(sse, ssim_sum, a.cpu().numpy(), b.cpu().numpy(), None)


@pytest.mark.parametrize("shape", [(2, 3, 12, 27), (1, 2, TILE[0] + 13, 2 * TILE[1] + 11), R.EVAL_SHAPE],
                         ids=lambda s: "x".join(map(str, s)))
def test_identical_values_at_other_addresses_are_exact(shape):
    a, _, _ = _case("noise", shape)
    N, T, H, W = shape
    want = 3.0 * (H - 10) * (W - 10)
    x = _dev(a)
    others = {"copy": x.clone(), "planar": x.permute(0, 4, 1, 2, 3).contiguous().permute(0, 2, 3, 4, 1),
              "interior": _inside(x, "random"), "repeated": x.repeat_interleave(4, dim=1)[:, ::4]}
    for name, y in others.items():
        assert y.data_ptr() != x.data_ptr()
        sse, ssim_sum = ops.frame_metrics(x, y)
        assert bool((sse == 0).all()) and bool((ssim_sum == want).all()), (name, sse, ssim_sum, want)
        sse, ssim_sum = ops.frame_metrics(y, x)
        assert bool((sse == 0).all()) and bool((ssim_sum == want).all()), (name, sse, ssim_sum, want)


@pytest.mark.parametrize("shape", [(2, 3, 12, 27), (2, 2, TILE[0] + 13, TILE[1] + 12)],
                         ids=lambda s: "x".join(map(str, s)))
def test_layouts_give_the_same_bits(shape):
    a, b, ref = _case("near", shape)
    x, y = _dev(a), _dev(b)
    sse0, sum0 = ops.frame_metrics(x, y)
    _check(sse0, sum0, a, b, ref)

    def planar(v):   # the saved grids' layout [n, 3, T, H, W]
        return v.permute(0, 4, 1, 2, 3).contiguous()

    def repeated(v):   # [:, ::4] of the clip the tower sees
        return v.repeat_interleave(4, dim=1).contiguous()[:, ::4]

    runs = {
        "planar, channels=1": ops.frame_metrics(planar(x), planar(y), channels=1),
        "planar as a channels-last view": ops.frame_metrics(planar(x).permute(0, 2, 3, 4, 1), planar(y).permute(0, 2, 3, 4, 1)),
        "[:, ::4] of the repeated clips": ops.frame_metrics(repeated(x), repeated(y)),
        "a planar, b channels-last": ops.frame_metrics(planar(x).permute(0, 2, 3, 4, 1), y),
        "a repeated, b planar": ops.frame_metrics(repeated(x), planar(y).permute(0, 2, 3, 4, 1)),
        "interior of a 255 buffer": ops.frame_metrics(_inside(x, 255), _inside(y, 255)),
        "interior of random buffers": ops.frame_metrics(_inside(x, "random", 1), _inside(y, "random", 2)),
        "a interior, b planar": ops.frame_metrics(_inside(x, "random", 3), planar(y).permute(0, 2, 3, 4, 1)),
    }
    for name, (sse, ssim_sum) in runs.items():
        assert torch.equal(sse, sse0) and torch.equal(ssim_sum, sum0), name
    assert repeated(x).stride(1) == 4 * x.stride(1) and not planar(x).permute(0, 2, 3, 4, 1).is_contiguous()


def _guarded(n_elems, dtype, fill):
    """a buffer of n_elems inside 32-element guards -> (whole, view)"""
    whole = torch.full((n_elems + 64,), fill, dtype=dtype, device=DEV)
    return whole, whole[32:32 + n_elems]


def test_outputs_and_workspace_stay_inside_their_guards():
    shape = (2, 3, TILE[0] + 13, 2 * TILE[1] + 11)
    a, b, ref = _case("noise", shape)
    N, T, H, W = shape
    nan = float("nan")
    sent = -0x0123456789ABCDEF
    wsse, vsse = _guarded(N * T, torch.int64, sent)
    wsum, vsum = _guarded(N * T, torch.float64, nan)
    need = ops.frame_metrics_workspace_bytes(*shape)
    wwork, vwork = _guarded(need // 8, torch.float64, nan)
    sse, ssim_sum = ops.frame_metrics(_dev(a), _dev(b), sse=vsse.view(N, T), ssim_sum=vsum.view(N, T), work=vwork)
    _check(sse, ssim_sum, a, b, ref)
    assert bool((wsse[:32] == sent).all()) and bool((wsse[-32:] == sent).all())
    assert bool(torch.isnan(wsum[:32]).all()) and bool(torch.isnan(wsum[-32:]).all())
    assert bool(torch.isnan(wwork[:32]).all()) and bool(torch.isnan(wwork[-32:]).all())
    assert not bool(torch.isnan(vwork).any())   # every slot of the queried size is written: the query is exact


def test_relaunch_and_a_garbage_workspace_are_bit_equal():
    shape = R.EVAL_SHAPE
    a, b, _ = _case("near", shape)
    x, y = _dev(a), _dev(b)
    need = ops.frame_metrics_workspace_bytes(*shape)
    work = torch.zeros(need // 8, dtype=torch.float64, device=DEV)
    sse0, sum0 = ops.frame_metrics(x, y, work=work)
    sse1, sum1 = ops.frame_metrics(x, y, work=work)
    g = torch.Generator(device=DEV).manual_seed(3)
    junk = torch.randint(-2 ** 62, 2 ** 62, (need // 8,), generator=g, dtype=torch.int64, device=DEV).view(torch.float64)
    sse2, sum2 = ops.frame_metrics(x, y, work=junk)
    assert torch.equal(sse0, sse1) and torch.equal(sum0, sum1) and torch.equal(sse0, sse2) and torch.equal(sum0, sum2)


def _raw(**over):
    """one raw call of the entry point on valid operands with `over` replacing arguments -> the output tensors"""
    from unified_video_action_amd.native.lib import lib
    N, T, H, W = 1, 2, 12, 13
    t = dict(a=torch.zeros(N, T, H, W, 3, dtype=torch.uint8, device=DEV),
             b=torch.full((N, T, H, W, 3), 2, dtype=torch.uint8, device=DEV),
             sse=torch.full((N * T,), -7, dtype=torch.int64, device=DEV),
             ssim_sum=torch.full((N * T,), -7.0, dtype=torch.float64, device=DEV),
             work=torch.full((ops.frame_metrics_workspace_bytes(N, T, H, W) // 8,), -7.0, dtype=torch.float64, device=DEV))
    sa = (ctypes.c_longlong * 5)(*over.pop("strides_a", t["a"].stride()))
    sb = (ctypes.c_longlong * 5)(*over.pop("strides_b", t["b"].stride()))
    g = (ctypes.c_double * 11)(*ops.ssim_window().tolist())
    args = dict(a=t["a"].data_ptr(), stride_a=ctypes.addressof(sa), b=t["b"].data_ptr(), stride_b=ctypes.addressof(sb),
                window=ctypes.addressof(g), N=N, T=T, H=H, W=W, sse=t["sse"].data_ptr(), ssim_sum=t["ssim_sum"].data_ptr(),
                work=t["work"].data_ptr(), work_bytes=t["work"].numel() * 8)
    args.update(over)
    try:
        lib().call("uva_frame_metrics", *args.values(), torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    return t


REFUSED = [dict(H=10), dict(W=10), dict(N=0), dict(T=0), dict(N=-1), dict(a=None), dict(b=None), dict(sse=None),
           dict(ssim_sum=None), dict(work=None), dict(window=None), dict(stride_a=None), dict(work_bytes=8),
           dict(work_bytes=-1), dict(strides_a=(0, 0, -39, 3, 1)), dict(strides_b=(0, 0, 39, 3, -1))]


def test_the_unrefused_call_launches():
    t = _raw()
    assert bool((t["sse"] == 3 * 12 * 13 * 4).all()) and bool((t["ssim_sum"] > 0).all())


@pytest.mark.parametrize("over", REFUSED, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_refusals_leave_everything_untouched(over):
    from unified_video_action_amd.native.lib import lib
    N, T, H, W = 1, 2, 12, 13
    sse = torch.full((N * T,), -7, dtype=torch.int64, device=DEV)
    ssim_sum = torch.full((N * T,), -7.0, dtype=torch.float64, device=DEV)
    work = torch.full((ops.frame_metrics_workspace_bytes(N, T, H, W) // 8,), -7.0, dtype=torch.float64, device=DEV)
    o = dict(over)
    for k, v in (("sse", sse), ("ssim_sum", ssim_sum), ("work", work)):
        o.setdefault(k, v.data_ptr())
    with pytest.raises(RuntimeError, match="hipError 1"):   # hipErrorInvalidValue
        _raw(**o)
    assert bool((sse == -7).all()) and bool((ssim_sum == -7.0).all()) and bool((work == -7.0).all())
    assert lib().query("uva_frame_metrics_workspace_bytes", 1, 2, 10, 13) == -1


def test_op_refuses_outputs_and_workspace_it_cannot_hand_to_the_kernel():
    x = torch.zeros(1, 2, 12, 13, 3, dtype=torch.uint8, device=DEV)
    need = ops.frame_metrics_workspace_bytes(1, 2, 12, 13)
    ok = dict(sse=torch.empty(1, 2, dtype=torch.int64, device=DEV), ssim_sum=torch.empty(1, 2, dtype=torch.float64, device=DEV),
              work=torch.empty(need // 8, dtype=torch.float64, device=DEV))
    ops.frame_metrics(x, x, **ok)
    bad = [dict(sse=ok["sse"].cpu()), dict(ssim_sum=ok["ssim_sum"].cpu()), dict(work=ok["work"].cpu()),
           dict(work=torch.empty(need // 4, dtype=torch.float64, device=DEV)[::2]),      # the bytes, but strided
           dict(work=torch.empty(need // 8 - 1, dtype=torch.float64, device=DEV)),
           dict(sse=torch.empty(1, 4, dtype=torch.int64, device=DEV)[:, ::2])]
    for over in bad:
        with pytest.raises(ValueError):
            ops.frame_metrics(x, x, **dict(ok, **over))


def test_report_worst_error():
    """Reports only: the figures DESIGN §5j records, gathered from the comparisons above through the module-global
    WORST, so it relies on file order.  Run alone (or under -k) it prints zeros and asserts nothing; the bound
    itself is asserted by every comparison (R.compare: ratio <= 1)."""
    print(f"frame_metrics: worst |error| / bound {WORST['ratio']:.3f}, worst |mean ssim error| {WORST['mean_err']:.2e}")
    assert WORST["ratio"] <= 1.0
