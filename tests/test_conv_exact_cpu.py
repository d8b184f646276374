"""Controls of the per-element conv comparisons (tests/conv_ref.py), no GPU: the comparison functions
of test_conv_exact_gpu.py are fed a "kernel output" that the float64 reference computed under one
deliberate defect, stored the way a kernel stores it (rounded once to bf16), at (2, 16, 16, 64 -> 128),
3x3, GroupNorm prologue, bias and residual.  Every defect must be rejected by link 1 (exact data, bit
equality) and by link 2 (SiLU data, 2^-8 |ref| + (9 Ci + 8) u S); the unperturbed reference must pass.

Defects: two neighbouring channels' scales swapped in one image; one tap dropped on the last output
column only; the padding filled with act(shift) instead of zero; the residual added after a first bf16
rounding (rounded twice); the bias shifted by one channel; for the fused GroupNorm partial sums, one
pixel counted twice.

The same defects on the data and under the rule of test_conv_halo_gpu.py, max|got - ref| < 1e-2 max|ref| on
randn data against an fp32 F.conv2d (test_old_rule_control; (2, 16, 16, 128 -> 128) with SiLU, seed 0, run
on the CPU; 65536 outputs, max|ref| 6.7, so the old threshold is 0.067 absolute against a median per-element
bound of 0.0050).  Max-norm figure, elements at or over the old threshold, elements over the new bound:
    clean reference            2.3e-3      0      0
    residual rounded twice     4.5e-3      0   2903   <- passes the old rule
    one channel of one tap     7.5e-2   1999  35114
    scales swapped             8.0e-2  11267  30311
    tap dropped, last column   2.2e-1   3217   3792
    padding = act(shift)       1.4e-1  10438  15064
    bias shifted by one        6.7e-2  40046  62700
With randn scales, shifts and biases of the sizes those tests draw, the old rule does reject the gross forms
of five of the six, on the tail of the moved elements; it lets the double rounding through outright, and any
defect that moves an output by less than 0.067 -- 13 times the median of what the per-element bound
allows, and unbounded relative to a small output.  It never looks at the raw partial sums: a pixel counted
twice moves an image's sum of squares by about 1 / HW, so the scale by about half of that: its 1e-4
finalize comparison sees this at HW 256 (2e-3) and barely at HW 4096 (1.2e-4); the raw comparison's bound is
(T + 8) u = 3.1e-5 of the image's sum at Co 128, 8x below the defect at HW 4096, the largest map these
tests use.
"""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R
from conv_ref import BF16, SAME3

N, H, W, CI, CO, KS = 2, 16, 16, 64, 128, 3
K = KS * KS * CI
DEFECTS = ["scales_swapped", "tap_dropped", "pad_act_shift", "residual_rounded_twice", "bias_shifted"]


def stored(out):
    """what a kernel leaves in a bf16 output: the fp32 value rounded once, to nearest even"""
    return out.float().to(BF16)


def defective(case, silu, defect):
    """the reference's output (float64, before the store) under one defect; None = unperturbed"""
    x, w, bias, res = case["x"], case["w"], case["bias"], case["res"]
    scale, shift = case["scale"], case["shift"]
    if defect == "scales_swapped":
        scale = scale.clone()
        scale[1, [10, 11]] = scale[1, [11, 10]]
    if defect == "bias_shifted":
        bias = torch.roll(bias, 1)
    a = R.activate(x, scale, shift, silu, BF16)
    ap = R.zero_pad(a, SAME3)
    if defect == "pad_act_shift":
        fill = R.activate(torch.zeros(N, 1, 1, CI), scale, shift, silu, BF16)
        ap = fill.expand(N, H + 2, W + 2, CI).clone()
        ap[:, 1:H + 1, 1:W + 1] = a
    out = R.conv_taps(ap, w.double(), KS, 1)
    if defect == "tap_dropped":   # tap (0, 1) missing at the last output column
        t = (R.tap_slice(ap, 0, 1, 1, H, W) @ w.double()[:, 0, 1, :].t()).view(N, H, W, CO)
        out[:, :, W - 1] -= t[:, :, W - 1]
    out = out + bias.double()
    if defect == "residual_rounded_twice":
        return stored(out).double() + res.double()
    return out + res.double()


@pytest.fixture(scope="module")
def link1():
    case = R.exact_case(11, N, H, W, CI, CO, KS, H, W, gn=True, residual=True)
    ref, S, a = R.conv_ref(case["x"], case["w"], KS, 1, SAME3, case["bias"], case["res"], case["scale"],
                           case["shift"], silu=False, store=BF16)
    R.assert_exact_regime(a, S)
    return case, ref, S


@pytest.fixture(scope="module")
def link2():
    case = R.silu_case(12, N, H, W, CI, CO, KS, H, W, residual=True)
    R.assert_silu_regime(case["x"], case["scale"], case["shift"])
    ref, S, _ = R.conv_ref(case["x"], case["w"], KS, 1, SAME3, case["bias"], case["res"], case["scale"],
                           case["shift"], silu=True, store=BF16)
    return case, ref, S


def test_silu_grid_exclusions():
    """of the 65 quarter-grid values only -5.25 and -4.5 come within 2^-14 of a bf16 tie; the rest clear it
    by >= 6.1e-5 relative, ~30x the error of an exp2 / rcp SiLU at |z| <= 8"""
    excl, margin = R.silu_excluded()
    assert excl.tolist() == [-5.25, -4.5]
    assert margin >= 6.1e-5


def test_case_grids():
    """the generated inputs sit on the grids the exactness argument needs"""
    c = R.exact_case(3, 3, 16, 16, 64, 128, 3, 16, 16, gn=True, residual=True)
    assert float(c["x"].double().abs().max()) <= 8 and torch.equal(c["x"].double(), c["x"].double().round())
    assert set(c["scale"].unique().tolist()) <= {0.5, 1.0, 2.0, 4.0}
    assert (c["scale"][:, 1:] != c["scale"][:, :-1]).all() and (c["scale"][1:] != c["scale"][:-1]).all()
    assert torch.equal(c["w"].double() * 16, (c["w"].double() * 16).round()) and float(c["w"].double().abs().max()) <= 3 / 16
    assert torch.equal(c["bias"] * 16, (c["bias"] * 16).round()) and float(c["bias"].abs().max()) <= 4
    s = R.silu_case(3, 3, 16, 16, 64, 128, 3, 16, 16)
    assert set(s["scale"].unique().tolist()) <= {0.25, 0.5, 1.0}
    assert (s["scale"][:, 1:] != s["scale"][:, :-1]).all() and (s["scale"][1:] != s["scale"][:-1]).all()
    R.assert_silu_regime(s["x"], s["scale"], s["shift"])
    c8 = R.exact_case(4, 1, 16, 16, 8, 128, 3, 16, 16, ci_used=3)
    assert not c8["x"][..., 3:].any() and not c8["w"][..., 3:].any() and c8["x"][..., :3].any()


def test_link1_accepts_the_reference(link1):
    case, ref, S = link1
    R.assert_bit_equal(stored(defective(case, False, None)), ref)
    R.assert_bit_equal(defective(case, False, None).float(), ref)   # an fp32 output


@pytest.mark.parametrize("defect", DEFECTS)
def test_link1_rejects(link1, defect):
    case, ref, S = link1
    with pytest.raises(AssertionError, match="elements differ"):
        R.assert_bit_equal(stored(defective(case, False, defect)), ref, defect)


def test_link1_rejects_an_unwritten_element(link1):
    case, ref, S = link1
    got = stored(ref)
    got.view(-1)[77] = float("nan")
    with pytest.raises(AssertionError, match="1 of"):
        R.assert_bit_equal(got, ref)


def test_link2_accepts_the_reference(link2):
    case, ref, S = link2
    R.assert_silu_close(stored(defective(case, True, None)), ref, S, K)


@pytest.mark.parametrize("defect", DEFECTS)
def test_link2_rejects(link2, defect):
    case, ref, S = link2
    with pytest.raises(AssertionError, match="out of bound"):
        R.assert_silu_close(stored(defective(case, True, defect)), ref, S, K, defect)


def test_link2_bound_is_tighter_than_the_old_rule(link2):
    """median bound against what 1e-2 of the tensor's maximum allows on the same data"""
    case, ref, S = link2
    b = R.silu_bound(ref, S, K)
    assert float(b.median()) * 5 < 1e-2 * float(ref.abs().max())


@pytest.mark.parametrize("link", [1, 2])
def test_partials_accept_and_reject(link1, link2, link):
    case, ref, S = link1 if link == 1 else link2
    out = stored(ref)
    part = R.tile_partials(out, CO)
    R.assert_partials(part, out, N, CO)
    # one pixel counted twice: pixel 37 of image 1 enters its tile's sums a second time
    o = out.double().reshape(N, H * W, 32, CO // 32)[1, 37]
    twice = part.clone().view(N, -1, 32, 2)
    twice[1, 0, :, 0] += o.sum(dim=1).float()
    twice[1, 0, :, 1] += (o * o).sum(dim=1).float()
    with pytest.raises(AssertionError, match="out of bound"):
        R.assert_partials(twice.view_as(part), out, N, CO)
    # a tile's pair written to the neighbouring group's slot
    moved = part.clone()
    moved[3, [4, 5]] = moved[3, [5, 4]]
    with pytest.raises(AssertionError, match="out of bound"):
        R.assert_partials(moved, out, N, CO)


def test_old_rule_control():
    """the record in this module's docstring: the same defects on the data and under the rule of
    test_conv_halo_gpu.py (randn, w ~ 0.05 randn, an fp32 F.conv2d on the bf16-rounded activated input,
    max|got - ref| < 1e-2 max|ref|), next to the per-element bound of link 2 against the float64 reference
    on that same data (its activated input is the reference's own, so the bound holds there too)"""
    g = torch.Generator().manual_seed(0)
    n, Hh, Ww, Ci, Co = 2, 16, 16, 128, 128
    x = torch.randn(n, Hh, Ww, Ci, generator=g).to(BF16)
    w = (torch.randn(Co, 3, 3, Ci, generator=g) * 0.05).to(BF16)
    bias = torch.randn(Co, generator=g) * 0.1
    sc = torch.rand(n, Ci, generator=g) + 0.5
    sh = torch.randn(n, Ci, generator=g) * 0.3
    res = torch.randn(n, Hh, Ww, Co, generator=g).to(BF16)

    def run(defect):
        s, b = sc, bias
        if defect == "scales_swapped":
            s = sc.clone()
            s[1, [10, 11]] = s[1, [11, 10]]
        if defect == "bias_shifted":
            b = bias.view(-1, 4)[:, [3, 0, 1, 2]].reshape(-1)
        a = R.activate(x, s, sh, True, BF16)
        ap = R.zero_pad(a, SAME3)
        if defect == "pad_act_shift":
            fill = R.activate(torch.zeros(n, 1, 1, Ci), s, sh, True, BF16)
            ap = fill.expand(n, Hh + 2, Ww + 2, Ci).clone()
            ap[:, 1:Hh + 1, 1:Ww + 1] = a
        out = R.conv_taps(ap, w.double(), 3, 1)
        if defect == "tap_dropped":
            t = (R.tap_slice(ap, 0, 1, 1, Hh, Ww) @ w.double()[:, 0, 1, :].t()).view(n, Hh, Ww, Co)
            out[:, :, Ww - 1] -= t[:, :, Ww - 1]
        if defect == "tap_one_channel":   # input channel 5 of tap (0, 1) missing, everywhere
            out -= (R.tap_slice(ap, 0, 1, 1, Hh, Ww)[:, 5:6] @ w.double()[:, 0, 1, 5:6].t()).view(n, Hh, Ww, Co)
        out = out + b.double()
        if defect == "residual_rounded_twice":
            return stored(stored(out).double() + res.double())
        return stored(out + res.double())

    a32 = F.silu(x.float() * sc[:, None, None, :] + sh[:, None, None, :]).to(BF16).float()
    ref32 = F.conv2d(a32.permute(0, 3, 1, 2), w.float().permute(0, 3, 1, 2), bias, padding=1).permute(0, 2, 3, 1)
    ref32 = ref32 + res.float()
    ref, S, _ = R.conv_ref(x, w, 3, 1, SAME3, bias, res, sc, sh, silu=True, store=BF16)
    bound = R.silu_bound(ref, S, 9 * Ci)
    thr = 1e-2 * float(ref32.abs().max())
    rec = {}
    for d in [None, "tap_one_channel"] + DEFECTS:
        got = run(d).double()
        rec[d] = (R.old_rule(got, ref32), int(((got - ref32.double()).abs() >= thr).sum()),
                  int(((got - ref).abs() > bound).sum()))
    print({k: (f"{v[0]:.2e}", v[1], v[2]) for k, v in rec.items()}, f"of {ref.numel()}; median bound "
          f"{float(bound.median()):.3g}, old threshold {thr:.3g}")
    assert rec[None][0] < 1e-2 and rec[None][2] == 0
    assert rec["residual_rounded_twice"][0] < 1e-2 < 100 * rec["residual_rounded_twice"][2]   # let through / caught
    for d in ["tap_one_channel"] + DEFECTS:   # the per-element bound flags every element the old threshold does
        assert rec[d][2] > 0 and rec[d][2] >= rec[d][1], (d, rec[d])
