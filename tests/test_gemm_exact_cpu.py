"""Controls of the per-element GEMM comparisons (tests/gemm_ref.py), no GPU: each comparison of
test_gemm_exact_gpu.py is fed a "kernel output" that the float64 reference computed under one deliberate
defect, stored the way a kernel stores it.  Every defect must be rejected, the unperturbed reference accepted.

The case: batch 2 of (130, 136, 72) with the whole epilogue at once -- alpha 1/2, bias, dropout 1/2, gate
out of a [M, 3N] buffer, residual with ldr = N + 8, beta -1/2 on C0 -- under link 1 (integer operands; bf16
and fp32 outputs, bit equality) and link 2 (randn operands, (K + 8) u S + 2^-8 |ref|); the activation defects
under link 3 (gelu forward with aux, gelu backward with dropout).

Defects: the last k term dropped; the last 8-chunk dropped in one 64 x 64 corner only; one split slice
(k 24..47) dropped; a bf16 store by truncation; round-half-away instead of nearest-even; a double rounding
through bf16 before the residual is added; alpha applied to the bias; beta ignored; bias shifted by one
column; gate / residual read with ld = N; the dropout index taken with ldc; without the batch base; the
dropout scale applied to the dropped lanes (v * scale where 0 belongs, kept lanes right); the keep mask
inverted; aux stored after the activation; act' evaluated on the
output instead of the pre-activation.

Link 2 cannot see the two tie-only defects on randn data (no output is an exact rounding tie: round-half-away
gives the same bits; the double rounding moves an output by at most 2^-9 of the pre-residual value, inside
2^-8 |ref| wherever the residual does not cancel it) -- link 1 is what holds those, on every element.

Also here: float32 restatements of erf_fast / gelu_erf / gelu_erf_grad / sigmoid_fast / silu / silu_grad
inside link 3's counted bounds over the whole pre-activation grid; assert_exact_regime; the magnitude and tie
shares of the generated inputs at every (K, alpha) the GPU file asserts them for."""
import numpy as np
import pytest
import torch

import gemm_ref as R
from gemm_ref import BF16, F32, GELU, SILU

Z, M, N, K = 2, 130, 136, 72
LDX = N + 8
SEED = 0x5EED1234ABCD
ALPHA, BETA = 0.5, -0.5
GRID = 0.125

DATA = ["last_k_dropped", "last_chunk_corner", "split_slice_dropped", "alpha_on_bias", "beta_ignored",
        "bias_shifted", "gate_ld_n", "residual_ld_n", "drop_index_ldc", "drop_no_batch_base", "drop_scale_on_dropped",
        "drop_mask_inverted"]
ROUNDING = ["bf16_truncation", "round_half_away", "double_rounding"]


def misread(x, ld):
    """x [.., M, N] as stored in rows of ld > N (junk 3 in the padding) and read with ld = N"""
    phys = torch.full(x.shape[:-1] + (ld,), 3.0, dtype=x.dtype)
    phys[..., :N] = x
    flat = phys.reshape(x.shape[:-2] + (-1,))
    return flat[..., :M * N].reshape(x.shape)


def store_trunc(v):
    """fp32 -> bf16 by dropping the low 16 bits"""
    bits = v.float().contiguous().view(torch.int32) & -65536
    return bits.view(F32).to(BF16)


def store_half_away(v):
    """fp32 -> bf16 rounding half away from zero (add half an ulp to the magnitude bits, truncate)"""
    bits = v.float().contiguous().view(torch.int32)
    return ((bits + 0x8000) & -65536).view(F32).to(BF16)


def make_case(link, seed):
    g = R.gen(seed)
    if link == 2:
        a, b = R.randn_operands(seed, Z, M, N, K)
    else:
        a, b = R.exact_operands(seed, Z, M, N, K, R.amp_for(K, ALPHA))
    thresh, scale = R.drop_half()
    return dict(a=a, b=b, bias=R.ints(g, 64, (N,), zero=True), gate=R.gate_values(g, (M, N)),
                res=R.ints(g, 64, (Z, M, N), zero=True), c0=R.ints(g, 64, (Z, M, N), zero=True),
                drop=(SEED, thresh, scale))


def output(c, dtype, defect=None):
    """the stored output of the whole-epilogue case under one defect (None: the clean kernel)"""
    a, b, bias, gate, res, c0 = c["a"], c["b"], c["bias"], c["gate"], c["res"], c["c0"]
    seed, thresh, scale = c["drop"]
    P = a @ b.transpose(1, 2)
    if defect == "last_k_dropped":
        P = P - a[..., -1:] @ b[..., -1:].transpose(1, 2)
    if defect == "last_chunk_corner":
        P = P.clone()
        P[:, 64:128, 64:128] -= a[:, 64:128, -8:] @ b[:, 64:128, -8:].transpose(1, 2)
    if defect == "split_slice_dropped":
        P = P - a[..., 24:48] @ b[..., 24:48].transpose(1, 2)
    if defect == "bias_shifted":
        bias = torch.roll(bias, 1)
    v = ALPHA * (P + bias) if defect == "alpha_on_bias" else ALPHA * P + bias
    keep = R.keep_mask(seed, Z, M, N, thresh, with_base=defect != "drop_no_batch_base",
                       ld=LDX if defect == "drop_index_ldc" else None)
    if defect == "drop_mask_inverted":
        keep = ~keep
    # drop_scale_on_dropped: the kept lanes are right, the dropped ones hold v * scale instead of 0
    v = v * scale if defect == "drop_scale_on_dropped" else torch.where(keep, v * scale, torch.zeros_like(v))
    v = v * (misread(gate, 3 * N) if defect == "gate_ld_n" else gate)
    if defect == "double_rounding":
        v = R.store(v, BF16)
    v = v + (misread(res, LDX) if defect == "residual_ld_n" else res)
    if defect != "beta_ignored":
        v = v + BETA * c0
    if defect == "bf16_truncation":
        return store_trunc(v)
    if defect == "round_half_away":
        return store_half_away(v)
    return v.float().to(dtype)


def reference(c, dtype):
    return R.gemm_ref(c["a"], c["b"], dtype, alpha=ALPHA, bias=c["bias"], drop=c["drop"], gate=c["gate"],
                      residual=c["res"], beta=BETA, c0=c["c0"])


@pytest.fixture(scope="module")
def link1():
    c = make_case(1, 11)
    r = reference(c, BF16)
    R.assert_exact_regime(r.S, r.out, GRID)
    assert R.bf16_shares(r.out)[2] >= 1   # exact rounding ties among the outputs
    return c, r


@pytest.fixture(scope="module")
def link2():
    c = make_case(2, 12)
    return c, reference(c, BF16)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_link1_accepts_the_reference(link1, dtype):
    c, r = link1
    R.assert_bit_equal(output(c, dtype), r.out)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("defect", DATA)
def test_link1_rejects_data_defects(link1, defect, dtype):
    c, r = link1
    with pytest.raises(AssertionError):
        R.assert_bit_equal(output(c, dtype, defect), r.out)


@pytest.mark.parametrize("defect", ROUNDING)
def test_link1_rejects_rounding_defects(link1, defect):
    c, r = link1
    with pytest.raises(AssertionError):
        R.assert_bit_equal(output(c, BF16, defect), r.out)


def test_link1_rejects_nan(link1):
    c, r = link1
    got = output(c, F32)
    got[1, 77, 5] = float("nan")
    with pytest.raises(AssertionError):
        R.assert_bit_equal(got, r.out)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_link2_accepts_the_reference(link2, dtype):
    c, r = link2
    R.assert_link2(output(c, dtype), r.out, r.S, K)


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
@pytest.mark.parametrize("defect", DATA)
def test_link2_rejects_data_defects(link2, defect, dtype):
    c, r = link2
    with pytest.raises(AssertionError):
        R.assert_link2(output(c, dtype, defect), r.out, r.S, K)


def test_link2_rejects_truncation_and_nan(link2):
    c, r = link2
    with pytest.raises(AssertionError):
        R.assert_link2(output(c, BF16, "bf16_truncation"), r.out, r.S, K)
    got = output(c, BF16)
    got[0, 3, 9] = float("nan")
    with pytest.raises(AssertionError):
        R.assert_link2(got, r.out, r.S, K)


def test_link2_is_blind_to_tie_defects(link2):
    """the record of why link 1 exists: on randn data round-half-away passes link 2"""
    c, r = link2
    R.assert_link2(output(c, BF16, "round_half_away"), r.out, r.S, K)
    assert R.bf16_shares(r.out)[2] == 0


# ---------------------------------------------------------------- link 3
@pytest.fixture(scope="module")
def link3():
    amp, alpha = R.act_scaling(K)
    a, b = R.exact_operands(13, Z, M, N, K, amp)
    g = R.gen(14)
    bias = R.ints(g, 2, (N,), zero=True)
    pre_saved = R.ints(g, 32, (Z, M, N), zero=True) / 8
    thresh, scale = R.drop_half()
    P, Pabs = R.product(a, b)
    return dict(P=P, Pabs=Pabs, alpha=alpha, bias=bias, pre_saved=pre_saved, drop=(SEED, thresh, scale))


@pytest.mark.parametrize("kind", [GELU, SILU])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_link3_forward(link3, kind, dtype):
    """clean accepted; aux stored after the activation and the last k term dropped rejected"""
    c = link3
    r = R.epilogue_ref(c["P"], c["Pabs"], dtype, alpha=c["alpha"], bias=c["bias"], act=kind)
    R.assert_act_grid(r.pre)
    bound = R.link3_fwd_bound(kind, r, 1.0, dtype)
    R.assert_within(r.out.float().to(dtype), r.out, bound, "clean")
    R.assert_bit_equal(r.pre.float().to(dtype), r.pre, "clean aux")
    with pytest.raises(AssertionError):
        R.assert_bit_equal(R.act64(kind, r.pre).float().to(dtype), r.pre, "aux after the activation")
    bad = R.act64(kind, r.pre - c["alpha"])   # one k term of magnitude 1: the pre-activation moves by alpha
    with pytest.raises(AssertionError):
        R.assert_within(bad.float().to(dtype), r.out, bound, "k term dropped")


@pytest.mark.parametrize("kind", [GELU, SILU])
@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_link3_backward(link3, kind, dtype):
    """clean accepted; act' evaluated on act(pre) instead of pre, and the inverted keep mask, rejected"""
    c = link3
    r = R.epilogue_ref(c["P"], c["Pabs"], dtype, alpha=c["alpha"], drop=c["drop"], residual=c["pre_saved"],
                       act=16 + kind)
    bound = R.link3_bwd_bound(kind, r, c["pre_saved"], dtype)
    R.assert_within(r.out.float().to(dtype), r.out, bound, "clean")
    bad = r.v * R.act_grad64(kind, R.act64(kind, c["pre_saved"]))
    with pytest.raises(AssertionError):
        R.assert_within(bad.float().to(dtype), r.out, bound, "act' on the output")
    inv = R.epilogue_ref(c["P"], c["Pabs"], dtype, alpha=c["alpha"], drop=c["drop"], residual=c["pre_saved"],
                         act=16 + kind, keep=~r.keep)
    with pytest.raises(AssertionError):
        R.assert_within(inv.out.float().to(dtype), r.out, bound, "mask inverted")


def test_link3_counts_hold_for_the_float32_restatements():
    """each float32 restatement of common.h's functions stays inside its counted bound against float64 over
    the whole pre-activation grid (multiples of 1/128 in [-32, 32])"""
    x = torch.arange(-int(R.XMAX * R.XGRID), int(R.XMAX * R.XGRID) + 1, dtype=torch.float64) / R.XGRID
    R.assert_act_grid(x)
    xn = x.numpy()
    for name, f32, kind, grad in (("gelu", R.gelu32, GELU, False), ("gelu'", R.gelu_grad32, GELU, True),
                                  ("silu", R.silu32, SILU, False), ("silu'", R.silu_grad32, SILU, True)):
        got = torch.from_numpy(f32(xn).astype(np.float64))
        ref = R.act_grad64(kind, x) if grad else R.act64(kind, x)
        bound = R.act_bound(kind, x, grad)
        ratio = ((got - ref).abs() / bound.clamp_min(1e-300))[bound > 0]
        print(f"{name}: worst |f32 - f64| / bound = {float(ratio.max()):.3f}")
        R.assert_within(got, ref, bound, name)
    erf = torch.from_numpy(R.erf_fast32(xn).astype(np.float64))
    R.assert_within(erf, torch.erf(x), R.ERF_ABS + R.U * R._erf_terms(x), "erf_fast")


# ---------------------------------------------------------------- input conditions
def test_drop_half_is_exact():
    assert R.dropmask.drop_params(0.5) == (32768, 2.0)
    assert R.drop_half() == (32768, 2.0)


def test_exact_regime_check():
    a, b = R.exact_operands(1, 1, 8, 8, 16, 4)
    r = R.gemm_ref(a, b, F32, alpha=0.5)
    R.assert_exact_regime(r.S, r.out, 0.5)
    with pytest.raises(AssertionError):   # half-integers are off the integer grid
        R.assert_exact_regime(r.S, r.out + 0.25, 0.5)
    with pytest.raises(AssertionError):   # partial sums past 2^24 grid units
        R.assert_exact_regime(r.S * 2.0 ** 20, r.out, 0.5)
    assert not (a == 0).any() and not (b == 0).any()


@pytest.mark.parametrize("Mx,Nx,Kx,alpha", [(65, 67, 2, 1.0), (65, 67, 17, 1.0), (65, 67, 33, 1.0), (65, 67, 17, 0.5),
                                            (130, 136, 72, 1.0), (264, 72, 200, 1.0), (70, 12, 8200, 1.0),
                                            (300, 200, 512, -2.0), (1000, 776, 384, 1.0)])
def test_generated_inputs_have_the_bf16_shares(Mx, Nx, Kx, alpha):
    """amp_for's operands and an integer bias at the GPU file's (K, alpha): >= 75 % of the outputs below 256,
    >= 0.2 % at or above it, exact rounding ties among them; all in the exact regime.  (At amp 1 every
    product is +-1 and the sum has K's parity: the bias is what brings odd outputs, hence ties, at K 8200.)"""
    amp = R.amp_for(Kx, alpha)
    a, b = R.exact_operands(5, 1, Mx, Nx, Kx, amp)
    assert float(a.abs().max()) <= amp and float(a.abs().min()) >= 1 and torch.equal(a, a.round())
    r = R.gemm_ref(a, b, BF16, alpha=alpha, bias=R.ints(R.gen(6), 64, (Nx,), zero=True))
    R.assert_exact_regime(r.S, r.out, 0.5 if alpha == 0.5 else 1.0)
    R.assert_bf16_shares(r.out)


def test_old_rule_passes_what_link1_rejects(link1):
    """the max-norm rule of the existing GEMM tests (1e-2 for bf16) on the same outputs: truncation, half-away
    and the double rounding pass it"""
    c, r = link1
    ref = r.out
    for defect in ("bf16_truncation", "round_half_away", "double_rounding"):
        assert R.old_rule(output(c, BF16, defect), ref) < 1e-2, defect


@pytest.mark.parametrize("Mx,Nx,Kx", [(65, 67, 17), (130, 136, 72), (70, 12, 8200)])
def test_scaled_inputs_have_the_restated_shares(Mx, Nx, Kx):
    """with the dropout scale 2 and a gate of 1/2, 1 or 2 the 256 mark moves with the factor: of the kept
    outputs more than half are bf16 numbers, >= 0.1 % need rounding, exact ties among them; a reference with
    no tie (every kept output made even) is turned down"""
    a, b = R.exact_operands(7, 1, Mx, Nx, Kx, R.amp_for(Kx))
    g = R.gen(8)
    thresh, scale = R.drop_half()
    r = R.gemm_ref(a, b, BF16, bias=R.ints(g, 64, (Nx,), zero=True), drop=(SEED, thresh, scale),
                   gate=R.gate_values(g, (Mx, Nx)))
    R.assert_exact_regime(r.S, r.out, 0.5)
    R.assert_bf16_shares_scaled(r.out, "output", r.keep)
    with pytest.raises(AssertionError):
        R.assert_bf16_shares_scaled(torch.round(r.out / 8) * 8, "output", r.keep)
