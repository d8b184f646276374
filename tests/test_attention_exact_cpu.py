"""The comparisons of tests/attn_ref.py held to their own controls, without a GPU:
  * the backward formulas (with O_used = out) against float64 autograd, 1e-12 relative;
  * the bf16 kernels' rounding points emulated in float64 stay inside every per-element bound at the inputs of
    every GPU case (the worst error / bound is printed);
  * the reference under another seed's mask, and with the last key tile left out of the sums, falls outside;
  * the fp8 restatement in float32 against float64 stays at or below a quarter of the flip cap;
  * the fp8 restatement under another seed's mask, with the keys of every tile permuted on the V side (i <-> 63 - i), and with
    exact (unrounded) P, each put at least 30 % of the elements outside the tight bound."""
import functools

import pytest
import torch

import attn_ref as R

IDS = [R.case_id(c) for c in R.BF16_CASES]
FP8_IDS = [R.case_id(c) for c in R.FP8_CASES]
DROP_CASES = [c for c in R.BF16_CASES if c[3] > 0]
TAIL_CASES = [c for c in R.BF16_CASES if c[2] > 64]  # more than one key tile


@pytest.mark.parametrize("hd,H,N,p", [(64, 3, 128, 0.0), (64, 3, 128, 0.1), (80, 2, 64, 0.1), (128, 1, 192, 0.5)])
def test_backward_formulas_are_autograd(hd, H, N, p):
    B = 2
    qkv, dout = R.make_inputs(B, H, N, hd, 11 + hd)
    q, k, v = (t.requires_grad_(True) for t in R.heads(qkv, H, hd))
    do = R.rows(dout, H, hd)
    keep, ds = R.keep_scale(R.SEED, B, H, N, p)
    P = torch.softmax((q @ k.transpose(-1, -2)) * hd ** -0.5, dim=-1)
    out = (P if keep is None else P * keep * ds) @ v
    out.backward(do)
    r = R.reference(qkv, dout, H, hd, R.SEED, p, o_used=out.detach())
    assert (r["out"] - out.detach()).abs().max().item() <= 1e-12 * out.abs().max().item()
    for name, t in (("dq", q), ("dk", k), ("dv", v)):
        err = (r[name] - t.grad).abs().max().item()
        assert err <= 1e-12 * t.grad.abs().max().item(), (name, err)


@functools.lru_cache(maxsize=None)
def _ref(case):
    B, H, N, p, spread = case
    qkv, dout = R.bf16_case_inputs(*case)
    return qkv, dout, R.reference(qkv, dout, H, 64, R.SEED, p)


@pytest.mark.parametrize("case", R.BF16_CASES, ids=IDS)
def test_bf16_rounding_emulation_is_inside_every_bound(case):
    B, H, N, p, spread = case
    _, _, r = _ref(case)
    keep, ds = R.keep_scale(R.SEED, B, H, N, p)
    e = R.emulate_bf16(r, keep, ds)
    for name, bound in (("out", "B_O"), ("dq", "B_dq"), ("dk", "B_dk"), ("dv", "B_dv")):
        worst, share = R.ratio(e[name], r[name], r[bound])
        print(f"{name}: worst error / bound {worst:.3f}")
        assert share == 0.0 and worst <= 1.0, (name, worst, share)


@pytest.mark.parametrize("case", DROP_CASES, ids=[R.case_id(c) for c in DROP_CASES])
def test_wrong_seed_is_rejected(case):
    B, H, N, p, spread = case
    qkv, dout, r = _ref(case)
    w = R.reference(qkv, dout, H, 64, R.OTHER_SEED, p)
    for name, bound in (("out", "B_O"), ("dq", "B_dq"), ("dk", "B_dk"), ("dv", "B_dv")):
        _, share = R.ratio(w[name], r[name], r[bound])
        print(f"{name}: share outside under another seed's mask {share:.3f}")
        assert share >= 0.3, (name, share)


@pytest.mark.parametrize("case", TAIL_CASES, ids=[R.case_id(c) for c in TAIL_CASES])
def test_dropped_last_key_tile_is_rejected(case):
    B, H, N, p, spread = case
    qkv, dout, r = _ref(case)
    w = R.reference(qkv, dout, H, 64, R.SEED, p, last_tile=False)
    for name, bound in (("out", "B_O"), ("dq", "B_dq"), ("dk", "B_dk"), ("dv", "B_dv")):
        _, share = R.ratio(w[name], r[name], r[bound])
        print(f"{name}: share outside without the last key tile {share:.3f}")
        assert share >= 0.3, (name, share)
    assert (w["lse2"] - r["lse2"]).abs().max().item() > R.lse_bound(r["lse2"])


def test_ramp_and_spike_take_their_steps():
    for hd in (64, 80, 128):
        R.assert_ramp_steps(R.ramp_inputs(hd, 2), 2, hd)
        t = R.tile_maxima_log2(R.spiked_inputs(hd, 2), 2, hd)
        rise = t[..., 6] - t[..., :6].amax(-1)
        assert rise.min().item() > 8.0, rise.min().item()  # the lazy rescale fires in every row
    # the ramp after the fp8 pass (constant keys stay constant vectors on the e4m3 grid)
    x = R.ramp_inputs(64, 2).reshape(1, 512, 3, 2, 64)
    xr, _, _ = R.fp8_round(x)
    R.assert_ramp_steps(xr, 2, 64)


@functools.lru_cache(maxsize=None)
def _fp8(case):
    N, p, peak = case
    _, xr, _, _, _ = R.fp8_case_inputs(*case)
    keep, ds = R.keep_scale(R.SEED, R.FP8_B, R.FP8_H, N, p)
    return xr, R.fp8_forward(xr, R.FP8_H, 0.125, keep, ds)


@pytest.mark.parametrize("case", R.FP8_CASES, ids=FP8_IDS)
def test_fp8_restatement_float32_control(case):
    """the same restatement in float32 (scores, exp2, sums) against float64: what an exp2 or a sum that differs in
    its last bits moves across e4m3 boundaries stays at or below a quarter of the cap"""
    N, p, peak = case
    xr, f = _fp8(case)
    keep, ds = R.keep_scale(R.SEED, R.FP8_B, R.FP8_H, N, p)
    g = R.fp8_forward(xr, R.FP8_H, 0.125, keep, ds, dtype=torch.float32)
    share, worst_in, worst_loose = R.fp8_compare(g["out"], f, N)
    print(f"float32 restatement: outside tight {share:.5f}, worst err/tight inside {worst_in:.2e}, "
          f"worst err/(tight + step) {worst_loose:.3f}")
    assert share <= R.FLIP_CAP / 4 and worst_loose <= 1.0
    assert (g["lse2"] - f["lse2"]).abs().max().item() < R.lse_bound(f["lse2"])


@pytest.mark.parametrize("case", R.FP8_CASES, ids=FP8_IDS)
def test_fp8_mutations_are_rejected(case):
    """the V-side mutation is a key permutation of every tile (i <-> 63 - i), as a v8_pos error gives: it moves
    every key, so it reaches the rows that a few keys carry (the peaked case) as well"""
    N, p, peak = case
    xr, f = _fp8(case)
    keep, ds = R.keep_scale(R.SEED, R.FP8_B, R.FP8_H, N, p)
    muts = {"V keys i and 63 - i of every tile exchanged": R.fp8_forward(xr, R.FP8_H, 0.125, keep, ds, reverse_v=True),
            "exact P": R.fp8_forward(xr, R.FP8_H, 0.125, keep, ds, exact_p=True)}
    if p > 0:
        k2, _ = R.keep_scale(R.OTHER_SEED, R.FP8_B, R.FP8_H, N, p)
        muts["another seed's mask"] = R.fp8_forward(xr, R.FP8_H, 0.125, k2, ds)
    for name, g in muts.items():
        share, _, _ = R.fp8_compare(g["out"], f, N)
        print(f"{name}: outside tight {share:.3f}")
        assert share >= 0.3, (name, share)


def test_fp8_round_is_the_definition():
    """fp8_round on a hand-made tensor: all-zero tile (e = 0), amax exactly 448 (e = 0, codes = values), the next
    bf16 above 448 (e = 1), a bf16 denormal amax (e = -126)"""
    x = torch.zeros(1, 256, 3, 1, 64, dtype=torch.bfloat16)
    x[0, 64:128, 0, 0, :] = 448.0
    x[0, 128:192, 0, 0, 3] = 450.0
    x[0, 128:192, 0, 0, 4] = 3.0
    tiny = torch.tensor([0x0040], dtype=torch.int16).view(torch.bfloat16)  # 2^-127
    x[0, 192:, 0, 0, 9] = tiny
    xr, e, code = R.fp8_round(x)
    assert e[0, :, 0, 0].tolist() == [0, 0, 1, -126]
    assert torch.equal(xr[0, 64:128, 0], x[0, 64:128, 0]) and code[0, 64, 0, 0, 0] == 448
    assert xr[0, 128, 0, 0, 3] == 448.0 and code[0, 128, 0, 0, 3] == 224  # 450 / 2 = 225 -> 224 (step 16)
    assert xr[0, 128, 0, 0, 4] == 3.0
    assert torch.equal(xr[0, 192:, 0], x[0, 192:, 0]) and code[0, 192, 0, 0, 9] == 0.5
