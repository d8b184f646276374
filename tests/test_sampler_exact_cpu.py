"""The reference-only conditions and the controls of tests/test_sampler_exact_gpu.py (no GPU): every regime
assertion of tests/sampler_ref.py holds on the cases the GPU tests run, a clean stored reference passes its own
comparison, and a reference computed under one planted defect misses the bound of the case meant to catch it."""
import numpy as np
import pytest
import torch

import sampler_ref as sr
from conv_ref import assert_bit_equal
from edge_helpers import assert_within
from gemm_ref import BF16, F32, F64, U, gen, store

LIN = [(R, N, K, v) for (R, N, K, _) in sr.LINEAR_CASES for v in sr.VARIANTS]
EDGE_CASES = [(224, 512, 256), (225, 512, 256)]   # the LN edge rows ride on these (randn regime)
SHARES = {}


def _edges(R, N, K):
    return (R, N, K) in EDGE_CASES


def _stored(c):
    return store(c.lin.out, c.dtype).to(c.dtype)


def _rejects(fn):
    with pytest.raises(AssertionError):
        fn()


def test_route_query_matches_the_cases():
    from unified_video_action_amd.native import ops
    for R, N, K, route in sr.LINEAR_CASES:
        assert ops.sampler_linear_route(R, N, K) == route, (R, N, K)
    assert ops.sampler_linear_route(224, 512, 1024) == "narrow" and ops.sampler_linear_route(225, 512, 1024) == "wide"
    assert ops.sampler_linear_route(2048, 1024, 1024) == "wide" and ops.sampler_linear_route(2016, 64, 512) == "narrow"
    for bad in ((16, 16, 128), (0, 16, 256), (16, 0, 256)):
        with pytest.raises(ValueError):
            ops.sampler_linear_route(*bad)


@pytest.mark.parametrize("regime", ["int", "randn"])
@pytest.mark.parametrize("R,N,K,variant", LIN)
def test_linear_reference_conditions(R, N, K, variant, regime):
    """the integer regime's assertions / the two randn conditions (<= 2 % ambiguous, mean allowance below the mean
    (K + 8) u S term), and the clean reference passes its own comparison"""
    c = sr.linear_case(regime, variant, R, N, K, edges=_edges(R, N, K))
    r = sr.assert_linear_regime(c)
    if regime == "randn" and c.ln:
        SHARES[(R, N, K, variant)] = r
        print(f"ambiguous {r[0]:.4%} allowance / accumulation {r[1]:.3f}")
    sr.check_linear(_stored(c), c, "clean")


@pytest.mark.parametrize("K", [256, 512, 1024])
def test_enclosure_holds_an_fp32_layernorm(K):
    """a float32 restatement of the A tile (torch's own summation order) lands inside [lo, hi] everywhere, on the
    reference's own value wherever the element is not ambiguous"""
    c = sr.linear_case("randn", "ln_f32", 33, 16, K, edges=True)
    x = c.A.float()
    mean = x.mean(1, keepdim=True)
    d = x - mean
    rstd = torch.rsqrt((d * d).mean(1, keepdim=True) + np.float32(c.eps))
    h = (d * rstd * c.lnw.float() + c.lnb.float()) * (1 + c.scale.float()) + c.shift.float()
    a = h.to(BF16).double()
    assert bool(((a >= c.tile.lo) & (a <= c.tile.hi)).all())
    assert bool((a == c.tile.a)[~c.tile.amb].all())
    assert float((h.double() - c.tile.h).abs().max()) > 0  # the restatement does differ from float64


# ------------------------------------------------------------------ controls: uva_sampler_linear
TILE_CONTROLS = [
    ("trunc_a", "randn", "ln_f32", 16, 16, 512), ("trunc_a", "randn", "ln_silu", 33, 64, 512),
    ("onepass", "randn", "ln_f32", 225, 512, 256), ("var_km1", "randn", "ln_f32", 32, 20, 256),
    ("no_eps", "randn", "ln_f32_noaffine", 224, 512, 256), ("no_lnb", "int", "ln_f32", 16, 16, 512),
    ("no_lnb", "randn", "ln_silu", 31, 17, 1024), ("scale_no1", "int", "ln_f32_noaffine", 1, 1, 256),
    ("swap_mod", "int", "ln_silu", 33, 64, 512), ("swap_mod", "randn", "ln_f32", 16, 65, 1024),
    (("skip", 3), "int", "ln_f32", 16, 16, 512), (("dup", 5), "int", "gate", 31, 17, 1024),
    (("skip", 7), "randn", "plain_silu", 16, 1024, 1024), (("skip", 0), "randn", "ln_f32_noaffine", 32, 20, 256),
    ("gate_stride", "int", "gate", 16, 16, 512), ("gate_stride", "randn", "gate", 33, 64, 512),
]


@pytest.mark.parametrize("defect,regime,variant,R,N,K", TILE_CONTROLS)
def test_linear_control_is_rejected(defect, regime, variant, R, N, K):
    c = sr.linear_case(regime, variant, R, N, K, edges=_edges(R, N, K))
    bad = sr.linear_case(regime, variant, R, N, K, edges=_edges(R, N, K), defect=defect)
    _rejects(lambda: sr.check_linear(_stored(bad), c, str(defect)))


@pytest.mark.parametrize("regime,variant", [("int", "ln_silu"), ("randn", "ln_silu"), ("randn", "plain_silu")])
def test_truncating_store_is_rejected(regime, variant):
    c = sr.linear_case(regime, variant, 16, 16, 512)
    _rejects(lambda: sr.check_linear(sr.trunc_bf16(c.lin.out).to(BF16), c, "truncating store"))


def _guard_image(c, extra_row=False, extra_col=False, ld_pad=5, off=3):
    """a host image of the GPU tests' guarded output: sentinel outside the view, the stored reference inside; the
    planted defects store a row >= R (row 0's values, as an unzeroed tail row would give) or a column >= N"""
    R, N = c.R, c.N
    ld = N + ld_pad
    buf = torch.full((64 + (R + 1) * ld + 64,), 12345.0, dtype=F64)
    img = buf[64:64 + (R + 1) * ld].view(R + 1, ld)
    out = _stored(c).double()
    img[:R, off:off + N] = out
    if extra_row:
        img[R, off:off + N] = out[0]
    if extra_col:
        img[:R, off + N] = out[:, 0]
    inside = torch.zeros_like(buf, dtype=torch.bool)
    inside[64:64 + (R + 1) * ld].view(R + 1, ld)[:R, off:off + N] = True
    return buf, inside


def _check_guard(buf, inside):
    assert bool((buf[~inside] == 12345.0).all()), "write outside the output view"


@pytest.mark.parametrize("R,N,K", [(31, 17, 1024), (33, 64, 512), (993, 65, 512)])
def test_guard_rejects_tail_row_and_column(R, N, K):
    c = sr.linear_case("int", "ln_f32", R, N, K)
    _check_guard(*_guard_image(c))
    _rejects(lambda: _check_guard(*_guard_image(c, extra_row=True)))
    _rejects(lambda: _check_guard(*_guard_image(c, extra_col=True)))


# ------------------------------------------------------------------ p_sample
def _p_sample32(eps_, v, x, noise, k, clip):
    """float32 restatement of p_sample_step_kernel, one rounding per operation"""
    f32 = np.float32
    eps_, v, x, noise = (t.numpy().astype(f32) for t in (eps_, v, x, noise))
    k = [f32(c) for c in k]
    f = (v + f32(1)) / f32(2)
    lv = f * k[5] + (f32(1) - f) * k[4]
    x0 = k[0] * x - k[1] * eps_
    if clip:
        x0 = np.clip(x0, f32(-1), f32(1))
    mean = k[2] * x0 + k[3] * x
    return torch.from_numpy((mean + k[6] * np.exp(f32(0.5) * lv) * noise * k[7]).astype(np.float64))


def p_sample_inputs(rows, C, seed=0):
    g = gen(500 + rows + C + seed)
    out = torch.randn(rows, 2 * C, generator=g).float().double()
    out[:, C:] = out[:, C:].clamp(-1, 1)
    x = (torch.randn(rows, C, generator=g) * 2).float().double()
    noise = torch.randn(rows, C, generator=g).float().double()
    return out, x, noise


@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("nonzero", [1.0, 0.0])
def test_p_sample_bound_holds_fp32_and_rejects_controls(clip, nonzero):
    out, x, noise = p_sample_inputs(257, 10)
    kc = [1.3, 0.7, 0.4, 0.55, -6.0, -3.5, nonzero, 0.95]
    C = 10
    ref, b = sr.p_sample(out[:, :C], out[:, C:], x, noise, kc, clip)
    assert float(b.mean() / ref.abs().mean()) < 16 * U  # a few u
    assert_within(_p_sample32(out[:, :C], out[:, C:], x, noise, kc, clip), ref, b, "fp32 restatement")
    if nonzero:
        bad, _ = sr.p_sample(out[:, :C], out[:, C:], x, noise, kc, clip, defect="f_no1")
        _rejects(lambda: assert_within(bad, ref, b, "f_no1"))
    if clip:
        bad, _ = sr.p_sample(out[:, :C], out[:, C:], x, noise, kc, clip, defect="clip_mean")
        _rejects(lambda: assert_within(bad, ref, b, "clip_mean"))


# ------------------------------------------------------------------ the persistent kernel
@pytest.mark.parametrize("j", range(sr.DEPTH))
def test_live_block_integer_regime_and_controls(j):
    c = sr.ps_case("live", 16, 10, "int", live=j)
    st = sr.ps_reference(c)[0]
    sr.assert_live_regime(c, st)
    hx, ha = sr.live_expected(c, st)
    assert torch.equal(hx, st.hx[sr.DEPTH - 1]) and torch.equal(sr.ps_reference(c)[0].ha[j], ha)
    assert_bit_equal(store(hx, F32).float(), hx, "clean")
    # every block's weights, modulation columns and LN affine are its own: another block's give other rows
    for name in ("w2_prev", "mod_prev", "trunc_fc1"):
        if j == 0 and name != "trunc_fc1":
            continue
        bad = sr.ps_reference(c, defect=(name, j))[0]
        _rejects(lambda: assert_bit_equal(bad.hx[sr.DEPTH - 1].float(), hx, name))
    # the ping-pong side swapped: the observed side holds the block before the last
    _rejects(lambda: assert_bit_equal(st.hx[sr.DEPTH - 2].float(), hx, "pingpong")) if j == sr.DEPTH - 1 else None


def test_tail_rows_of_ha_control():
    """R = 5: rows >= R of the A tile are zero, so ha's tail rows are SiLU(b1) = b1; a tile whose tail rows leak row 0
    gives row 0's fc1 output there"""
    j = sr.DEPTH - 1
    c = sr.ps_case("live", 5, 16, "int", live=j)
    st = sr.ps_reference(c)[0]
    sr.assert_live_regime(c, st)
    tail = store(c.pack["b1"][j], BF16).expand(11, sr.W_PS)
    assert float(c.pack["b1"][j].min()) >= sr.SILU_ID
    _rejects(lambda: assert_bit_equal(st.ha[j][:1].expand(11, sr.W_PS).to(BF16), tail, "leaked row 0"))


def test_x0_integer_regime_has_ties_that_round_up():
    c = sr.ps_case("eps", 16, 10)
    xn = store(c.x0, BF16)
    ulp = torch.exp2(torch.floor(torch.log2(c.x0.abs().clamp_min(1e-30))) - 7)
    assert int(((c.x0 - xn).abs() == ulp / 2).sum()) >= 16 and int((xn.abs() > c.x0.abs()).sum()) >= 16
    # (LayerNorm hides a rescaled h0 from the final layer: the residual stream of a live block shows it)
    c = sr.ps_case("live", 16, 10, "int", live=0)
    st = sr.ps_reference(c)[0]
    bad = sr.ps_reference(c, defect=("trunc_x", 0))[0]
    _rejects(lambda: assert_bit_equal(bad.hx[-1].float(), st.hx[-1], "trunc_x"))


@pytest.mark.parametrize("kind", ["eps", "clip", "var"])
@pytest.mark.parametrize("C", [1, 8, 9, 16])
@pytest.mark.parametrize("R", [1, 5, 16])
def test_final_layer_integer_regime(kind, R, C):
    c = sr.ps_case(kind, R, C)
    st = sr.ps_reference(c)[0]
    sr.assert_tile_regime(st.tiles[-1][0])
    assert torch.equal(st.h0, st.hx[-1]) and bool(sr.exact_sum_rows(st.h0).all())
    assert torch.equal(st.out * 8, torch.round(st.out * 8)) and float(st.out.abs().max()) < 64
    if kind != "var":
        assert torch.equal(st.x, store(st.x, F32))


def test_clip_case_lands_on_both_sides_and_on_the_mark():
    c = sr.ps_case("clip", 16, 16)
    st = sr.ps_reference(c)[0]
    x0 = 0.5 * c.x0 + st.out[:, :16]
    assert int((x0.abs() == 1).sum()) >= 1 and int((x0 > 1).sum()) >= 8 and int((x0 < -1).sum()) >= 8
    assert int((x0.abs() < 1).sum()) >= 8
    bad = sr.ps_reference(c, defect=("clip_mean", 0))[0]
    _rejects(lambda: assert_bit_equal(bad.x.float(), st.x, "clip_mean"))


def test_second_final_tile_and_variance_half_controls():
    c = sr.ps_case("var", 16, 9)
    st = sr.ps_reference(c)[0]
    ref, b = sr.p_sample(st.out[:, :9], st.out[:, 9:], c.x0, c.noise[0], sr.KC_VAR, False)
    assert torch.equal(ref, st.x) and float((b / ref).max()) < 128 * U
    for name in ("drop_tile2", "f_no1"):
        bad = sr.ps_reference(c, defect=(name, 0))[0]
        _rejects(lambda: assert_within(bad.x, ref, b, name))


def test_steps_integer_regime_and_controls():
    c = sr.ps_case("steps", 16, 10)
    steps = sr.ps_reference(c)
    for st in steps:
        sr.assert_tile_regime(st.tiles[-1][0])
        assert bool(sr.exact_sum_rows(st.h0).all())
        assert float((st.ex / st.x.abs().clamp_min(0.25)).max()) < 1e-4
    x = [c.x0[:, 0]] + [st.x[:, 0] for st in steps]
    assert all(torch.equal(x[k + 1], m * x[k]) for k, m in enumerate((-2.0, -1.0, 2.0)))
    ref, b = steps[-1].x, steps[-1].ex
    for defect in (("coef_prev", 1), ("coef_prev", 2)):
        bad = sr.ps_reference(c, defect=defect)
        _rejects(lambda: assert_within(bad[-1].x, ref, b, str(defect)))
    # a step reading another step's table row or noise, or a stale x
    for k in (1, 2):
        d = sr.ps_case("steps", 16, 10)
        d.mod[k] = c.mod[k - 1]
        _rejects(lambda: assert_within(sr.ps_reference(d)[-1].x, ref, b, "mod row"))
        d = sr.ps_case("steps", 16, 10)
        d.noise[k] = c.noise[k - 1]
        _rejects(lambda: assert_within(sr.ps_reference(d)[-1].x, ref, b, "noise row"))


def test_stale_slice_control_integer_regime():
    """S = 3 with block 5 alone live: the rows the kernel leaves in hx are block 5 on the last step's h0, bit for
    bit; one workgroup's 16 columns of block 5's input taken from the step before gives other rows"""
    c = sr.ps_case("steps", 16, 10, live=sr.DEPTH - 1)
    steps = sr.ps_reference(c)
    sr.assert_live_regime(c, steps[-1])
    hx, ha = sr.live_expected(c, steps[-1])
    assert torch.equal(hx, steps[-1].hx[-1])
    for wg in (0, 37, 63):
        bad = sr.ps_reference(c, stale_at=(2, sr.DEPTH - 1, wg))
        _rejects(lambda: assert_bit_equal(bad[-1].hx[-1].float(), hx, "stale slice"))
        _rejects(lambda: assert_bit_equal(bad[-1].ha[-1].to(BF16), ha, "stale slice"))


@pytest.mark.parametrize("j", range(sr.DEPTH))
def test_live_block_randn_conditions(j):
    """first level (the A tile of block j): the two randn conditions.  Second level (the fc1 output): the share is
    reported, see DESIGN.md -- (K + 8) u S there is about half a bf16 ulp of the SiLU outputs"""
    c = sr.ps_case("live", 16, 10, "randn", live=j)
    st = sr.ps_reference(c)[0]
    t1, ta = st.tiles[j]
    l1, l2 = st.lins[j]
    share, ratio = sr.assert_randn_conditions(t1, l1, f"block {j}")
    print(f"block {j}: A ambiguous {share:.4%} allowance / accumulation {ratio:.3f}; fc1 output ambiguous "
          f"{float(ta.amb.double().mean()):.2%}; hx bound / max|hx| {float(st.ehx[-1].max() / st.hx[-1].abs().max()):.3g}")
    for name in ("w2_prev", "mod_prev"):
        if j:
            bad = sr.ps_reference(c, defect=(name, j))[0]
            _rejects(lambda: assert_within(bad.hx[-1], st.hx[-1], st.ehx[-1], name))


@pytest.mark.parametrize("R,C", [(16, 10), (5, 16)])
def test_all_live_forced_block_and_stale_slice(R, C):
    """all blocks live, S = 3: the propagated enclosure diverges (printed), so the chain is held where the kernel's
    own state can be read back -- the last step's last block, from the rows block 4 left in hx"""
    c = sr.ps_case("all", R, C, "randn")
    steps = sr.ps_reference(c)
    st = steps[-1]
    print("propagated bound / max|x| per step:", [float(s.ex.max() / s.x.abs().max()) for s in steps])
    t1, l1, l2 = sr.forced_block(c, 2, st.hx[-2], st.ha[-1])
    sr.assert_randn_conditions(t1, l1, "forced block")
    assert_within(st.ha[-1], l1.out, sr.out_bound(l1, BF16), "clean ha")
    assert_within(store(st.hx[-1], F32), l2.out, l2.err, "clean hx")
    for wg in (0, 41):
        bad = sr.ps_reference(c, stale_at=(2, sr.DEPTH - 1, wg))[-1]
        _rejects(lambda: assert_within(bad.ha[-1], l1.out, sr.out_bound(l1, BF16), "stale slice"))
    bad = sr.ps_reference(c, defect=("trunc_fc1", sr.DEPTH - 1))[-1]
    _, _, l2b = sr.forced_block(c, 2, st.hx[-2], st.ha[-1])
    _rejects(lambda: assert_within(bad.hx[-1], l2b.out, l2b.err, "hx from a truncated ha against the rounded one"))
