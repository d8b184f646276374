"""csrc/sampler.hip (uva_sampler_linear, uva_sampler_persistent) and uva_p_sample_step per element against the
float64 restatements of tests/sampler_ref.py: bit equality in the integer regime, the per-element bound with
rounding-interval allowances in the randn regime (see that module for both, tests/test_sampler_exact_cpu.py for
the reference-only conditions and the planted-defect controls).  Operands are strided (modulation columns out of
one wide bf16 table, padded leading dimensions), outputs sit in sentinel-guarded NaN-filled buffers."""
import pytest
import torch

import sampler_ref as sr
from conv_ref import assert_bit_equal
from edge_helpers import DEV, Guarded, assert_within
from gemm_ref import BF16, F32, bf16_shares, gen, store

pytestmark = pytest.mark.gpu
W, DEPTH = sr.W_PS, sr.DEPTH
RATIO = {}


def _ops():
    from unified_video_action_amd.native import ops
    return ops


def _record(kind, got, ref, bound):
    e = (got.double().cpu() - ref).abs() / bound.clamp_min(1e-300)
    RATIO[kind] = max(RATIO.get(kind, 0.0), float(e.max()))


def _padded(t, dtype, pad):
    """t [R, K] float64 -> a [R, K] device view with leading dimension K + pad"""
    R, K = t.shape
    buf = torch.full((R, K + pad), 7.0, dtype=dtype, device=DEV)
    buf[:, :K] = t.to(dtype)
    return buf[:, :K]


def _f32(t):
    return None if t is None else t.float().to(DEV).contiguous()


# ------------------------------------------------------------------ uva_sampler_linear
def _launch_linear(c, out):
    K, N = c.K, c.N
    tbl = c.tbl.to(BF16).to(DEV)
    _ops().sampler_linear(
        _padded(c.A, F32 if c.ln else BF16, sr.PAD_A), c.W.to(BF16).to(DEV).contiguous(), out, bias=_f32(c.bias),
        act="silu" if c.act else "none", ln=c.ln, lnw=_f32(c.lnw), lnb=_f32(c.lnb),
        shift=tbl[:, :K] if c.ln else None, scale=tbl[:, K:2 * K] if c.ln else None, eps=c.eps,
        gate=tbl[:, 2 * K:2 * K + N] if c.variant == "gate" else None,
        residual=_padded(c.res, F32, sr.PAD_RES) if c.variant == "gate" else None)


@pytest.mark.parametrize("regime", ["int", "randn"])
@pytest.mark.parametrize("variant", sr.VARIANTS)
@pytest.mark.parametrize("R,N,K,route", sr.LINEAR_CASES)
def test_sampler_linear(R, N, K, route, variant, regime):
    assert _ops().sampler_linear_route(R, N, K) == route
    c = sr.linear_case(regime, variant, R, N, K, edges=(R >= 224 and K == 256))
    sr.assert_linear_regime(c)
    out = Guarded(R, N, c.dtype, ld=N + 5, off=3)
    _launch_linear(c, out.view)
    out.check()
    got = out.view.cpu()
    sr.check_linear(got, c, f"{variant} {regime} R {R} N {N} K {K} {route}")
    if regime == "randn" or c.act:
        b = c.bound if regime == "randn" else sr.act_bound(sr.SILU, c.lin.pre) + 2.0 ** -8 * c.lin.out.abs()
        _record(f"sampler_linear {variant} {regime}", got, c.lin.out, b)


@pytest.mark.parametrize("R,N,K,route", [(33, 64, 512, "narrow"), (225, 449, 1024, "wide")])
def test_sampler_linear_relaunch_is_bit_equal(R, N, K, route):
    assert _ops().sampler_linear_route(R, N, K) == route
    for variant in ("ln_silu", "gate"):
        c = sr.linear_case("randn", variant, R, N, K)
        outs = []
        for _ in range(2):
            out = Guarded(R, N, c.dtype, ld=N + 5, off=3)
            _launch_linear(c, out.view)
            out.check()
            outs.append(out.view.clone())
        assert torch.equal(outs[0], outs[1])


def _raw_linear(**over):
    """uva_sampler_linear through the C ABI with one argument replaced (the refusals: nothing may launch)"""
    from unified_video_action_amd.native.lib import lib
    R, N, K = 16, 16, 256
    t = {
        "x": torch.zeros(R + 1, K + 8, device=DEV), "a": torch.zeros(R + 1, K + 8, dtype=BF16, device=DEV),
        "lnw": torch.ones(K + 8, device=DEV), "lnb": torch.zeros(K + 8, device=DEV),
        "tbl": torch.zeros(R + 1, 3 * K + 8, dtype=BF16, device=DEV), "w": torch.zeros(N + 1, K, dtype=BF16, device=DEV),
        "bias": torch.zeros(N, device=DEV), "res": torch.zeros(R, N, device=DEV),
        "o32": torch.zeros(R, N, device=DEV), "o16": torch.zeros(R, N, dtype=BF16, device=DEV),
    }
    ln = over.get("ln", 1)
    a = dict(ln=ln, A=(t["x"] if ln else t["a"]).data_ptr(), lda=K + 8, lnw=t["lnw"].data_ptr(),
             lnb=t["lnb"].data_ptr(), shift=t["tbl"].data_ptr(), scale=t["tbl"].data_ptr() + 2 * K, ldm=3 * K + 8,
             eps=1e-6, W=t["w"].data_ptr(), bias=t["bias"].data_ptr(), act=0, gate=None, ldg=0, res=None, ldr=0,
             odt=0, out=None, ldo=N, R=R, N=N, K=K)
    for k, v in over.items():
        if k.startswith("off_"):  # a base pointer moved by v bytes
            a[k[4:]] = a[k[4:]] + v
        elif k == "gate" and v:
            a["gate"], a["ldg"] = t["tbl"].data_ptr() + 4 * K, 3 * K + 8
        elif k == "res" and v:
            a["res"], a["ldr"] = t["res"].data_ptr(), N
        else:
            a[k] = v
    a["out"] = (t["o32"] if a["odt"] == 0 else t["o16"]).data_ptr()
    lib().call("uva_sampler_linear", *a.values(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return t


def test_sampler_linear_accepts_the_four_variants_raw():
    _raw_linear(ln=1, act=2, odt=1)
    _raw_linear(ln=1, act=0, odt=0)
    _raw_linear(ln=1, act=0, odt=0, lnw=None, lnb=None)
    _raw_linear(ln=0, act=0, odt=0, gate=1, res=1)
    _raw_linear(ln=0, act=2, odt=1)


VALID = {(1, 2, 0, 1), (1, 0, 0, 0), (0, 0, 1, 0), (0, 2, 0, 1)}
REFUSED = [dict(K=128), dict(K=768), dict(R=0), dict(N=0), dict(lda=258), dict(ldm=3 * 256 + 2),
           dict(ln=0, act=2, odt=1, lda=256 + 4), dict(ln=0, gate=1), dict(ln=0, res=1), dict(shift=None),
           dict(scale=None), dict(act=1), dict(act=3), dict(lnb=None),
           # pointer alignment of the vector loads (16 bytes: X / bf16 A / W / lnw / lnb; 8 bytes: shift / scale)
           dict(off_A=4), dict(off_A=8), dict(ln=0, act=2, odt=1, off_A=2), dict(ln=0, act=2, odt=1, off_A=8),
           dict(off_W=2), dict(off_W=8), dict(off_lnw=4), dict(off_lnb=8), dict(off_shift=2), dict(off_scale=4)]
REFUSED += [dict(ln=l, act=a, gate=g, res=g, odt=o) for l in (0, 1) for a in (0, 2) for g in (0, 1) for o in (0, 1)
            if (l, a, g, o) not in VALID]


@pytest.mark.parametrize("over", REFUSED, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_sampler_linear_refusals(over):
    with pytest.raises(RuntimeError):
        _raw_linear(**over)


# ------------------------------------------------------------------ uva_p_sample_step
def _p_sample_case(rows, C, odt, clip, nonzero):
    g = gen(40 + rows + C)
    out = torch.randn(rows, 2 * C, generator=g).to(odt).double()
    out[:, C:] = out[:, C:].clamp(-1, 1)
    x = (torch.randn(rows, C, generator=g) * 2).float().double()
    noise = torch.randn(rows, C, generator=g).float().double()
    kc = [1.0, 0.5, 0.4, 0.55, -6.0, -3.5, nonzero, 0.95]
    # x0 = x - eps / 2 exactly at, just inside and just outside +-1
    marks = [(0.5, -1.0), (-0.5, 1.0), (0.5, -1.0 + 2.0 ** -7), (0.5, -1.0 - 2.0 ** -7), (-0.5, 1.0 - 2.0 ** -7),
             (-0.5, 1.0 + 2.0 ** -7)]
    for i, (xv, ev) in enumerate(marks[:rows * C]):
        x.view(-1)[i] = xv
        out[i // C, i % C] = ev
    return out, x, noise, kc


@pytest.mark.parametrize("clip,nonzero", [(True, 1.0), (False, 1.0), (True, 0.0)])
@pytest.mark.parametrize("odt", [F32, BF16])
@pytest.mark.parametrize("C", [1, 10, 16])
@pytest.mark.parametrize("rows", [1, 257])
def test_p_sample_step(rows, C, odt, clip, nonzero):
    out, x, noise, kc = _p_sample_case(rows, C, odt, clip, nonzero)
    ref, b = sr.p_sample(out[:, :C], out[:, C:], x, noise, kc, clip)
    wide = torch.full((rows, 2 * C + 6), float("nan"), dtype=odt, device=DEV)  # ld_out > 2C inside a wider buffer
    wide[:, 2:2 * C + 2] = out.to(odt)
    for inplace in (False, True):
        xd = x.float().to(DEV)
        fresh, net = Guarded(rows, C, F32), Guarded(rows, C, BF16)
        xn = xd if inplace else fresh.view
        _ops().p_sample_step(wide[:, 2:2 * C + 2], xd, noise.float().to(DEV), kc, xn, net.view, clip=clip)
        net.check(), fresh.check()
        assert_within(xn.cpu(), ref, b, f"p_sample rows {rows} C {C} inplace {inplace}")
        assert torch.equal(net.view, xn.to(BF16))  # x_net = the fp32 result rounded once
        if not inplace:
            assert torch.equal(xd.cpu(), x.float())
        _record("p_sample_step", xn.cpu(), ref, b)


def test_p_sample_step_x_net_rounds_ties_to_even():
    """dyadic coefficients, operands on the grid 1/256, nonzero = 0: x_new is exact (bit-equal to float64), x_net its
    bf16 rounding with exact ties among them"""
    rows, C = 257, 10
    g = gen(3)
    out = torch.randint(-512, 513, (rows, 2 * C), generator=g).double() / 256
    x = torch.randint(-512, 513, (rows, C), generator=g).double() / 256
    kc = [1.0, 0.5, 1.0, 0.25, -6.0, -3.5, 0.0, 1.0]
    ref, _ = sr.p_sample(out[:, :C], out[:, C:], x, torch.ones(rows, C).double(), kc, False)
    below, big, ties = bf16_shares(ref * 256)   # on the integer grid: >= 256 needs rounding
    assert ties >= 8 and big >= 0.2
    xn, net = Guarded(rows, C, F32), Guarded(rows, C, BF16)
    _ops().p_sample_step(out.float().to(DEV), x.float().to(DEV), torch.ones(rows, C, device=DEV), kc, xn.view, net.view,
                         clip=False)
    xn.check(), net.check()
    assert_bit_equal(xn.view.cpu(), ref, "x_new")
    assert_bit_equal(net.view.cpu(), ref, "x_net")


def test_p_sample_step_refuses_a_short_ld_out():
    rows, C = 4, 10
    out = torch.zeros(rows * 2 * C, device=DEV).as_strided((rows, 2 * C), (C, 1))
    x = torch.zeros(rows, C, device=DEV)
    with pytest.raises(RuntimeError):
        _ops().p_sample_step(out, x, x.clone(), [1.0] * 8, x.clone())


# ------------------------------------------------------------------ uva_sampler_persistent
_DEV_PACKS = {}


def _fits():
    if not _ops().sampler_persistent_fits(DEV):
        pytest.skip("fewer than 64 CUs: the persistent sampler's workgroups cannot all be resident")


def _dev_pack(c):
    key = id(c.pack)
    if key not in _DEV_PACKS:
        _DEV_PACKS.clear()  # one at a time: 25 MB each
        p = c.pack
        _DEV_PACKS[key] = {k: (p[k].to(BF16) if k in ("w1", "w2", "win", "wf") else p[k].float()).to(DEV).contiguous()
                           for k in ("w1", "b1", "w2", "b2", "lnw", "lnb", "win", "bin", "wf", "bfin")}
    return _DEV_PACKS[key]


class Run:
    pass


def _launch_ps(c, work=None):
    ops = _ops()
    r = Run()
    r.work = ops.sampler_persistent_workspace(W, DEV) if work is None else work
    if work is None:
        r.work.fill_(0xFF)
    r.out = Guarded(c.R, c.C, F32)
    ops.sampler_persistent(_dev_pack(c), c.mod.to(BF16).to(DEV), c.coef.float().to(DEV), c.noise.float().to(DEV),
                           c.x0.float().to(DEV), r.out.view, r.work, clip=c.clip, eps=c.eps)
    r.out.check()
    assert ops.sampler_persistent_status(r.work) == 0
    # the layout of work (include/uva_hip.h): hx [2, 16, W] fp32 at byte 256, then ha [16, W] bf16
    r.hx = r.work[256:256 + 2 * 16 * W * 4].view(F32).view(2, 16, W).cpu()
    r.ha = r.work[256 + 2 * 16 * W * 4:256 + 2 * 16 * W * 4 + 16 * W * 2].view(BF16).view(16, W).cpu()
    r.x = r.out.view.cpu()
    return r


@pytest.mark.parametrize("j", range(DEPTH))
def test_persistent_live_block_integer(j):
    """block j alone has a nonzero gate: the rows left in hx are block j on h0 with block j's own weights, LN affine
    and modulation columns, bit for bit; for the last block ha holds its fc1 output"""
    _fits()
    for R, C in ((16, 10), (5, 16)) if j == DEPTH - 1 else ((16, 10),):
        c = sr.ps_case("live", R, C, "int", live=j)
        st = sr.ps_reference(c)[0]
        sr.assert_live_regime(c, st)
        hx, ha = sr.live_expected(c, st)
        r = _launch_ps(c)
        side = (DEPTH - 1) & 1
        assert_bit_equal(r.hx[side, :R], hx, f"hx, block {j} live, R {R} C {C}")
        assert not bool(r.hx[side, R:].any())
        if j == DEPTH - 1:
            assert_bit_equal(r.ha[:R], ha, "ha")
            if R < 16:  # rows >= R: SiLU(b1) = b1
                assert_bit_equal(r.ha[R:], store(c.pack["b1"][j], BF16).expand(16 - R, W), "ha tail rows")
            assert_bit_equal(r.hx[side ^ 1, :R], st.h0, "hx, the other side: block 4 passed h0 through")


@pytest.mark.parametrize("j", range(DEPTH))
def test_persistent_live_block_randn(j):
    _fits()
    c = sr.ps_case("live", 16, 10, "randn", live=j)
    st = sr.ps_reference(c)[0]
    r = _launch_ps(c)
    side = (DEPTH - 1) & 1
    assert_within(r.hx[side], st.hx[-1], st.ehx[-1], f"hx, block {j} live")
    _record("hx (propagated)", r.hx[side], st.hx[-1], st.ehx[-1])
    if j == DEPTH - 1:
        t1, l1, l2 = sr.forced_block(c, 0, r.hx[side ^ 1].double(), r.ha.double())
        assert_within(r.ha, l1.out, sr.out_bound(l1, BF16), "ha")
        assert_within(r.hx[side], l2.out, l2.err, "hx from the kernel's own ha")
        _record("ha", r.ha, l1.out, sr.out_bound(l1, BF16))
        _record("hx (from the kernel's ha)", r.hx[side], l2.out, l2.err)
        assert_within(r.hx[side ^ 1], st.h0, st.eh0, "h0")


@pytest.mark.parametrize("kind", ["eps", "clip", "var"])
@pytest.mark.parametrize("C", [1, 8, 9, 16])
@pytest.mark.parametrize("R", [1, 5, 16])
def test_persistent_final_layer_and_p_sample(kind, R, C):
    """every gate 0: x_out shows the final layer's eps half exactly (N2 = 2, 16, 18, 32), through the clip, and its
    variance half through exp"""
    _fits()
    c = sr.ps_case(kind, R, C)
    st = sr.ps_reference(c)[0]
    sr.assert_tile_regime(st.tiles[-1][0])
    r = _launch_ps(c)
    if kind == "var":
        ref, b = sr.p_sample(st.out[:, :C], st.out[:, C:], c.x0, c.noise[0], sr.KC_VAR, False)
        assert_within(r.x, ref, b, f"x_out var R {R} C {C}")
        _record("x_out (variance half)", r.x, ref, b)
    else:
        assert_bit_equal(r.x, st.x, f"x_out {kind} R {R} C {C}")
    assert_bit_equal(r.hx[(DEPTH - 1) & 1, :R], st.h0, "h0 through six dead blocks")


def test_persistent_steps():
    """S = 3, every gate 0, mod[k], coef[k], noise[k] all different, x[:, 0] (the only column input_proj reads)
    changing sign and size from step to step"""
    _fits()
    c = sr.ps_case("steps", 16, 10)
    steps = sr.ps_reference(c)
    for st in steps:
        sr.assert_tile_regime(st.tiles[-1][0])
    r = _launch_ps(c)
    assert_within(r.x, steps[-1].x, steps[-1].ex, "x_out after 3 steps")
    assert_bit_equal(r.x[:, 0], steps[-1].x[:, 0], "x_out column 0")
    _record("x_out (3 steps)", r.x, steps[-1].x, steps[-1].ex)
    # and with the last block live: the exchange buffers hold the LAST step's rows
    c = sr.ps_case("steps", 16, 10, live=DEPTH - 1)
    steps = sr.ps_reference(c)
    sr.assert_live_regime(c, steps[-1])
    hx, ha = sr.live_expected(c, steps[-1])
    r = _launch_ps(c)
    assert_bit_equal(r.hx[(DEPTH - 1) & 1], hx, "hx of step 2")
    assert_bit_equal(r.ha, ha, "ha of step 2")


@pytest.mark.parametrize("R,C", [(16, 10), (5, 16)])
def test_persistent_all_blocks_live(R, C):
    """every block live, randn.  The enclosure propagated through all levels diverges, so the chain is
    held where the kernel's own state can be read back: after S = 3 the last block from the rows block 4 left in hx
    and the fc1 output in ha; after S = 1 also the final layer and p_sample from the last residual rows"""
    _fits()
    side = (DEPTH - 1) & 1
    c = sr.ps_case("all", R, C, "randn")
    r = _launch_ps(c)
    assert bool(torch.isfinite(r.x).all())
    t1, l1, l2 = sr.forced_block(c, 2, r.hx[side ^ 1, :R].double(), r.ha[:R].double())
    assert_within(r.ha[:R], l1.out, sr.out_bound(l1, BF16), "ha, step 2")
    assert_within(r.hx[side, :R], l2.out, l2.err, "hx, step 2")
    _record("ha", r.ha[:R], l1.out, sr.out_bound(l1, BF16))
    _record("hx (from the kernel's ha)", r.hx[side, :R], l2.out, l2.err)
    c.S, c.mod, c.coef, c.noise = 1, c.mod[:1], c.coef[:1], c.noise[:1]
    r = _launch_ps(c)
    tf, lf, xn, b = sr.forced_final(c, r.hx[side, :R].double(), c.x0)
    assert_within(r.x, xn, b, "x_out from the kernel's last rows")
    _record("x_out (from the kernel's hx)", r.x, xn, b)


def test_persistent_relaunch_is_bit_equal():
    _fits()
    c = sr.ps_case("all", 16, 10, "randn")
    a = _launch_ps(c)
    b = _launch_ps(c, work=a.work)   # the same work, counters left by the first launch
    f = _launch_ps(c)                # a fresh one
    for o in (b, f):
        assert torch.equal(a.x, o.x) and torch.equal(a.hx, o.hx) and torch.equal(a.ha, o.ha)


PS_REFUSED = [dict(R=0), dict(R=17), dict(C=0), dict(C=17), dict(W=512), dict(W=2048), dict(depth=5), dict(depth=7),
              dict(S=0), dict(work_bytes=-1), dict(off_work=128), dict(off_work=4), dict(ldmod=20 * 1024 - 4),
              dict(ldmod=20 * 1024 + 2), dict(off_w1=2), dict(off_w2=8), dict(off_lnw=4), dict(off_lnb=8),
              dict(off_wf=2), dict(off_bin=4), dict(off_mod=2), dict(work=None)]


@pytest.mark.parametrize("over", PS_REFUSED, ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_persistent_refusals(over):
    from unified_video_action_amd.native.lib import lib
    _fits()
    R, C, S = 4, 2, 1
    z = lambda *s, dt=F32: torch.zeros(*s, dtype=dt, device=DEV)  # noqa: E731
    t = dict(w1=z(DEPTH * W * W + 8, dt=BF16), b1=z(DEPTH, W), w2=z(DEPTH * W * W + 8, dt=BF16), b2=z(DEPTH, W),
             lnw=z(DEPTH * W + 8), lnb=z(DEPTH * W + 8), win=z(W, C, dt=BF16), bin=z(W + 8), wf=z(2 * C * W + 8, dt=BF16),
             bfin=z(2 * C), mod=z(S * R * 20 * W + 8, dt=BF16), coef=z(S, 8), noise=z(S, R, C), x0=z(R, C), x_out=z(R, C))
    work = _ops().sampler_persistent_workspace(W, DEV)
    big = torch.zeros(work.numel() + 512, dtype=torch.uint8, device=DEV)
    a = dict(R=R, C=C, W=W, depth=DEPTH, S=S, clip=1, eps=1e-6)
    a.update({k: t[k].data_ptr() for k in ("w1", "b1", "w2", "b2", "lnw", "lnb", "win", "bin", "wf", "bfin", "mod")})
    a["ldmod"] = 20 * W
    a.update({k: t[k].data_ptr() for k in ("coef", "noise", "x0", "x_out")})
    a["work"], a["work_bytes"] = big.data_ptr(), work.numel()
    for k, v in over.items():
        if k.startswith("off_"):
            a[k[4:]] = a[k[4:]] + v
        elif k == "work_bytes":
            a[k] = a[k] + v
        else:
            a[k] = v
    with pytest.raises(RuntimeError):
        lib().call("uva_sampler_persistent", *a.values(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


def test_zz_report_worst_ratios():
    """the worst measured error / bound per output kind of this run (DESIGN.md quotes them)"""
    for k in sorted(RATIO):
        print(f"worst error / bound  {k}: {RATIO[k]:.3f}")
    assert all(v <= 1.0 for v in RATIO.values())
