"""Every dense route of uva_gemm (csrc/gemm.hip: gemm_generic and its split-K, gemm_mfma_v2 and its
split-K, gemm_8ph at BN 256 / 384 fast, ragged and split, gemm_8pp, splitk_reduce and splitk_reduce_f32x4;
csrc/gemm4.hip gemm_4w plain and dW; csrc/gemm8w.hip plain and dW under its switch) per element against the
float64 reference of tests/gemm_ref.py.

Link 1: integer operands, dyadic epilogue inputs, dropout p = 1/2: output torch.equal to the reference
(rounded once to nearest even for bf16).  Link 2: randn operands rounded to bf16, (K + 8) u S (+ 2^-8 |ref|).
Link 3: gelu / silu (forward, and 16 + kind backward with dropout) on exact pre-activations inside the
counted bounds of gemm_ref.py; relu and relu' go through link 1's bit equality.  Every bf16 link 1 case
asserts the magnitude and tie shares of its reference (restated for outputs behind the dropout scale or a
gate).  Every case asserts its route through
uva_gemm_route before it launches; every output, aux and C0 buffer is a NaN-filled (or C0-holding) view with
ldc > N and a column offset inside sentinel guards; residual and gate have ldr / ldg > N (gate out of a
[M, 3N] buffer); A and B sit in wider junk-filled rows.  Batched cases use two-level strides with an unused
batch slot between the outer batches (it must stay untouched).  The controls of the comparisons run on
the CPU (test_gemm_exact_cpu.py)."""
import functools

import pytest
import torch

import edge_helpers as E
import gemm_ref as R
from gemm_ref import BF16, F32, GELU, RELU, SILU

pytestmark = pytest.mark.gpu

JUNK = 3.0     # fills operand padding: a read past K or past a row changes every output it reaches
SEED = 0x5EED1234ABCD


def _ops():
    from unified_video_action_amd.native import ops
    return ops


@pytest.fixture(autouse=True)
def default_switches():
    """the library's default routing whatever an earlier test's RT.begin_forward() left: gemm_8w's plain and dW
    routes off, gemm_4w on with its automatic tile, gemm_8pp off; restored afterwards"""
    ops = _ops()
    p8, p4, pp = ops.gemm8w_set(0, 0), ops.gemm4_set(1, -1), ops.gemm_set_persist(False)
    yield
    ops.gemm8w_set(*p8)
    ops.gemm4_set(*p4)
    ops.gemm_set_persist(pp)


@pytest.fixture(autouse=True, scope="module")
def release_cases():
    """the cached float64 operands and products leave the device with this module"""
    yield
    _case64.cache_clear()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=3)
def _case64(seed, Z, M, N, K, amp, link):
    """operands (float64, on the device) and their float64 products, built once per (shape, seed) and shared
    by the epilogue variants"""
    a, b = R.randn_operands(seed, Z, M, N, K) if link == 2 else R.exact_operands(seed, Z, M, N, K, amp)
    a, b = a.to(E.DEV), b.to(E.DEV)
    return (a, b) + R.product(a, b)


def _strided(x, dtype, ld_extra, off, zo, zi):
    """x [zo * zi, rows, cols] float64 -> (view [zo, zi, rows, cols] of a junk-filled buffer
    [zo, zi + 1, rows, cols + ld_extra] starting at column `off`, ld, (outer, inner) batch strides)"""
    Z, rows, cols = x.shape
    ld = cols + ld_extra
    extra = 1 if zo * zi > 1 else 0
    buf = torch.full((zo, zi + extra, rows, ld), JUNK, dtype=dtype, device=E.DEV)
    view = buf[:, :zi, :, off:off + cols]
    view.copy_(x.view(zo, zi, rows, cols))
    return view, ld, ((zi + extra) * rows * ld, rows * ld)


def _guarded(Zg, M, N, dtype, ld_extra, off, init=None):
    return E.Guarded(Zg * M, N, dtype, ld=N + ld_extra, off=off, init=init)


def run(M, N, K, route, ta=0, tb=0, in_dt=BF16, out_dt=BF16, zo=1, zi=1, alpha=1.0, bias=False, beta=0.0,
        res=None, gate=None, aux=False, drop=False, act=0, link=1, wide=True, odd=False, force_generic=False,
        seed=1, splitk=True, ldc_odd=False):
    """one uva_gemm launch into guarded buffers against the float64 reference.  route: the keys of
    ops.gemm_route this case means to test (a value, or a predicate on it).  res / gate: None or the operand's
    dtype.  odd: leading dimensions and offsets that are no multiple of 8 (the VALU kernel); else multiples of
    8 (16-byte rows); ldc_odd: only C / aux / C0 so.  -> (output [Z, M, N], Ref, route)"""
    ops = _ops()
    Z = zo * zi
    kind = act - 16 if act >= 16 else act
    exact = link == 1 and kind in (0, RELU)
    if link == 3:
        amp, alpha = R.act_scaling(K)
    else:
        amp = R.amp_for(K, alpha)
    a, b, P, Pabs = _case64(seed, Z, M, N, K, amp, link)
    g = R.gen(seed + 77)
    ex, off = (3, 1) if odd else (8, 8)
    # ---- operands in wider rows
    pa = a if ta == 0 else a.transpose(1, 2)
    pb = b if tb == 0 else b.transpose(1, 2)
    Av, lda, sA = _strided(pa, in_dt, ex if wide else 0, off if wide else 0, zo, zi)
    Bv, ldb, sB = _strided(pb, in_dt, ex if wide else 0, off if wide else 0, zo, zi)
    # ---- epilogue inputs
    epi, kw = {}, {}
    if bias:
        bv = R.ints(g, 2 if link == 3 else 64, (N,), zero=True)
        epi["bias"] = bv.to(E.DEV)
        kw["bias"] = bv.float().to(E.DEV)
    if res is not None:
        rv = R.ints(g, 32, (Z, M, N), zero=True) / 8 if act >= 16 else R.ints(g, 64, (Z, M, N), zero=True)
        Rv, ldr, sR = _strided(rv, res, ex, off, zo, zi)
        epi["residual"] = rv.to(E.DEV)
        kw.update(residual=Rv, ldr=ldr, sR=sR)
    if gate is not None:
        gv = R.gate_values(g, (M, N))
        gbuf = torch.full((M, 3 * N), JUNK, dtype=gate, device=E.DEV)
        gbuf[:, N:2 * N].copy_(gv)
        epi["gate"] = gv.to(E.DEV)
        kw.update(gate=gbuf[:, N:2 * N], ldg=3 * N)
    if drop:
        thresh, scale = R.drop_half()
        epi["drop"] = (SEED + seed, thresh, scale)
        kw.update(drop_p=0.5, seed=SEED + seed)
    Zg = zo * (zi + 1) if Z > 1 else 1    # batch slots of the output buffers (one unused slot per outer batch)
    c0 = None
    if beta != 0.0:
        c0 = R.ints(g, 64, (Zg, M, N), zero=True)
        epi.update(beta=beta, c0=c0.view(zo, -1, M, N)[:, :zi].reshape(Z, M, N).to(E.DEV))
    r = R.epilogue_ref(P, Pabs, out_dt, alpha=alpha, act=act, **epi)
    # ---- input conditions
    if exact:
        grid = (0.5 if alpha == 0.5 else 1.0) * (0.5 if gate is not None else 1.0) * (0.5 if beta == -0.5 else 1.0)
        R.assert_exact_regime(r.S, r.out, grid)
        if out_dt == BF16 and (drop or gate is not None):
            R.assert_bf16_shares_scaled(r.out, "output", r.keep)
        elif out_dt == BF16:
            R.assert_bf16_shares(r.out, "output")
    elif link == 3:
        R.assert_act_grid(r.pre)
    # ---- guarded outputs
    cex, coff = (3, 1) if ldc_odd else (ex, off)
    og = _guarded(Zg, M, N, out_dt, cex, coff, init=None if c0 is None else c0.view(Zg * M, N).to(out_dt))
    ag = _guarded(Zg, M, N, out_dt, cex, coff) if aux else None
    ldc = N + cex
    sC = ((zi + 1) * M * ldc, M * ldc) if Z > 1 else (0, 0)
    args = (Av, Bv, og.view, M, N, K, lda, ldb, ldc)
    kw.update(ta=ta, tb=tb, batch=Z, inner=zi, sA=sA, sB=sB, sC=sC, aux=ag.view if aux else None, act=act,
              alpha=alpha, beta=beta, force_generic=force_generic, splitk=splitk)
    got_route = ops.gemm_route(*args, **kw)
    for k, want in route.items():
        assert want(got_route[k]) if callable(want) else got_route[k] == want, (k, got_route)
    ops.gemm(*args, **kw)
    raw = torch.int16 if out_dt == BF16 else torch.int32

    def payload(gd, what):
        """guards checked; the unused batch slot untouched, bit for bit -> the written batches [Z, M, N]"""
        gd.check()
        full = gd.view.view(zo, -1, M, N)
        if Z > 1:
            before = gd.before[E.PAD:-E.PAD].view(Zg * M, ldc)[:, coff:coff + N].view(zo, -1, M, N)[:, zi]
            assert torch.equal(full[:, zi].view(raw), before.view(raw)), f"{what}: write into the unused batch slot"
        return full[:, :zi].reshape(Z, M, N)

    got = payload(og, "output")
    if drop and gate is None and res is None and beta == 0.0:   # the dropout value itself is what is stored
        assert not got.contiguous().view(raw)[~r.keep].any(), "a dropped element is not +0"
        assert (got[r.keep & (r.out != 0)] != 0).all(), "a kept element with a nonzero reference is zero"
    if exact:
        R.assert_bit_equal(got, r.out, "output")
    elif link == 2:
        bound = R.link2_bound(r.out, r.S, K, out_dt)
        print(f"link 2 worst |got - ref| / bound = {float(((got.double() - r.out).abs() / bound).max()):.3f}")
        R.assert_link2(got, r.out, r.S, K, "output")
    else:
        bound = (R.link3_bwd_bound(kind, r, epi["residual"], out_dt) if act >= 16
                 else R.link3_fwd_bound(kind, r, 2.0 if drop else 1.0, out_dt))
        ratio = ((got.double() - r.out).abs() / bound.clamp_min(1e-300))[bound > 0]
        print(f"link 3 worst |got - ref| / bound = {float(ratio.max()):.3f}")
        E.assert_within(got, r.out, bound, "output")
    if aux:   # the pre-activation is exact in links 1 and 3
        R.assert_bit_equal(payload(ag, "aux"), r.pre, "aux")
    return got, r, got_route


# the epilogue matrix, run once per epilogue implementation; act >= 16 = activation backward on the "residual"
EPI = dict(
    bias_bf16=dict(bias=True),
    bias_f32=dict(bias=True, out_dt=F32),
    alpha_half=dict(alpha=0.5, bias=True),
    alpha_neg2_f32=dict(alpha=-2.0, bias=True, out_dt=F32),
    beta_f32=dict(beta=1.0, out_dt=F32),
    beta_bf16=dict(beta=-0.5, bias=True),
    res_bf16_out_bf16=dict(res=BF16),
    res_f32_out_bf16=dict(res=F32, bias=True),
    res_bf16_out_f32=dict(res=BF16, out_dt=F32),
    res_f32_out_f32=dict(res=F32, out_dt=F32, alpha=0.5),
    gate_bf16=dict(gate=BF16, bias=True),
    gate_f32=dict(gate=F32),
    gate_f32_out_f32=dict(gate=F32, out_dt=F32, bias=True),
    aux_bf16=dict(aux=True, bias=True, alpha=0.5),
    aux_f32=dict(aux=True, bias=True, out_dt=F32),
    drop_bf16=dict(drop=True, bias=True),
    drop_f32=dict(drop=True, out_dt=F32),
    gate_res_drop=dict(gate=BF16, res=F32, drop=True, bias=True),
    gate_res_drop_f32=dict(gate=F32, res=BF16, drop=True, bias=True, out_dt=F32, alpha=0.5),
    gelu=dict(act=GELU, link=3, bias=True, aux=True, out_dt=F32),
    gelu_bf16=dict(act=GELU, link=3, bias=True, aux=True),
    silu=dict(act=SILU, link=3, bias=True, out_dt=F32),
    silu_drop_bf16=dict(act=SILU, link=3, bias=True, drop=True),
    relu=dict(act=RELU, bias=True, aux=True, drop=True),
    dgelu_drop=dict(act=16 + GELU, link=3, res=F32, drop=True, out_dt=F32),
    dgelu_drop_bf16=dict(act=16 + GELU, link=3, res=BF16, drop=True),
    dsilu_drop=dict(act=16 + SILU, link=3, res=BF16, drop=True, out_dt=F32),
    drelu_drop=dict(act=16 + RELU, res=F32, drop=True, out_dt=F32),
    drelu_drop_bf16=dict(act=16 + RELU, res=BF16, drop=True, bias=True),
)
# gemm_8pp takes no row inputs: bias, aux + activation, dropout
EPI_8PP = ["bias_bf16", "bias_f32", "aux_bf16", "aux_f32", "drop_bf16", "drop_f32", "gelu", "gelu_bf16",
           "silu_drop_bf16", "relu"]
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
DT_IDS = dict(argvalues=[BF16, F32], ids=["bf16", "f32"])


# ---------------------------------------------------------------- gemm_generic
GEN = dict(kernel="generic", splits=1, reduce=None)
GEN_SPLIT = dict(kernel="generic", splits=lambda s: s > 1, reduce="scalar")


@pytest.mark.parametrize("out_dt", **DT_IDS)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("K", [2, 17, 33])
def test_generic_f32_operands(K, ta, tb, out_dt):
    """fp32 operands, ragged 64-tiles (65 x 67), a BK = 16 tail of 1 or 2, odd leading dimensions and offsets"""
    run(65, 67, K, GEN, ta=ta, tb=tb, in_dt=F32, out_dt=out_dt, bias=True, odd=True, seed=10 + K)


@pytest.mark.parametrize("why", ["k_not_8", "ld_unaligned", "forced"])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_generic_bf16_operands(ta, tb, why):
    """bf16 operands on the VALU kernel: K no multiple of 8, an unaligned leading dimension, force_generic"""
    K = 17 if why == "k_not_8" else 24
    run(65, 67, K, GEN, ta=ta, tb=tb, bias=True, odd=why != "forced", force_generic=why == "forced", seed=20)


@pytest.mark.parametrize("out_dt", **DT_IDS)
def test_generic_batched_two_level(out_dt):
    run(65, 67, 17, GEN, in_dt=F32, out_dt=out_dt, zo=2, zi=3, bias=True, res=F32, drop=True, odd=True, seed=30)


@pytest.mark.parametrize("M,N,K", [(16, 4, 4100), (70, 12, 8200)])
def test_generic_splitk(M, N, K):
    """gemm_generic<SPLIT>: K >= 4096 under 64 blocks, a short last slice; bf16 output + bias: the scalar
    splitk_reduce"""
    _, _, rt = run(M, N, K, GEN_SPLIT, in_dt=F32, bias=True, alpha=-2.0 if M == 16 else 1.0, odd=True, seed=40)
    kps = (-(-K // rt["splits"]) + 15) // 16 * 16
    assert K % kps != 0


@pytest.mark.parametrize("name", list(EPI))
def test_generic_epilogues(name):
    """epi_store on the smallest ragged shape (res_dt != the output type on the VALU kernel included)"""
    run(65, 67, 17, GEN, in_dt=F32, odd=True, seed=50, **EPI[name])


@pytest.mark.parametrize("name", ["res_f32_out_bf16", "gate_res_drop", "aux_f32", "beta_f32", "gelu_bf16",
                                  "dgelu_drop"])
def test_generic_splitk_epilogues(name):
    """epi_store inside splitk_reduce"""
    run(70, 12, 8200, GEN_SPLIT, in_dt=F32, odd=True, seed=60, **EPI[name])


def test_generic_link2():
    run(65, 67, 33, GEN, in_dt=F32, out_dt=F32, bias=True, odd=True, link=2, seed=70)
    run(70, 12, 8200, GEN_SPLIT, bias=True, odd=True, link=2, seed=71)


# ---------------------------------------------------------------- gemm_mfma_v2 (128 x 128)
DMA = dict(kernel="dma128", splits=1, reduce=None)


@pytest.mark.parametrize("out_dt", **DT_IDS)
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,N,K", [(130, 136, 72), (128, 128, 8), (264, 72, 200)])
def test_dma128_layouts(M, N, K, ta, tb, out_dt):
    """ragged 128-tiles, one 8-wide K chunk, three row tiles (M-contiguous A needs M % 8 == 0: 130 -> 136)"""
    if ta == 1 and M % 8:
        M = 136
    run(M, N, K, DMA, ta=ta, tb=tb, out_dt=out_dt, bias=ta == tb, seed=100 + K)


@pytest.mark.parametrize("out_dt", **DT_IDS)
def test_dma128_batched_two_level(out_dt):
    run(130, 136, 72, DMA, out_dt=out_dt, zo=2, zi=3, bias=True, res=BF16, drop=True, seed=110)


@pytest.mark.parametrize("reduce", ["f32x4", "f32x4_beta", "scalar_bias", "scalar_bf16"])
@pytest.mark.parametrize("M,N,K,ta,tb,skinny", [(136, 72, 1096, 0, 0, False), (264, 16, 8200, 0, 0, True),
                                               (16, 264, 8200, 1, 1, True)])
def test_dma128_splitk(M, N, K, ta, tb, skinny, reduce):
    """split-K with a ragged last slice; the skinny cap of 128 slices (N <= 64 or M <= 64): more than 16;
    the reduce as splitk_reduce_f32x4 (plain fp32) and as splitk_reduce (bias / bf16 output)"""
    route = dict(kernel="dma128", splits=lambda s: s > (16 if skinny else 1),
                 reduce="f32x4" if reduce.startswith("f32x4") else "scalar")
    _, _, rt = run(M, N, K, route, ta=ta, tb=tb, out_dt=BF16 if reduce == "scalar_bf16" else F32,
                   bias=reduce.startswith("scalar"), beta=1.0 if reduce == "f32x4_beta" else 0.0,
                   alpha=0.5 if reduce == "f32x4_beta" else 1.0, seed=120)
    kps = (-(-K // rt["splits"]) + 63) // 64 * 64
    assert K % kps != 0


@pytest.mark.parametrize("name", list(EPI))
def test_dma128_epilogues(name):
    """the 128 x 128 kernel's row epilogue (epi_load_row8 / epi_apply_row8) on (130, 136, 72)"""
    run(130, 136, 72, DMA, seed=130, **EPI[name])


@pytest.mark.parametrize("name", ["bias_bf16", "res_bf16_out_f32", "gate_f32", "drop_f32", "aux_bf16", "dsilu_drop"])
def test_dma128_epilogues_unaligned_ldc(name):
    """ldc no multiple of 8 and an odd column offset: the tile epilogue's per-element path (epi_store)"""
    run(130, 136, 72, DMA, seed=130, ldc_odd=True, **EPI[name])


@pytest.mark.parametrize("name", ["res_f32_out_bf16", "gate_res_drop", "aux_bf16", "gelu", "dgelu_drop_bf16"])
def test_dma128_splitk_epilogues(name):
    """splitk_reduce's epi_store behind the 128 x 128 kernel"""
    run(136, 72, 1096, dict(kernel="dma128", splits=lambda s: s > 1, reduce="scalar"), seed=140, **EPI[name])


def test_dma128_link2():
    run(130, 136, 200, DMA, bias=True, link=2, seed=150)
    run(136, 72, 1096, dict(kernel="dma128", reduce="f32x4"), out_dt=F32, link=2, seed=151)


# ---------------------------------------------------------------- gemm_8ph
def ph8(bn, fast=None, splits=1, reduce=None):
    """fast None: either variant"""
    route = dict(kernel="8ph", bn=bn, splits=splits, reduce=reduce, persist=False)
    if fast is not None:
        route["fast"] = fast
    return route


@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("M,N,K,fast", [(5000, 3000, 136, False), (5376, 3072, 128, True)])
def test_8ph_bn256_layouts(M, N, K, fast, ta, tb):
    """ragged tiles with a K tail (the general variant) and whole tiles (the precomputed-source variant)"""
    run(M, N, K, ph8(256, fast), ta=ta, tb=tb, out_dt=BF16 if ta == tb else F32, bias=True, res=BF16, seed=200 + K)


@pytest.fixture
def gemm4_off():
    ops = _ops()
    prev = ops.gemm4_set(on=0)
    yield
    ops.gemm4_set(on=prev[0], force=prev[1])


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("M,N,K", [(768, 768, 4096), (776, 760, 4104)])
def test_8ph_splitk_dw(M, N, K, beta, gemm4_off):
    """the dW form on gemm_8ph's split-K (gemm_4w switched off: it takes the first shape otherwise), whole and
    ragged tiles / slices, reduced by splitk_reduce_f32x4"""
    run(M, N, K, ph8(256, K % 64 == 0 and M % 256 == 0, splits=lambda s: s > 1, reduce="f32x4"), ta=1, tb=1,
        out_dt=F32, beta=beta, seed=210)


def test_8ph_splitk_scalar_reduce(gemm4_off):
    run(776, 760, 4104, ph8(256, False, splits=lambda s: s > 1, reduce="scalar"), ta=1, tb=1, bias=True, res=F32,
        drop=True, seed=210)


@pytest.mark.parametrize("out_dt", **DT_IDS)
def test_8ph_batched_two_level(out_dt):
    """2 x 3 batches of 5 x 5 tiles (150 workgroups) with two-level strides on A, B, C and the residual"""
    run(1280, 1280, 72, ph8(256, False), out_dt=out_dt, zo=2, zi=3, bias=True, res=BF16, drop=True, seed=215)


@pytest.mark.parametrize("M,N,K,fast", [(6144, 768, 128, True), (6100, 768, 136, False)])
def test_8ph_bn384(M, N, K, fast):
    run(M, N, K, ph8(384, fast), bias=True, gate=BF16, seed=220)
    run(M, N, K, ph8(384, fast), out_dt=F32, aux=True, res=BF16, seed=220)


@pytest.mark.parametrize("name", list(EPI))
def test_8ph_epilogues(name):
    """gemm_8ph's staged epilogue on the smallest ragged shape the plan gives it (11 x 12 tiles)"""
    run(2600, 3000, 136, ph8(256, False), seed=230, **EPI[name])


def test_8ph_link2():
    run(6100, 768, 136, ph8(384, False), bias=True, res=F32, link=2, seed=240)


# ---------------------------------------------------------------- gemm_8pp
@pytest.fixture
def persist_on():
    ops = _ops()
    prev = ops.gemm_set_persist(True)
    yield
    ops.gemm_set_persist(prev)


PP = dict(kernel="8pp", persist=True, fast=True, splits=1)


@pytest.mark.parametrize("name", EPI_8PP)
def test_8pp_epilogues(name, persist_on):
    """gemm_8pp on 132 tiles: fewer than workgroups, every epilogue it is eligible for"""
    run(3072, 2816, 128, PP, seed=300, **EPI[name])


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_8pp_layouts(ta, tb, persist_on):
    """252 tiles: a second, partial round of the persistent loop where the chip has fewer CUs"""
    run(5376, 3072, 128, PP, ta=ta, tb=tb, out_dt=BF16 if ta == tb else F32, bias=True, seed=310)


def test_8pp_link2(persist_on):
    run(3072, 2816, 128, PP, bias=True, link=2, seed=320)


# ---------------------------------------------------------------- gemm_4w / gemm_8w through uva_gemm
@pytest.mark.parametrize("out_dt", **DT_IDS)
@pytest.mark.parametrize("M,N,K", [(300, 200, 512), (1000, 776, 384), (4096, 768, 256)])
def test_4w_plain(M, N, K, out_dt):
    """gemm_4w: ragged 256 x 192 tiles, fewer tiles than CUs, whole tiles; bias and alpha"""
    assert _ops().gemm4_plan(M, N, K) is not None
    run(M, N, K, dict(kernel="4w"), out_dt=out_dt, bias=True, alpha=0.5 if out_dt == F32 else -2.0, seed=400)
    run(M, N, K, dict(kernel="4w"), out_dt=out_dt, seed=400)


@pytest.fixture
def gemm8w_on():
    ops = _ops()
    prev = ops.gemm8w_set(on=1, mode=128)
    yield
    ops.gemm8w_set(on=prev[0], mode=prev[1])


@pytest.mark.parametrize("out_dt", **DT_IDS)
@pytest.mark.parametrize("M,N,K", [(300, 200, 512), (1000, 776, 384)])
def test_8w_plain(M, N, K, out_dt, gemm8w_on):
    """gemm_8w's plain form under its measurement switch"""
    run(M, N, K, dict(kernel="8w"), out_dt=out_dt, bias=True, alpha=0.5 if out_dt == F32 else 1.0, seed=410)


DW_CASES = [(304, 200, 512), (1000, 584, 4096)]   # dW needs M % 8 == 0: 300 -> 304


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("M,N,K", DW_CASES)
def test_4w_dw(M, N, K, beta):
    """gemm_4w's dW form (ta = tb = 1, fp32): direct at one slice and beta 0, else slabs + reduce"""
    plan = _ops().gemm4_plan_tt(M, N, K)
    assert plan is not None
    direct = plan[0] == 1 and beta == 0.0
    run(M, N, K, dict(kernel="4w", splits=plan[0], reduce=None if direct else "f32x4"), ta=1, tb=1, out_dt=F32,
        alpha=0.5, beta=beta, seed=420)


@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("M,N,K", DW_CASES)
def test_8w_dw(M, N, K, beta, gemm8w_on):
    run(M, N, K, dict(kernel="8w"), ta=1, tb=1, out_dt=F32, alpha=0.5, beta=beta, seed=420)


def test_ring_link2(gemm8w_on):
    ops = _ops()
    run(1000, 776, 384, dict(kernel="8w"), bias=True, link=2, seed=430)
    ops.gemm8w_set(on=0, mode=0)
    run(1000, 776, 384, dict(kernel="4w"), bias=True, link=2, seed=430)
    run(1000, 584, 4096, dict(kernel="4w"), ta=1, tb=1, out_dt=F32, beta=1.0, link=2, seed=431)
