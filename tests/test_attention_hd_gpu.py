"""Fused bf16 attention at head_dim 128 and 80 (csrc/attention_hd.hip) against fp64 torch on the same bf16
inputs.  The keep mask of the reference comes from oracle/dropmask.py (keep_attn), never from a kernel.

Shapes, for (hd, H) in {(128, 2), (80, 3)} at B 2 (batch * head strides; three heads of 80: the
non-power-of-two head stride): N 64 (a single tile), 192 (an odd tile count: the last 128-wide backward block
is half full), 1088 (17 tiles, the Libero length); p = 0 and p = 0.1.

Bounds.
 forward, per element: |out - ref| <= 2^-8 (|ref| + sum_k |Pd_k v_k|): the two bf16 roundings (P before the PV
   product, the stored output) are a half-ulp of 2^-9 each, with a margin of 2; fp32 accumulation and exp2 are
   orders of magnitude below.
 lse2: 5e-6 max|ref| + 1e-5 (tests/test_attention_gpu.py's bound at head_dim 64).
 backward: dq / dk / dv max-over-max < 3e-2 against autograd of the masked fp64 reference (that file's bound),
   and relative RMS per tensor <= max(1.5e-2, 3 x the error of the same torch attention under bf16 autocast with
   the same mask) (the rule of tests/test_block_dropout_gpu.py); both figures are printed.
 dbias: the fp64 column sums of the stored bf16 dqkv within rows * 2^-24 * sum|terms| (fp32 summation).
 control: the fp64 reference under a mask from another seed misses the backward RMS bound by >= 3 x; with
   columns 64..79 of the head_dim-80 inputs zeroed in the reference the forward bound fails."""
import functools

import pytest
import torch

import dropmask as DM
from edge_helpers import assert_within

pytestmark = pytest.mark.gpu
DEV = "cuda"
FLOOR = 1.5e-2
U8, U24 = 2.0 ** -8, 2.0 ** -24
LN2 = 0.6931471805599453
HEADS = [(128, 2), (80, 3)]
LENGTHS = [64, 192, 1088]
B = 2
SEED, OTHER_SEED = 777, 778
CASES = [(hd, H, N, p) for hd, H in HEADS for N in LENGTHS for p in (0.0, 0.1)]
CASE_IDS = [f"hd{hd}-H{H}-N{N}-p{p}" for hd, H, N, p in CASES]


def _keep_scale(seed, H, N, p, dtype):
    if p == 0.0:
        return None
    th, scale = DM.drop_params(p)
    return torch.from_numpy(DM.keep_attn(seed, B, H, N, th)).to(DEV).to(dtype) * scale


def _heads(t, H, hd, dtype):
    """[B, N, 3*H*hd] -> q, k, v [B, H, N, hd] leaves of `dtype`"""
    t = t.to(dtype).view(t.shape[0], t.shape[1], 3, H, hd).permute(2, 0, 3, 1, 4)
    return [t[i].clone().requires_grad_(True) for i in range(3)]


def _attn(q, k, v, ks, hd, autocast):
    """timm Attention / SDPA in plain torch: softmax(q k^T / sqrt(hd)), dropout by keep * scale, times v"""
    with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
        a = torch.softmax((q * hd ** -0.5) @ k.transpose(-2, -1), dim=-1)
        ad = a if ks is None else (a * ks).to(a.dtype)
        o = ad @ v
    Bq, H, N, _ = q.shape
    return o.transpose(1, 2).reshape(Bq, N, H * hd), ad


def _fwd64(qkv, H, hd, ks):
    """fp64 forward -> (out, the forward bound per element, lse2) with no graph kept"""
    with torch.no_grad():
        q, k, v = _heads(qkv, H, hd, torch.float64)
        s = (q * hd ** -0.5) @ k.transpose(-2, -1)
        lse2 = torch.logsumexp(s, dim=-1) / LN2
        ad = torch.softmax(s, dim=-1)
        if ks is not None:
            ad = ad * ks
        Bq, _, N, _ = q.shape
        out = (ad @ v).transpose(1, 2).reshape(Bq, N, H * hd)
        mag = (ad.abs() @ v.abs()).transpose(1, 2).reshape(Bq, N, H * hd)
    return out, U8 * (out.abs() + mag), lse2


def _grads(qkv, dout, H, hd, ks, dtype):
    q, k, v = _heads(qkv, H, hd, dtype)
    o, _ = _attn(q, k, v, ks, hd, autocast=dtype == torch.float32)
    o.backward(dout.to(o.dtype))
    return [t.grad.double() for t in (q, k, v)]


def _run(qkv, dout, H, hd, N, p, dbias=None, accum=True):
    from unified_video_action_amd.native import ops
    scale = hd ** -0.5
    out = torch.full((B, N, H * hd), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.full((B, H, N), float("nan"), device=DEV)
    mask = ops.attn_fwd_hd(qkv, out, lse, B, N, H, hd, scale, drop_p=p, seed=SEED)
    dqkv = torch.full_like(qkv, float("nan"))
    dvec = torch.empty(B, H, N, device=DEV)
    ops.attn_bwd_hd(qkv, out, dout, lse, dvec, dqkv, B, N, H, hd, scale, drop_p=p, seed=SEED, mask=mask, dbias=dbias,
                    accum_bias=accum)
    torch.cuda.synchronize()
    return out, lse, dqkv


@functools.lru_cache(maxsize=None)
def _case(hd, H, N, p):
    """inputs, one launch of forward + backward, and the references of one case (computed once, read-only)"""
    g = torch.Generator(device="cpu").manual_seed(1000 + hd + N)
    qkv = torch.randn(B, N, 3 * H * hd, generator=g).to(torch.bfloat16).to(DEV)
    dout = torch.randn(B, N, H * hd, generator=g).to(torch.bfloat16).to(DEV)
    out, lse, dqkv = _run(qkv, dout, H, hd, N, p)
    ks = _keep_scale(SEED, H, N, p, torch.float64)
    ref, bound, lse_ref = _fwd64(qkv, H, hd, ks)
    g64 = _grads(qkv, dout, H, hd, ks, torch.float64)
    gbf = _grads(qkv, dout, H, hd, None if ks is None else ks.float(), torch.float32)
    return dict(qkv=qkv, dout=dout, out=out, lse=lse, dqkv=dqkv, ref=ref, bound=bound, lse_ref=lse_ref, g64=g64,
                gbf=gbf)


def _rms(a, ref):
    return ((a.double() - ref).norm() / ref.norm()).item()


def _kernel_grads(dqkv, H, hd):
    d = dqkv.view(dqkv.shape[0], dqkv.shape[1], 3, H, hd)
    return [d[:, :, i].permute(0, 2, 1, 3) for i in range(3)]


@pytest.mark.parametrize("hd,H,N,p", CASES, ids=CASE_IDS)
def test_forward_per_element_and_lse(hd, H, N, p):
    c = _case(hd, H, N, p)
    assert_within(c["out"], c["ref"], c["bound"], "out")
    err = (c["lse"].double() - c["lse_ref"]).abs().max().item()
    print(f"lse2 max error {err:.3e}")
    assert err < 5e-6 * c["lse_ref"].abs().max().item() + 1e-5


@pytest.mark.parametrize("hd,H,N,p", CASES, ids=CASE_IDS)
def test_backward_vs_fp64_autograd(hd, H, N, p):
    c = _case(hd, H, N, p)
    assert not torch.isnan(c["dqkv"].float()).any(), "unwritten dqkv element"
    bounds = []
    for name, got, r64, rbf in zip("qkv", _kernel_grads(c["dqkv"], H, hd), c["g64"], c["gbf"]):
        mx = ((got.double() - r64).abs().max() / (r64.abs().max() + 1e-12)).item()
        e, e_bf = _rms(got, r64), _rms(rbf, r64)
        bound = max(FLOOR, 3.0 * e_bf)
        bounds.append(bound)
        print(f"d{name}: max/max {mx:.3e}; relative RMS torch-bf16 {e_bf:.3e} this build {e:.3e} (bound {bound:.3e})")
        assert mx < 3e-2, (name, mx)
        assert e <= bound, (name, e, bound)
    if p > 0:
        # control: the planes matter -- the fp64 reference under another seed's mask is far outside the bound
        wrong = _grads(c["qkv"], c["dout"], H, hd, _keep_scale(OTHER_SEED, H, N, p, torch.float64), torch.float64)
        for name, w, r64, bound in zip("qkv", wrong, c["g64"], bounds):
            ew = _rms(w, r64)
            print(f"control d{name}: wrong-seed error {ew:.3e} (bound {bound:.3e})")
            assert ew >= 3.0 * bound, (name, ew, bound)


@pytest.mark.parametrize("N", LENGTHS)
def test_forward_sees_the_tail_columns_of_head_dim_80(N):
    """control of the forward bound: against a reference whose inputs have columns 64..79 of every head zeroed
    (what a kernel that stopped after two 32-deep steps, or read stale padding, would compute) the bound fails"""
    hd, H = 80, 3
    c = _case(hd, H, N, 0.1)
    cut = c["qkv"].clone().view(B, N, 3, H, hd)
    cut[..., 64:] = 0
    ref, bound, _ = _fwd64(cut.view(B, N, -1), H, hd, _keep_scale(SEED, H, N, 0.1, torch.float64))
    miss = ((c["out"].double() - ref).abs() > bound).double().mean().item()
    print(f"elements outside the bound against the truncated reference: {miss:.3f}")
    assert miss > 0.15  # the 16 of 80 output columns whose reference (and bound) is exactly zero alone are 0.2


@pytest.mark.parametrize("accum", [True, False], ids=["accum", "set"])
@pytest.mark.parametrize("hd,H,N,p", CASES, ids=CASE_IDS)
def test_dbias_from_epilogue_partials(hd, H, N, p, accum):
    c = _case(hd, H, N, p)
    db = torch.full((3 * H * hd,), 0.75, device=DEV)
    _, _, d1 = _run(c["qkv"], c["dout"], H, hd, N, p, dbias=db, accum=accum)
    assert torch.equal(d1, c["dqkv"]), "dqkv bits differ between dbias = NULL and dbias given"
    cols = c["dqkv"].double().reshape(-1, 3 * H * hd)
    base = 0.75 if accum else 0.0
    assert_within(db, cols.sum(0) + base, B * N * U24 * (cols.abs().sum(0) + base), "dbias")


@pytest.mark.parametrize("hd,H,N,p", [c for c in CASES if c[2] != 64], ids=[i for i in CASE_IDS if "N64" not in i])
def test_bitwise_reproducible(hd, H, N, p):
    c = _case(hd, H, N, p)
    db0 = torch.zeros(3 * H * hd, device=DEV)
    db1 = torch.zeros(3 * H * hd, device=DEV)
    o0, l0, d0 = _run(c["qkv"], c["dout"], H, hd, N, p, dbias=db0, accum=False)
    o1, l1, d1 = _run(c["qkv"], c["dout"], H, hd, N, p, dbias=db1, accum=False)
    for a, b_ in ((o0, o1), (l0, l1), (d0, d1), (db0, db1), (o0, c["out"]), (l0, c["lse"]), (d0, c["dqkv"])):
        assert torch.equal(a, b_)


@pytest.mark.parametrize("hd", [80, 128])
def test_rescale_branch_forced(hd):
    """one spiked key late in the sweep (key 400 of 512, the seventh of eight tiles).  Every query is 1 + 0.5 randn
    per component and the spiked key is a constant vector, so its score in the log2 domain is 14 +- 4 % for every
    query while the other keys' stay below about 3: each row's running max grows by about 11 > 8 in that tile (the
    lazy rescale fires), and the other 511 keys keep a few per cent of the row's mass, so the rescaled partial sums
    still show in the output"""
    from unified_video_action_amd.native import ops
    Bq, N, H = 1, 512, 2
    g = torch.Generator(device="cpu").manual_seed(5)
    qkv = torch.randn(Bq, N, 3, H, hd, generator=g) * 0.5
    qkv[:, :, 0] += 1.0
    qkv[0, 400, 1] = 14.0 / (1.4426950408889634 * hd ** 0.5)
    qkv = qkv.reshape(Bq, N, -1).to(torch.bfloat16).to(DEV)
    out = torch.full((Bq, N, H * hd), float("nan"), device=DEV, dtype=torch.bfloat16)
    lse = torch.empty(Bq, H, N, device=DEV)
    ops.attn_fwd_hd(qkv, out, lse, Bq, N, H, hd, hd ** -0.5)
    ref, bound, lse_ref = _fwd64(qkv, H, hd, None)
    assert_within(out, ref, bound, "out")
    assert (lse.double() - lse_ref).abs().max().item() < 5e-6 * lse_ref.abs().max().item() + 1e-5


def test_refusals_do_not_launch():
    """N = 72, head_dim = 96 and drop_p > 0 without planes each fail in the C ABI before any launch (the outputs
    keep their fill); the Python wrappers refuse the same shapes by assertion"""
    from unified_video_action_amd.native import ops
    from unified_video_action_amd.native.lib import lib
    H = 2
    st = ops.stream()

    def call(N, hd, p):
        qkv = torch.randn(1, N, 3 * H * hd, device=DEV).to(torch.bfloat16)
        out = torch.full((1, N, H * hd), 7.0, device=DEV, dtype=torch.bfloat16)
        lse = torch.full((1, H, N), 7.0, device=DEV)
        dqkv = torch.full_like(qkv, 7.0)
        dvec = torch.full((1, H, N), 7.0, device=DEV)
        with pytest.raises(RuntimeError, match="uva_attn_fwd_hd"):
            lib().call("uva_attn_fwd_hd", qkv.data_ptr(), out.data_ptr(), lse.data_ptr(), None, 1, N, H, hd,
                       hd ** -0.5, p, st)
        with pytest.raises(RuntimeError, match="uva_attn_bwd_hd"):
            lib().call("uva_attn_bwd_hd", qkv.data_ptr(), out.data_ptr(), out.data_ptr(), lse.data_ptr(), None,
                       dvec.data_ptr(), dqkv.data_ptr(), None, 0, None, 1, N, H, hd, hd ** -0.5, p, st)
        torch.cuda.synchronize()
        for t in (out, lse, dqkv, dvec):
            assert (t == 7.0).all()
        return qkv, out, lse

    call(72, 128, 0.0)
    call(72, 80, 0.0)
    call(64, 96, 0.0)
    qkv, out, lse = call(64, 80, 0.1)
    with pytest.raises(AssertionError):
        ops.attn_fwd_hd(torch.empty(1, 72, 3 * H * 80, device=DEV, dtype=torch.bfloat16),
                        torch.empty(1, 72, H * 80, device=DEV, dtype=torch.bfloat16), torch.empty(1, H, 72, device=DEV),
                        1, 72, H, 80, 80 ** -0.5)
    with pytest.raises(AssertionError):
        ops.attn_fwd_hd(torch.empty(1, 64, 3 * H * 96, device=DEV, dtype=torch.bfloat16),
                        torch.empty(1, 64, H * 96, device=DEV, dtype=torch.bfloat16), torch.empty(1, H, 64, device=DEV),
                        1, 64, H, 96, 96 ** -0.5)
