"""The head_dim-64 bf16 attention (csrc/attention.hip), the fp8 route (csrc/attention_fp8.hip) and the backward of
the head_dim 80 / 128 kernels (csrc/attention_hd.hip), per element against the float64 restatement of
tests/attn_ref.py (bounds and their derivation there; its own controls in tests/test_attention_exact_cpu.py).
Keep masks come from oracle/dropmask.py only.  Every output sits NaN-filled in a sentinel-guarded buffer.

bf16 route, (B, H) = (2, 3), N 64 / 192 / 320 (one, three, five key tiles; a half-empty last 128-row block each;
320 leaves a partial group of four mask tiles; 6 / 12 / 18 workgroups), (4, 2, 128) (8 workgroups), p 0 / 0.1 and
0.5 at N 320: out, lse2, dq, dk, dv inside their bounds, no NaN left, sentinels intact, dqkv bit-equal with and
without dbias, dbias the column sums of the stored dqkv (fp32 summation), a second launch bit-equal.
Softmax sweep at N 512: the spiked key (row max jumps by about 11) and the stale-max ramp (+7, then +14).
fp8 route: the pass on edge tiles (bit-exact against attn_ref.fp8_round), the forward against the restatement
of its own e4m3 rounding, the bf16 backward after it.  Refusals leave every buffer untouched.
"""
import functools

import pytest
import torch

import attn_ref as R
from edge_helpers import BF16, DEV, F32, Guarded, assert_within
from test_attention_hd_gpu import HEADS

pytestmark = pytest.mark.gpu
IDS = [R.case_id(c) for c in R.BF16_CASES]
PAIRS = (("dq", "B_dq"), ("dk", "B_dk"), ("dv", "B_dv"))


def _report(what, got, ref, bound):
    worst, _ = R.ratio(got, ref, bound)
    print(f"{what}: worst error / bound {worst:.3f}")
    assert_within(got, ref, bound, what)


def _run64(qkv, dout, B, H, N, p, dbias=None, accum=True, bwd=True):
    """forward (+ backward) of the head_dim-64 kernels into guarded buffers -> dict of host-checked views"""
    from unified_video_action_amd.native import ops
    g = dict(out=Guarded(B * N, H * 64, BF16), lse=Guarded(B * H, N, F32))
    mask = ops.attn_fwd(qkv, g["out"].view, g["lse"].view, B, N, H, 0.125, drop_p=p, seed=R.SEED)
    for t in g.values():
        t.check()
    if bwd:
        g.update(dvec=Guarded(B * H, N, F32), dqkv=Guarded(B * N, 3 * H * 64, BF16))
        ops.attn_bwd(qkv, g["out"].view, dout, g["lse"].view, g["dvec"].view, g["dqkv"].view, B, N, H, 0.125,
                     drop_p=p, seed=R.SEED, mask=mask, dbias=dbias, accum_bias=accum)
        for t in g.values():
            t.check()
    return {k: t.view for k, t in g.items()}


@functools.lru_cache(maxsize=None)
def _case(case):
    """inputs, one launch and the reference of one bf16 case (computed once, read-only)"""
    B, H, N, p, spread = case
    qkv, dout = R.bf16_case_inputs(*case)
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    got = _run64(qkv, dout, B, H, N, p)
    return dict(qkv=qkv, dout=dout, ref=R.reference(qkv, dout, H, 64, R.SEED, p), **got)


@pytest.mark.parametrize("case", R.BF16_CASES, ids=IDS)
def test_forward_per_element(case):
    B, H, N, p, _ = case
    c = _case(case)
    r = c["ref"]
    _report("out", R.rows(c["out"].view(B, N, H * 64), H, 64), r["out"], r["B_O"])
    err = (c["lse"].view(B, H, N).double().cpu() - r["lse2"]).abs().max().item()
    print(f"lse2: max error {err:.3e} (bound {R.lse_bound(r['lse2']):.3e})")
    assert err < R.lse_bound(r["lse2"])


@pytest.mark.parametrize("case", R.BF16_CASES, ids=IDS)
def test_backward_per_element(case):
    B, H, N, p, _ = case
    c = _case(case)
    r = c["ref"]
    assert not torch.isnan(c["dvec"]).any(), "unwritten D element"
    for (name, bound), got in zip(PAIRS, R.kernel_grads(c["dqkv"].view(B, N, -1), H, 64)):
        _report(name, got, r[name], r[bound])
    if p > 0:  # control on the GPU run's result: the reference under another seed's mask is far outside
        w = R.reference(c["qkv"], c["dout"], H, 64, R.OTHER_SEED, p)
        for (name, bound), got in zip(PAIRS, R.kernel_grads(c["dqkv"].view(B, N, -1), H, 64)):
            _, share = R.ratio(got, w[name], w[bound])
            print(f"control {name}: share outside under another seed's mask {share:.3f}")
            assert share >= 0.3, (name, share)


@pytest.mark.parametrize("accum", [True, False], ids=["accum", "set"])
@pytest.mark.parametrize("case", R.BF16_CASES, ids=IDS)
def test_dbias_and_second_launch(case, accum):
    """dqkv with dbias is bit-equal to dqkv without; dbias is the column sums of the stored dqkv within fp32
    summation of B N rows; this second launch reproduces every output of the first bit for bit"""
    B, H, N, p, _ = case
    c = _case(case)
    gdb = Guarded(1, 3 * H * 64, F32, init=torch.full((3 * H * 64,), 0.75, device=DEV))
    got = _run64(c["qkv"], c["dout"], B, H, N, p, dbias=gdb.view.view(-1), accum=accum)
    gdb.check()
    for k in ("out", "lse", "dqkv", "dvec"):
        assert torch.equal(got[k], c[k]), f"{k} bits differ between launches / with dbias"
    cols = c["dqkv"].double()
    base = 0.75 if accum else 0.0
    assert_within(gdb.view.view(-1), cols.sum(0) + base, B * N * R.U24 * (cols.abs().sum(0) + base), "dbias")


SWEEPS = {"spike": R.spiked_inputs, "ramp": R.ramp_inputs}


@pytest.mark.parametrize("kind", list(SWEEPS))
def test_softmax_sweep_hd64(kind):
    """B 1, H 2, N 512, p 0: the spiked key 400 (the lazy rescale fires late in the sweep) and the stale-max ramp
    (tile 1 runs with P up to 2^7 against tile 0's maximum, tile 2 rescales); the steps are asserted on the
    float64 scores first"""
    H, N = 2, 512
    qkv = SWEEPS[kind](64, H)
    t = R.tile_maxima_log2(qkv, H, 64)
    if kind == "ramp":
        R.assert_ramp_steps(qkv, H, 64)
    else:
        assert (t[..., 6] - t[..., :6].amax(-1)).min().item() > 8.0
    qkv = qkv.to(DEV)
    got = _run64(qkv, None, 1, H, N, 0.0, bwd=False)
    q, k, v = R.heads(qkv, H, 64)
    f = R.forward(q, k, v, 0.125)
    _report(f"{kind} out", R.rows(got["out"].view(1, N, H * 64), H, 64), f["out"], f["B_O"])
    err = (got["lse"].view(1, H, N).double().cpu() - f["lse2"]).abs().max().item()
    print(f"{kind} lse2: max error {err:.3e}")
    assert err < R.lse_bound(f["lse2"])


# ---- head_dim 80 / 128: the backward per element -------------------------------------------------------
HD_CASES = [(hd, H, N, p) for hd, H in HEADS for N in (64, 192) for p in (0.0, 0.1)]


@pytest.mark.parametrize("hd,H,N,p", HD_CASES, ids=[R.case_id(c) for c in HD_CASES])
def test_hd_backward_per_element(hd, H, N, p):
    from unified_video_action_amd.native import ops
    B = 2
    qkv, dout = R.make_inputs(B, H, N, hd, 2000 + N + hd)
    qkv, dout = qkv.to(DEV), dout.to(DEV)
    g = dict(out=Guarded(B * N, H * hd, BF16), lse=Guarded(B * H, N, F32), dvec=Guarded(B * H, N, F32),
             dqkv=Guarded(B * N, 3 * H * hd, BF16))
    mask = ops.attn_fwd_hd(qkv, g["out"].view, g["lse"].view, B, N, H, hd, hd ** -0.5, drop_p=p, seed=R.SEED)
    ops.attn_bwd_hd(qkv, g["out"].view, dout, g["lse"].view, g["dvec"].view, g["dqkv"].view, B, N, H, hd, hd ** -0.5,
                    drop_p=p, seed=R.SEED, mask=mask)
    for t in g.values():
        t.check()
    r = R.reference(qkv, dout, H, hd, R.SEED, p)
    _report("out", R.rows(g["out"].view.view(B, N, H * hd), H, hd), r["out"], r["B_O"])
    for (name, bound), got in zip(PAIRS, R.kernel_grads(g["dqkv"].view.view(B, N, -1), H, hd)):
        _report(name, got, r[name], r[bound])


# ---- fp8 route -----------------------------------------------------------------------------------------
class GuardedBytes:
    """the fp8 workspace (uint8, 256-byte aligned) between two 256-byte runs of 0xA5"""

    def __init__(self, n):
        self.buf = torch.full((256 + n + 256,), 0xA5, dtype=torch.uint8, device=DEV)
        self.view = self.buf[256:256 + n]
        assert self.view.data_ptr() % 256 == 0
        self.n = n

    def check(self):
        torch.cuda.synchronize()
        assert (self.buf[:256] == 0xA5).all() and (self.buf[256 + self.n:] == 0xA5).all(), "write outside the workspace"


def _quant(x):
    """x [B, N, 3, H, 64] bf16 (host) -> (x~ in its guarded buffer, the guarded workspace)"""
    from unified_video_action_amd.native import ops
    B, N, _, H, _ = x.shape
    gx = Guarded(B * N, 3 * H * 64, BF16, init=x.reshape(B * N, -1).to(DEV))
    ws = GuardedBytes(ops.attn_fp8_workspace(B, N, H, DEV).numel())
    ops.attn_quant_fp8(gx.view, ws.view, B, N, H)
    gx.check()
    ws.check()
    return gx, ws


def _assert_pass_outputs(x, gx, ws):
    """the present fp8 test's assertions against attn_ref.fp8_round: the in-place rounding bit-exact, the qk8
    bytes, v8t under the key permutation, the scales"""
    B, N, _, H, _ = x.shape
    xr, e, code = R.fp8_round(x)
    y = gx.view.view(B, N, 3, H, 64).cpu()
    assert torch.equal(y, xr), f"in-place rounding: {(y != xr).sum().item()} elements differ"
    w = ws.view.cpu()
    n8 = B * N * H * 64
    qk8 = w[:2 * n8].view(torch.float8_e4m3fn).to(torch.float64).reshape(B, N, 2, H, 64)
    assert torch.equal(qk8, code[:, :, :2]), "qk8"
    v8t = w[2 * n8:3 * n8].view(torch.float8_e4m3fn).to(torch.float64).reshape(B, H, 64, N // 64, 64)
    key = torch.tensor(R.v8_key_of_pos())
    want = code[:, :, 2].reshape(B, N // 64, 64, H, 64)[:, :, key].permute(0, 3, 4, 1, 2)  # [B, H, d, tile, pos]
    assert torch.equal(v8t, want), "v8t"
    off = (3 * n8 + 255) // 256 * 256
    sc = w[off:off + 4 * B * 3 * H * (N // 64)].view(torch.float32).reshape(B, 3, H, N // 64)
    assert torch.equal(sc.double(), torch.exp2(e.double()).permute(0, 2, 3, 1)), "scales"
    return xr, e


def _edge_tiles():
    """B 1, H 3, N 192: 27 tiles of randn * 1.5; nine of them replaced.  -> (x, {slot: (name, want e)})"""
    B, N, H = 1, 192, 3
    x = (torch.randn(B, N, 3, H, 64, generator=torch.Generator().manual_seed(9)) * 1.5).to(torch.bfloat16)
    g = torch.Generator().manual_seed(10)
    bits = lambda v: torch.tensor([v], dtype=torch.int16).view(torch.bfloat16)[0]  # noqa: E731
    tiles = [("all zero", None, 0)]
    for kexp in (-3, 0, 5):
        a = torch.tensor(448.0 * 2.0 ** kexp, dtype=torch.bfloat16)
        assert float(a) == 448.0 * 2.0 ** kexp
        tiles.append((f"amax 448 * 2^{kexp}", a, kexp))
        nxt = (a.view(torch.int16) + 1).view(torch.bfloat16)
        tiles.append((f"next bf16 above 448 * 2^{kexp}", nxt, kexp + 1))
    tiles.append(("largest finite bf16", bits(0x7F7F), 120))
    tiles.append(("bf16 denormal amax", bits(0x007F), -126))
    slots = {}
    for i, (name, amax, e) in enumerate(tiles):
        rt, t = i % 3, i // 3
        h = (i + t) % 3
        if amax is None:
            tile = torch.zeros(64, 64, dtype=torch.bfloat16)
        elif name.startswith("bf16 denormal"):
            tile = torch.randint(-0x7F, 0x80, (64, 64), generator=g).to(torch.int16)
            tile = torch.where(tile < 0, (-tile) | -0x8000, tile).to(torch.int16).view(torch.bfloat16)
            tile[17, 5] = amax
        else:
            a = float(amax)
            tile = (torch.randn(64, 64, generator=g).double() * (a / 3)).clamp(-a, a).to(torch.bfloat16)
            tile[17, 5] = amax
            tile[40, 63] = -amax
        x[0, rt * 64:(rt + 1) * 64, t, h] = tile
        slots[(rt, t, h)] = (name, e)
    return x, slots


def test_quant_edge_tiles():
    """the pass on tiles at the edges of fp8_tile_exp, all inputs finite: all zero, amax 448 * 2^k and the next bf16
    above it (k -3, 0, 5), the largest finite bf16 (e = 120: elements from 249 * 2^120 up round to 256 * 2^120 = Inf,
    in the kernel's fp32 product as in the restatement), a bf16-denormal amax (the lower clamp, e = -126)"""
    x, slots = _edge_tiles()
    assert torch.isfinite(x.float()).all()
    gx, ws = _quant(x)
    _, e = _assert_pass_outputs(x, gx, ws)
    for (rt, t, h), (name, want) in slots.items():
        assert e[0, rt, t, h].item() == want, (name, e[0, rt, t, h].item(), want)
    y = gx.view.view(1, 192, 3, 3, 64).cpu()
    # an amax on the e4m3 grid survives; one bf16 above 448 * 2^k rounds back to 448 * 2^k
    for (rt, t, h), (name, want) in slots.items():
        tile = y[0, rt * 64:(rt + 1) * 64, t, h].double()
        if name.startswith(("amax 448", "next bf16")):
            assert tile.abs().max().item() == 448.0 * 2.0 ** (want if name.startswith("amax") else want - 1), name
        if name.startswith("bf16 denormal"):  # k 2^-133 * 2^126 = k 2^-7 on the e4m3 grid: the amax 127 -> 128
            assert tile.abs().max().item() == 2.0 ** -126 and (tile != 0).any(), name


FP8_ALL = R.FP8_CASES + ["ramp"]
FP8_IDS = [c if isinstance(c, str) else R.case_id(c) for c in FP8_ALL]


@functools.lru_cache(maxsize=None)
def _fp8_case(case):
    """pass + forward of one fp8 case on the GPU and its restatement (computed once, read-only)"""
    from unified_video_action_amd.native import ops
    if case == "ramp":
        B, H, N, p = 1, 2, 512, 0.0
        x = R.ramp_inputs(64, H).reshape(B, N, 3, H, 64)
        dout = None
    else:
        N, p, peak = case
        B, H = R.FP8_B, R.FP8_H
        x, _, _, _, dout = R.fp8_case_inputs(*case)
    gx, ws = _quant(x)
    xr, _ = _assert_pass_outputs(x, gx, ws)
    go, gl = Guarded(B * N, H * 64, BF16), Guarded(B * H, N, F32)
    mask = ops.attn_fwd_fp8(ws.view, go.view, gl.view, B, N, H, 0.125, drop_p=p, seed=R.SEED)
    for t in (go, gl, ws, gx):
        t.check()
    keep, ds = R.keep_scale(R.SEED, B, H, N, p)
    f = R.fp8_forward(xr, H, 0.125, keep, ds)
    return dict(B=B, H=H, N=N, p=p, xr=xr, gx=gx, out=go.view, lse=gl.view, mask=mask, f=f, dout=dout)


@pytest.mark.parametrize("case", FP8_ALL, ids=FP8_IDS)
def test_fp8_forward_against_its_rounding(case):
    """out within the tight bound but for at most 0.5 % of a case's elements, those within one e4m3 step more.
    MI355X: 0.0000-0.0008 outside (0.0032 on the ramp), worst 0.24 of tight + step.  With Q K^T on the fp8 MFMA
    (which drops what lies 16 bits below its largest product) the share was 0.0083-0.0096 at N 192 / 320: the
    forward forms S on the bf16 MFMA over the e4m3 codes since."""
    c = _fp8_case(case)
    if case == "ramp":
        R.assert_ramp_steps(c["xr"], c["H"], 64)
    got = R.rows(c["out"].view(c["B"], c["N"], c["H"] * 64), c["H"], 64)
    assert not torch.isnan(got).any(), "unwritten output element"
    R.assert_fp8_forward(got, c["f"], c["N"], "fp8 out")


@pytest.mark.parametrize("case", FP8_ALL, ids=FP8_IDS)
def test_fp8_forward_lse2(case):
    """lse2 against the restatement's, at the bf16 route's bound 5e-6 max|ref| + 1e-5.  MI355X: 1.2e-6 .. 2.2e-6
    (1.1e-5 in the peaked case, lse2 up to 178), the bf16 kernel's own figures on the same x~; with Q K^T on the
    fp8 MFMA it was 3.2e-4 .. 5.9e-4 (4.1e-3 peaked), outside the bound."""
    c = _fp8_case(case)
    f = c["f"]
    err = (c["lse"].view(c["B"], c["H"], c["N"]).double().cpu() - f["lse2"]).abs().max().item()
    print(f"fp8 lse2: max error {err:.3e} (bound {R.lse_bound(f['lse2']):.3e})")
    assert err < R.lse_bound(f["lse2"])


@pytest.mark.parametrize("case", FP8_ALL, ids=FP8_IDS)
def test_fp8_forward_controls(case):
    """on the GPU run's result: each wrong restatement leaves at least 30 % of the elements outside the tight
    bound, in every case; the V-side one is a key permutation of every tile (i <-> 63 - i), as a v8_pos error gives"""
    c = _fp8_case(case)
    B, H, N, p = c["B"], c["H"], c["N"], c["p"]
    got = R.rows(c["out"].view(B, N, H * 64), H, 64)
    keep, ds = R.keep_scale(R.SEED, B, H, N, p)
    wrong = {"exact P": R.fp8_forward(c["xr"], H, 0.125, keep, ds, exact_p=True)}
    wrong["V keys i and 63 - i exchanged"] = R.fp8_forward(c["xr"], H, 0.125, keep, ds, reverse_v=True)
    if p > 0:
        wrong["another seed's mask"] = R.fp8_forward(c["xr"], H, 0.125, R.keep_scale(R.OTHER_SEED, B, H, N, p)[0], ds)
    for name, w in wrong.items():
        share, _, _ = R.fp8_compare(got, w, N)
        print(f"control {name}: outside tight {share:.3f}")
        assert share >= 0.3, (name, share)


FP8_BWD = [c for c in R.FP8_CASES if c[0] in (192, 320) and c[2] == 1.0]


@pytest.mark.parametrize("case", FP8_BWD, ids=[R.case_id(c) for c in FP8_BWD])
def test_backward_after_fp8_forward(case):
    """what fp8_attn training runs: the bf16 backward on x~ with the fp8 forward's lse2, O and mask -- the
    straight-through gradient: exact P of x~, D from the fp8 O.  O_used is the restated fp8 O rounded to bf16 and
    dD is built from the fp8 forward bound as the forward check grants it (attn_ref.fp8_stored_o_bound: tight, and
    the one-e4m3-step allowance only on the elements that take it).  Control: the reference under another seed's
    mask leaves at least 30 % of each of dq, dk, dv outside"""
    from unified_video_action_amd.native import ops
    c = _fp8_case(case)
    B, H, N, p, f = c["B"], c["H"], c["N"], c["p"], c["f"]
    dout = c["dout"].to(DEV)
    gd, gq = Guarded(B * H, N, F32), Guarded(B * N, 3 * H * 64, BF16)
    ops.attn_bwd(c["gx"].view, c["out"], dout, c["lse"], gd.view, gq.view, B, N, H, 0.125, drop_p=p, seed=R.SEED,
                 mask=c["mask"])
    gd.check()
    gq.check()
    b_o = R.fp8_stored_o_bound(R.rows(c["out"].view(B, N, H * 64), H, 64), f, N)
    r = R.reference(c["xr"], dout, H, 64, R.SEED, p, o_used=R.bf16r(f["out"]), b_o_used=b_o)
    grads = R.kernel_grads(gq.view.view(B, N, -1), H, 64)
    for (name, bound), got in zip(PAIRS, grads):
        _report(f"fp8 route {name}", got, r[name], r[bound])
    if p > 0:
        w = R.reference(c["xr"], dout, H, 64, R.OTHER_SEED, p, o_used=R.bf16r(f["out"]), b_o_used=b_o)
        for (name, bound), got in zip(PAIRS, grads):
            _, share = R.ratio(got, w[name], w[bound])
            print(f"control {name}: share outside under another seed's mask {share:.3f}")
            assert share >= 0.3, (name, share)


# ---- refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,p", [(72, 0.0), (64, 0.1)], ids=["N72", "p0.1-null-mask"])
def test_refusals_do_not_launch(N, p):
    """N = 72, and drop_p > 0 with a null mask, fail in the C ABI before any launch: every buffer keeps its fill.
    uva_attn_quant_fp8 takes no drop_p: it refuses N = 72 only"""
    from unified_video_action_amd.native import ops
    from unified_video_action_amd.native.lib import lib
    H = 2
    st = ops.stream()
    fill = lambda *s, dtype=BF16: torch.full(s, 7.0, device=DEV, dtype=dtype)  # noqa: E731
    qkv, out, dout, dqkv = fill(1, N, 3 * H * 64), fill(1, N, H * 64), fill(1, N, H * 64), fill(1, N, 3 * H * 64)
    lse, dvec = fill(1, H, N, dtype=F32), fill(1, H, N, dtype=F32)
    ws = torch.full((lib().query("uva_attn_fp8_workspace", 1, 128, H),), 7, dtype=torch.uint8, device=DEV)
    assert ws.data_ptr() % 256 == 0
    P = lambda t: t.data_ptr()  # noqa: E731
    with pytest.raises(RuntimeError, match="uva_attn_fwd failed"):
        lib().call("uva_attn_fwd", P(qkv), P(out), P(lse), None, 1, N, H, 0.125, p, st)
    with pytest.raises(RuntimeError, match="uva_attn_bwd failed"):
        lib().call("uva_attn_bwd", P(qkv), P(out), P(dout), P(lse), None, P(dvec), P(dqkv), None, 1, N, H, 0.125, p, st)
    with pytest.raises(RuntimeError, match="uva_attn_fwd_fp8 failed"):
        lib().call("uva_attn_fwd_fp8", P(ws), P(out), P(lse), None, 1, N, H, 0.125, p, st)
    if p == 0.0:
        with pytest.raises(RuntimeError, match="uva_attn_quant_fp8 failed"):
            lib().call("uva_attn_quant_fp8", P(qkv), P(ws), 1, N, H, st)
    torch.cuda.synchronize()
    for t in (qkv, out, dout, dqkv, lse, dvec, ws):
        assert (t == 7).all()
