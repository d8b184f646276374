"""Float64 restatement of the fused attention (csrc/attention.hip, attention_hd.hip, attention_fp8.hip) and
the comparisons of tests/test_attention_exact_gpu.py and tests/test_attention_exact_cpu.py.  Plain torch on
the host, generic in head_dim; keep masks come from oracle/dropmask.py (drop_params, keep_attn) only.

The op, per (batch, head), on the bf16 (or fp8-rounded) inputs, ks = keep * drop scale (1 without dropout):

    S = scale Q K^T;  P = softmax(S);  lse2 = log2 sum exp(S);  Pd = P o ks;  out = Pd V

and the backward as the kernels implement it, O_used being the O the backward reads (the stored bf16 one):

    D = rowsum(dO o O_used);  dP = dO V^T;  dS = P o (ks o dP - D)
    dQ = scale dS K;  dK = scale dS^T Q;  dV = Pd^T dO

With O_used = out this is float64 autograd of the forward (test_attention_exact_cpu.py, 1e-12).

Per-element bounds.  u = 2^-9 is half a bf16 ulp; every bound is a sum of magnitudes in float64 and allows two
such roundings per product chain (the factor 2^-8): the rounded probability (P o keep, or dS) that enters the
MFMA and the stored bf16 output.  fp32 accumulation and exp2 are four orders below.

    B_O  = 2^-8 (|out| + |Pd| |V|)
    dD_q = sum_d |dO_qd| B_O[q, d]          D is computed from the stored O, which carries B_O
    B_dV = 2^-8 (|dV| + |Pd|^T |dO|)
    B_dQ = 2^-8 (|dQ| + scale |dS| |K|) + scale (P o dD) |K|
    B_dK = 2^-8 (|dK| + scale |dS|^T |Q|) + scale (P o dD)^T |Q|
    lse2: 5e-6 max|ref| + 1e-5

The fp8 forward has its own restatement (fp8_forward): its P is rounded to e4m3 against the kernel's lazy
running maximum, which an exact softmax does not describe (3 mantissa bits, subnormal flush).
"""
import math

import numpy as np
import torch

import dropmask as DM

F64 = torch.float64
U8, U24 = 2.0 ** -8, 2.0 ** -24
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
KT = 64  # key tile of every attention kernel


def bf16r(t):
    """round to bf16 (nearest even) and back to float64"""
    return t.to(torch.float32).to(torch.bfloat16).to(F64)


def keep_scale(seed, B, H, N, p):
    """(keep [B, H, N, N] float64 of 0 / 1, drop scale) from the counter hash; (None, 1.0) at p = 0"""
    if p == 0.0:
        return None, 1.0
    th, ds = DM.drop_params(p)
    return torch.from_numpy(DM.keep_attn(seed, B, H, N, th)).to(F64), ds


def heads(qkv, H, hd):
    """[B, N, 3 H hd] (any device / dtype) -> q, k, v [B, H, N, hd] float64 on the host"""
    t = qkv.detach().cpu().to(F64)
    t = t.reshape(t.shape[0], t.shape[1], 3, H, hd).permute(2, 0, 3, 1, 4)
    return t[0].contiguous(), t[1].contiguous(), t[2].contiguous()


def rows(t, H, hd):
    """[B, N, H hd] -> [B, H, N, hd] float64 on the host (out, dout)"""
    t = t.detach().cpu().to(F64)
    return t.reshape(t.shape[0], t.shape[1], H, hd).permute(0, 2, 1, 3).contiguous()


def kernel_grads(dqkv, H, hd):
    """the kernels' dqkv [B, N, 3 H hd] -> dq, dk, dv [B, H, N, hd] float64 on the host"""
    return heads(dqkv, H, hd)


def make_inputs(B, H, N, hd, seed, spread=1.0):
    """(qkv [B, N, 3 H hd], dout [B, N, H hd]) bf16 on the host; Q and K are randn * spread"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, N, 3, H, hd, generator=g)
    x[:, :, :2] *= spread
    dout = torch.randn(B, N, H * hd, generator=g)
    return x.reshape(B, N, 3 * H * hd).to(torch.bfloat16), dout.to(torch.bfloat16)


def forward(q, k, v, scale, keep=None, ds=1.0):
    """-> dict(out, lse2, B_O, P, Pd): exact softmax attention in float64 and the forward bound"""
    S = (q @ k.transpose(-1, -2)) * scale
    lse = torch.logsumexp(S, dim=-1)
    P = torch.exp(S - lse[..., None])
    Pd = P if keep is None else P * keep * ds
    out = Pd @ v
    return dict(out=out, lse2=lse / LN2, B_O=U8 * (out.abs() + Pd.abs() @ v.abs()), P=P, Pd=Pd)


def lse_bound(ref):
    return 5e-6 * ref.abs().max().item() + 1e-5


def backward(q, k, v, do, scale, f, keep=None, ds=1.0, o_used=None, b_o_used=None):
    """the kernels' backward formulas on the forward dict `f` -> dict(dq, dk, dv, B_dq, B_dk, B_dv, D, dD).
    o_used: the O that D is computed from (default: the reference out rounded to bf16); b_o_used: the
    per-element bound of that O against what the kernel stored (default: f["B_O"])."""
    P, Pd = f["P"], f["Pd"]
    o_used = bf16r(f["out"]) if o_used is None else o_used
    b_o = f["B_O"] if b_o_used is None else b_o_used
    D = (do * o_used).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    if keep is not None:
        dP = dP * keep * ds
    dS = P * (dP - D)
    dq, dk, dv = scale * (dS @ k), scale * (dS.transpose(-1, -2) @ q), Pd.transpose(-1, -2) @ do
    dD = (do.abs() * b_o).sum(-1, keepdim=True)
    PdD = P * dD
    aS = dS.abs()
    return dict(dq=dq, dk=dk, dv=dv, D=D, dD=dD,
                B_dq=U8 * (dq.abs() + scale * (aS @ k.abs())) + scale * (PdD @ k.abs()),
                B_dk=(U8 * (dk.abs() + scale * (aS.transpose(-1, -2) @ q.abs()))
                      + scale * (PdD.transpose(-1, -2) @ q.abs())),
                B_dv=U8 * (dv.abs() + Pd.abs().transpose(-1, -2) @ do.abs()))


def reference(qkv, dout, H, hd, seed=0, p=0.0, o_used=None, b_o_used=None, last_tile=True):
    """forward + backward of one case -> one dict (the two above merged, plus q, k, v, do).  last_tile=False
    leaves the last 64-key tile out of every sum over keys (a control: what a dropped tail tile computes)."""
    q, k, v = heads(qkv, H, hd)
    do = rows(dout, H, hd)
    B, _, N, _ = q.shape
    keep, ds = keep_scale(seed, B, H, N, p)
    scale = hd ** -0.5
    if not last_tile:
        f = forward(q, k[:, :, :N - KT], v[:, :, :N - KT], scale, None if keep is None else keep[..., :N - KT], ds)
        pad = lambda t: torch.nn.functional.pad(t, (0, KT))  # noqa: E731
        f["P"], f["Pd"] = pad(f["P"]), pad(f["Pd"])
    else:
        f = forward(q, k, v, scale, keep, ds)
    r = backward(q, k, v, do, scale, f, keep, ds, o_used, b_o_used)
    r.update(f)
    r.update(q=q, k=k, v=v, do=do, scale=scale)
    return r


def ratio(got, ref, bound):
    """max over elements of |got - ref| / bound and the share of elements outside (NaN counts as outside)"""
    err = (got.double().cpu() - ref).abs()
    bad = ~(err <= bound)
    r = (err / bound.clamp_min(1e-300))
    r = torch.where(torch.isnan(r), torch.full_like(r, float("inf")), r)
    return r.max().item(), bad.double().mean().item()


# ---- the bf16 kernels' rounding points, emulated (the bounds' own control) -----------------------------
def emulate_bf16(r, keep=None, ds=1.0):
    """the rounding points of the bf16 kernels in float64 arithmetic: P o keep to bf16 before the PV and dV
    products, dS to bf16 before the dQ / dK products, D from the stored bf16 O, outputs to bf16.
    r: reference() output -> dict(out, dq, dk, dv)"""
    q, k, v, do, scale, P = r["q"], r["k"], r["v"], r["do"], r["scale"], r["P"]
    Pk = bf16r(P if keep is None else P * keep)
    out = bf16r(ds * (Pk @ v))
    D = (do * out).sum(-1, keepdim=True)
    dP = do @ v.transpose(-1, -2)
    if keep is not None:
        dP = dP * keep * ds
    dS = bf16r(P * (dP - D))
    return dict(out=out, dq=bf16r(scale * (dS @ k)), dk=bf16r(scale * (dS.transpose(-1, -2) @ q)),
                dv=bf16r(ds * (Pk.transpose(-1, -2) @ do)))


# ---- softmax-sweep inputs ----------------------------------------------------------------------------
def _const_key(level, hd):
    """component of a constant-vector key whose score against the all-ones query is `level` in the log2
    domain (scale = hd^-1/2): level = a hd hd^-1/2 log2(e)"""
    return level / (LOG2E * hd ** 0.5)


def spiked_inputs(hd, H, N=512, seed=5):
    """one spiked key late in the sweep (key 400): queries 1 + 0.5 randn per component, every other key 0.5 randn,
    the spiked key a constant vector at level 14: each row's running max grows by about 11 > 8 in its tile"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(1, N, 3, H, hd, generator=g) * 0.5
    x[:, :, 0] += 1.0
    x[0, 400, 1] = _const_key(14.0, hd)
    return x.reshape(1, N, 3 * H * hd).to(torch.bfloat16)


RAMP_LEVELS = (4.0, 11.0, 25.0)  # constant-key levels of tiles 0, 1, 2: steps of about 7 and 14


def ramp_inputs(hd, H, N=512, seed=6):
    """the stale-max ramp.  Queries 1 + 0.25 randn per component, so a constant-vector key at level L scores
    L r for a row with r = mean(q) = 1 +- 3 %; every other key 0.5 randn (scores within about +-3).  Tile 0
    holds one key at level 4, tile 1 eight keys at levels 11 - j / 4, tile 2 one key at level 25 whose V row is
    zero.  So per row the tile maxima are 4 r, 11 r, 25 r: tile 1 rises by 7 r < 8 and runs against the stale
    maximum of tile 0 with P up to 2^7, tile 2 rises by 14 r and forces the rescale, and because its key
    carries no V the output (and its bound) is the rescaled mix of the eight tile-1 keys' V rows."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(1, N, 3, H, hd, generator=g) * 0.5
    x[:, :, 0] = 1.0 + 0.5 * x[:, :, 0]
    x[0, 7, 1] = _const_key(RAMP_LEVELS[0], hd)
    for j in range(8):
        x[0, 64 + 5 * j + 3, 1] = _const_key(RAMP_LEVELS[1] - 0.25 * j, hd)
    x[0, 150, 1] = _const_key(RAMP_LEVELS[2], hd)
    x[0, 150, 2] = 0.0
    return x.reshape(1, N, 3 * H * hd).to(torch.bfloat16)


def tile_maxima_log2(qkv, H, hd):
    """[B, H, N, N / 64] float64: per row the maximum score of each 64-key tile in the log2 domain"""
    q, k, _ = heads(qkv, H, hd)
    S = (q @ k.transpose(-1, -2)) * (hd ** -0.5 * LOG2E)
    return S.reshape(*S.shape[:3], -1, KT).amax(-1)


def assert_ramp_steps(qkv, H, hd):
    """the ramp really takes its steps on these (rounded) inputs: tile 1 rises by 6..8 over tile 0 (stale
    maximum, P up to 2^6..2^8), tile 2 by more than 12 over tile 1, no later tile comes near"""
    t = tile_maxima_log2(qkv, H, hd)
    s1, s2 = t[..., 1] - t[..., 0], t[..., 2] - t[..., 1]
    assert 6.0 < s1.min().item() and s1.max().item() < 8.0, (s1.min().item(), s1.max().item())
    assert s2.min().item() > 12.0, s2.min().item()
    assert (t[..., 3:].amax(-1) < t[..., 2] - 12.0).all()
    return s1, s2


# ---- fp8 route ---------------------------------------------------------------------------------------
def fp8_tile_exp(amax):
    """csrc/fp8_scale.h: smallest e with amax 2^-e <= 448, clamped to +-126; 0 for amax = 0"""
    if amax == 0:
        return 0
    f, x = math.frexp(amax)
    return min(max(x - 9 if f * 8 <= 7 else x - 8, -126), 126)


def fp8_round(x):
    """uva_attn_quant_fp8's rounding of qkv [B, N, 3, H, 64] bf16 (host) -> (x~ bf16, e int [B, N/64, 3, H],
    codes float64 [B, N, 3, H, 64] = the e4m3 values x 2^-e rounds to).  Per (b, 64-row tile, q|k|v, head):
    e from the tile's amax, x~ = e4m3_rne(x 2^-e) 2^e.  The scalings are exact in float64 and x 2^-e is exact in
    float32 (a bf16 value moved by a power of two, |x 2^-e| <= 448 and, e being clamped at -126, never below 2^-7)."""
    B, N, _, H, D = x.shape
    xf = x.to(F64).reshape(B, N // KT, KT, 3, H, D)
    amax = xf.abs().amax(dim=(2, 5))
    e = torch.tensor([fp8_tile_exp(a) for a in amax.reshape(-1).tolist()], dtype=torch.int64).reshape(amax.shape)
    s = torch.exp2(e.to(F64))[:, :, None, :, :, None]
    code = (xf / s).to(torch.float32).to(torch.float8_e4m3fn).to(F64)
    xr = (code * s).reshape(B, N, 3, H, D)
    # exact in bf16, but for a code rounded up past the largest bf16 (amax >= 249 * 2^120 rounds to 256 * 2^120 =
    # 2^128): Inf in fp32 and in bf16, as the kernel's fp32 product gives
    xb = xr.to(torch.float32).to(torch.bfloat16)
    assert torch.equal(xb.to(F64)[xr.abs() < 2.0 ** 128], xr[xr.abs() < 2.0 ** 128]), "x~ is not exact in bf16"
    return xb, e, code.reshape(B, N, 3, H, D)


def v8_key_of_pos():
    """position inside a permuted 64-key tile of v8t -> key: position 32 h + 16 s + i holds key
    32 s + (i & 3) + 8 (i >> 2) + 4 h (attention_fp8.hip)"""
    return [32 * s + (i & 3) + 8 * (i >> 2) + 4 * h for h in range(2) for s in range(2) for i in range(16)]


def fp8_forward(xq, H, scale, keep=None, ds=1.0, dtype=F64, exact_p=False, reverse_v=False):
    """the fp8 forward's rounding restated on the rounded inputs xq [B, N, 3 H 64]: per row and 64-key tile,
    scores in `dtype`; the lazy running maximum with its decision in float32 as the kernel takes it
    (mx = fp32(tile max) fp32(c), c = fp32(scale) fp32(log2 e); m <- mx iff mx > m + 8); P8 = e4m3_rne(exp2(s c - m)
    keep); the row sum over the unrounded P; out = ds sum P8 v / rowsum.
    -> dict(out, lse2, mag, maxterm): mag = ds sum_k P8_k |v_k| / rowsum, maxterm = ds max_k P8_k |v_k| / rowsum.
    Controls: exact_p keeps P unrounded; reverse_v reads the V row of key 63 - i for key i of every tile (a key
    permutation error on the V side, what a wrong v8_pos gives: every key moves)."""
    q, k, v = heads(xq, H, 64)
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    B, _, N, _ = q.shape
    c32 = np.float32(scale) * np.float32(LOG2E)
    c = float(c32)
    S = q @ k.transpose(-1, -2)
    m = torch.full((B, H, N), float("-inf"), dtype=torch.float32)
    rs = torch.zeros(B, H, N, dtype=dtype)
    acc = torch.zeros(B, H, N, 64, dtype=dtype)
    mag = torch.zeros(B, H, N, 64, dtype=dtype)
    mt = torch.zeros(B, H, N, 64, dtype=dtype)
    for t in range(N // KT):
        sl = slice(t * KT, (t + 1) * KT)
        st, vt = S[..., sl], v[:, :, sl]
        if reverse_v:
            vt = vt.flip(2)
        mx = st.amax(-1).to(torch.float32) * torch.tensor(c32)
        need = mx > m + 8.0
        mn = torch.where(need, mx, m)
        a = torch.exp2((m - mn).to(dtype))
        m = mn
        p = torch.exp2(st * c - m.to(dtype)[..., None])
        pk = p if keep is None else p * keep[..., sl].to(dtype)
        p8 = pk if exact_p else pk.to(torch.float32).to(torch.float8_e4m3fn).to(dtype)
        rs = rs * a + p.sum(-1)
        acc = acc * a[..., None] + p8 @ vt
        mag = mag * a[..., None] + p8 @ vt.abs()
        mt = torch.maximum(mt * a[..., None], (p8[..., :, None] * vt.abs()[:, :, None, :, :]).amax(-2))
    w = (ds / rs)[..., None]
    return dict(out=(acc * w).to(F64), lse2=(m.to(dtype) + torch.log2(rs)).to(F64), mag=(mag * w).to(F64),
                maxterm=(mt * w).to(F64))


def fp8_bounds(f, N):
    """(tight, loose) per element: tight = 2^-8 |ref| + (N + 64) 2^-24 mag (the stored bf16 output with a margin
    of 2, fp32 accumulation of N products and the rescale factors); loose = tight + 2^-3 maxterm, one e4m3 step
    of the largest term (an exp2 differing in its last bits moves a probability across a rounding boundary)"""
    tight = U8 * f["out"].abs() + (N + 64) * U24 * f["mag"]
    return tight, tight + 0.125 * f["maxterm"]


def fp8_stored_o_bound(got, f, N):
    """per-element bound of the stored fp8 O against O_used = bf16(restated O), for dD of the backward after the
    fp8 forward: the forward bound as the forward check grants it -- tight, and tight + one e4m3 step only on the
    elements that take the step (at most FLIP_CAP of a case, which that check asserts) -- plus the half ulp
    2^-9 |ref| of rounding the restated O to bf16.  Asserts that the stored O is inside it."""
    tight, loose = fp8_bounds(f, N)
    err = (got.double().cpu() - f["out"]).abs()
    b = torch.where(err <= tight, tight, loose)
    assert (err <= b).all(), "stored O outside the forward bound"
    return b + 2.0 ** -9 * f["out"].abs()


FLIP_CAP = 5e-3  # share of a case's elements allowed outside the tight bound (each inside the loose one)


def fp8_compare(got, f, N):
    """-> (share outside tight, worst err / tight among the others, worst err / loose)"""
    tight, loose = fp8_bounds(f, N)
    err = (got.double().cpu() - f["out"]).abs()
    out = ~(err <= tight)
    inside = torch.where(out, torch.zeros_like(err), err / tight.clamp_min(1e-300))
    rl = err / loose.clamp_min(1e-300)
    rl = torch.where(torch.isnan(rl), torch.full_like(rl, float("inf")), rl)
    return out.double().mean().item(), inside.max().item(), rl.max().item()


def assert_fp8_forward(got, f, N, what=""):
    share, worst_in, worst_loose = fp8_compare(got, f, N)
    print(f"{what}: outside tight {share:.5f} (cap {FLIP_CAP}), worst err/tight inside {worst_in:.3f}, "
          f"worst err/(tight + step) {worst_loose:.3f}")
    assert share <= FLIP_CAP, (what, share)
    assert worst_loose <= 1.0, (what, worst_loose)
    return share, worst_in, worst_loose


def fp8_qkv(B, N, H, seed, peak=1.0):
    """the existing fp8 test's inputs (randn * 1.5, Q rows scaled 0.2 .. 3.0 along N: tile-varying ranges) on
    the host, Q and K times `peak` -> [B, N, 3, H, 64] bf16"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, N, 3, H, 64, generator=g) * 1.5
    x[:, :, 0] *= torch.linspace(0.2, 3.0, N)[None, :, None, None]
    x[:, :, :2] *= peak
    return x.to(torch.bfloat16).contiguous()


# ---- the cases both test files run ---------------------------------------------------------------------
SEED, OTHER_SEED = 777, 778
# (B, H, N, p, spread of Q and K) at head_dim 64: one, three and five key tiles, each with a half-empty last
# 128-row block; 6, 12, 18 workgroups; (4, 2, 128): 8 workgroups; p = 0.5: the drop scale is exactly 2
BF16_CASES = ([(2, 3, N, p, 1.0) for N in (64, 192, 320) for p in (0.0, 0.1)]
              + [(2, 3, 320, 0.5, 1.0), (2, 3, 192, 0.1, 2.5), (4, 2, 128, 0.0, 1.0), (4, 2, 128, 0.1, 1.0)])
# (N, p, factor on Q and K) of the fp8 route at (B, H) = (2, 3); 2.5: probabilities flush to e4m3 subnormals
FP8_B, FP8_H = 2, 3
FP8_CASES = [(N, p, 1.0) for N in (64, 192, 320) for p in (0.0, 0.1)] + [(320, 0.1, 2.5)]


def case_id(c):
    return "-".join(str(x) for x in c)


def bf16_case_inputs(B, H, N, p, spread, hd=64):
    return make_inputs(B, H, N, hd, 2000 + N + hd, spread)


def fp8_case_inputs(N, p, peak):
    """-> (x bf16 [B, N, 3, H, 64] before the pass, x~ after it, tile exponents, codes, dout)"""
    x = fp8_qkv(FP8_B, N, FP8_H, 3000 + N, peak)
    xr, e, code = fp8_round(x)
    g = torch.Generator(device="cpu").manual_seed(4000 + N)
    dout = torch.randn(FP8_B, N, FP8_H * 64, generator=g).to(torch.bfloat16)
    return x, xr, e, code, dout
