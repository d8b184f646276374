"""Float64 restatement of the DDIM update (uva_ddim_step; gaussian_diffusion.py:543-590 ddim_sample for the eps
model), its schedule coefficients, and the sampling loop over the oracle's SimpleMLPAdaLN.  No GPU code here.

One step, in the kernel's own order (k = the step's fp32 coefficient row {k0, k1, a, b, s}, T = temperature):

    kx  = k0 x
    x0  = kx - k1 eps_model            [clamped to +-1 when clip]
    eps = (kx - x0) / k1               (re-derived: != eps_model where x0 was clipped)
    x'  = a x0 + b eps + s noise T     (the noise term only when s != 0)

with k0 = sqrt(1 / ac), k1 = sqrt(1 / ac - 1), a = sqrt(ac_prev), b = sqrt(max(0, 1 - ac_prev - sigma^2)),
s = sigma [t != 0], sigma = eta sqrt((1 - ac_prev) / (1 - ac)) sqrt(1 - ac / ac_prev), formed in float64 from the
spaced alphas_cumprod and cast once to fp32 (`coef`).

The bound of `ddim_step` is a count of the fp32 roundings of those operations times the magnitudes they act on,
u = 2^-24, as sampler_ref.p_sample derives its own.  Every product and sum is counted as its own rounding; a
multiply-add contraction only removes some, so the bound holds either way:

    kx:   one rounding                                   e_kx  = u |kx|
    x0:   the product k1 eps_model and the difference    e_x0  = e_kx + u |k1 eps_model| + u (|kx| + |k1 eps_model|)
          (the last term bounds u |x0| before the clamp; the clamp is 1-Lipschitz and exact, so e_x0 holds after
          it, also where the fp32 value falls on the other side of +-1 than the float64 one)
    d = kx - x0:  one rounding on inputs off by e_kx, e_x0     e_d = e_kx + e_x0 + u |d|
    eps = d / k1: the division is correctly rounded on this target; counted as 1 ulp = 2 u as the other
          transcendental / division steps of sampler_ref are       e_eps = e_d / |k1| + 2 u |eps|
    a x0, b eps, their sum: three roundings              e_m   = |a| e_x0 + |b| e_eps + 3 u (|a x0| + |b eps|)
    s noise T: two roundings, the last sum one more      e_n   = 3 u |s noise T| + u |x'|

and 1.001 on the total for the second-order terms.  No constant here is fitted to a measured error.
"""
import numpy as np
import torch

from gemm_ref import F64, U

DEFECTS_COEF = ("ac_not_prev", "no_sigma2", "unmasked")
DEFECTS_STEP = ("eps_not_rederived", "temp_on_mean")


def sigma64(ac, ac_prev, eta):
    return eta * np.sqrt((1.0 - ac_prev) / (1.0 - ac)) * np.sqrt(1.0 - ac / ac_prev)


def radicand64(ac, ac_prev, eta):
    s = sigma64(ac, ac_prev, eta)
    return 1.0 - ac_prev - s * s


def coef(ac, ac_prev, eta, nonzero, defect=None):
    """-> [k0, k1, a, b, s] float64 values of the fp32 casts.  ac / ac_prev: float64 scalars of the step;
    nonzero: t != 0.  defect: one of DEFECTS_COEF (the controls)."""
    ac, ac_prev = np.float64(ac), np.float64(ac_prev)
    sg = sigma64(ac, ac_prev, eta)
    a = np.sqrt(ac if defect == "ac_not_prev" else ac_prev)
    rad = 1.0 - ac_prev - (0.0 if defect == "no_sigma2" else sg * sg)
    b = np.sqrt(max(0.0, rad))
    s = sg if (nonzero or defect == "unmasked") else 0.0
    row = [np.sqrt(1.0 / ac), np.sqrt(1.0 / ac - 1.0), a, b, s]
    return [float(np.float32(v)) for v in row]


def schedule(ac, eta):
    """spaced alphas_cumprod [S] (float64) -> the S coefficient rows in loop order (t = S - 1 .. 0)"""
    ac = np.asarray(ac, np.float64)
    ac_prev = np.concatenate([[1.0], ac[:-1]])
    return [coef(ac[t], ac_prev[t], eta, t != 0) for t in reversed(range(len(ac)))]


def ddim_step(eps_model, x, noise, kc, clip, temperature=1.0, defect=None):
    """eps_model / x / noise: float64 tensors holding the kernel's input values (noise may be None when kc[4] == 0);
    kc: 5 floats (fp32 values).  -> (x', per-element bound on |kernel fp32 value - x'|)"""
    k0, k1, a, b, s = (float(np.float32(c)) for c in kc)
    T = float(np.float32(temperature))
    kx = k0 * x
    p = k1 * eps_model
    x0 = kx - p
    e_kx = U * kx.abs()
    e_x0 = e_kx + U * p.abs() + U * (kx.abs() + p.abs())
    if clip:
        x0 = x0.clamp(-1, 1)
    d = kx - x0
    e_d = e_kx + e_x0 + U * d.abs()
    eps = eps_model if defect == "eps_not_rederived" else d / k1
    e_eps = e_d / abs(k1) + 2 * U * eps.abs()
    m = a * x0 + b * eps
    e_m = abs(a) * e_x0 + abs(b) * e_eps + 3 * U * ((a * x0).abs() + (b * eps).abs())
    n = torch.zeros_like(x) if s == 0.0 else s * noise * T
    if defect == "temp_on_mean":
        m = m * T
        n = torch.zeros_like(x) if s == 0.0 else s * noise
    xn = m + n
    return xn, (e_m + 3 * U * n.abs() + U * xn.abs()) * 1.001


def ddim_step32(eps_model, x, noise, kc, clip, temperature=1.0):
    """float32 restatement of ddim_step_kernel, one rounding per operation (no contraction)"""
    f32 = np.float32
    em, xx = eps_model.numpy().astype(f32), x.numpy().astype(f32)
    k0, k1, a, b, s = (f32(c) for c in kc)
    kx = k0 * xx
    x0 = kx - k1 * em
    if clip:
        x0 = np.clip(x0, f32(-1), f32(1))
    eps = (kx - x0) / k1
    xn = a * x0 + b * eps
    if s != 0:
        xn = xn + s * noise.numpy().astype(f32) * f32(temperature)
    assert xn.dtype == np.float32
    return torch.from_numpy(xn.astype(np.float64))


# ------------------------------------------------------------------ the loop over the oracle's network
def oracle_net(C, width, z, depth, state_dict):
    """the oracle's SimpleMLPAdaLN in float64 holding `state_dict`'s values (fp32 or bf16-rounded, exact in float64)"""
    import uva_oracle as O
    net = O.SimpleMLPAdaLN(C, width, 2 * C, z, depth)
    net.load_state_dict({k: v.detach().float().cpu() for k, v in state_dict.items()})
    return net.double().eval()


def net_forward(net, x, t, c):
    """uva_oracle.SimpleMLPAdaLN.forward on float64 rows; the timestep features stay the fp32 values every
    implementation feeds (uva_oracle.timestep_features), widened exactly"""
    import uva_oracle as O
    h = net.input_proj(x)
    y = net.time_embed.mlp(O.timestep_features(t).double()) + net.cond_embed(c)
    for blk in net.res_blocks:
        h = blk(h, y)
    return net.final_layer(h, y)


@torch.no_grad()
def ddim_loop(net, c, noise, step_noise, ac, tmap, eta, clip, temperature=1.0):
    """float64 DDIM loop.  ac: spaced alphas_cumprod [S] float64; tmap: base timestep of every spaced step [S];
    step_noise [S, R, C] or None (eta = 0).  Every step's x is rounded to fp32 as every implementation stores it.
    -> (x after every step [S, R, C] float64, share of x0 elements the clamp changed per step [S])"""
    rows = schedule(ac, eta)
    S = len(rows)
    x = noise.double()
    C = x.shape[1]
    c = c.double()
    traj, shares = [], []
    for k in range(S):
        t = torch.full((x.shape[0],), int(tmap[S - 1 - k]), dtype=torch.long)
        out = net_forward(net, x, t, c)
        em = out[:, :C]
        kc = rows[k]
        raw = kc[0] * x - kc[1] * em
        shares.append(float((raw.abs() > 1).double().mean()) if clip else 0.0)
        nz = None if kc[4] == 0.0 else step_noise[k].double()
        x, _ = ddim_step(em, x, nz, kc, clip, temperature)
        x = x.float().double()
        traj.append(x)
    return torch.stack(traj), shares


def rel_l2(got, ref):
    got, ref = got.double().reshape(-1), ref.double().reshape(-1)
    return float((got - ref).norm() / ref.norm().clamp_min(1e-300))


# ------------------------------------------------------------------ the golden's cases (tests/golden/g9_ddim.npz)
HEADS = {"action": dict(R=16, C=10, clip=True), "video": dict(R=32, C=16, clip=False)}
Z, WIDTH, DEPTH = 768, 1024, 6
SPACINGS = ("ddim10", "10")
ETAS = (0.0, 0.5)
PREFIX = {"action": "ddim_act_net.", "video": "ddim_vid_net."}


def case_key(head, spacing, eta):
    return f"{head}_{spacing}_eta{eta:g}"


_NETS = {}


def golden_net(head, bf16=False):
    """the oracle's float64 net of a golden head with the hash-initialised weights (bf16: the Linear weight matrices
    rounded to bf16 first, as the bf16 compute path reads them; biases and LN affines stay fp32 there); built once,
    read-only"""
    if (head, bf16) not in _NETS:
        import uva_oracle as O
        from hashinit import hash_init_
        C = HEADS[head]["C"]
        net = hash_init_(O.SimpleMLPAdaLN(C, WIDTH, 2 * C, Z, DEPTH), PREFIX[head])
        sd = {k: (v.to(torch.bfloat16) if bf16 and v.dim() == 2 else v) for k, v in net.state_dict().items()}
        _NETS[(head, bf16)] = oracle_net(C, WIDTH, Z, DEPTH, sd)
    return _NETS[(head, bf16)]


_LOOPS = {}


def golden_loop(g, head, spacing, eta, bf16=False):
    """the float64 loop of one golden case (computed once, shared by the tests) -> (trajectory, clamp shares)"""
    key = (head, spacing, eta, bf16)
    if key not in _LOOPS:
        c, noise, sn = golden_inputs(g, head)
        _LOOPS[key] = ddim_loop(golden_net(head, bf16), c, noise, sn, g[f"{spacing}_ac"], g[f"{spacing}_tmap"], eta,
                                HEADS[head]["clip"])
    return _LOOPS[key]


def golden_inputs(g, head):
    """(c, noise, step_noise) of a head as float32 tensors"""
    return tuple(torch.from_numpy(g[f"{head}_{k}"]) for k in ("c", "noise", "step_noise"))
