"""DDIM sampling on the GPU: uva_ddim_step per element against tests/ddim_ref.py (strided NaN-filled `out` with a NaN
variance half, sentinel-guarded outputs, aliasing, x_net dtypes, the launcher's refusals), ActionSampler(method=
"ddim") eager against captured graph, eta = 0 determinism, the loop against the reference's DDIM run
(tests/golden/g9_ddim.npz) in fp32 and bf16, and the plumbing through the heads, MAR.sample_tokens and the policy."""
from functools import partial

import pytest
import torch
import torch.nn as nn

import cases
import ddim_ref as dr
import replay
from edge_helpers import DEV, Guarded, assert_within
from gemm_ref import BF16, F32, gen
from hashinit import hash_init_, hash_normal

pytestmark = pytest.mark.gpu
RATIO = {}


def _ops():
    from unified_video_action_amd.native import ops
    return ops


def _precision(name):
    from unified_video_action_amd.runtime import RT
    RT.set_precision(name)


# ------------------------------------------------------------------ uva_ddim_step
# (ac, ac_prev, t != 0, eta): a middle step at eta 0 / 0.5 / 1, and the t = 0 step of the schedule (ac_prev = 1)
KINDS = [(0.30, 0.55, True, 0.0), (0.30, 0.55, True, 0.5), (0.30, 0.55, True, 1.0), (0.99995, 1.0, False, 0.5)]


def _step_case(rows, C, odt):
    g = gen(90 + rows + C)
    em = torch.randn(rows, C, generator=g).to(odt).double()
    x = (torch.randn(rows, C, generator=g) * 0.6).float().double()
    noise = torch.randn(rows, C, generator=g).float().double()
    return em, x, noise


@pytest.mark.parametrize("odt", [F32, BF16])
@pytest.mark.parametrize("C", [2, 9, 16])
@pytest.mark.parametrize("rows", [1, 17, 257])
def test_ddim_step(rows, C, odt):
    ops = _ops()
    em, x, noise = _step_case(rows, C, odt)
    # ld_out = 2C + 6 > 2C inside a NaN-filled buffer; the variance half is NaN too: it must not be read
    wide = torch.full((rows, 2 * C + 6), float("nan"), dtype=odt, device=DEV)
    wide[:, 2:2 + C] = em.to(odt)
    out = wide[:, 2:2 * C + 2]
    nd = noise.float().to(DEV)
    T = 0.95
    for ac, ac_prev, nonzero, eta in KINDS:
        kc = dr.coef(ac, ac_prev, eta, nonzero)
        for clip in (True, False):
            ref, b = dr.ddim_step(em, x, noise, kc, clip, T)
            # x_new apart from x / aliasing x; x_net bf16 / fp32 / absent; noise absent where s == 0
            for inplace, ndt in ((False, BF16), (True, F32), (True, None), (False, None)):
                xd = x.float().to(DEV)
                fresh = Guarded(rows, C, F32)
                net = None if ndt is None else Guarded(rows, C, ndt)
                xn = xd if inplace else fresh.view
                nz = None if (kc[4] == 0.0 and inplace) else nd
                ops.ddim_step(out, xd, nz, kc + [T], xn, None if net is None else net.view, clip=clip)
                fresh.check()
                what = f"ddim rows {rows} C {C} {odt} kind {(ac, eta)} clip {clip} inplace {inplace}"
                assert_within(xn.cpu(), ref, b, what)
                if net is not None:
                    net.check()
                    assert torch.equal(net.view, xn.to(ndt)), what  # the stored x_new rounded once, to nearest even
                if not inplace:
                    assert torch.equal(xd.cpu(), x.float())
                e = (xn.cpu().double() - ref).abs() / b.clamp_min(1e-300)
                RATIO["ddim_step"] = max(RATIO.get("ddim_step", 0.0), float(e.max()))


def test_ddim_step_clip_marks_and_x_net_ties():
    """dyadic coefficients and operands on the grid 1/256: every operation is exact, so x_new is bit-equal to float64,
    with x0 exactly at, just inside and just outside +-1, and x_net = its bf16 rounding with exact ties among them"""
    rows, C = 257, 9
    g = gen(5)
    em = torch.randint(-512, 513, (rows, C), generator=g).double() / 256
    x = torch.randint(-512, 513, (rows, C), generator=g).double() / 256
    marks = [(0.5, -1.0), (-0.5, 1.0), (0.5, -1.0 + 2.0 ** -7), (0.5, -1.0 - 2.0 ** -7), (-0.5, 1.0 - 2.0 ** -7),
             (-0.5, 1.0 + 2.0 ** -7)]  # kc: x0 = x - eps / 2
    for i, (xv, ev) in enumerate(marks):
        x.view(-1)[i], em.view(-1)[i] = xv, ev
    kc = [1.0, 0.5, 0.75, 0.25, 0.0]
    for clip in (True, False):
        ref, _ = dr.ddim_step(em, x, None, kc, clip)
        assert torch.equal(ref.float().double(), ref)
        near = ref.float().to(BF16).double()
        half_ulp = torch.exp2(torch.frexp(ref.abs().clamp_min(2.0 ** -20))[1].double() - 9)  # bf16: 8 significant bits
        assert int(((ref - near).abs() == half_ulp).sum()) >= 8  # exact ties among the values that need rounding
        xn, net = Guarded(rows, C, F32), Guarded(rows, C, BF16)
        out = torch.cat([em.float(), torch.full((rows, C), float("nan"))], 1).to(DEV)
        _ops().ddim_step(out, x.float().to(DEV), None, kc + [1.0], xn.view, net.view, clip=clip)
        xn.check(), net.check()
        assert torch.equal(xn.view.cpu().double(), ref)
        assert torch.equal(net.view.cpu(), ref.float().to(BF16))


def _raw(**over):
    from unified_video_action_amd.native.lib import lib
    import ctypes
    rows, C = 4, 10
    t = dict(out=torch.zeros(rows, 2 * C, device=DEV), x=torch.zeros(rows, C, device=DEV),
             noise=torch.zeros(rows, C, device=DEV), x_new=torch.full((rows, C), 7.0, device=DEV))
    k = (ctypes.c_float * 6)(*over.pop("coef", [1.0, 0.5, 0.75, 0.25, 0.5, 1.0]))
    a = dict(odt=0, out=t["out"].data_ptr(), ld_out=2 * C, x=t["x"].data_ptr(), noise=t["noise"].data_ptr(),
             coef=ctypes.cast(k, ctypes.c_void_p), x_new=t["x_new"].data_ptr(), xdt=0, x_net=None, clip=1, rows=rows,
             C=C)
    a.update(over)
    try:
        lib().call("uva_ddim_step", *a.values(), torch.cuda.current_stream().cuda_stream)
    finally:
        torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("over", [dict(rows=0), dict(rows=-1), dict(C=0), dict(C=-2), dict(ld_out=19), dict(noise=None)],
                         ids=lambda d: ",".join(f"{k}={v}" for k, v in d.items()))
def test_ddim_step_refusals(over):
    assert bool((_raw()["x_new"] == 0).all())  # the same call without the override launches
    with pytest.raises(RuntimeError):
        _raw(**over)
    _raw(noise=None, coef=[1.0, 0.5, 0.75, 0.25, 0.0, 1.0])  # s == 0: a null noise is legal


def test_ops_ddim_step_argument_checks():
    ops = _ops()
    x = torch.zeros(4, 10, device=DEV)
    out = torch.zeros(4, 20, device=DEV)
    kc = [1.0, 0.5, 0.75, 0.25, 0.5, 1.0]
    with pytest.raises(RuntimeError):  # ld_out < 2C through the wrapper, as ops.p_sample_step
        ops.ddim_step(torch.zeros(80, device=DEV).as_strided((4, 20), (10, 1)), x, x.clone(), kc, x.clone())
    for bad in (lambda: ops.ddim_step(out[:, :18], x, x.clone(), kc, x.clone()),
                lambda: ops.ddim_step(out, x, x.clone().to(BF16), kc, x.clone()),
                lambda: ops.ddim_step(out, x, x.clone(), kc, x.clone()[:, :5]),
                lambda: ops.ddim_step(out, x, x.clone(), kc, x.clone(), torch.zeros(4, 12, device=DEV)[:, :10]),
                lambda: ops.ddim_step(out, x, None, kc, x.clone()),
                lambda: ops.ddim_step(out, x, x.clone(), kc[:5], x.clone())):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------ the loop on the golden's two heads
_HEAD = {}


def _head(head):
    """(product net on the device, c, noise, step_noise) of a golden head; built once"""
    if head not in _HEAD:
        from unified_video_action_amd.model.autoregressive.diffusion_loss import SimpleMLPAdaLN
        C = dr.HEADS[head]["C"]
        net = hash_init_(SimpleMLPAdaLN(C, dr.WIDTH, 2 * C, dr.Z, dr.DEPTH), dr.PREFIX[head]).to(DEV).eval()
        g = replay.load("g9_ddim.npz")
        _HEAD[head] = (net,) + tuple(t.to(DEV) for t in dr.golden_inputs(g, head))
    return _HEAD[head]


def _sampler(head, spacing, eta, **kw):
    from unified_video_action_amd.model.autoregressive.sampler import ActionSampler
    return ActionSampler(_head(head)[0], spacing, clip_denoised=dr.HEADS[head]["clip"], method="ddim", eta=eta, **kw)


@pytest.mark.parametrize("eta", dr.ETAS)
@pytest.mark.parametrize("head", list(dr.HEADS))
def test_ddim_graph_matches_eager_and_reuses_capture(head, eta):
    net, c, noise, sn = _head(head)
    graph = _sampler(head, "ddim10", eta)
    a = graph(c, noise, sn, 0.95)
    st = graph._cache
    assert st["graph"] is not None and st["persist"] is False  # DDIM: never the persistent kernel, R = 16 included
    n2 = noise.flip(0).contiguous()
    b = graph(c, n2, sn, 0.95)
    assert graph._cache is st and st["graph"] is not None
    eager = _sampler(head, "ddim10", eta, use_graph=False)
    assert torch.equal(a, eager(c, noise, sn, 0.95)) and torch.equal(b, eager(c, n2, sn, 0.95))
    assert eager._cache["graph"] is None
    assert not torch.equal(a, b) and torch.isfinite(a).all()
    assert (st["noise"] is None) == (eta == 0.0)


@pytest.mark.parametrize("head", list(dr.HEADS))
def test_ddim_eta0_is_deterministic_and_ignores_step_noise(head):
    net, c, noise, sn = _head(head)
    s = _sampler(head, "10", 0.0)
    a = s(c, noise, None, 0.95)
    assert torch.equal(a, s(c, noise, None, 0.95))
    assert torch.equal(a, s(c, noise, torch.full_like(sn, float("nan")), 0.5))  # nor on the temperature
    assert torch.isfinite(a).all()
    with pytest.raises(ValueError):
        _sampler(head, "10", 0.5)(c, noise, None, 0.95)


@pytest.mark.parametrize("eta", dr.ETAS)
@pytest.mark.parametrize("spacing", dr.SPACINGS)
@pytest.mark.parametrize("head", list(dr.HEADS))
def test_ddim_fp32_vs_reference(head, spacing, eta):
    """fp32 precision mode against the final x_0 of the reference's fp32 DDIM run: relative L2 <= 1e-4"""
    g = replay.load("g9_ddim.npz")
    net, c, noise, sn = _head(head)
    _precision("fp32")
    try:
        x = _sampler(head, spacing, eta)(c, noise, sn, 1.0).cpu()
    finally:
        _precision("bf16")
    e = dr.rel_l2(x, torch.from_numpy(g[f"{dr.case_key(head, spacing, eta)}_x"][-1]))
    print(f"{dr.case_key(head, spacing, eta)}: fp32 rel L2 {e:.3e}")
    assert e <= 1e-4, e


@pytest.mark.parametrize("eta", dr.ETAS)
@pytest.mark.parametrize("spacing", dr.SPACINGS)
@pytest.mark.parametrize("head", list(dr.HEADS))
def test_ddim_bf16_within_3x_the_references_own_bf16_error(head, spacing, eta):
    """the standing bf16 rule: the error against the float64 loop on the same bf16-rounded weights is at most 3x the
    deviation of the reference's own bf16-autocast run from its fp32 run (both relative L2 of the final x_0)"""
    g = replay.load("g9_ddim.npz")
    key = dr.case_key(head, spacing, eta)
    net, c, noise, sn = _head(head)
    _precision("bf16")
    x = _sampler(head, spacing, eta)(c, noise, sn, 1.0).cpu()
    want = dr.golden_loop(g, head, spacing, eta, bf16=True)[0][-1]
    ours = dr.rel_l2(x, want)
    theirs = dr.rel_l2(torch.from_numpy(g[f"{key}_x0_bf16"]), torch.from_numpy(g[f"{key}_x"][-1]))
    print(f"{key}: bf16 rel L2 {ours:.3e}; the reference's own bf16 deviation {theirs:.3e}")
    assert torch.isfinite(x).all()
    assert ours <= 3.0 * theirs, (ours, theirs)


# ------------------------------------------------------------------ heads, MAR, policy
class _Count:
    def __init__(self, monkeypatch):
        ops = _ops()
        self.n = {"ddim_step": 0, "p_sample_step": 0}
        for name in self.n:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def f(*a, **k):
            self.n[name] += 1
            return fn(*a, **k)
        return f


class _Draws:
    """records the shape of every torch.randn draw"""

    def __init__(self, monkeypatch):
        self.shapes = []
        real = torch.randn

        def f(*shape, **k):
            self.shapes.append(tuple(shape[0]) if len(shape) == 1 and not isinstance(shape[0], int) else tuple(shape))
            return real(*shape, **k)
        monkeypatch.setattr(torch, "randn", f)


def test_heads_reach_ddim_step(monkeypatch):
    from unified_video_action_amd.model.autoregressive.diffusion_action_loss import DiffActLoss
    from unified_video_action_amd.model.autoregressive.diffusion_loss import DiffLoss
    cnt, draws = _Count(monkeypatch), _Draws(monkeypatch)
    act = DiffActLoss(2, 64, 2, 64, "100", n_frames=4, act_diff_testing_steps="ddim10", act_sampler="ddim")
    act = hash_init_(act, "act_conv_fc.").to(DEV).eval()
    z = torch.from_numpy(hash_normal("act_conv_fc/z", (2, 1024, 64))).to(DEV)
    x = act.sample(z)
    assert x.shape == (2, 16, 2) and torch.isfinite(x).all() and float(x.abs().max()) <= 1.0
    assert act._sampler.method == "ddim" and act._sampler.eta == 0.0 and act._sampler.sched.S == 10
    assert cnt.n == {"ddim_step": 10, "p_sample_step": 0}  # one eager step + nine captured
    assert draws.shapes == [(32, 2)]  # x_T only: no per-step noise at eta = 0
    # injected draws are still accepted; eta = 0 ignores the per-step ones
    nz = torch.randn(32, 2, device=DEV)
    assert torch.equal(act.sample(z, noise=nz), act.sample(z, noise=nz, step_noise=torch.full((10, 32, 2), float("nan"))))

    vid = DiffLoss(16, 64, 2, 64, "ddim10", video_sampler="ddim", video_ddim_eta=0.5)
    vid = hash_init_(vid, "vid.").to(DEV).eval()
    cnt.n["ddim_step"], draws.shapes[:] = 0, []
    zr = torch.from_numpy(hash_normal("vid/z", (40, 64))).to(DEV)
    y = vid.sample(zr)
    assert y.shape == (40, 16) and torch.isfinite(y).all()
    assert vid._sampler.method == "ddim" and vid._sampler.eta == 0.5 and not vid._sampler.clip
    assert cnt.n == {"ddim_step": 10, "p_sample_step": 0}
    assert draws.shapes == [(40, 16), (10, 40, 16)]  # eta > 0 draws the per-step noise
    sn = torch.randn(10, 40, 16, device=DEV)
    n0 = torch.randn(40, 16, device=DEV)
    assert torch.equal(vid.sample(zr, noise=n0, step_noise=sn), vid.sample(zr, noise=n0, step_noise=sn))
    assert not torch.equal(vid.sample(zr, noise=n0, step_noise=sn), vid.sample(zr, noise=n0, step_noise=sn.flip(0)))


def test_sample_tokens_video_mode_with_ddim(monkeypatch):
    """the MaskGIT loop with video_sampler = ddim at eta = 0 on the smallest golden MAR: the video head runs
    uva_ddim_step and draws no per-step noise; the action head, left at its default, still draws its own"""
    from unified_video_action_amd.model.autoregressive.mar_con_unified import MAR
    kw = dict(cases.mar_kwargs("pusht"), num_sampling_steps="ddim10", video_sampler="ddim")
    m = hash_init_(MAR(norm_layer=partial(nn.LayerNorm, eps=1e-6), **cases.MAR_GOLDEN, **kw), "mar.").to(DEV).eval()
    assert m.diffloss.video_sampler == "ddim" and m.diffactloss.act_sampler == "ddpm"
    inp = {k: torch.from_numpy(x).to(DEV) for k, x in cases.mar_inputs("pusht").items()}
    cnt, draws = _Count(monkeypatch), _Draws(monkeypatch)
    tok, act = m.sample_tokens(bsz=cases.B_MAR, cond=inp["c"], num_iter=cases.VIDEO_SAMPLE_ITERS, cfg=1.0,
                               temperature=cases.SAMPLE_TEMPERATURE, task_mode="video_model",
                               rng={"orders": cases.sample_rng("pusht")["orders"]})
    assert torch.isfinite(tok).all() and torch.isfinite(act).all()
    assert m.diffloss._sampler.method == "ddim" and m.diffactloss._sampler.method == "ddpm"
    assert cnt.n["ddim_step"] >= 10 and cnt.n["p_sample_step"] >= 100
    three = [s for s in draws.shapes if len(s) == 3]
    assert three and all(s[2] == 2 for s in three), three  # per-step draws of the action head (Da = 2) only
    assert any(len(s) == 2 and s[1] == 16 for s in draws.shapes)  # the video head's x_T


def test_policy_keys_and_the_default_route():
    from unified_video_action_amd.model.autoregressive import mar_con_unified as pmar
    from unified_video_action_amd.model.common.normalizer import LinearNormalizer
    from unified_video_action_amd.policy.unified_video_action_policy import UnifiedVideoActionPolicy
    pmar.mar_golden = lambda **kw: pmar.MAR(norm_layer=partial(nn.LayerNorm, eps=1e-6), **cases.MAR_GOLDEN, **kw)

    def policy(**keys):
        amp = dict(pretrained_model_path=None, model_size="mar_golden", num_iter=1, cfg=1, cfg_schedule="linear",
                   temperature=cases.SAMPLE_TEMPERATURE)
        amp.update({k: cases.MAR_KW[k] for k in cases.POLICY_AMP_KEYS})
        amp.update(diffloss_act_d=6, diffloss_act_w=1024)  # the production action head: the persistent route's shape
        amp.update(keys)
        pol = UnifiedVideoActionPolicy(
            vae_model_params=dict(autoencoder_path=None, ddconfig=dict(vae_embed_dim=16, ch_mult=[1, 1, 2, 2, 4])),
            autoregressive_model_params=amp, action_model_params=dict(predict_action=True, act_model_type="conv_fc"),
            shape_meta={"action": {"shape": [2]}}, n_action_steps=8, shift_action=True, language_emb_model=None,
            task_name="pusht", task_modes=[], normalizer_type="all", selected_training_mode=None,
            use_history_action=False, use_proprioception=False, action_mask_ratio=0.5, different_history_freq=False,
            predict_wrist_img=False, predict_proprioception=False)
        hash_init_(pol.vae_model, "vae.")
        hash_init_(pol.model, "mar.")
        pol = pol.to(DEV).eval()
        norm = LinearNormalizer()
        lim = torch.zeros(2, 2)
        lim[1] = 512.0
        norm.fit({"action": lim, "agent_pos": lim})
        pol.set_normalizer(norm)
        return pol

    b = cases.policy_batch()
    obs = {"image": torch.from_numpy(b["image"]).to(DEV), "agent_pos": torch.from_numpy(b["agent_pos"]).to(DEV)}
    pol = policy()
    res = pol.predict_action(dict(obs))
    smp = pol.model.diffactloss._sampler
    assert smp.method == "ddpm" and smp.sched.S == 100 and pol.model.diffloss.video_sampler == "ddpm"
    assert smp._cache["R"] == 16 and smp._cache["persist"] == _ops().sampler_persistent_fits(torch.device(DEV))
    assert torch.isfinite(res["action_pred"]).all()

    pol = policy(act_sampler="ddim", act_diff_testing_steps="ddim10", act_ddim_eta=0.0, video_sampler="ddim",
                 video_ddim_eta=0.25, num_sampling_steps="ddim10")
    res = pol.predict_action(dict(obs))
    smp = pol.model.diffactloss._sampler
    assert smp.method == "ddim" and smp.eta == 0.0 and smp.sched.S == 10
    assert smp._cache["persist"] is False and smp._cache["graph"] is not None
    assert (pol.model.diffloss.video_sampler, pol.model.diffloss.video_ddim_eta) == ("ddim", 0.25)
    assert torch.isfinite(res["action_pred"]).all()
    with pytest.raises(ValueError):
        policy(act_sampler="euler")
    with pytest.raises(ValueError):
        policy(video_sampler="plms")


def test_zz_report_worst_ratio():
    for k in sorted(RATIO):
        print(f"worst error / bound  {k}: {RATIO[k]:.3f}")
    assert all(v <= 1.0 for v in RATIO.values())
