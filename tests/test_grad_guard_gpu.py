"""Gradient norm, clipping and the non-finite step guard on the GPU.

uva_grad_sumsq (deterministic fp64 sum of squares over ranges of the flat fp32 gradient buffer), uva_grad_guard
(the device record: total norm, clip coefficient, skip flag, part norms), uva_adamw_ema_guarded (the clip
coefficient folded into AdamW's gradient scaling, the step skipped on a non-finite norm), and their way up
through FusedAdamWEMA, EMAModel and the workspace's log.

The bound on a slot sum: every product (double)g * (double)g is exact (24 x 24 significand bits), the terms are
non-negative, and a term passes through at most L additions (csrc/optim.hip's header; ops.grad_norm_chain_len),
each within 2^-53 relative: |got - exact| <= ((1 + 2^-53)^L - 1) * exact <= (L + 1) * 2^-53 * exact, and
math.fsum's own rounding of the exact sum is the last 2^-53: (L + 2) * 2^-53 * fsum."""
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

import cases
import replay
from hashinit import hash_init_

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -53
F32_ULP_REL = 2.0 ** -24  # round-to-nearest fp32 cast: half an ulp, relative


def rel_err(a, b):
    a, b = a.double(), b.double()
    return ((a - b).abs().max() / (b.abs().max() + 1e-12)).item()


def _ops():
    from unified_video_action_amd.native import ops
    return ops


def _chunk():
    return _ops().grad_norm_chunk_elems()


def _lengths():
    c = _chunk()
    return [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, c - 1, c, c + 1, 2 * c + 7, 2 ** 20 + 3]


def _sumsq(buf, ranges, n_slots, nan_work=True):
    """-> the device slot sums (fp64) of one launch, the workspace NaN-filled before it"""
    ops = _ops()
    work = torch.empty(ops.grad_norm_workspace_bytes(buf.numel(), len(ranges)) // 8, dtype=torch.float64, device=DEV)
    if nan_work:
        work.fill_(float("nan"))
    sums = torch.full((n_slots,), float("nan"), dtype=torch.float64, device=DEV)
    ops.grad_sumsq(buf, ranges, n_slots, sums, work)
    return sums


def _record(sums, n_slots, grad_scale=1.0, max_norm=None, skip=False):
    rec = torch.full((4 + n_slots,), float("nan"), dtype=torch.float32, device=DEV)
    _ops().grad_guard(sums, n_slots, grad_scale, max_norm, skip, rec)
    return rec


def _embed(values, phase):
    """values (fp32 numpy) at element offset 4 + phase of a NaN-filled device buffer -> (buffer, offset)"""
    off = 4 + phase
    buf = torch.full((off + len(values) + 9,), float("nan"), dtype=torch.float32, device=DEV)
    buf[off:off + len(values)] = torch.from_numpy(values).to(DEV)
    return buf, off


_INTS = {}


def _ints():
    if "v" not in _INTS:
        _INTS["v"] = np.random.default_rng(20240607).integers(-3, 4, size=max(_lengths())).astype(np.float32)
    return _INTS["v"]


# ---- the sum -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("phase", [0, 1, 2, 3])
def test_exact_integer_sums(phase):
    data = _ints()
    got = []
    for n in _lengths():
        buf, off = _embed(data[:n], phase)
        assert (buf.data_ptr() // 4 + off) % 4 == phase
        got.append(_sumsq(buf, [(off, n, 0)], 1))
    got = torch.cat(got).cpu().tolist()
    for n, s in zip(_lengths(), got):
        want = int((data[:n].astype(np.int64) ** 2).sum())
        assert s == want, (n, phase, s, want)


def test_wide_range_within_the_derived_bound():
    rng = np.random.default_rng(7)
    for n in _lengths():
        x = (rng.standard_normal(n) * 10.0 ** rng.integers(-20, 19, size=n)).astype(np.float32)
        assert np.isfinite(x).all()
        x64 = x.astype(np.float64)
        want = math.fsum(x64 * x64)  # each product is exact in fp64
        buf, off = _embed(x, 1)
        got = _sumsq(buf, [(off, n, 0)], 1).item()
        L = _ops().grad_norm_chain_len(n, 1)
        print(f"n {n}: got {got!r} fsum {want!r} rel {abs(got - want) / want:.3e} bound {(L + 2) * U:.3e}")
        assert abs(got - want) <= (L + 2) * U * want, (n, got, want, L)


def test_slots_equal_single_range_launches():
    c = _chunk()
    n = 2 * c + 359
    g = torch.randn(n + 8, device=DEV)
    g[n:] = float("nan")
    # slot 0: one range over two chunks and a bit; slot 1: two short ranges; slot 2: a length-1 range;
    # slot 3: an empty range only; slot 4: a length-1 range and the last 300 elements.  Interleaved; [7, 9) is
    # in no range.  Two one-chunk ranges of a slot meet in a single addition, so the sums below are bit-equal
    ranges = [(0, 3, 1), (3, 1, 2), (4, 0, 3), (4, 1, 4), (5, 2, 1), (9, 2 * c + 50, 0), (2 * c + 59, n - 2 * c - 59, 4)]
    g[7:9] = float("nan")
    sums = _sumsq(g, ranges, 5)
    single = [_sumsq(g, [(o, k, 0)], 1) for o, k, _ in ranges]
    sums, single = sums.cpu().tolist(), [s.item() for s in single]
    assert sums[0] == single[5]
    assert sums[1] == single[0] + single[4]  # one chunk each: summed by one addition
    assert sums[2] == single[1] == float(g[3].double() ** 2)
    assert sums[3] == 0.0 == single[2]
    assert sums[4] == single[3] + single[6]
    rec = _record(torch.tensor(sums, dtype=torch.float64, device=DEV), 5).cpu().tolist()
    tot = 0.0
    for s in sums:
        tot += s
    assert abs(rec[0] - np.float32(math.sqrt(tot))) <= np.spacing(np.float32(math.sqrt(tot)))
    assert rec[1] == 1.0 and rec[2] == 0.0 and rec[3] == 0.0
    for i, s in enumerate(sums):
        assert abs(rec[4 + i] - np.float32(math.sqrt(s))) <= np.spacing(np.float32(math.sqrt(s)))


def test_relaunch_is_bit_equal():
    c = _chunk()
    n = 5 * c + 13
    g = torch.randn(n, device=DEV) * 3.0
    ranges = [(1, 2 * c, 0), (2 * c + 1, 17, 1), (2 * c + 18, n - 2 * c - 18, 0)]
    recs = []
    for _ in range(3):
        sums = _sumsq(g, ranges, 2, nan_work=True)
        recs.append((_record(sums, 2, 0.5, 1.0, True).view(torch.int32).cpu(), sums.view(torch.int64).cpu()))
    assert torch.isfinite(_record(sums, 2)).all()
    for rec, sums in recs[1:]:
        assert torch.equal(rec, recs[0][0]) and torch.equal(sums, recs[0][1])


def test_non_finite_sets_the_skip_flag():
    c = _chunk()
    n = 2 * c + 7
    g = torch.randn(4 + 1 + n + 8, device=DEV)
    off = 5  # phase 1: every chunk starts with a 3-element scalar head, chunk 0 ends in a 1-element scalar tail
    rng = [(off, n, 0)]
    places = {"first (scalar head)": 0, "inside the scalar head": 1, "body": c + 5, "before the chunk boundary "
              "(scalar tail)": c - 1, "after the chunk boundary": c, "head of the last chunk": 2 * c + 2, "last": n - 1}
    recs = {}
    recs["finite", "on"] = _record(_sumsq(g, rng, 1), 1, skip=True)
    recs["finite", "off"] = _record(_sumsq(g, rng, 1), 1, skip=False)
    for name, pos in places.items():
        for val in (float("nan"), float("inf"), float("-inf")):
            keep = g[off + pos].clone()
            g[off + pos] = val
            sums = _sumsq(g, rng, 1)
            recs[name, val, "on"] = _record(sums, 1, max_norm=1.0, skip=True)
            recs[name, val, "off"] = _record(sums, 1, max_norm=1.0, skip=False)
            g[off + pos] = keep
    # outside the range nothing counts
    g[off - 1] = float("nan")
    g[off + n] = float("inf")
    recs["finite outside", "on"] = _record(_sumsq(g, rng, 1), 1, skip=True)
    for key, rec in recs.items():
        r = rec.cpu().tolist()
        if key[0].startswith("finite"):
            assert r[2] == 0.0 and math.isfinite(r[0]), (key, r)
            continue
        assert r[2] == (1.0 if key[2] == "on" else 0.0), (key, r)
        assert not math.isfinite(r[0]), (key, r)
        # the coefficient torch's clip_grad_norm_ gives: 0 for an infinite norm, NaN for a NaN one
        if math.isnan(key[1]):
            assert math.isnan(r[0]) and math.isnan(r[1]), (key, r)
        else:
            assert r[0] == float("inf") and r[1] == 0.0, (key, r)


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
def test_guard_arithmetic_matches_python_doubles(grad_scale):
    max_norm = 1.0
    for total in (1e6, 1.0000001, 1.0 + 2e-6, 1.0, 0.5, 1e-3):  # norms far above, just above, at and below
        target = total / grad_scale
        slots = [0.25 * target ** 2, 0.0, 0.5 * target ** 2, 0.25 * target ** 2]
        rec = _record(torch.tensor(slots, dtype=torch.float64, device=DEV), 4, grad_scale, max_norm, True).cpu().numpy()
        tot = 0.0
        for s in slots:
            tot += s
        tn = math.sqrt(tot) * grad_scale
        coef = min(1.0, max_norm / (tn + 1e-6))
        want = [tn, coef, 0.0, 0.0] + [math.sqrt(s) * grad_scale for s in slots]
        for i, w in enumerate(want):
            w32 = np.float32(w)
            assert abs(rec[i] - w32) <= np.spacing(w32), (total, i, rec[i], w)
        off = _record(torch.tensor(slots, dtype=torch.float64, device=DEV), 4, grad_scale, None, False).cpu().numpy()
        assert off[1] == 1.0 and off[0] == rec[0]


# ---- the optimizer ----------------------------------------------------------------------------------------
N_A, N_B = 4099, 2051  # two param groups, each with a 3-element scalar tail


class _Tiny(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(N_A, generator=g))
        self.b = torch.nn.Parameter(torch.randn(N_B, generator=g))
        self.opt = None

    def bound_optimizer(self):
        return self.opt


def _tiny(ema=True, **guard):
    """(module, optimizer, EMAModel or None): decay group `a` (wd 0.02), no-decay group `b`, on the GPU"""
    from unified_video_action_amd.model.autoregressive.ema_model import EMAModel
    from unified_video_action_amd.runtime import RT
    from unified_video_action_amd.workspace.optim import FusedAdamWEMA
    RT.set_precision("bf16")  # the bf16 shadow is part of the step
    mod = _Tiny().to(DEV)
    ema_mod = copy.deepcopy(mod) if ema else None
    opt = FusedAdamWEMA([{"params": [mod.a], "weight_decay": 0.02}, {"params": [mod.b], "weight_decay": 0.0}],
                        lr=1e-3, betas=(0.9, 0.95), named=list(mod.named_parameters()), **guard)
    mod.opt = opt
    # update_after_step < 0: a non-zero decay from the first call on
    return mod, opt, (EMAModel(ema_mod, update_after_step=-10, power=0.75) if ema else None)


def _grads(step, scale=1.0):
    g = torch.Generator().manual_seed(100 + step)
    return torch.randn(N_A, generator=g) * scale, torch.randn(N_B, generator=g) * scale


def _set_grads(opt, mod, ga, gb):
    mod.a.grad.copy_(ga.to(DEV))
    mod.b.grad.copy_(gb.to(DEV))
    assert opt.store.is_bound()


def _state(opt, ema=None):
    st = opt.store
    out = [st.flat.clone(), opt.m.clone(), opt.v.clone(), st.shadow.clone()]
    if ema is not None:
        out.append(ema.flat.clone())
    return out


@pytest.mark.parametrize("gscale,max_norm,grad_scale", [(100.0, 78.0, 1.0), (1.0, 1e3, 1.0), (100.0, 39.0, 0.5)])
def test_clipped_adamw_matches_torch(gscale, max_norm, grad_scale):
    """coefficient ~ 0.01 (the norm of 6150 N(0, 100^2) values is ~ 7842), coefficient 1, and ~ 0.01 under
    grad_scale 0.5; the reference: torch.optim.AdamW + clip_grad_norm_ in float64 on the CPU"""
    mod, opt, ema = _tiny(max_grad_norm=max_norm)
    opt.grad_scale = grad_scale
    ra = torch.nn.Parameter(mod.a.detach().double().cpu())
    rb = torch.nn.Parameter(mod.b.detach().double().cpu())
    ref = torch.optim.AdamW([{"params": [ra], "weight_decay": 0.02}, {"params": [rb], "weight_decay": 0.0}],
                            lr=1e-3, betas=(0.9, 0.95))
    ema_ref = torch.cat([ra.detach(), rb.detach()]).clone()
    for step in range(3):
        ga, gb = _grads(step, gscale)
        _set_grads(opt, mod, ga, gb)
        grad_before = opt.store.grad.clone()
        opt.step()
        d = ema.get_decay(ema.optimization_step)
        ema.step(mod)
        ra.grad, rb.grad = ga.double() * grad_scale, gb.double() * grad_scale
        norm = torch.nn.utils.clip_grad_norm_([ra, rb], max_norm)
        ref.step()
        ema_ref = d * ema_ref + (1 - d) * torch.cat([ra.detach(), rb.detach()])
        stats = opt.grad_stats()
        coef = min(1.0, max_norm / (norm.item() + 1e-6))
        assert abs(stats["grad_norm"] - norm.item()) <= 2 * F32_ULP_REL * norm.item()
        assert abs(stats["grad_clip_coef"] - coef) <= 2 * F32_ULP_REL * coef
        assert (coef == 1.0) if gscale == 1.0 else (0.009 < coef < 0.011)
        assert stats["skipped"] == 0
        assert torch.equal(opt.store.grad, grad_before)  # the gradient buffer itself is not rescaled
        assert rel_err(mod.a.detach().cpu(), ra.detach()) < 1e-6
        assert rel_err(mod.b.detach().cpu(), rb.detach()) < 1e-6
    assert rel_err(torch.cat([ema.averaged_model.a, ema.averaged_model.b]).detach().cpu(), ema_ref) < 1e-6
    st = opt.store
    assert torch.equal(st.shadow, st.flat.to(torch.bfloat16))
    sd = opt.state_dict()["state"]
    assert rel_err(sd[0]["exp_avg"].cpu(), ref.state[ra]["exp_avg"]) < 1e-6
    assert rel_err(sd[1]["exp_avg_sq"].cpu(), ref.state[rb]["exp_avg_sq"]) < 1e-6
    assert float(sd[0]["step"]) == 3


def test_guard_on_but_never_active_is_bit_equal():
    mod0, opt0, ema0 = _tiny()
    mod1, opt1, ema1 = _tiny(max_grad_norm=1e30, skip_nonfinite=True)
    for step in range(3):
        ga, gb = _grads(step)
        for mod, opt, ema in ((mod0, opt0, ema0), (mod1, opt1, ema1)):
            _set_grads(opt, mod, ga, gb)
            opt.step()
            ema.step(mod)
    for x, y in zip(_state(opt0, ema0), _state(opt1, ema1)):
        assert torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x.view(torch.int16),
                           y.view(torch.int32) if y.dtype == torch.float32 else y.view(torch.int16))
    assert opt0.grad_record is None and opt0.grad_stats() == {} and opt0.skipped_steps == 0
    assert opt1.grad_stats()["grad_clip_coef"] == 1.0 and opt1.skipped_steps == 0
    assert opt0.step_count == opt1.step_count == 3


def test_skipped_step_leaves_the_state_and_the_step_count():
    mod0, opt0, _ = _tiny(ema=False)  # unguarded: sees only the finite gradients
    mod1, opt1, ema = _tiny(skip_nonfinite=True)
    finite = [_grads(s) for s in (0, 2, 3)]
    calls = [finite[0], _grads(1), finite[1], finite[2]]
    calls[1][0][N_A // 2] = float("nan")  # one NaN in one gradient element of call 2
    ema_ref = torch.cat([mod1.a, mod1.b]).detach().double().cpu()
    n_unguarded = 0
    for i, (ga, gb) in enumerate(calls):
        _set_grads(opt1, mod1, ga, gb)
        before = _state(opt1)
        d = ema.get_decay(ema.optimization_step)
        opt1.step()
        ema.step(mod1)
        after = _state(opt1)
        ema_ref = d * ema_ref + (1 - d) * torch.cat([mod1.a, mod1.b]).detach().double().cpu()
        # exactly one EMA update per call, skipped or not, against the closed form
        assert rel_err(torch.cat([ema.averaged_model.a, ema.averaged_model.b]).detach().cpu(), ema_ref) < 1e-6, i
        if i == 1:
            for x, y in zip(before, after):
                assert torch.equal(x, y)  # p, m, v and the shadow untouched (finite values: equal = bit-equal)
            assert opt1.grad_stats()["skipped"] == 1 and math.isnan(opt1.grad_stats()["grad_norm"])
            continue
        _set_grads(opt0, mod0, ga, gb)
        opt0.step()
        n_unguarded += 1
        for x, y in zip(_state(opt0), after):
            assert torch.equal(x, y), (i, "differs from the unguarded optimizer after", n_unguarded, "steps")
        assert not torch.equal(before[0], after[0])
    assert 0.5 < d < 1.0 and ema.optimization_step == 4
    assert opt1.skipped_steps == 1 and opt1.step_calls == 4 and opt1.step_count == 3
    assert float(opt1.state_dict()["state"][0]["step"]) == 3
    assert torch.isfinite(ema.flat).all() and torch.isfinite(opt1.store.flat).all()


# ---- the workspace ------------------------------------------------------------------------------------------
def _yaml(v):
    return f"'{v}'" if isinstance(v, str) else str(v).lower() if isinstance(v, bool) else str(v)


def _golden_workspace(tmp_path, extra=()):
    """the smallest config of the workspace GPU tests (tests/test_workspace_gpu.py)"""
    import train
    from unified_video_action_amd import config as C
    replay.golden_policy(normalizer=False)  # registers model_size "mar_golden"
    L = cases.TRACE_LR
    cfg = train.build_cfg([
        "--config-name=uva_pusht", "model.policy.autoregressive_model_params.model_size=mar_golden",
        "model.policy.action_model_params.predict_action=true", f"training.lr_warmup_steps={L['warmup']}",
        "training.num_epochs=1", "dataloader.batch_size=1", "dataloader.num_workers=0",
        f"task.dataset.n_samples={L['total']}", "training.resume=false", "training.mixed_precision=bf16",
        f"multi_run.run_dir={tmp_path}"] + [f"+model.policy.autoregressive_model_params.{k}={_yaml(v)}"
                                            for k, v in cases.MAR_KW.items() if k in cases.POLICY_AMP_KEYS]
        + list(extra))
    return C.get_class(cfg.model._target_)(cfg)


TODAYS_KEYS = {"train_loss", "diffusion_loss", "action_loss", "global_step", "epoch", "lr"}
PARTS = ["encoder", "decoder", "video_head", "action_head", "rest"]
GUARD_KEYS = ["+training.max_grad_norm=0.05", "+training.skip_nonfinite_steps=true", "+training.log_grad_norm=true"]


def _step_logs(tmp_path):
    logs = [json.loads(x) for x in open(os.path.join(tmp_path, "logs.json.txt"))]
    return [r for r in logs if not r.get("epoch_end")]


def test_workspace_guard_active_reports_the_norm(tmp_path):
    from unified_video_action_amd.runtime import RT
    RT.set_precision("bf16")
    ws = _golden_workspace(tmp_path, GUARD_KEYS)
    # hash weights: the default initialisation zeroes the heads' output layers, which would leave the
    # encoder, the decoder and the rest without gradient at the first step
    hash_init_(ws.model.model, "mar.")
    ws.setup(device=DEV)
    opt = ws.optimizer
    assert opt.grad_part_names == PARTS and opt.max_grad_norm == 0.05 and opt.skip_nonfinite
    batch = replay.device_batch(cases.trace_batch(0), DEV)
    raw, _ = ws.model(batch, rng=cases.trace_rng(0))
    raw.backward()
    st = opt.store
    want = st.grad.double().norm().item()  # the padding between the groups stays zero
    before = st.flat.clone()
    opt.step()
    stats = opt.grad_stats()
    L = _ops().grad_norm_chain_len(st.total, len(opt._guard["table"]))
    # the sum of squares is within (L + 2) * 2^-53 (above) and so is torch's own fp64 reduction, far inside
    # it; the square root halves that, and the record's fp32 cast adds half an fp32 ulp
    tol = F32_ULP_REL + 2 * (L + 2) * U
    print(f"grad_norm {stats['grad_norm']!r} torch fp64 {want!r} rel {abs(stats['grad_norm'] - want) / want:.3e}")
    assert want > 0 and abs(stats["grad_norm"] - want) <= tol * want
    parts = [stats[f"grad_norm/{n}"] for n in PARTS]
    assert all(p > 0 for p in parts), parts
    # each part norm carries its own fp32 rounding (2^-24 relative), as does the total
    assert abs(math.sqrt(sum(p * p for p in parts)) - stats["grad_norm"]) <= 2 * tol * stats["grad_norm"]
    mar = ws.model.model
    named = {"encoder": [mar.encoder_blocks], "decoder": [mar.decoder_blocks], "video_head": [mar.diffloss],
             "action_head": [mar.diffactloss]}
    seen = {id(p) for mods in named.values() for m in mods for p in m.parameters()}
    named["rest"] = [[p for _, p in st.order if id(p) not in seen]]
    for name, mods in named.items():
        ps = [p for m in mods for p in (m.parameters() if hasattr(m, "parameters") else m)]
        ref = math.sqrt(sum(float(p.grad.double().pow(2).sum()) for p in ps))
        print(f"grad_norm/{name} {stats[f'grad_norm/{name}']!r} torch fp64 {ref!r}")
        assert abs(stats[f"grad_norm/{name}"] - ref) <= tol * ref, name
    coef = min(1.0, 0.05 / (want + 1e-6))
    assert abs(stats["grad_clip_coef"] - coef) <= 2 * F32_ULP_REL * coef and stats["skipped"] == 0
    # (the schedule's first warm-up step has lr 0: the weights stay, the moments take the clipped gradient)
    assert torch.equal(before, st.flat) == (opt.param_groups[0]["lr"] == 0.0) and opt.step_count == 1
    assert rel_err(opt.m, st.grad * (0.1 * stats["grad_clip_coef"])) < 1e-5


def test_workspace_log_gains_the_keys_only_when_asked(tmp_path):
    from unified_video_action_amd.runtime import RT
    RT.set_precision("bf16")
    ws = _golden_workspace(tmp_path, ["training.max_train_steps=2"] + GUARD_KEYS)
    ws.run()
    steps = _step_logs(tmp_path)
    assert len(steps) == 2
    want = TODAYS_KEYS | {"grad_norm", "grad_clip_coef", "skipped_steps"} | {f"grad_norm/{n}" for n in PARTS}
    for r in steps:
        assert set(r) == want, sorted(set(r) ^ want)
        assert r["grad_norm"] > 0 and 0 < r["grad_clip_coef"] <= 1 and r["skipped_steps"] == 0
    assert ws.optimizer.skipped_steps == 0 and ws.optimizer.step_count == 2 and ws.ema.optimization_step == 2


def test_workspace_keys_absent_logs_todays_keys(tmp_path):
    from unified_video_action_amd.runtime import RT
    RT.set_precision("bf16")
    ws = _golden_workspace(tmp_path, ["training.max_train_steps=2"])
    ws.run()
    steps = _step_logs(tmp_path)
    assert len(steps) == 2
    for r in steps:
        assert set(r) == TODAYS_KEYS, sorted(set(r) ^ TODAYS_KEYS)
    assert getattr(ws.optimizer, "grad_record", None) is None
