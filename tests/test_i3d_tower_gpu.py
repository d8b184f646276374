"""The HIP I3D tower (fvd/i3d.py) on hash weights against the reference's recorded endpoints and logits
(tests/golden/g8_i3d_fvd.npz, written by tests/golden/make_i3d_golden.py from the reference's InceptionI3d)."""
import numpy as np
import pytest
import torch

import i3d_ref as R
from unified_video_action_amd.fvd.i3d import InceptionI3dTower

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def tower():
    t = InceptionI3dTower(400)
    t.load_state_dict(R.hash_state({k: tuple(v.shape) for k, v in t.state_dict().items()}))
    return t.to(DEV)


@pytest.fixture(scope="module")
def fp32_run(tower):
    tower.set_precision("fp32")
    eps = {}
    logits = tower(R.clips(), endpoints=eps)
    torch.cuda.synchronize()
    return logits, eps


def test_fp32_endpoints_and_logits_match_the_reference(golden, fp32_run):
    logits, eps = fp32_run
    for name in R.RECORDED:
        got = R.subsample(eps[name]).float().cpu()
        want = torch.from_numpy(golden["ep_" + name])
        assert got.shape == want.shape, name
        err = R.rel_l2(got, want)
        print(f"{name}: rel L2 {err:.3e}")
        assert err <= 1e-4, (name, err)
    err = R.rel_l2(logits, golden["logits_f32"])
    print(f"logits fp32: rel L2 {err:.3e}")
    assert tuple(logits.shape) == (2, 400) and logits.dtype == torch.float32
    assert err <= 1e-4, err


def test_bf16_logits_within_three_times_the_references_own_bf16_error(golden, tower):
    tower.set_precision("bf16")
    try:
        logits = tower(R.clips())
    finally:
        tower.set_precision("fp32")
    err = R.rel_l2(logits, golden["logits_f32"])
    print(f"logits bf16: rel L2 {err:.3e} (reference bf16 autocast {float(golden['bf16_rel_l2']):.3e})")
    assert err <= 3.0 * float(golden["bf16_rel_l2"]), (err, float(golden["bf16_rel_l2"]))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_inception_slices_equal_separate_calls(tower, precision):
    """the four branches of Mixed_4b written straight into their slices of one [M, 512] buffer equal four
    separate calls into buffers of their own, concatenated, bit for bit"""
    tower.set_precision(precision)
    try:
        dtype = torch.float32 if precision == "fp32" else torch.bfloat16
        x = torch.randn(1, 2, 7, 7, 480, generator=torch.Generator().manual_seed(1)).to(dtype).to(DEV)
        fused = tower._mixed("Mixed_4b", x)
        n = "Mixed_4b."
        parts = [tower._point(n + "b0", x), tower._conv(n + "b1b", tower._point(n + "b1a", x)),
                 tower._conv(n + "b2b", tower._point(n + "b2a", x)),
                 tower._point(n + "b3b", tower._pool(x, (3, 3, 3), (1, 1, 1)))]
        want = torch.cat(parts, dim=-1)
    finally:
        tower.set_precision("fp32")
    assert tuple(fused.shape) == (1, 2, 7, 7, 512)
    assert not torch.isnan(fused.float()).any()
    assert torch.equal(fused, want)


def test_relaunch_is_bit_equal(tower, fp32_run):
    tower.set_precision("fp32")
    again = tower(R.clips())
    assert torch.equal(again, fp32_run[0])
    tower.set_precision("bf16")
    try:
        a, b = tower(R.clips()[:1]), tower(R.clips()[:1])
    finally:
        tower.set_precision("fp32")
    assert torch.equal(a, b)
