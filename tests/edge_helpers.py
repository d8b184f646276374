"""Shared pieces of the float64 edge-shape tests (test_vae_plumbing_gpu.py, test_small_kernels_gpu.py):
sentinel-guarded NaN-filled outputs and the per-element bound check."""
import torch

DEV = "cuda"
F32, BF16 = torch.float32, torch.bfloat16
SENTINEL = 12345.0
PAD = 64  # guard elements before and after (keeps 16-byte alignment of the payload)


class Guarded:
    """a [rows, cols] output view (leading dimension ld, column offset off) inside a sentinel-filled
    flat buffer; the view itself starts NaN-filled (or holds `init`)."""

    def __init__(self, rows, cols, dtype, ld=None, off=0, init=None):
        ld = cols if ld is None else ld
        assert off + cols <= ld
        self.buf = torch.full((PAD + rows * ld + PAD,), SENTINEL, dtype=dtype, device=DEV)
        self.view = self.buf[PAD:PAD + rows * ld].view(rows, ld)[:, off:off + cols]
        inside = torch.zeros_like(self.buf, dtype=torch.bool)
        inside[PAD:PAD + rows * ld].view(rows, ld)[:, off:off + cols] = True
        self.outside = ~inside
        if init is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(init)
        self.before = self.buf.clone()

    def check(self):
        torch.cuda.synchronize()
        assert torch.equal(self.buf[self.outside], self.before[self.outside]), "write outside the output view"


def flat_out(n, dtype):
    g = Guarded(1, n, dtype)
    return g, g.view.view(-1)


def assert_within(got, ref, bound, what=""):
    """per element |got - ref| <= bound (float64 tensors on the host); a NaN fails"""
    got, ref, bound = got.double().cpu(), ref.double().cpu(), bound.double().cpu()
    assert not torch.isnan(got).any(), f"{what}: NaN (unwritten or invalid element)"
    err = (got - ref).abs()
    bad = err > bound
    if bad.any():
        i = torch.argmax(err / bound.clamp_min(1e-300))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements out of bound; worst at flat "
                             f"index {int(i)}: got {got.reshape(-1)[i]:.9g} ref {ref.reshape(-1)[i]:.9g} "
                             f"err {err.reshape(-1)[i]:.3g} bound {bound.reshape(-1)[i]:.3g}")


def gen(seed):
    return torch.Generator(device="cpu").manual_seed(seed)
