"""The kernels of csrc/i3d.hip per element against the float64 restatements of tests/i3d_ref.py, at the smallest
shapes at which each form can go wrong.  Every conv case asserts its form through uva_conv3d_route and writes
into a NaN-filled guarded buffer through an ldc wider than Co at a non-zero channel offset."""
import pytest
import torch

import i3d_ref as R
from conv_ref import assert_bit_equal
from edge_helpers import BF16, DEV, F32, Guarded, assert_within, gen
from unified_video_action_amd.native import ops
from unified_video_action_amd.native.lib import lib

pytestmark = pytest.mark.gpu
INVALID = 1  # hipErrorInvalidValue
LD_EXTRA, OFF = 16, 8


def _data(g, shape, ints, lo, hi):
    if ints:
        return torch.randint(lo, hi + 1, shape, generator=g).double()
    return torch.randn(shape, generator=g, dtype=torch.float64)


def _conv_case(seed, N, size, Ci, Co, kernel, stride, dtype, ints, relu, ci_used=None):
    g = gen(seed)
    x = _data(g, (N, *size, Ci), ints, -8, 8)
    w = _data(g, (Co, *kernel, Ci), ints, -3, 3)
    b = _data(g, (Co,), ints, -16, 16)
    if not ints:
        w = w / (kernel[0] * kernel[1] * kernel[2] * Ci) ** 0.5
    if ci_used is not None:
        x[..., ci_used:] = 0
        w[..., ci_used:] = 0
    x, w = x.float().to(dtype), w.float().to(dtype)  # the bf16 route's inputs are rounded to bf16 first
    b = b.float()
    pads = R.same_pad(size, kernel, stride)
    front, out_size = tuple(p[0] for p in pads), tuple(p[2] for p in pads)
    ref, S = R.conv3d(x, w, stride, front, out_size, bias=b, relu=relu)
    M = N * out_size[0] * out_size[1] * out_size[2]
    gd = Guarded(M, Co, dtype, ld=Co + LD_EXTRA, off=OFF)
    rows = gd.buf[64:64 + M * (Co + LD_EXTRA)].view(M, Co + LD_EXTRA)
    kw = dict(bias=b.to(DEV), stride=stride, pads=front, out_size=out_size, coff=OFF, act="relu" if relu else "none")
    return x.to(DEV), w.to(DEV), rows, gd, kw, ref.reshape(M, Co), S.reshape(M, Co)


def _check_conv(gd, ref, S, K, dtype, ints, what):
    gd.check()
    if ints:
        assert float(S.max()) < 2 ** 24
        assert_bit_equal(gd.view.cpu(), ref, what)
    else:
        assert_within(gd.view, ref, R.conv_bound(S, K, ref, bf16_out=dtype == BF16), what)


SHAPES_333 = [((1, 7, 7), 16, 32), ((2, 9, 14), 24, 48), ((5, 14, 7), 48, 208), ((2, 9, 14), 112, 32),
              ((1, 7, 7), 96, 48), ((5, 14, 7), 16, 208)]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("size,Ci,Co", SHAPES_333)
def test_conv3d_333(size, Ci, Co, dtype, ints, relu):
    x, w, rows, gd, kw, ref, S = _conv_case(11, 2, size, Ci, Co, (3, 3, 3), (1, 1, 1), dtype, ints, relu)
    assert ops.conv3d_route(x, w, rows, **kw) == ("f32_valu" if dtype == F32 else "mfma_333")
    ops.conv3d(x, w, rows, **kw)
    _check_conv(gd, ref, S, 27 * Ci, dtype, ints, f"conv3d 3x3x3 {size} Ci{Ci} Co{Co}")


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("size", [(16, 18, 18), (5, 17, 20)])
def test_conv3d_stem(size, dtype, ints):
    """7x7x7 / stride 2 on the 8-channel padded RGB input; (5, 17, 20): odd extents, so compute_pad's
    s % stride != 0 branch and the asymmetric front / back split are both taken"""
    x, w, rows, gd, kw, ref, S = _conv_case(12, 2, size, 8, 64, (7, 7, 7), (2, 2, 2), dtype, ints, True, ci_used=3)
    assert ops.conv3d_route(x, w, rows, **kw) == ("f32_valu" if dtype == F32 else "mfma_general")
    ops.conv3d(x, w, rows, **kw)
    _check_conv(gd, ref, S, 343 * 8, dtype, ints, f"stem {size}")


POOLS = [((1, 3, 3), (1, 2, 2)), ((3, 3, 3), (2, 2, 2)), ((3, 3, 3), (1, 1, 1)), ((2, 2, 2), (2, 2, 2))]


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("C,negative", [(8, False), (40, False), (8, True)])
@pytest.mark.parametrize("size", [(4, 9, 9), (3, 14, 7), (2, 7, 7)])
@pytest.mark.parametrize("kernel,stride", POOLS)
def test_maxpool3d(kernel, stride, size, C, dtype, negative):
    """bit-equal to the zero-padding restatement; negative: inputs below zero everywhere, so only the padding
    can produce the border maxima (0)"""
    x = torch.randn((2, *size, C), generator=gen(13), dtype=torch.float64)
    if negative:
        x = -x.abs() - 0.25
    x = x.float().to(dtype)
    pads = R.same_pad(size, kernel, stride)
    front, out_size = tuple(p[0] for p in pads), tuple(p[2] for p in pads)
    ref = R.maxpool3d(x, kernel, stride, front, out_size)
    gd = Guarded(2 * out_size[0] * out_size[1] * out_size[2], C, dtype)
    out = gd.view.view(2, *out_size, C)
    ops.maxpool3d(x.to(DEV), out, kernel, stride, front, out_size)
    gd.check()
    assert_bit_equal(out.cpu(), ref, f"maxpool {kernel}/{stride} {size}")
    if negative and any(p[0] + p[1] for p in pads):
        assert float(out.float().max()) == 0.0


@pytest.mark.parametrize("ints", [True, False])
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("T,classes", [(2, 400), (4, 24)])
def test_i3d_head(T, classes, dtype, ints):
    """integers on a grid that keeps the pool's and the time mean's divisions exact (x in 294 {-1, 0, 1}: the
    98-term mean is 3 x an integer, so are the logits, and their sum over T - 1 <= 3 positions divides)"""
    g = gen(14)
    C = 1024
    if ints:
        x = torch.randint(-1, 2, (2, T, 7, 7, C), generator=g).double() * 294
        w = torch.randint(-1, 2, (classes, C), generator=g).double()
        b = torch.randint(-4, 5, (classes,), generator=g).double() * 3
    else:
        x = torch.randn((2, T, 7, 7, C), generator=g, dtype=torch.float64)
        w = torch.randn((classes, C), generator=g, dtype=torch.float64) / 32
        b = torch.randn((classes,), generator=g, dtype=torch.float64)
    x, w, b = x.float().to(dtype), w.float(), b.float()
    ref, S = R.head(x, w, b)
    gd = Guarded(2, classes, F32)
    out = gd.view
    assert out.is_contiguous()
    ops.i3d_head(x.to(DEV), w.to(DEV), b.to(DEV), out)
    gd.check()
    if ints:
        assert_bit_equal(out.cpu(), ref, f"head T{T}")
    else:
        assert_within(out, ref, R.head_bound(S, C), f"head T{T}")


def test_i3d_head_refusals():
    L = lib()
    x = torch.zeros(2, 2, 6, 7, 64, device=DEV)
    w, b = torch.zeros(8, 64, device=DEV), torch.zeros(8, device=DEV)
    gd = Guarded(2, 8, F32)
    ws = torch.empty(1 << 12, device=DEV)
    args = lambda T, H, W: (0, x.data_ptr(), w.data_ptr(), b.data_ptr(), gd.view.data_ptr(), 2, T, H, W, 64, 8,
                            ws.data_ptr(), ws.numel(), ops.stream())  # noqa: E731
    assert L.query("uva_i3d_head", *args(2, 6, 7)) == INVALID
    assert L.query("uva_i3d_head", *args(1, 7, 7)) == INVALID
    gd.check()
    assert torch.isnan(gd.view).all()


@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("shape", [(2, 3, 96, 128, 3), (1, 2, 130, 100, 3)])
def test_fvd_preprocess(shape, dtype):
    v = torch.randint(0, 256, shape, generator=gen(15), dtype=torch.uint8)
    ref = R.preprocess(v)
    B, T = shape[:2]
    gd = Guarded(B * T * 224 * 224, 8, dtype)
    out = gd.view.view(B, T, 224, 224, 8)
    ops.fvd_preprocess(v.to(DEV), out)
    gd.check()
    assert_within(out[..., :3], ref, R.preprocess_bound(ref, bf16_out=dtype == BF16), f"preprocess {shape}")
    assert (out[..., 3:] == 0).all()


def test_fvd_preprocess_exact_on_dyadic_weights():
    """an exact 2x upscale (112 -> 224): weights 1/4, 3/4; on {0, 255} inputs every value is exact in fp32"""
    v = torch.randint(0, 2, (1, 2, 112, 112, 3), generator=gen(16), dtype=torch.uint8) * 255
    ref = R.preprocess(v)
    gd = Guarded(2 * 224 * 224, 8, F32)
    out = gd.view.view(1, 2, 224, 224, 8)
    ops.fvd_preprocess(v.to(DEV), out)
    gd.check()
    assert_bit_equal(out[..., :3].cpu().contiguous(), ref, "preprocess 2x")


def test_conv3d_refusals_launch_nothing():
    L = lib()
    N, size, Co = 1, (2, 7, 7), 32
    M = N * 2 * 7 * 7

    def call(x, w, out, Ci, dtype_code, ldc=Co, coff=0):
        return L.query("uva_conv3d", dtype_code, x, w, out, None, N, *size, Ci, Co, 3, 3, 3, 1, 1, 1, 1, 1, 1, *size,
                       ldc, coff, 0, ops.stream())

    gd = Guarded(M, Co, BF16)
    xb = torch.zeros(M * 16 + 8, dtype=BF16, device=DEV)
    wb = torch.zeros(Co * 27 * 16 + 8, dtype=BF16, device=DEV)
    o = gd.view.data_ptr()
    assert call(xb.data_ptr(), wb.data_ptr(), o, 16, 1) == 0          # the well-formed call is accepted
    torch.cuda.synchronize()
    gd.view.fill_(float("nan"))
    assert call(xb.data_ptr() + 2, wb.data_ptr(), o, 16, 1) == INVALID    # input off the 16-byte vector
    assert call(xb.data_ptr(), wb.data_ptr() + 2, o, 16, 1) == INVALID    # weight off the 16-byte vector
    assert call(xb.data_ptr(), wb.data_ptr(), o + 2, 16, 1) == INVALID    # output off the 8-byte vector
    assert call(xb.data_ptr(), wb.data_ptr(), o, 12, 1) == INVALID        # Ci % 8 != 0 on the MFMA route
    assert call(xb.data_ptr(), wb.data_ptr(), o, 16, 1, ldc=Co + 2) == INVALID   # row stride off the vector
    assert call(None, wb.data_ptr(), o, 16, 1) == INVALID                 # null pointer
    assert call(xb.data_ptr(), wb.data_ptr(), o, 16, 1, ldc=Co, coff=4) == INVALID  # slice past the row
    assert L.query("uva_conv3d_route", 1, xb.data_ptr(), wb.data_ptr(), o, None, N, *size, 12, Co, 3, 3, 3, 1, 1, 1,
                   1, 1, 1, *size, Co, 0, 0) == -INVALID
    gf = Guarded(M, Co, F32)
    xf = torch.zeros(M * 16 + 8, dtype=F32, device=DEV)
    wf = torch.zeros(Co * 27 * 16 + 8, dtype=F32, device=DEV)
    assert call(xf.data_ptr() + 4, wf.data_ptr(), gf.view.data_ptr(), 16, 0) == INVALID
    assert call(xf.data_ptr(), wf.data_ptr(), gf.view.data_ptr(), 6, 0) == INVALID   # Ci % 4 != 0, fp32 route
    gd.check()
    gf.check()
    assert torch.isnan(gd.view).all() and torch.isnan(gf.view).all()
