"""The tile exponent of the fp8 attention quantisation pass (csrc/fp8_scale.h, fp8_tile_exp) on the CPU:
tests/host/fp8_scale_main.cpp includes the header and prints the exponent of every bf16 bit pattern of a
non-negative amax -- 0, the 127 positive denormals, the 32 512 positive normals (32 639 positive finite
patterns in all; with 0 the 32 640 non-negative finite ones), +Inf and every NaN -- plus fp32-only patterns
around the 0.875 mantissa boundary.  The reference is integer arithmetic on math.frexp: the smallest e with
amax * 2^-e <= 448, clamped to [-126, 126].  This is the only place Inf and NaN reach the function: no GPU
test feeds them to the pass.  No GPU: the program is built with --offload-host-only."""
import math
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_MIN, E_MAX = -126, 126


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    from unified_video_action_amd import build_native
    hipcc = build_native.HIPCC
    if not os.path.exists(hipcc):
        pytest.skip(f"no hipcc at {hipcc}: the host known-answer program cannot be built")
    exe = str(tmp_path_factory.mktemp("fp8_scale") / "fp8_scale_main")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-I" + build_native.CSRC,
           os.path.join(ROOT, "tests", "host", "fp8_scale_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, args=()):
    r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [tuple(int(t) for t in line.split()) for line in r.stdout.split("\n") if line]


def _f32(bits):
    return struct.unpack("f", struct.pack("I", bits))[0]


def unclamped_exponent(amax):
    """smallest integer e with amax * 2^-e <= 448, exactly: amax = f * 2^x (f in [0.5, 1)) and 448 = 7 * 2^6, so
    amax * 2^-e <= 448 <=> f * 2^(x - e - 6) <= 7; f * 8 <= 7 decides between x - e = 9 and 8.  f is a dyadic
    rational with at most 24 bits, so f * 8 <= 7 is exact in float64."""
    f, x = math.frexp(amax)
    return x - 9 if f * 8 <= 7 else x - 8


def want_exponent(bits):
    a = _f32(bits)
    if a == 0:
        return 0
    if math.isinf(a) or math.isnan(a):
        return E_MAX
    return min(max(unclamped_exponent(a), E_MIN), E_MAX)


def test_every_bf16_amax(prog):
    got = _run(prog)
    assert len(got) == 0x8000 and [b for b, _ in got] == [h << 16 for h in range(0x8000)]
    finite_pos = 0
    for bits, e in got:
        assert e == want_exponent(bits), (hex(bits), e, want_exponent(bits))
        a = _f32(bits)
        if 0 < a < math.inf:
            finite_pos += 1
            if E_MIN < e < E_MAX or (e in (E_MIN, E_MAX) and unclamped_exponent(a) == e):
                # inside the clamp: the definition itself, in exact arithmetic (ldexp by a power of two)
                assert math.ldexp(a, -e) <= 448.0 < math.ldexp(a, -(e - 1)), hex(bits)
            assert E_MIN <= e <= E_MAX
    assert finite_pos == 0x7F80 - 1  # 0x0001 .. 0x7F7F
    by = dict(got)
    assert by[0] == 0
    assert by[0x7F80 << 16] == E_MAX  # +Inf
    assert all(by[h << 16] == E_MAX for h in range(0x7F81, 0x8000))  # NaNs
    assert all(by[h << 16] == E_MIN for h in range(1, 0x80))  # bf16 denormals: the lower clamp
    assert by[0x7F7F << 16] == 120  # largest finite bf16: 1.9921875 * 2^127 = 0.996 * 2^128 -> 128 - 8
    assert by[0x43E0 << 16] == 0 and by[0x43E1 << 16] == 1  # 448 and the next bf16 above it
    assert by[0x3F80 << 16] == -8  # 1.0 = 0.5 * 2^1 -> 1 - 9


def test_fp32_patterns_around_the_boundary_and_the_clamps(prog):
    """fp32-only neighbours of 448 * 2^k (the mantissa comparison is on all 23 bits), the smallest normals
    (where the lower clamp starts to bind: 448 * 2^-126 has e = -126 unclamped, 2^-126 itself e = -134) and
    the largest (FLT_MAX: e = 120, the upper clamp never binds on a finite fp32)"""
    b448 = 0x43E00000
    bits = []
    for k in (-130, -126, -100, -3, 0, 5, 100, 118):
        base = b448 + (k << 23)
        if 0 < base < 0x7F800000:
            bits += [base - 1, base, base + 1]
    bits += [0x00800000, 0x00800001, 0x00FFFFFF, 0x007FFFFF, 0x00000001, 0x7F7FFFFF, 0x7F800000, 0x7FC00000,
             0x7F800001]
    got = _run(prog, bits)
    assert [b for b, _ in got] == bits
    for b, e in got:
        assert e == want_exponent(b), (hex(b), e, want_exponent(b))
    by = dict(got)
    assert by[b448 - 1] == 0 and by[b448] == 0 and by[b448 + 1] == 1
    assert by[0x7F7FFFFF] == 120 and by[0x00800000] == E_MIN and by[0x00000001] == E_MIN
    assert by[b448 + (-126 << 23)] == E_MIN and unclamped_exponent(_f32(b448 + (-126 << 23))) == E_MIN
