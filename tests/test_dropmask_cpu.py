"""oracle/dropmask.py (the dropout counter hash restated in numpy integer code) against the real
csrc/common.h, compiled for the host: tests/host/drop_hash_main.cpp includes the header (its hash functions
are __host__ __device__) and prints uva_drop_params, drop_key and dropout_keep for the cases given on its
command line.  Every keep decision is compared, none sampled.  The index runs that straddle 2^33 and 2^40
reach the rotl(pair >> 32, 11) term of the first word, which no GPU test reaches at a sane tensor size.
No GPU: the program is built with --offload-host-only and runs on the CPU."""
import os
import struct
import subprocess

import numpy as np
import pytest

import dropmask as DM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rt_seed():
    from unified_video_action_amd.runtime import _Runtime
    rt = _Runtime()
    rt.seed(77)
    rt.next_seed()
    return rt.next_seed()


# seeds without / with high 32 bits, and one of the values a training step draws (RT.next_seed())
SEEDS = [0, 1234, 0xFFFFFFFF, 0xABCDEF0123456789, 1 << 63, _rt_seed()]
PS = [0.1, 0.5, 1e-6, 0.9999, 0.0]
# (first index, count): the low range; pair >> 32 turns non-zero at idx 2^33; a higher bit of it at 2^40
RUNS = [(0, 4096), ((1 << 33) - 300, 600), ((1 << 40) - 300, 600)]


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    from unified_video_action_amd import build_native
    hipcc = build_native.HIPCC
    if not os.path.exists(hipcc):
        pytest.skip(f"no hipcc at {hipcc}: the host known-answer program cannot be built")
    exe = str(tmp_path_factory.mktemp("drop_hash") / "drop_hash_main")
    cmd = [hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-I" + build_native.CSRC,
           os.path.join(ROOT, "tests", "host", "drop_hash_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def _run(exe, cases):
    """cases: [(p, seed, idx0, count)] -> [(thresh, scale, key, keep bool array)]"""
    args = []
    for p, seed, idx0, count in cases:
        args += [repr(float(np.float32(p))), str(seed), str(idx0), str(count)]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.split("\n")
    out = []
    for i, (p, seed, idx0, count) in enumerate(cases):
        P, K = lines[2 * i].split(), lines[2 * i + 1].split()
        assert P[0] == "P" and int(P[2]) == seed, P
        assert K[0] == "K" and int(K[1]) == idx0 and int(K[2]) == count and len(K[3]) == count, K[:3]
        scale = struct.unpack("f", struct.pack("I", int(P[4])))[0]
        out.append((int(P[3]), scale, int(P[5]), np.frombuffer(K[3].encode(), dtype=np.uint8) == ord("1")))
    return out


def test_params_match_header(prog):
    want = {0.1: 6554, 0.5: 32768, 1e-6: 1, 0.9999: 65529, 0.0: 0}  # round(p * 65536), clamped to 1..65535
    for p, (th, scale, _, _) in zip(PS, _run(prog, [(p, 1, 0, 1) for p in PS])):
        assert DM.drop_params(p) == (th, scale), p
        assert th == want[p], (p, th)
        assert scale == float(np.float32(65536.0) / np.float32(65536 - th))
    # half to even: 0.5 + 2^-17 -> p * 65536 = 32768.5 -> 32768
    (th, scale, _, _), = _run(prog, [(0.5 + 2.0 ** -17, 1, 0, 1)])
    assert th == 32768 and DM.drop_params(0.5 + 2.0 ** -17) == (th, scale)
    assert DM.drop_params(-1.0) == (0, 1.0)


def test_key_and_keep_match_header(prog):
    cases = [(p, seed, idx0, count) for seed in SEEDS for p in PS for idx0, count in RUNS]
    got = _run(prog, cases)
    for (p, seed, idx0, count), (th, scale, key, keep) in zip(cases, got):
        assert DM.drop_key(seed) == key, hex(seed)
        assert DM.drop_params(p) == (th, scale)
        idx = np.uint64(idx0) + np.arange(count, dtype=np.uint64)
        mine = DM.keep(seed, idx, th)
        assert np.array_equal(mine, keep), (p, hex(seed), idx0, int(np.argmax(mine != keep)))
        if p == 0.0:
            assert keep.all()


def test_high_index_term_is_live(prog):
    """the header's decisions above 2^33 and 2^40 differ from those at the same low 33 bits below: the
    rotl(pair >> 32, 11) term enters the hash (a restatement and a header that both ignored it would still agree)"""
    cases = [(0.5, seed, base, 4096) for seed in SEEDS[:2] for base in (0, 1 << 33, 1 << 40)]
    got = [k for _, _, _, k in _run(prog, cases)]
    for i in (0, 3):
        lo, at33, at40 = got[i:i + 3]
        assert not np.array_equal(lo, at33) and not np.array_equal(lo, at40) and not np.array_equal(at33, at40)
        for k in (lo, at33, at40):
            assert abs(k.mean() - 0.5) < 0.05


def test_layout_helpers_are_the_flat_index():
    """the layout helpers against keep() on the index formula written out element by element"""
    seed, (th, _) = 0xABCDEF0123456789, DM.drop_params(0.1)
    M, N = 5, 7
    flat = DM.keep_flat(seed, M, N, th)
    for r in range(M):
        for c in range(N):
            assert flat[r, c] == DM.keep(seed, [r * N + c], th)[0]
    B, H, L = 2, 2, 64
    att = DM.keep_attn(seed, B, H, L, th)
    mq, mk = DM.attn_planes(seed, B, H, L, th)
    assert mq.shape == (B * H, 1, L) and mk.shape == (B * H, 1, L) and mq.dtype == np.uint64
    for b, h, q, k in [(0, 0, 0, 0), (1, 1, 63, 62), (1, 0, 17, 40), (0, 1, 5, 6)]:
        want = DM.keep(seed, [((b * H + h) * L + q) * L + k], th)[0]
        assert att[b, h, q, k] == want
        assert (int(mq[b * H + h, 0, q]) >> DM.mask_pos(k)) & 1 == int(want)
        assert (int(mk[b * H + h, 0, k]) >> DM.mask_pos(q)) & 1 == int(want)
    assert sorted(DM.mask_pos(k) for k in range(64)) == list(range(64))
    n = 70
    words = DM.plane_words(seed, n, th)
    assert words.shape == (3,) and words.dtype == np.uint32
    want = DM.keep(seed, np.arange(96, dtype=np.uint64), th)
    for i in range(96):
        assert (int(words[i // 32]) >> (i % 32)) & 1 == int(want[i])
