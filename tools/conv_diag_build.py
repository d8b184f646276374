"""Diagnostic builds of the GN halo conv and the persistent sampler (timing only; results are WRONG by
construction): each variant patches a copy of a csrc file by exact text match, compiles it, and links
abx/diag_<name>.so from the in-tree objects with that object replaced.  A variant whose text no longer
matches the source raises instead of building the unpatched file.  Run the timings with
tools/conv_diag.sh / tools/ps_diag.sh on the GPU box."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "unified_video_action_amd", "csrc")
OBJ = os.path.join(ROOT, "unified_video_action_amd", "build_obj")
AB = os.path.join(ROOT, "abx")
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-munsafe-fp-atomics", "-Wno-unused-result",
         "-I" + CSRC] + os.environ.get("DIAG_FLAGS", "").split()

# every stride-1 / stride-2 halo kernel of conv.hip maps its block id here
ANCHOR = "  const int pid = xcd_remap(blockIdx.x, nblk);"
MFMA_F_OUTER = """        for (int f = 0; f < G::FM; ++f)
#pragma unroll
          for (int g = 0; g < G::FN; ++g)
            acc[f][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[cur][ks][g], fa[ks][f], acc[f][g], 0, 0, 0);"""
MFMA_G_OUTER = """        for (int g = 0; g < G::FN; ++g)
#pragma unroll
          for (int f = 0; f < G::FM; ++f)
            acc[f][g] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[cur][ks][g], fa[ks][f], acc[f][g], 0, 0, 0);"""
VARIANTS = {
    "base": [],
    # weight fragments always from step 0's offset (L1/L2-hot lines: the weight stream's latency)
    "bhot": [("const int soff = __builtin_amdgcn_readfirstlane((tap * Ci + cc * 64) * 2);",
              "const int soff = 0;")],
    # conv3x3_halo_gn: MFMA loop with the weight fragment outer
    "gouter": [(MFMA_F_OUTER, MFMA_G_OUTER)],
    # conv3x3_halo_gn: accumulators not seeded with the bias
    "zinit": [("    if (bias) {\n      const float4 b = *(const float4*)(bias + n0 + wn * (G::FN * 16) + j * 16 + fk * 4);",
               "    if (false) {\n      const float4 b = *(const float4*)(bias + n0 + wn * (G::FN * 16) + j * 16 + fk * 4);")],
    # operands in the pixel-major order (wrong layout for the epilogue; timing only)
    "aorder": [("mfma_f32_16x16x32_bf16(bq[cur][ks][g], fa[ks][f], acc[f][g], 0, 0, 0)",
                "mfma_f32_16x16x32_bf16(fa[ks][f], bq[cur][ks][g], acc[f][g], 0, 0, 0)")],
    # the second co-resident workgroup of each CU (dispatch slots 256..511) starts ~half a tile late
    "stag2": [(ANCHOR, "  if (blockIdx.x >= 256 && blockIdx.x < 512) for (int i = 0; i < 2; ++i) __builtin_amdgcn_s_sleep(127);\n" + ANCHOR)],
    "stag4": [(ANCHOR, "  if (blockIdx.x >= 256 && blockIdx.x < 512) for (int i = 0; i < 4; ++i) __builtin_amdgcn_s_sleep(127);\n" + ANCHOR)],
    "stag8": [(ANCHOR, "  if (blockIdx.x >= 256 && blockIdx.x < 512) for (int i = 0; i < 8; ++i) __builtin_amdgcn_s_sleep(127);\n" + ANCHOR)],
    # persistent sampler: hand-off waits skipped (results wrong; the latency of the waits)
    "ps_nowait": [("      if (__hip_atomic_load((gu32*)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= target) break;",
                   "      break;")],
    # persistent sampler: exchanged rows not re-loaded (stale registers / LDS; latency of the sc1 loads)
    "ps_noload": [("        if (r < R)\n          v = __builtin_bit_cast", "        if (r < 0)\n          v = __builtin_bit_cast"),
                  ("        const u32x4v v = __builtin_amdgcn_raw_buffer_load_b128(rs_ha, (row * W + c8) * 2, 0, PS_SC1);\n        *(u32x4v*)(sA + row * PS_LDA + c8) = v;",
                   "        (void)row; (void)c8;")],
}


FILES = {"ps_nowait": "sampler.hip", "ps_noload": "sampler.hip"}


def build(name, subs, whole=None):
    """whole: path of a complete replacement for the source file (an A/B of a rewritten kernel)."""
    fn = FILES.get(name, "conv.hip")
    src = open(whole or os.path.join(CSRC, fn)).read()
    for a, b in subs:
        if a not in src:
            raise RuntimeError(f"variant {name}: text to patch not found in {fn}:\n{a}")
        src = src.replace(a, b)
    tmp = os.path.join(CSRC, f"_diag_{name}.hip")
    open(tmp, "w").write(src)
    try:
        obj = os.path.join(AB, f"{fn[:-4]}_{name}.o")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-c", tmp, "-o", obj], check=True)
    finally:
        os.remove(tmp)
    objs = [os.path.join(OBJ, f) for f in sorted(os.listdir(OBJ)) if f.endswith(".o") and f != fn[:-4] + ".o"] + [obj]
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o",
                    os.path.join(AB, f"diag_{name}.so")] + objs, check=True)
    os.remove(obj)


if __name__ == "__main__":
    os.makedirs(AB, exist_ok=True)
    if len(sys.argv) == 4 and sys.argv[1] == "--file":  # --file NAME PATH: conv.hip replaced by PATH
        build(sys.argv[2], [], whole=sys.argv[3])
        print("built", sys.argv[2])
        sys.exit(0)
    for n in (sys.argv[1:] or VARIANTS):
        build(n, VARIANTS[n])
        print("built", n)
