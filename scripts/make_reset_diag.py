"""Builds the reset-phase-timer diagnostic library (scripts/reset_stamps.py reads it): a COPY of
csrc/env_step.hip with s_memtime stamps after each phase of env_reset_kernel, written to
dgppo_fov_amd/_build/rdiag/env_step.hip and compiled with -DDGPPO_ENV_STAMPS into
dgppo_fov_amd/lib/libdgppo_hip_rdiag.so (the shipped sources stay stamp-free, so their hash does not move).
Run `make` first: every other object is the in-tree build."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = open(os.path.join(ROOT, "dgppo_fov_amd/csrc/env_step.hip")).read()
RSTAMP = """
  uint64_t rs_t = __builtin_amdgcn_s_memtime();
#ifndef RSTAMP
#define RSTAMP(k) do { if (threadIdx.x == 0) { const uint64_t now_ = __builtin_amdgcn_s_memtime(); \\
    atomicAdd(&wv::g_env_stamps[k], (unsigned long long)(now_ - rs_t)); rs_t = now_; } } while (0)
#endif
"""
# the sampling phases live in sample_states (shared with the persistent rollout's reset_first prologue), the store /
# graph phases in env_reset_kernel: each gets its own running stamp
k0 = src.index("__device__ __forceinline__ void sample_states(const dgppo_env_cfg& cfg, Rng rng, int tid, int n, int O, "
               "Sync sync,\n", src.index("__device__ __forceinline__ void WaveSync::operator()"))
b0 = src.index("{", k0) + 1
src = src[:b0] + RSTAMP + src[b0:]
k1 = src.index("void env_reset_kernel(dgppo_env_cfg cfg, dgppo_env_reset_io io, int states_only) {")
b1 = src.index("{", k1) + 1
src = src[:b1] + RSTAMP + src[b1:]
marks = [("  uint32_t rng_count = (uint32_t)n_ob_draws;\n  sync();\n", 0),
         ("    tab[2 * k + 1] = r.uniform(0.0f, area);\n  }\n  sync();\n", 1),
         ("    if (NTHR > 64 && tid == 0) *count_slot = rng.count;\n  }\n  sync();\n", 2),
         ("    goal[idx] = c < 2 ? gl[2 * i + c] : 0.0f;\n  }\n  sync();\n", 3),
         ("        for (int c = 0; c < SD; ++c) third[o * SD + c] = c == 0 ? cx : (c == 1 ? cy : 0.0f);\n"
          "      }\n    }\n  }\n  sync();\n", 4),
         ("  if (states_only) {  // the wave step kernel builds the graph from these rows (dgppo_env_reset)\n", 5),
         ("  graph_of_staged_rows<ENGINE, GOAL, SD, BLOCK>(cfg, io, d, cv, lds, env);\n", 7)]  # (ray cast + graph)
pos = b0
for anchor, k in marks:
    i = src.index(anchor, pos) + len(anchor)
    src = src[:i] + f"  RSTAMP({k});\n" + src[i:]
    pos = i
out = os.path.join(ROOT, "dgppo_fov_amd/_build/rdiag")
os.makedirs(out, exist_ok=True)
open(os.path.join(out, "env_step.hip"), "w").write(src)
hipcc = "/opt/rocm/bin/hipcc"
obj = os.path.join(ROOT, "dgppo_fov_amd/_build/env_step_rdiag.o")
subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Iinclude", "-Idgppo_fov_amd/csrc",
                       "-DDGPPO_ENV_STAMPS", "-c", os.path.join(out, "env_step.hip"), "-o", obj], cwd=ROOT)
objs = [o for o in sorted(glob.glob(os.path.join(ROOT, "dgppo_fov_amd/_build/*.o"))) if "env_step" not in os.path.basename(o)]
subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-o",
                       os.path.join(ROOT, "dgppo_fov_amd/lib/libdgppo_hip_rdiag.so")] + objs + [obj], cwd=ROOT)
print("built dgppo_fov_amd/lib/libdgppo_hip_rdiag.so")
