"""Build libunimm_hip.so (all HIP kernels + the C ABI) in-tree with hipcc for gfx950, and beside it the extension library
libraries libunimm_mix.so (csrc/mix/, include/unimm_mix.h: ensemble answer generation) and libunimm_reward.so (csrc/reward/,
include/unimm_reward.h: the CIDEr-D consensus reward) the same way.

hipcc cross-compiles without a GPU, so this runs in the CPU-only build container; the .so travels
to the GPU box with the repo snapshot (it is git-ignored, not gpurun-ignored)."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libunimm_hip.so")
OBJ = os.path.join(CSRC, "_obj")
MIX_SRC = os.path.join(CSRC, "mix")
MIX_LIB = os.path.join(PKG, "libunimm_mix.so")
REWARD_SRC = os.path.join(CSRC, "reward")
REWARD_LIB = os.path.join(PKG, "libunimm_reward.so")
ARCH = "gfx950"
FLAGS = ["--offload-arch=" + ARCH, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=fast", "-Wno-unused-result"]


def sources(directory=CSRC):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.endswith(".hip"))


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        raise RuntimeError("hipcc not found: cannot build libunimm_hip.so")
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(PKG), "include", "unimm_hip.h"))
    mix_headers = headers + [os.path.join(os.path.dirname(PKG), "include", "unimm_mix.h")]
    mix_obj = lambda s: os.path.join(OBJ, "mix_" + os.path.basename(s)[:-4] + ".o")     # noqa: E731
    jobs = []
    for src in sources():
        obj = os.path.join(OBJ, os.path.basename(src)[:-4] + ".o")
        if force or _stale(obj, [src] + headers):
            jobs.append((src, obj))
    mix_jobs = [(src, mix_obj(src)) for src in sources(MIX_SRC) if force or _stale(mix_obj(src), [src] + mix_headers)]
    reward_headers = headers + [os.path.join(os.path.dirname(PKG), "include", "unimm_reward.h")]
    reward_obj = lambda s: os.path.join(OBJ, "reward_" + os.path.basename(s)[:-4] + ".o")     # noqa: E731
    reward_jobs = [(src, reward_obj(src)) for src in sources(REWARD_SRC) if force or _stale(reward_obj(src), [src] + reward_headers)]

    def compile_one(job):
        src, obj = job
        cmd = [hipcc] + FLAGS + ["-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr}")
        if verbose:
            print("compiled", os.path.basename(src), file=sys.stderr)

    with ThreadPoolExecutor(max_workers=8) as ex:
        list(ex.map(compile_one, jobs + mix_jobs + reward_jobs))
    objs = [os.path.join(OBJ, os.path.basename(s)[:-4] + ".o") for s in sources()]
    if force or jobs or _stale(LIB, objs):
        r = subprocess.run([hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", LIB] + objs,
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n" + r.stderr)
    objs = [mix_obj(s) for s in sources(MIX_SRC)]
    if force or mix_jobs or _stale(MIX_LIB, objs):
        r = subprocess.run([hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", MIX_LIB] + objs,
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n" + r.stderr)
    objs = [reward_obj(s) for s in sources(REWARD_SRC)]
    if force or reward_jobs or _stale(REWARD_LIB, objs):
        r = subprocess.run([hipcc, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", REWARD_LIB] + objs,
                           capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("link failed:\n" + r.stderr)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
