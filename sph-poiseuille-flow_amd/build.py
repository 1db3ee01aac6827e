"""Build libsphx.so (HIP kernels + C ABI) for gfx950 with hipcc, in-tree.

hipcc cross-compiles without a GPU.  The shared object lands next to the sources
(sph-poiseuille-flow_amd/csrc/libsphx.so) so it travels with the tree to the GPU box.
"""
from __future__ import annotations

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SOURCES = ["sphx_common.hip", "sphx_pairlist.hip", "sphx_resident.hip"]
HEADERS = ["sphx_common.hpp", "sphx_device.hpp", "sphx_kernels.hpp", "sphx_slot_sample.hpp", "sphx_flow_stats.hpp", "sphx_history.hpp", "sphx_field_map.hpp",
           "sphx_probes.hpp", "sphx_profile_series.hpp", "sphx_pair_dist.hpp", "sphx_grad_stats.hpp", "sphx_tracers.hpp", "sphx_dens_stats.hpp", "sphx_modes.hpp", "sphx_sampler_state.hpp", "sphx_samplers.hpp", "sphx_batch.hpp", "sphx_xcd_block.hpp", os.path.join("..", "..", "include", "sphx.h")]
LIB = os.path.join(CSRC, "libsphx.so")
FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC",
         "-fvisibility=hidden", "-Wall", "-Wno-unused-function"]
# sphx_resident.hip: the leading scalar / pointer parameters of a kernel, up to 14 dwords, arrive in registers with the wave
# (csrc/sphx_kernels.hpp, "Leading arguments"); the option counts parameters and stops at the first struct passed by value
SOURCE_FLAGS = {"sphx_resident.hip": ["-mllvm", "-amdgpu-kernarg-preload-count=14"],
                "sphx_devtest.hip": ["-mllvm", "-amdgpu-kernarg-preload-count=14"]}
# Test-only second library (csrc/sphx_devtest.hip): the __device__ functions of the headers, each wrapped in a kernel of its own
# for tests/devtest.py.  Built with sphx_resident.hip's flags from the same headers; never linked into libsphx.so.
DEVTEST_SOURCE = "sphx_devtest.hip"
DEVTEST_LIB = os.path.join(CSRC, "libsphx_devtest.so")


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (need ROCm to build libsphx.so)")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps if os.path.exists(d))


def build(force: bool = False, verbose: bool = False) -> str:
    hipcc = _hipcc()
    srcs = [os.path.join(CSRC, s) for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    hdrs = [os.path.join(CSRC, h) for h in HEADERS]
    objs = []
    for src in srcs:
        obj = src[:-4] + ".o"
        if force or _stale(obj, [src, os.path.abspath(__file__)] + hdrs):
            cmd = [hipcc] + FLAGS + SOURCE_FLAGS.get(os.path.basename(src), []) + ["-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd))
            subprocess.check_call(cmd)
        objs.append(obj)
    if force or _stale(LIB, objs):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB] + objs
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    build_devtest(force=force, verbose=verbose)
    return LIB


def build_devtest(force: bool = False, verbose: bool = False, csrc: str = CSRC, lib: str | None = None) -> str:
    """The test-only harness library.  csrc / lib: build it from another copy of csrc/ (a deliberately altered header, see
    profiles/r33_device_formulas.txt) into another file, for tests/devtest.py's SPHX_DEVTEST_LIB."""
    hipcc = _hipcc()
    lib = lib or (DEVTEST_LIB if csrc == CSRC else os.path.join(csrc, "libsphx_devtest.so"))
    src = os.path.join(csrc, DEVTEST_SOURCE)
    obj = src[:-4] + ".o"
    hdrs = [os.path.join(csrc, h) for h in HEADERS]
    if force or _stale(obj, [src, os.path.abspath(__file__)] + hdrs):
        cmd = [hipcc] + FLAGS + SOURCE_FLAGS[DEVTEST_SOURCE] + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    if force or _stale(lib, [obj]):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, obj]
        if verbose:
            print(" ".join(cmd))
        subprocess.check_call(cmd)
    return lib


if __name__ == "__main__":
    print(build(verbose=True))
