"""In-tree builds for the fiber_amd native extensions.

  python setup.py build_ext --inplace

Builds:
  fiber_amd._transport — C++ shm-ring engine (host-only, g++)
  fiber_amd._ops       — CDNA4 HIP kernels (hipcc --offload-arch=gfx950)

The HIP extension is compiled with hipcc directly (no torch headers), so
the whole build cross-compiles on a GPU-less box in seconds.
"""

import os
import subprocess
import sys

import pybind11
from setuptools import setup
from setuptools.command.build_ext import build_ext as _build_ext
from setuptools.extension import Extension

ROOT = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GFX_ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")


def ext_suffix():
    import sysconfig

    return sysconfig.get_config_var("EXT_SUFFIX")


class build_ext(_build_ext):
    def run(self):
        super().run()
        self.build_hip_ops()

    def build_hip_ops(self):
        out = os.path.join(ROOT, "fiber_amd", "_ops" + ext_suffix())
        srcs = [
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "es_kernels.hip"),
            # includes the shared device code of es_kernels.hip, but is a
            # translation unit of its own (register budget, see the file)
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "es_pairs_kernels.hip"),
            # novelty-search rollout + kNN kernels: the same arrangement
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "ns_kernels.hip"),
            # separable-NES rollout + two-row gradient: the same arrangement
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "snes_kernels.hip"),
            # Deep GA rollout, truncation and seed-chain decode: the same
            # arrangement
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "ga_kernels.hip"),
            # safe-mutation steps (forward + backward of the policy) and
            # the GA rollout / survivors with a step row per parent: the
            # same arrangement
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "sm_kernels.hip"),
            # MAP-Elites rollout with a BC, archive insert and compaction:
            # the same arrangement
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "me_kernels.hip"),
            # PATA-EC novelty kernels: shares nothing with the rollout
            # kernels and stays out of their register allocation
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "poet_kernels.hip"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "conv_kernels.hip"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "bindings.cpp"),
        ]
        hdrs = [
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "philox.h"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "ga_shared.h"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "bc_epilogue.h"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "me_grid.h"),
        ]
        if os.path.exists(out):
            newest_src = max(os.path.getmtime(s) for s in srcs + hdrs)
            if os.path.getmtime(out) >= newest_src:
                print("fiber_amd._ops up to date")
                return
        cmd = [
            HIPCC,
            "--offload-arch=" + GFX_ARCH,
            "-O3",
            "-std=c++17",
            # VGPR-form MFMA: keeps accumulators in arch VGPRs so the
            # epilogue math needs no v_accvgpr_read moves (32/step in
            # the rollout loop, -8% issue count; occupancy unchanged —
            # gfx950's register file is unified anyway).
            "-mllvm",
            "-amdgpu-mfma-vgpr-form=1",
            "-fPIC",
            "-shared",
            "-I",
            pybind11.get_include(),
            "-I",
            os.path.join(sys.prefix, "include", "python%d.%d" % sys.version_info[:2]),
            "-I",
            "/usr/include/python%d.%d" % sys.version_info[:2],
        ] + srcs + ["-o", out]
        print(" ".join(cmd))
        subprocess.check_call(cmd)


setup(
    name="fiber_amd",
    version="0.1.0",
    packages=[
        "fiber_amd",
        "fiber_amd.backends",
        "fiber_amd.ops",
        "fiber_amd.es",
        "fiber_amd.experimental",
    ],
    ext_modules=[
        Extension(
            "fiber_amd._transport",
            sources=["fiber_amd/csrc/transport.cpp"],
            include_dirs=[pybind11.get_include()],
            extra_compile_args=["-O2", "-std=c++17"],
            libraries=["pthread", "rt"],
        )
    ],
    cmdclass={"build_ext": build_ext},
)
