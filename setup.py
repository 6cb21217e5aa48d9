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
            # low-rank correlated perturbations (LM-MA-ES): the policy fill
            # with its two passes over the direction rows, in front of the
            # shared step loop; the same arrangement, on this command 72
            # VGPRs and no scratch (profiles/lmmaes.md)
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "lowrank_kernels.hip"),
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
            # LSTM recurrent policy: a translation unit of its own like the
            # files above.  Unlike the GRU and wide files below it needs no
            # flag of its own: on this command es_rollout_lstm has 128 VGPRs
            # and no scratch, with packed fp32 off it spills
            # (profiles/lstm.md)
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "lstm_kernels.hip"),
            # CartPole environment for the MLP policy: the same arrangement,
            # on this command 72 VGPRs or fewer and no scratch
            # (profiles/cartpole.md)
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "cartpole_kernels.hip"),
            # LSTM policy on CartPole: includes the shared device code of
            # lstm_kernels.hip (LSTM_KERNELS_SHARED_ONLY) and cart_physics.h,
            # a translation unit of its own like the two above; on this
            # command 122 VGPRs and no scratch (profiles/lstm_cartpole.md)
            os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                         "lstm_cartpole_kernels.hip"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "bindings.cpp"),
        ]
        # GRU recurrent policy: shares es_kernels.hip's device code like the
        # files above, but is compiled on its own with packed fp32
        # instructions off, and joins the link as an object.  The flag is
        # what keeps es_rollout_gru free of scratch: with packed fp32 on
        # it spills 5 VGPRs (24 B/lane) at its 128-VGPR budget, with it off
        # it has 128 VGPRs and none (profiles/gru.md).  A flag on the one
        # command that compiles srcs would change every other kernel, hence
        # the separate compile.  The object reaches the link as -Wl,<path>:
        # named plainly next to the .hip sources, hipcc reads it as HIP
        # source text and the build fails.
        gru_src = os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                               "gru_kernels.hip")
        # wide MLP policies (hidden 128 / 256): the same arrangement, and
        # the same flag
        wide_src = os.path.join(ROOT, "fiber_amd", "csrc", "ops",
                                "wide_kernels.hip")
        hdrs = [
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "philox.h"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "ga_shared.h"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "bc_epilogue.h"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "me_grid.h"),
            os.path.join(ROOT, "fiber_amd", "csrc", "ops", "cart_physics.h"),
        ]
        if os.path.exists(out):
            newest_src = max(os.path.getmtime(s)
                             for s in srcs + hdrs + [gru_src, wide_src])
            if os.path.getmtime(out) >= newest_src:
                print("fiber_amd._ops up to date")
                return
        common = [
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
        ]
        os.makedirs(self.build_temp, exist_ok=True)
        objs = []
        for src in (gru_src, wide_src):
            obj = os.path.join(
                self.build_temp,
                os.path.splitext(os.path.basename(src))[0] + ".o")
            obj_cmd = common + [
                "-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops",
                "-c", src, "-o", obj,
            ]
            print(" ".join(obj_cmd))
            subprocess.check_call(obj_cmd)
            objs.append(obj)
        cmd = common + [
            "-shared",
            "-I",
            pybind11.get_include(),
            "-I",
            os.path.join(sys.prefix, "include", "python%d.%d" % sys.version_info[:2]),
            "-I",
            "/usr/include/python%d.%d" % sys.version_info[:2],
        ] + srcs + ["-Wl," + o for o in objs] + ["-o", out]
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
