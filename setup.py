"""In-tree extension build for spacy_ray_amd.

Build everything in place (the built .so files travel to the GPU box with the
repo snapshot):

    python setup.py build_ext --inplace

Two extensions:
  * spacy_ray_amd._srx_cpu — pybind11/C++ core (murmur hashing, transition
    systems).  Plain g++, no GPU needed.
  * spacy_ray_amd._srx_hip — CDNA4 (gfx950) HIP kernels as a torch extension;
    hipcc cross-compiles on a GPU-less box (PYTORCH_ROCM_ARCH=gfx950).  Every
    kernels/*.hip is one translation unit of it: srx_ext.hip (the module
    block), one srx_bind_<family>.hip of launchers per kernel family,
    srx_steploop.hip and srx_gpustate.hip.
  * spacy_ray_amd._srx_hip_vecsim — the cosine top-n kernels
    (srx_vecsim_ext.hip), compiled with packed fp32 instructions off.
"""
import os
import sys
from pathlib import Path

from setuptools import Extension, find_packages, setup

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

ROOT = Path(__file__).parent
CSRC = ROOT / "spacy_ray_amd" / "ops" / "csrc"
KERNELS = ROOT / "spacy_ray_amd" / "ops" / "kernels"

import pybind11

ext_modules = [
    Extension(
        "spacy_ray_amd._srx_cpu",
        sources=[
            str(CSRC / "cpu_ext.cpp"),
            str(CSRC / "transitions.cpp"),
        ],
        include_dirs=[pybind11.get_include()],
        extra_compile_args=["-O3", "-std=c++17", "-fvisibility=hidden", "-fopenmp"],
        extra_link_args=["-fopenmp"],
        language="c++",
    )
]

cmdclass = {}
# exclude hipify-generated *_hip.hip artifacts from previous builds
# srx_vecsim_ext.hip is an extension of its own (other compiler flags)
VECSIM_SRC = KERNELS / "srx_vecsim_ext.hip"
hip_sources = [p for p in sorted(KERNELS.glob("*.hip"))
               if not p.name.endswith("_hip.hip") and p != VECSIM_SRC]
if hip_sources and "SRX_SKIP_HIP" not in os.environ:
    from torch.utils.cpp_extension import BuildExtension, CUDAExtension

    ext_modules.append(
        CUDAExtension(
            "spacy_ray_amd._srx_hip",
            sources=[str(p) for p in hip_sources],
            extra_compile_args={
                "cxx": ["-O3", "-std=c++17"],
                "nvcc": ["-O3", "-std=c++17"],
            },
        )
    )
    if VECSIM_SRC.exists():
        # no v_pk_{add,mul,fma}_f32 in this module: scalar fp32 VALU only
        no_packed_fp32 = ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
        ext_modules.append(
            CUDAExtension(
                "spacy_ray_amd._srx_hip_vecsim",
                sources=[str(VECSIM_SRC)],
                extra_compile_args={
                    "cxx": ["-O3", "-std=c++17"],
                    "nvcc": ["-O3", "-std=c++17"] + no_packed_fp32,
                },
            )
        )
    cmdclass["build_ext"] = BuildExtension

setup(
    name="spacy_ray_amd",
    version="0.1.0",
    packages=find_packages(include=["spacy_ray_amd", "spacy_ray_amd.*"]),
    ext_modules=ext_modules,
    cmdclass=cmdclass,
    entry_points={
        "console_scripts": [
            "spacy-mi = spacy_ray_amd.cli.main:main",
            # reference-compatible command name: `spacy ray train ...`
            # (BASELINE.json CLI-compat requirement; only the `ray` sub-app
            # is provided)
            "spacy = spacy_ray_amd.cli.main:main",
        ]
    },
)
