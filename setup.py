"""In-tree build of the megatron_amd CDNA4 HIP extension.

    PYTORCH_ROCM_ARCH=gfx950 python setup.py build_ext --inplace

Builds megatron_amd/ops/_hip_ops.so next to the package sources so the
gpurun snapshot carries the binary (no site-packages install, no JIT cache).
"""

import os

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")

from setuptools import setup
from torch.utils.cpp_extension import BuildExtension, CppExtension, CUDAExtension

SRC = [
    "megatron_amd/ops/csrc/bindings.cpp",
    "megatron_amd/ops/csrc/rmsnorm.hip",
    "megatron_amd/ops/csrc/swiglu.hip",
    "megatron_amd/ops/csrc/rope.hip",
    "megatron_amd/ops/csrc/qkv_rope.hip",
    "megatron_amd/ops/csrc/adamw.hip",
    "megatron_amd/ops/csrc/wgrad.hip",
    "megatron_amd/ops/csrc/cross_entropy.hip",
    "megatron_amd/ops/csrc/grouped_gemm.cpp",
    "megatron_amd/ops/csrc/grouped_gemm_hip.hip",
    "megatron_amd/ops/csrc/mx_quant.hip",
    "megatron_amd/ops/csrc/mx_gemm.hip",
    "megatron_amd/ops/csrc/causal_conv1d.hip",
    "megatron_amd/ops/csrc/ssd_scan.hip",
    "megatron_amd/ops/csrc/attention_fwd.hip",
    "megatron_amd/ops/csrc/attention_bwd.hip",
    "megatron_amd/ops/csrc/attention_varlen.hip",
    "megatron_amd/ops/csrc/attention_decode.hip",
    "megatron_amd/ops/csrc/attention_prefill_paged.hip",
    "megatron_amd/ops/csrc/symm_allreduce.hip",
]

setup(
    name="megatron_amd_hip_ops",
    ext_modules=[
        CUDAExtension(
            name="megatron_amd.ops._hip_ops",
            sources=SRC,
            extra_compile_args={
                "cxx": ["-O3", "-std=c++17"],
                "nvcc": ["-O3", "-std=c++17", "--offload-arch=gfx950"]
                + os.environ.get("MEGATRON_AMD_HIPCC_EXTRA", "").split(),
            },
            libraries=["rocblas", "hipblaslt"],
        ),
        CppExtension(
            name="megatron_amd.datasets._data_helpers",
            sources=["megatron_amd/datasets/csrc/data_helpers.cpp"],
            extra_compile_args={"cxx": ["-O3", "-std=c++17"]},
        ),
    ],
    cmdclass={"build_ext": BuildExtension.with_options(use_ninja=True)},
)
