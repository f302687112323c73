"""The moe_grouped_gemm_kernel option and ops.grouped_linear(kernel=...) without
a GPU: CPU tensors take the per-expert loop unchanged."""

import pytest
import torch

from megatron_amd import ops
from megatron_amd.config import TransformerConfig
from tests.utils import init_single


def test_unknown_option_value_raises():
    from megatron_amd.moe.experts import GroupedMLP

    init_single()
    cfg = TransformerConfig(num_layers=1, hidden_size=32, num_attention_heads=4, vocab_size=64,
                            num_experts=4, moe_ffn_hidden_size=48, moe_grouped_gemm_kernel="triton")
    with pytest.raises(ValueError, match="moe_grouped_gemm_kernel"):
        GroupedMLP(cfg)


def test_unknown_kernel_name_raises():
    with pytest.raises(ValueError, match="kernel"):
        ops.grouped_linear(torch.zeros(2, 8), torch.zeros(1, 4, 8), [2], kernel="triton")


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_hip_on_cpu_tensors_is_the_loop(dtype):
    g = torch.Generator().manual_seed(0)
    a, w = torch.randn(9, 64, generator=g).to(dtype), torch.randn(3, 128, 64, generator=g).to(dtype)
    got = ops.grouped_linear(a, w, torch.tensor([4, 0, 5]), kernel="hip")
    assert torch.equal(got, ops.grouped_linear(a, w, [4, 0, 5]))
    assert torch.equal(got, torch.cat([a[:4] @ w[0].t(), a[4:] @ w[2].t()]))
    # sizes that sum to less than M: the rows past the sum are zeros on the fallback too
    short = ops.grouped_linear(a, w, torch.tensor([4, 0, 3]), kernel="hip")
    assert torch.equal(short[:7], torch.cat([a[:4] @ w[0].t(), a[4:7] @ w[2].t()]))
    assert short.shape == got.shape and (short[7:] == 0).all()
