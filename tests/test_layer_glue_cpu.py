"""Layer glue off the GPU: the fused ops fall back to the separate ones."""

import torch

from megatron_amd import ops
from megatron_amd.ops import reference as ref


def test_add_rms_norm_cpu_is_add_then_norm():
    torch.manual_seed(0)
    x = torch.randn(7, 32, requires_grad=True)
    r = torch.randn(7, 32, requires_grad=True)
    w = torch.randn(32, requires_grad=True)
    total, normed = ops.add_rms_norm(x, r, w, 1e-5)
    want_total = ops.bias_dropout_add(x, None, r, 0.0, True)
    assert torch.equal(total, want_total)
    assert torch.equal(normed, ops.rms_norm(want_total, w, 1e-5))
    (total.sum() + normed.sum()).backward()
    assert x.grad is not None and torch.equal(x.grad, r.grad)


def test_qkv_split_rope_not_fused_on_cpu_or_under_switch(monkeypatch):
    qkv = torch.randn(4, 1, 2, 4 * 16, dtype=torch.bfloat16)
    freqs = ref.rope_freqs(4, 16)
    assert not ops.qkv_split_rope_fused(qkv, freqs, 2)
    assert not ops.qkv_split_rope_fused(qkv, None, 2)
    monkeypatch.setenv("MEGATRON_AMD_UNFUSED_GLUE", "1")
    assert ops.unfused_glue()
    assert not ops.qkv_split_rope_fused(qkv, freqs, 2)
