"""ops.paged_prefill_attention on CPU (the reference path) against a gather
through the block table plus reference.attention, and the context option."""

import pytest
import torch

from megatron_amd import ops
from megatron_amd.inference.contexts import DynamicInferenceContext
from megatron_amd.ops import reference as ref


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("window", [None, 5])
def test_cpu_op_matches_gather_route(fp8, window):
    g = torch.Generator().manual_seed(0)
    bs, hkv, hq, d, prior, s = 4, 2, 6, 8, 7, 6
    table = torch.tensor([5, 2, 7, 1, 0])
    k = torch.randn(8 * bs, hkv, d, generator=g)
    v = torch.randn(8 * bs, hkv, d, generator=g)
    q = torch.randn(s, hq, d, generator=g)
    ks = vs = None
    if fp8:
        k, ks = DynamicInferenceContext._quantize(None, k)
        v, vs = DynamicInferenceContext._quantize(None, v)
    pos = torch.arange(prior + s)
    slots = table[pos // bs] * bs + pos % bs
    kg, vg = k[slots], v[slots]
    if fp8:
        kg, vg = kg.float() * ks[slots].unsqueeze(-1), vg.float() * vs[slots].unsqueeze(-1)
    want = ref.attention(q.unsqueeze(1), kg.unsqueeze(1), vg.unsqueeze(1), causal=True, scale=0.3,
                         window=window)[:, 0]
    got = ops.paged_prefill_attention(q, k.view(8, bs, hkv, d), v.view(8, bs, hkv, d), table, prior, 0.3,
                                      window, ks, vs)
    assert torch.equal(got, want)


@pytest.mark.parametrize("kv_cache_dtype", [None, "fp8"])
def test_cpu_context_paged_equals_gather(kv_cache_dtype):
    hq, hkv, d, bs, prior, s = 4, 2, 8, 4, 6, 5
    g = torch.Generator().manual_seed(1)
    new = [torch.randn(s, 1, h, d, generator=g) for h in (hq, hkv, hkv)]
    outs = []
    for mode in ("gather", "paged"):
        ctx = DynamicInferenceContext(1, hkv, d, num_blocks=8, block_size=bs, dtype=torch.float32,
                                      device="cpu", kv_cache_dtype=kv_cache_dtype, prefill_attention=mode)
        fill = torch.Generator().manual_seed(2)
        for cache in (ctx.k_cache[0], ctx.v_cache[0]):
            cache.copy_(torch.randn(cache.shape, generator=fill))
        ctx.begin_prefill([3, 6, 1], prior_len=prior)
        outs.append(ctx.attend(0, *new, d ** -0.5, window=7))
    assert torch.equal(outs[0], outs[1])
