"""Paged prefill attention (attention_prefill_paged.hip) on the GPU against
the fp32 reference: numerics over chunk offsets, q-block and tile edges, fp8
caches and sliding windows, independence from dead cache slots, and the
context option."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from megatron_amd import ops  # noqa: E402
from megatron_amd.inference.contexts import DynamicInferenceContext  # noqa: E402
from megatron_amd.ops import reference as ref  # noqa: E402

TOL = 2e-2  # test_gpu_paged_decode.py: same measure, same bound
HKV = 2
Q = 256     # q rows per block of the kernel


def _rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _case(prior, s, bs, rep, d, width=None, fp8=False, fill=1e4):
    """q, cache (+ scales) and a shuffled block table; block 0 and every slot
    at or past prior + s hold `fill`, unused table entries point at block 0."""
    g = torch.Generator().manual_seed(prior * 1000 + s + bs + rep + d)
    n = prior + s
    need = -(-n // bs)
    table = torch.zeros(width or need, dtype=torch.long)
    table[:need] = torch.randperm(need, generator=g) + 1
    k = torch.full(((need + 1) * bs, HKV, d), float(fill))
    v = torch.full(((need + 1) * bs, HKV, d), float(fill))
    pos = torch.arange(n)
    slots = table[pos // bs] * bs + pos % bs
    k[slots] = torch.randn(n, HKV, d, generator=g)
    v[slots] = torch.randn(n, HKV, d, generator=g)
    q = torch.randn(s, HKV * rep, d, generator=g).bfloat16().cuda()
    ks = vs = None
    if fp8:
        k, ks = DynamicInferenceContext._quantize(None, k)
        v, vs = DynamicInferenceContext._quantize(None, v)
        ks, vs = ks.cuda(), vs.cuda()
    else:
        k, v = k.bfloat16(), v.bfloat16()
    shape = (need + 1, bs, HKV, d)
    return q, k.view(shape).cuda(), v.view(shape).cuda(), table.cuda(), prior, d ** -0.5, ks, vs


SMALL = [(0, 1, 16), (0, 65, 16), (5, 1, 16), (17, 3, 16)]
LARGE = [(100, Q + 2, 16), (70, 2 * Q + 44, 16), (640, 40, 16), (300, 260, 256)]
CASES = (
    [(*c, rep, d, False, None) for c in SMALL for rep in (1, 4, 8) for d in (64, 128)]
    + [(*c, rep, d, False, None) for c in LARGE for rep, d in ((4, 128), (8, 64))]
    + [(*c, 4, d, True, None) for c in (SMALL[3], LARGE[0]) for d in (64, 128)]
    + [(*c, 4, 128, False, w) for c in (LARGE[0], LARGE[2]) for w in (1, 48, 200, 10000)]
)


@pytest.mark.parametrize("prior,s,bs,rep,d,fp8,window", CASES)
def test_matches_fp32_reference(prior, s, bs, rep, d, fp8, window):
    q, k, v, table, prior, scale, ks, vs = _case(prior, s, bs, rep, d, fp8=fp8)
    want = ref.paged_prefill_attention(q.float(), k.float(), v.float(), table, prior, scale, window, ks, vs)
    got = ops.paged_prefill_attention(q, k, v, table, prior, scale, window, ks, vs)
    again = ops.paged_prefill_attention(q, k, v, table, prior, scale, window, ks, vs)
    assert got.dtype == torch.bfloat16 and torch.isfinite(got).all()
    assert _rel_err(got, want) < TOL, _rel_err(got, want)
    assert torch.equal(got, again)


@pytest.mark.parametrize("fp8", [False, True])
def test_independent_of_dead_slots(fp8):
    outs = []
    for fill in (1e4, -3.0):
        q, k, v, table, prior, scale, ks, vs = _case(100, Q + 2, 16, 4, 128, width=40, fp8=fp8, fill=fill)
        outs.append(ops.paged_prefill_attention(q, k, v, table, prior, scale, None, ks, vs))
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("kv_cache_dtype", [None, "fp8"])
def test_context_paged_close_to_gather(kv_cache_dtype):
    hq, d, bs, prior, s = 4, 64, 16, 21, 19
    g = torch.Generator().manual_seed(3)
    new = [torch.randn(s, 1, h, d, generator=g).bfloat16().cuda() for h in (hq, HKV, HKV)]
    outs, caches = {}, {}
    for mode in ("gather", "paged"):
        ctx = DynamicInferenceContext(1, HKV, d, num_blocks=8, block_size=bs,
                                      kv_cache_dtype=kv_cache_dtype, prefill_attention=mode)
        fill = torch.Generator().manual_seed(4)
        for cache in (ctx.k_cache[0], ctx.v_cache[0]):
            cache.copy_(torch.randn(cache.shape, generator=fill))
        ctx.begin_prefill([4, 2, 7], prior_len=prior)
        outs[mode] = ctx.attend(0, *new, d ** -0.5)
        caches[mode] = [c.view(torch.uint8) if ctx.kv_fp8 else c for c in (ctx.k_cache[0], ctx.v_cache[0])]
        if ctx.kv_fp8:
            caches[mode] += [ctx.k_scale[0], ctx.v_scale[0]]
    assert outs["paged"].shape == outs["gather"].shape
    assert _rel_err(outs["paged"], outs["gather"]) < TOL
    assert all(torch.equal(a, b) for a, b in zip(caches["gather"], caches["paged"]))
