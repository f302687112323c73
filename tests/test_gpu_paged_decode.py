"""Paged split-KV decode attention (attention_decode.hip) on the GPU against
the fp32 reference: numerics, independence from stale cache contents, graph
replay with new tables and lengths, and the engine option."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from megatron_amd import ops  # noqa: E402
from megatron_amd.config import TransformerConfig  # noqa: E402
from megatron_amd.inference import DynamicInferenceEngine, SamplingParams  # noqa: E402
from megatron_amd.inference.contexts import DynamicInferenceContext  # noqa: E402
from megatron_amd.models.gpt import GPTModel  # noqa: E402
from megatron_amd.ops import reference as ref  # noqa: E402
from megatron_amd.parallel import grid as G  # noqa: E402
from megatron_amd.parallel.random import model_parallel_seed  # noqa: E402

TOL = 2e-2  # the `out` tolerance of test_gpu_attention_varlen.py, same measure
HKV = 2


def _rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _case(lens, bs, rep, d, width=None, fp8=False, fill=1e4):
    """q, cache (+ scales) and a shuffled block table; block 0 and every slot
    at or past lens[i] hold `fill`, unused table entries point at block 0."""
    g = torch.Generator().manual_seed(len(lens) * 1000 + bs + rep + d)
    need = [-(-n // bs) for n in lens]
    width = width or max(need)
    nblk = sum(need) + 1
    free = (torch.randperm(nblk - 1, generator=g) + 1).tolist()
    tables = torch.zeros(len(lens), width, dtype=torch.long)
    k = torch.full((nblk * bs, HKV, d), float(fill))
    v = torch.full((nblk * bs, HKV, d), float(fill))
    for i, n in enumerate(lens):
        tables[i, : need[i]] = torch.tensor([free.pop() for _ in range(need[i])])
        pos = torch.arange(n)
        slots = tables[i, pos // bs] * bs + pos % bs
        k[slots] = torch.randn(n, HKV, d, generator=g)
        v[slots] = torch.randn(n, HKV, d, generator=g)
    q = torch.randn(len(lens), HKV * rep, d, generator=g).bfloat16().cuda()
    ks = vs = None
    if fp8:
        k, ks = DynamicInferenceContext._quantize(None, k)
        v, vs = DynamicInferenceContext._quantize(None, v)
        ks, vs = ks.cuda(), vs.cuda()
    else:
        k, v = k.bfloat16(), v.bfloat16()
    shape = (nblk, bs, HKV, d)
    return (q, k.view(shape).cuda(), v.view(shape).cuda(), tables.cuda(),
            torch.tensor(lens, dtype=torch.long).cuda(), d ** -0.5, ks, vs)


EDGES = ([1, 15, 16, 17, 33], 16, None)   # single token, block edges, slice edge
SPLITS = ([1, 500, 129], 16, 32)          # several splits, most empty, ragged last
BIG = ([255, 256, 257, 700], 256, None)
ONE = ([77], 16, None)
CASES = (
    [(*EDGES, rep, d, False) for rep in (1, 4, 8, 16) for d in (64, 128)]
    + [(*s, rep, d, False) for s in (SPLITS, BIG, ONE) for rep, d in ((4, 128), (16, 64))]
    + [(*SPLITS, 4, d, True) for d in (64, 128)]
)


@pytest.mark.parametrize("lens,bs,width,rep,d,fp8", CASES)
def test_matches_fp32_reference(lens, bs, width, rep, d, fp8):
    q, k, v, tables, ln, scale, ks, vs = _case(lens, bs, rep, d, width, fp8)
    want = ref.paged_decode_attention(q.float(), k.float(), v.float(), tables, ln, scale, ks, vs)
    got = ops.paged_decode_attention(q, k, v, tables, ln, scale, ks, vs)
    again = ops.paged_decode_attention(q, k, v, tables, ln, scale, ks, vs)
    assert got.dtype == torch.bfloat16 and torch.isfinite(got).all()
    assert _rel_err(got, want) < TOL, _rel_err(got, want)
    assert torch.equal(got, again)


@pytest.mark.parametrize("fp8", [False, True])
def test_independent_of_masked_slots(fp8):
    outs = [ops.paged_decode_attention(*_case(*SPLITS[:2], 4, 128, SPLITS[2], fp8, fill=fill))
            for fill in (1e4, -3.0)]
    assert torch.equal(outs[0], outs[1])


def test_graph_replay_with_new_tables():
    q, k, v, tables, ln, scale, _, _ = _case(*SPLITS[:2], 4, 128, SPLITS[2])
    tbuf, lbuf = tables.roll(1, 0).contiguous(), ln.roll(1).contiguous()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            ops.paged_decode_attention(q, k, v, tbuf, lbuf, scale)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = ops.paged_decode_attention(q, k, v, tbuf, lbuf, scale)
    tbuf.copy_(tables)
    lbuf.copy_(ln)
    want = ops.paged_decode_attention(q, k, v, tables, ln, scale)
    for _ in range(2):
        graph.replay()
        assert torch.equal(out, want)


@pytest.fixture()
def gpu_model():
    G.destroy_model_parallel()
    G.initialize_model_parallel(world_size=1, rank=0)
    model_parallel_seed(77)
    cfg = TransformerConfig(
        num_layers=2, hidden_size=256, num_attention_heads=4, num_query_groups=2,
        ffn_hidden_size=512, vocab_size=512, max_position_embeddings=512, bf16=True,
    )
    yield GPTModel(cfg).cuda().eval()
    G.destroy_model_parallel()


def test_engine_paged_graph_matches_eager(gpu_model):
    prompts = [[3, 7, 11, 2, 9], [5, 1], list(range(40, 80))]
    params = SamplingParams(max_tokens=8, greedy=True, stop_on_eod=False)
    runs = [DynamicInferenceEngine(gpu_model, num_blocks=32, block_size=16, use_hip_graphs=graphs,
                                   decode_attention="paged").generate(prompts, params)
            for graphs in (False, True)]
    for a, b in zip(*runs):
        assert len(a.output_tokens) == 8 and a.output_tokens == b.output_tokens


@pytest.mark.parametrize("kv_cache_dtype", [None, "fp8"])
def test_context_paged_close_to_gather(kv_cache_dtype):
    hq, d, bs, lens = 4, 64, 16, [37, 5, 16]
    g = torch.Generator().manual_seed(3)
    tables = [[4, 2, 7], [5], [1, 6]]
    new = [torch.randn(1, len(lens), h, d, generator=g).bfloat16().cuda() for h in (hq, HKV, HKV)]
    outs = {}
    for mode in ("gather", "paged"):
        ctx = DynamicInferenceContext(1, HKV, d, num_blocks=8, block_size=bs,
                                      kv_cache_dtype=kv_cache_dtype, decode_attention=mode)
        fill = torch.Generator().manual_seed(4)
        for cache in (ctx.k_cache[0], ctx.v_cache[0]):
            cache.copy_(torch.randn(cache.shape, generator=fill))
        ctx.begin_decode(tables, lens)
        outs[mode] = ctx.attend(0, *new, d ** -0.5)
    assert _rel_err(outs["paged"], outs["gather"]) < TOL
