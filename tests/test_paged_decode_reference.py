"""ops.paged_decode_attention on CPU (the fp32 reference path) against the
gather + masked-attention route of the dynamic context, and the engine option."""

import torch

from megatron_amd import ops
from megatron_amd.config import TransformerConfig
from megatron_amd.inference import DynamicInferenceEngine, SamplingParams
from megatron_amd.inference.contexts import _masked_decode_attention
from megatron_amd.models.gpt import GPTModel
from megatron_amd.parallel import grid as G
from megatron_amd.parallel.random import model_parallel_seed


def test_cpu_op_matches_gather_route():
    g = torch.Generator().manual_seed(0)
    bs, hkv, hq, d = 4, 2, 6, 8
    lens = torch.tensor([1, 4, 9, 6])
    tables = torch.tensor([[5, 0, 0], [2, 0, 0], [7, 1, 4], [3, 6, 0]])
    k = torch.randn(8, bs, hkv, d, generator=g)
    v = torch.randn(8, bs, hkv, d, generator=g)
    q = torch.randn(4, hq, d, generator=g)
    slots = (tables.unsqueeze(-1) * bs + torch.arange(bs)).reshape(4, -1)
    want = _masked_decode_attention(q, k.view(-1, hkv, d)[slots], v.view(-1, hkv, d)[slots], lens, 0.3)
    got = ops.paged_decode_attention(q, k, v, tables, lens, 0.3)
    torch.testing.assert_close(got, want)


def test_cpu_engine_paged_matches_default():
    G.destroy_model_parallel()
    G.initialize_model_parallel(world_size=1, rank=0)
    model_parallel_seed(123)
    cfg = TransformerConfig(
        num_layers=2, hidden_size=64, num_attention_heads=4, num_query_groups=2,
        ffn_hidden_size=128, vocab_size=128, max_position_embeddings=256,
    )
    model = GPTModel(cfg).eval()
    prompts = [[3, 7, 11, 2, 9], [5, 1], [8, 8, 4, 2, 1, 0, 9]]
    params = SamplingParams(max_tokens=6, greedy=True, stop_on_eod=False)
    default = DynamicInferenceEngine(model, num_blocks=16, block_size=8).generate(prompts, params)
    paged = DynamicInferenceEngine(model, num_blocks=16, block_size=8,
                                   decode_attention="paged").generate(prompts, params)
    G.destroy_model_parallel()
    for a, b in zip(default, paged):
        assert a.output_tokens == b.output_tokens
