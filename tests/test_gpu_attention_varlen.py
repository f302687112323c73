"""GPU numerics of the packed-sequence (varlen) flash attention kernels
against the plain-PyTorch fp32 reference.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from megatron_amd import ops
    from megatron_amd.ops import reference as ref
else:
    pytest.skip("GPU-only tests", allow_module_level=True)

NAMES = ("out", "dq", "dk", "dv")


def _rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


@pytest.mark.parametrize("lengths,hq,hkv,d,causal", [
    ([40, 24], 2, 1, 64, True),                  # everything inside one tile
    ([64, 64, 128], 4, 2, 128, True),            # boundaries on tile edges
    ([1, 63, 65, 127, 200], 4, 2, 128, True),    # length-1 doc, off-edge boundaries, ragged tail
    ([5] * 40, 4, 2, 128, True),                 # several documents inside one wave's rows
    ([300], 8, 2, 128, True),                    # one document crossing a 256-row block
    ([100, 156], 4, 4, 128, False),              # non-causal
    ([130, 191], 2, 1, 64, False),               # non-causal, d = 64, ragged, boundary inside a tile
])
def test_varlen_fwd_bwd(lengths, hq, hkv, d, causal):
    torch.manual_seed(0)
    t = sum(lengths)
    q, k, v, dout = (torch.randn(t, 1, h, d, device="cuda", dtype=torch.bfloat16) for h in (hq, hkv, hkv, hq))
    cu = torch.tensor([0] + lengths, device="cuda").cumsum(0)

    qf, kf, vf = (x.float().requires_grad_(True) for x in (q, k, v))
    out_ref = ref.attention_varlen(qf, kf, vf, cu, causal=causal)
    want = (out_ref.detach(),) + torch.autograd.grad(out_ref, (qf, kf, vf), dout.float())

    runs = []
    for _ in range(2):
        qn, kn, vn = (x.clone().requires_grad_(True) for x in (q, k, v))
        out = ops.flash_attention_varlen(qn, kn, vn, cu, causal=causal)
        runs.append((out.detach(),) + torch.autograd.grad(out, (qn, kn, vn), dout))
    for name, a, a2, b, tol in zip(NAMES, runs[0], runs[1], want, (2e-2, 3e-2, 3e-2, 3e-2)):
        assert torch.isfinite(a).all(), name
        assert _rel_err(a, b) < tol, (name, _rel_err(a, b))
        assert torch.equal(a, a2), f"{name} differs between two runs"


@pytest.mark.parametrize("t,hq,hkv,d,causal", [
    (200, 4, 2, 128, True),
    (200, 4, 4, 128, False),
    (150, 2, 1, 64, True),
])
def test_varlen_single_document_is_dense_bwd(t, hq, hkv, d, causal):
    """A packed batch of one document is the dense layout at b = 1: both
    backward paths give the same values.  Value equality, not bit patterns: a
    skipped all-masked tile may leave +0 where the other path leaves -0."""
    torch.manual_seed(0)
    q, k, v, dout = (torch.randn(t, 1, h, d, device="cuda", dtype=torch.bfloat16) for h in (hq, hkv, hkv, hq))
    cu = torch.tensor([0, t], device="cuda", dtype=torch.int32)
    scale = d ** -0.5
    out, lse = ops._C.attn_varlen_fwd(q, k, v, cu, causal, scale)
    dense = ops._C.attn_bwd(dout, q, k, v, out, lse.view(1, hq, t), causal, scale, 0)
    packed = ops._C.attn_varlen_bwd(dout, q, k, v, out, lse, cu, causal, scale)
    for name, a, b in zip(NAMES[1:], dense, packed):
        assert torch.equal(a, b), name


def test_varlen_no_leak_across_documents():
    lengths, mid = [70, 90, 60], slice(70, 160)
    cu = torch.tensor([0] + lengths, device="cuda").cumsum(0)
    torch.manual_seed(1)
    base = [torch.randn(220, 1, h, 128, device="cuda", dtype=torch.bfloat16) for h in (4, 2, 2, 4)]
    changed = [x.clone() for x in base]
    for x in changed:
        x[mid] = torch.randn_like(x[mid])
    runs = []
    for q, k, v, dout in (base, changed):
        q, k, v = (x.requires_grad_(True) for x in (q, k, v))
        out = ops.flash_attention_varlen(q, k, v, cu, causal=True)
        runs.append((out.detach(),) + torch.autograd.grad(out, (q, k, v), dout))
    for name, a, b in zip(NAMES, *runs):
        assert torch.equal(a[:70], b[:70]) and torch.equal(a[160:], b[160:]), name
        assert not torch.equal(a[mid], b[mid]), name


def test_varlen_through_model():
    """Packed GPT forward at d = 64 (the HIP path) equals the separate
    forwards, and its backward reaches the QKV weight."""
    from megatron_amd.config import TransformerConfig
    from megatron_amd.models.gpt import GPTModel
    from megatron_amd.transformer.packed_seq import PackedSeqParams
    from tests.utils import init_single

    init_single()
    dev = torch.device("cuda:0")
    cfg = TransformerConfig(
        num_layers=1, hidden_size=256, num_attention_heads=4, num_query_groups=2,
        vocab_size=96, ffn_hidden_size=256, params_dtype=torch.bfloat16, bf16=True,
        gradient_accumulation_fusion=False, max_position_embeddings=128)
    torch.manual_seed(1)
    model = GPTModel(cfg).to(dev).eval()
    d1 = torch.randint(0, 96, (1, 40), device=dev)
    d2 = torch.randint(0, 96, (1, 24), device=dev)
    p = PackedSeqParams.from_lengths([40, 24], device=dev)
    out_p = model(torch.cat([d1, d2], dim=1), position_ids=None, attention_mask=None, packed_seq_params=p)
    with torch.no_grad():
        out_1 = model(d1, position_ids=None, attention_mask=None)
        out_2 = model(d2, position_ids=None, attention_mask=None)
    assert torch.allclose(out_p[:40].float(), out_1.float(), atol=5e-2, rtol=5e-2)
    assert torch.allclose(out_p[40:].float(), out_2.float(), atol=5e-2, rtol=5e-2)
    out_p.float().sum().backward()
    grad = model.decoder.layers[0].self_attention.linear_qkv.weight.grad
    assert grad is not None and torch.isfinite(grad).all() and grad.abs().max() > 0


def test_varlen_memory_is_linear_in_t():
    """fwd + bwd at t = 8192 never holds anything near the [hq, t, t] fp32
    scores the torch path allocates (2 GiB here): the HIP path is the one
    that ran."""
    t, hq, hkv, d = 8192, 8, 2, 128
    torch.manual_seed(3)
    q, k, v = (torch.randn(t, 1, h, d, device="cuda", dtype=torch.bfloat16, requires_grad=True) for h in (hq, hkv, hkv))
    dout = torch.randn(t, 1, hq, d, device="cuda", dtype=torch.bfloat16)
    cu = torch.tensor([0] + [2048] * 4, device="cuda").cumsum(0)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = ops.flash_attention_varlen(q, k, v, cu, causal=True)
    grads = torch.autograd.grad(out, (q, k, v), dout)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - before < hq * t * t * 4 // 4
    assert all(torch.isfinite(x).all() for x in (out,) + grads)
