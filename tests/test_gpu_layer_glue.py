"""GPU bitwise checks for the fused layer glue: QKV split + RoPE, residual add
+ RMSNorm, and a tiny model with and without MEGATRON_AMD_UNFUSED_GLUE=1.

The fused kernels evaluate the same fp32 expressions in the same order as the
separate ops, so every comparison here is torch.equal.
"""

import contextlib
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from megatron_amd import ops
    from megatron_amd.config import TransformerConfig
    from megatron_amd.models.gpt import GPTModel
    from megatron_amd.ops import reference as ref
    from megatron_amd.transformer.attention import SelfAttention
    from tests.utils import init_single
else:
    pytest.skip("GPU-only tests", allow_module_level=True)


@contextlib.contextmanager
def _unfused():
    old = os.environ.get("MEGATRON_AMD_UNFUSED_GLUE")
    os.environ["MEGATRON_AMD_UNFUSED_GLUE"] = "1"
    try:
        yield
    finally:
        if old is None:
            del os.environ["MEGATRON_AMD_UNFUSED_GLUE"]
        else:
            os.environ["MEGATRON_AMD_UNFUSED_GLUE"] = old


def _split_rope_unfused(qkv, freqs, rep, d):
    """The composition SelfAttention.forward runs under the switch."""
    s, b, ng, _ = qkv.shape
    q, k, v = torch.split(qkv, [rep * d, d, d], dim=3)
    q = ops.rope_apply(q.reshape(s, b, ng * rep, d), freqs)
    k = ops.rope_apply(k.reshape(s, b, ng, d), freqs)
    return q, k, v.reshape(s, b, ng, d).contiguous()


@pytest.mark.parametrize("s,b,ng,rep,d,d_rot", [
    (33, 2, 2, 4, 128, 128),
    (64, 1, 1, 1, 64, 64),
    (17, 3, 2, 2, 128, 64),  # partial rotary: passthrough tail
])
def test_qkv_split_rope_bitwise(s, b, ng, rep, d, d_rot):
    torch.manual_seed(0)
    qkv = torch.randn(s, b, ng, (rep + 2) * d, device="cuda", dtype=torch.bfloat16)
    freqs = ref.rope_freqs(s, d, base=500000.0, device="cuda", rotary_percent=d_rot / d)
    assert freqs.shape == (s, d_rot // 2)
    grads = [torch.randn(s, b, ng * rep, d, device="cuda", dtype=torch.bfloat16),
             torch.randn(s, b, ng, d, device="cuda", dtype=torch.bfloat16),
             torch.randn(s, b, ng, d, device="cuda", dtype=torch.bfloat16)]

    a = qkv.clone().requires_grad_(True)
    assert ops.qkv_split_rope_fused(a, freqs, rep)
    fused = ops.qkv_split_rope(a, freqs, rep)
    torch.autograd.backward(fused, grads)

    c = qkv.clone().requires_grad_(True)
    with _unfused():
        assert not ops.qkv_split_rope_fused(c, freqs, rep)
        plain = _split_rope_unfused(c, freqs, rep, d)
        torch.autograd.backward(plain, grads)

    for name, x, y in zip("qkv", fused, plain):
        assert x.is_contiguous(), name
        assert x.shape == y.shape, name
        assert torch.equal(x, y), name
    assert torch.equal(a.grad, c.grad)


@pytest.mark.parametrize("s,b,ng,rep,d,d_rot", [
    (64, 2, 2, 4, 128, 128),
    (64, 1, 2, 2, 128, 64),
])
def test_self_attention_switch_bitwise(s, b, ng, rep, d, d_rot):
    """SelfAttention.forward itself: fused by default, the old composition
    under the switch, same output and gradients."""
    init_single()
    cfg = TransformerConfig(num_layers=1, hidden_size=ng * rep * d, num_attention_heads=ng * rep,
                            num_query_groups=ng, ffn_hidden_size=256, vocab_size=128, bf16=True,
                            max_position_embeddings=64)
    torch.manual_seed(0)
    attn = SelfAttention(cfg).to("cuda")
    freqs = ref.rope_freqs(s, d, base=500000.0, device="cuda", rotary_percent=d_rot / d)
    x = torch.randn(s, b, cfg.hidden_size, device="cuda", dtype=torch.bfloat16)
    dout = torch.randn_like(x)

    def run():
        xi = x.clone().requires_grad_(True)
        for p in attn.parameters():
            p.grad = None
        out = attn(xi, rotary_freqs=freqs)
        out.backward(dout)
        return out.detach(), xi.grad, [p.grad.clone() for p in attn.parameters() if p.grad is not None]

    out_f, dx_f, gp_f = run()
    with _unfused():
        out_u, dx_u, gp_u = run()
    assert torch.equal(out_f, out_u)
    assert torch.equal(dx_f, dx_u)
    for f, u in zip(gp_f, gp_u):
        assert torch.equal(f, u)


@pytest.mark.parametrize("rows,h", [
    (33, 512),
    (512, 4096),
    (5, 16384),  # longer than the in-register row: two-pass bodies
])
def test_add_rms_norm_bitwise(rows, h):
    torch.manual_seed(0)
    x0 = torch.randn(rows, h, device="cuda", dtype=torch.bfloat16)
    r0 = torch.randn(rows, h, device="cuda", dtype=torch.bfloat16)
    w0 = torch.randn(h, device="cuda", dtype=torch.bfloat16)
    dsum = torch.randn(rows, h, device="cuda", dtype=torch.bfloat16)
    dnormed = torch.randn(rows, h, device="cuda", dtype=torch.bfloat16)

    def leaves():
        return [t.clone().requires_grad_(True) for t in (x0, r0, w0)]

    x, r, w = leaves()
    total, normed = ops.add_rms_norm(x, r, w, 1e-5)
    torch.autograd.backward([total, normed], [dsum, dnormed])

    x2, r2, w2 = leaves()
    total2 = ops.bias_dropout_add(x2, None, r2, 0.0, True)
    normed2 = ops.rms_norm(total2, w2, 1e-5)
    torch.autograd.backward([total2, normed2], [dsum, dnormed])

    assert torch.equal(total, total2)
    assert torch.equal(normed, normed2)
    assert torch.equal(x.grad, x2.grad)
    assert torch.equal(r.grad, r2.grad)
    assert torch.equal(w.grad, w2.grad)


def test_tiny_model_switch_bitwise():
    init_single()
    cfg = TransformerConfig(num_layers=2, hidden_size=256, num_attention_heads=4, num_query_groups=2,
                            ffn_hidden_size=512, vocab_size=1024, bf16=True, max_position_embeddings=64)
    torch.manual_seed(0)
    model = GPTModel(cfg).to("cuda")
    tokens = torch.randint(0, 1024, (2, 64), device="cuda")
    labels = torch.randint(0, 1024, (2, 64), device="cuda")

    def run():
        for p in model.parameters():
            p.grad = None
        loss = model(tokens, labels=labels).float().mean()
        loss.backward()
        return loss.detach(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}

    loss_f, grads_f = run()
    with _unfused():
        loss_u, grads_u = run()
    assert torch.equal(loss_f, loss_u)
    assert grads_f.keys() == grads_u.keys() and len(grads_f) > 0
    for n in grads_f:
        assert torch.equal(grads_f[n], grads_u[n]), n
