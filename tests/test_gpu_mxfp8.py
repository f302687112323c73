"""MXFP8 HIP kernels (csrc/mx_quant.hip, csrc/mx_gemm.hip) against the torch
reference of ops/mxfp8.py, the mxfp8 linear, and a short training run."""

import pytest
import torch

from megatron_amd import ops
from megatron_amd.ops.mxfp8 import dequantize_mxfp8, mxfp8_linear, quantize_mxfp8, quantize_mxfp8_dual
from tests.test_mxfp8_cpu import mx_input

pytestmark = pytest.mark.gpu


def assert_gemm_bound(out, aq, a_s, bq, b_s):
    """|out - ref| <= 2^-8 |ref| + max(K, 386) 2^-23 (|A| . |B|^T), ref the
    fp64 product of the dequantised operands: one bf16 rounding with slack,
    and two fp32 ulps per accumulated term.  The floor of 386 is the scaled
    MFMA's own summation error: measured against fp64 it needs up to 193 of
    these units whatever K is (193 at K = 128, 178 at 384, 186 at 1024, see
    profiles/README.md), and 386 is twice that."""
    A, B = dequantize_mxfp8(aq, a_s).double(), dequantize_mxfp8(bq, b_s).double()
    ref = A @ B.t()
    bound = 2.0 ** -8 * ref.abs() + max(A.shape[1], 386) * 2.0 ** -23 * (A.abs() @ B.abs().t())
    excess = ((out.double() - ref).abs() - bound).max().item()
    assert excess <= 0, f"worst excess over the bound {excess}"


def same_bytes(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.uint8), b.view(torch.uint8))


@pytest.mark.parametrize("K", [32, 160, 1024])
@pytest.mark.parametrize("R", [1, 33, 256])
def test_quantize_rowwise_matches_reference(R, K):
    t = mx_input(R, K, device="cuda")
    q, s = ops.mx_quantize(t)
    q_ref, s_ref = quantize_mxfp8(t)
    assert same_bytes(s, s_ref) and same_bytes(q, q_ref)


@pytest.mark.parametrize("K", [32, 160, 1024])
@pytest.mark.parametrize("R", [32, 288])
def test_quantize_dual_matches_reference(R, K):
    t = mx_input(R, K, seed=1, device="cuda")
    got = ops.mx_quantize(t, dual=True)
    for a, b in zip(got, quantize_mxfp8_dual(t)):
        assert same_bytes(a, b)


@pytest.mark.parametrize("K", [128, 384, 1024])
@pytest.mark.parametrize("N", [16, 272, 512])
@pytest.mark.parametrize("M", [1, 16, 272, 512])
def test_gemm_matches_fp64(M, N, K):
    aq, a_s = quantize_mxfp8(mx_input(M, K, seed=2, device="cuda"))
    bq, b_s = quantize_mxfp8(mx_input(N, K, seed=3, device="cuda"))
    out = ops.mx_gemm_nt(aq, a_s, bq, b_s)
    assert out.dtype == torch.bfloat16 and out.shape == (M, N)
    assert_gemm_bound(out, aq, a_s, bq, b_s)
    assert torch.equal(out, ops.mx_gemm_nt(aq, a_s, bq, b_s))


def test_gemm_lane_to_block_mapping():
    """Every block of A has its own scale and B is an fp8 identity with scales
    of its own: out[m, n] is A[m, n] times the scale of B's diagonal block,
    exactly, and a wrong lane-to-block reading is off by powers of two."""
    M, K = 16, 256
    aq, _ = quantize_mxfp8(mx_input(M, K, seed=4, device="cuda"))
    a_s = (64 + torch.arange(M * K // 32, device="cuda")).to(torch.uint8).reshape(M, K // 32)
    bq = torch.eye(K, device="cuda").to(torch.float8_e4m3fn)
    b_s = (125 + (torch.arange(K, device="cuda")[:, None] + torch.arange(K // 32, device="cuda")) % 5).to(torch.uint8)
    out = ops.mx_gemm_nt(aq, a_s, bq, b_s)
    ref = dequantize_mxfp8(aq, a_s).double() @ dequantize_mxfp8(bq, b_s).double().t()
    assert torch.equal(out.double(), ref)


def test_linear_matches_reference_and_bf16():
    torch.manual_seed(0)
    x = torch.randn(256, 512, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    w = (torch.randn(1024, 512, device="cuda", dtype=torch.bfloat16) * 0.02).requires_grad_()
    y = mxfp8_linear(x, w)
    dy = torch.randn_like(y)
    y.backward(dy)
    wq, ws, wqT, wsT = quantize_mxfp8_dual(w.detach())
    assert_gemm_bound(y.detach(), *quantize_mxfp8(x.detach()), wq, ws)
    assert_gemm_bound(x.grad, *quantize_mxfp8(dy), wqT, wsT)
    gx, gw = x.grad.clone(), w.grad.clone()
    x.grad = w.grad = None
    y_ref = x @ w.t()
    y_ref.backward(dy)
    for got, ref in ((y, y_ref), (gx, x.grad), (gw, w.grad)):
        assert (got - ref).float().norm() / ref.float().norm() < 0.06


def test_mxfp8_training_tracks_bf16():
    from megatron_amd.config import OptimizerConfig, TransformerConfig
    from megatron_amd.models.gpt import GPTModel
    from megatron_amd.parallel.random import model_parallel_seed
    from megatron_amd.training.training import setup_model_and_optimizer, train_step
    from tests.utils import init_single

    def run(fp8):
        init_single()
        model_parallel_seed(77)
        cfg = TransformerConfig(
            num_layers=4, hidden_size=256, num_attention_heads=8, num_query_groups=4,
            ffn_hidden_size=512, vocab_size=512, bf16=True, fp8=fp8,
            gradient_accumulation_fusion=True, max_position_embeddings=256,
        )
        opt_cfg = OptimizerConfig(lr=1e-3, bf16=True, use_distributed_optimizer=False)

        def provider(config, pre_process=True, post_process=True, vp_stage=None):
            return GPTModel(config, pre_process=pre_process, post_process=post_process)

        chunks, opt = setup_model_and_optimizer(provider, cfg, opt_cfg, device=torch.device("cuda"))
        g = torch.Generator(device="cpu").manual_seed(5)
        toks = torch.randint(0, 512, (4, 128), generator=g).cuda()
        labels = torch.randint(0, 512, (4, 128), generator=g).cuda()

        def fwd(it, model):
            def loss_func(loss_sb):
                s = loss_sb.sum()
                return s, torch.tensor(loss_sb.numel(), device="cuda"), {"loss_sum": s.detach()}

            return model(toks, labels=labels), loss_func

        return [train_step(fwd, None, chunks, opt, cfg, 1, 128, 4)["lm_loss"] for _ in range(20)]

    bf16_losses, mx_losses = run(None), run("mxfp8")
    for a, b in zip(bf16_losses[5:], mx_losses[5:]):
        assert abs(a - b) / max(abs(b), 1e-6) < 0.08, (bf16_losses, mx_losses)
    assert mx_losses[-1] < mx_losses[0], "mxfp8 run is not learning"
