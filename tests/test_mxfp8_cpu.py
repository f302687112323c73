"""MXFP8 format and torch reference (ops/mxfp8.py): the scale rule, the e4m3
rounding, the dual layout and the mode's plumbing, all on the CPU."""

import pytest
import torch

from megatron_amd import ops
from megatron_amd.ops.mxfp8 import dequantize_mxfp8, mxfp8_linear, quantize_mxfp8


def mx_input(R, K, seed=0, device="cpu"):
    """bf16 [R, K] with per-block magnitudes spread over 2^+-6.  Block 0 has
    an amax whose mantissa is exactly 1.75 (the m == 0.875 boundary of the
    scale rule) and block 1, where there is one, is all zero."""
    g = torch.Generator().manual_seed(seed)
    nb = R * K // 32
    t = torch.randn(nb, 32, generator=g) * torch.exp2(torch.randint(-6, 7, (nb, 1), generator=g).float())
    t[0] = t[0].clamp(-1, 1)
    t[0, 7] = -1.75 * 8
    if nb > 1:
        t[1] = 0
    return t.reshape(R, K).to(torch.bfloat16).to(device)


@pytest.mark.parametrize("R,K", [(1, 32), (33, 160), (64, 1024)])
def test_reference_rule(R, K):
    t = mx_input(R, K)
    q, s = quantize_mxfp8(t)
    assert q.dtype == torch.float8_e4m3fn and s.dtype == torch.uint8 and s.shape == (R, K // 32)
    assert int(s.max()) <= 254
    amax = t.float().reshape(-1, 32).abs().amax(-1)
    scaled = amax * torch.exp2(127 - s.reshape(-1).float())
    live = amax > 0
    assert (scaled[live] > 224).all() and (scaled[live] <= 448).all()
    assert scaled[0] == 448 and q.reshape(-1, 32)[0, 7].float() == -448  # boundary block: E = e - 9
    if live.numel() > 1:  # zero block: E = -127, zero elements
        assert s.reshape(-1)[1] == 0 and (q.reshape(-1, 32)[1].float() == 0).all()
    # round trip within half an e4m3 ulp of the scaled value (spacing 2^-9 below 2^-6)
    E = s.float() - 127
    v = t.float().reshape(R, K // 32, 32).abs() * torch.exp2(-E).unsqueeze(-1)
    half_ulp = torch.exp2((torch.frexp(v)[1] - 1).clamp(min=-6).float() - 4)
    err = (dequantize_mxfp8(q, s) - t.float()).abs().reshape(R, K // 32, 32)
    assert (err <= half_ulp * torch.exp2(E).unsqueeze(-1)).all()


def test_dual_is_rowwise_of_transpose():
    t = mx_input(64, 160, seed=1)
    q, s, qT, sT = ops.mx_quantize(t, dual=True)
    q2, s2 = ops.mx_quantize(t)
    qr, sr = ops.mx_quantize(t.t().contiguous())
    assert qT.shape == (160, 64) and sT.shape == (160, 2)
    for a, b in ((q, q2), (s, s2), (qT, qr), (sT, sr)):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_mode_plumbing():
    from megatron_amd.ops.fp8 import make_recipes
    from megatron_amd.ops.mxfp8 import MXFP8Recipe
    from megatron_amd.training.arguments import build_arg_parser

    assert isinstance(make_recipes("mxfp8"), MXFP8Recipe)
    assert len(make_recipes("hybrid")) == 3
    assert build_arg_parser().parse_args(["--fp8-format", "mxfp8"]).fp8_format == "mxfp8"


def test_linear_reference_tracks_bf16():
    torch.manual_seed(0)
    x = mx_input(64, 256, seed=2).requires_grad_()
    w = (torch.randn(128, 256) * 0.02).to(torch.bfloat16).requires_grad_()
    y = mxfp8_linear(x, w)
    dy = torch.randn_like(y)
    y.backward(dy)
    y_ref = x.detach().float() @ w.detach().float().t()
    dx_ref = dy.float() @ w.detach().float()
    dw_ref = dy.float().t() @ x.detach().float()
    for got, ref in ((y, y_ref), (x.grad, dx_ref), (w.grad, dw_ref)):
        assert (got.float() - ref).norm() / ref.norm() < 0.06
