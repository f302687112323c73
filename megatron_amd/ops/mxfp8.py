"""MXFP8 (OCP MX) linear path for CDNA4: block-scaled e4m3 GEMMs.

Format, fixed here once:
  * elements are torch.float8_e4m3fn;
  * scales are uint8 [R, K/32], biased e8m0 exponents (byte = E + 127);
  * blocks of 32 run along the last, contiguous dim.

Scale rule for a block with amax = max|x| in fp32: E is the smallest integer
with amax * 2^-E <= 448, clamped to [-127, 127]; amax == 0 gives E = -127 and
all-zero elements; byte 255 is never produced.  Elements are x * 2^-E in fp32
rounded to e4m3 nearest-even; the rule keeps them within 448, so saturation
never fires.

The torch functions below are the CPU path, the fallback for shapes the HIP
kernels (csrc/mx_quant.hip, csrc/mx_gemm.hip) do not serve, and the oracle of
their tests.  Forward and dgrad of mxfp8_linear run on the MX GEMM; wgrad
stays on the bf16 fp32-accumulate path, as in the tensorwise mode.
"""

from __future__ import annotations

import torch

BLOCK = 32


def quantize_mxfp8(t: torch.Tensor):
    """t [..., K] with K % 32 == 0 -> (q e4m3 like t, scales uint8 [..., K/32])."""
    assert t.shape[-1] % BLOCK == 0, "quantize_mxfp8: last dim must be a multiple of 32"
    blocks = t.float().reshape(*t.shape[:-1], t.shape[-1] // BLOCK, BLOCK)
    amax = blocks.abs().amax(dim=-1)
    m, e = torch.frexp(amax)  # amax = m * 2^e, m in [0.5, 1)
    E = torch.where(m <= 0.875, e - 9, e - 8)
    E = torch.where(amax == 0, torch.full_like(E, -127), E).clamp(-127, 127)
    # 2^-E from its bits (exponent field 127 - E in [0, 254]): exact on any device
    inv = ((127 - E).to(torch.int32) << 23).view(torch.float32)
    q = (blocks * inv.unsqueeze(-1)).to(torch.float8_e4m3fn)
    return q.reshape(t.shape), (E + 127).to(torch.uint8)


def dequantize_mxfp8(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 values of an (elements, scales) pair."""
    blocks = q.double().reshape(*q.shape[:-1], q.shape[-1] // BLOCK, BLOCK)
    # 2^E from its fp64 bits; the product is exact and fits fp32 (subnormals included)
    scale = ((scales.to(torch.int64) + (1023 - 127)) << 52).view(torch.float64)
    return (blocks * scale.unsqueeze(-1)).float().reshape(q.shape)


def quantize_mxfp8_dual(t: torch.Tensor):
    """t [R, K] -> (q, s, qT, sT): the rowwise pair and the pair of t^T
    ([K, R], [K, R/32]), whose blocks run along R."""
    return (*quantize_mxfp8(t), *quantize_mxfp8(t.t().contiguous()))


def gemm_nt_reference(aq, a_s, bq, b_s) -> torch.Tensor:
    """dequantise, matmul in fp32, round to bf16."""
    return (dequantize_mxfp8(aq, a_s) @ dequantize_mxfp8(bq, b_s).t()).to(torch.bfloat16)


class MXFP8Recipe:
    """Marker for the mxfp8 mode: scales come from the current block, so there
    is no amax history and no data-parallel amax all-reduce."""


def mxfp8_eligible(x: torch.Tensor, w: torch.Tensor) -> bool:
    """MX blocks lie along the reduction: the input features for the forward,
    the output features for dgrad."""
    return x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.shape[0] % BLOCK == 0 \
        and w.shape[1] % BLOCK == 0


def linear_fwd(x2d: torch.Tensor, w: torch.Tensor):
    """y = x2d @ w^T on the MX GEMM; returns (y, wqT, wsT) with the transposed
    weight pair that dgrad reduces over."""
    from megatron_amd import ops

    xq, xs = ops.mx_quantize(x2d)
    wq, ws, wqT, wsT = ops.mx_quantize(w, dual=True)
    return ops.mx_gemm_nt(xq, xs, wq, ws), wqT, wsT


def linear_dgrad(dy2d: torch.Tensor, wqT: torch.Tensor, wsT: torch.Tensor) -> torch.Tensor:
    """dx = dy2d @ w as an NT GEMM against the transposed weight pair."""
    from megatron_amd import ops

    dyq, dys = ops.mx_quantize(dy2d)
    return ops.mx_gemm_nt(dyq, dys, wqT, wsT)


class _Mxfp8LinearFn(torch.autograd.Function):
    """y = x @ w^T, x [*, in], w [out, in]: MXFP8 forward and dgrad, bf16 wgrad."""

    @staticmethod
    def forward(ctx, x, w):
        x2d = x.reshape(-1, x.shape[-1])
        out, wqT, wsT = linear_fwd(x2d, w)
        ctx.save_for_backward(x2d, wqT, wsT)
        ctx.in_shape = x.shape
        return out.reshape(*x.shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2d, wqT, wsT = ctx.saved_tensors
        dy2d = dy.reshape(-1, dy.shape[-1])
        dx = linear_dgrad(dy2d, wqT, wsT)
        dw = torch.matmul(dy2d.t(), x2d)  # bf16 wgrad (accuracy-critical)
        return dx.reshape(ctx.in_shape), dw


def mxfp8_linear(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    assert mxfp8_eligible(x, w), "mxfp8_linear: bf16 operands with features in multiples of 32"
    return _Mxfp8LinearFn.apply(x, w)
