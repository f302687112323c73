"""Fused-op layer: CDNA4 HIP kernels with torch reference fallback.

Dispatch rule (enforces "the HIP path is the one that runs" on GPU):
  * tensor on a HIP device  -> native extension kernel; if the extension is
    missing the op RAISES (no silent eager fallback on a GPU box).
  * tensor on CPU           -> differentiable torch reference
    (megatron_amd/ops/reference.py) so every code path tests on CPU.

Set MEGATRON_AMD_FORCE_REFERENCE=1 to force the torch path on GPU
(used only by numerics tests that compare kernel vs reference).
"""

from __future__ import annotations

import math
import os
from typing import Optional

import torch

from megatron_amd.ops import reference as ref

_C = None
_IMPORT_ERROR: Optional[str] = None
try:
    from megatron_amd.ops import _hip_ops as _C  # built in-tree by setup.py / __graft_entry__.build()
except Exception as e:  # noqa: BLE001
    _IMPORT_ERROR = repr(e)


def has_native() -> bool:
    return _C is not None and os.environ.get("MEGATRON_AMD_FORCE_REFERENCE", "0") != "1"


def _use_native(x: torch.Tensor) -> bool:
    if not x.is_cuda:
        return False
    if os.environ.get("MEGATRON_AMD_FORCE_REFERENCE", "0") == "1":
        return False
    if _C is None:
        raise RuntimeError(
            f"megatron_amd native HIP extension not built but a GPU tensor hit the ops layer "
            f"(import error: {_IMPORT_ERROR}). Run __graft_entry__.build() / setup.py build_ext --inplace."
        )
    return True


def unfused_glue() -> bool:
    """MEGATRON_AMD_UNFUSED_GLUE=1 (read per call): attention and the layer
    compose split + rope_apply and bias_dropout_add + rms_norm from the
    separate ops instead of the fused kernels (A/B runs, bitwise tests)."""
    return os.environ.get("MEGATRON_AMD_UNFUSED_GLUE", "0") == "1"


# ---------------------------------------------------------------------------
# RMSNorm  (K3)
# ---------------------------------------------------------------------------


class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        x2d = x.reshape(-1, x.shape[-1])
        out, rstd = _C.rmsnorm_fwd(x2d, weight, eps)
        ctx.save_for_backward(x2d, weight, rstd)
        return out.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        x2d, weight, rstd = ctx.saved_tensors
        dy2d = dy.contiguous().reshape(-1, dy.shape[-1])
        dx, dw = _C.rmsnorm_bwd(dy2d, x2d, weight, rstd)
        return dx.view_as(dy), dw, None


def rms_norm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if _use_native(x):
        return _RMSNormFn.apply(x.contiguous(), weight, eps)
    return ref.rms_norm(x, weight, eps)


class _AddRMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, eps):
        h = x.shape[-1]
        total, normed, rstd = _C.add_rmsnorm_fwd(x.reshape(-1, h), residual.reshape(-1, h), weight, eps)
        ctx.save_for_backward(total, weight, rstd)
        return total.view_as(x), normed.view_as(x)

    @staticmethod
    def backward(ctx, dsum, dnormed):
        total, weight, rstd = ctx.saved_tensors
        h = total.shape[-1]
        dx, dw = _C.rmsnorm_bwd(dnormed.contiguous().reshape(-1, h), total, weight, rstd,
                                dsum.contiguous().reshape(-1, h))
        dx = dx.view_as(dsum)
        return dx, dx, dw, None


def add_rms_norm(x: torch.Tensor, residual: torch.Tensor, weight: torch.Tensor, eps: float):
    """(residual + x, rms_norm(residual + x)) in one kernel; the backward folds
    the sum's own gradient into the norm's dx.  Same bits as bias_dropout_add
    followed by rms_norm."""
    if _use_native(x) and x.dtype == torch.bfloat16 and residual.shape == x.shape:
        return _AddRMSNormFn.apply(x.contiguous(), residual.contiguous(), weight, eps)
    total = residual + x
    return total, rms_norm(total, weight, eps)


# ---------------------------------------------------------------------------
# SwiGLU  (K5)
# ---------------------------------------------------------------------------


class _SwigluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x2d = x.reshape(-1, x.shape[-1])
        out = _C.swiglu_fwd(x2d)
        ctx.save_for_backward(x2d)
        return out.view(*x.shape[:-1], x.shape[-1] // 2)

    @staticmethod
    def backward(ctx, dy):
        (x2d,) = ctx.saved_tensors
        dy2d = dy.contiguous().reshape(-1, dy.shape[-1])
        dx = _C.swiglu_bwd(dy2d, x2d)
        return dx.view(*dy.shape[:-1], dy.shape[-1] * 2)


def swiglu(x: torch.Tensor) -> torch.Tensor:
    if _use_native(x):
        return _SwigluFn.apply(x.contiguous())
    return ref.swiglu(x)


def geglu(x: torch.Tensor) -> torch.Tensor:
    return ref.geglu(x)


def squared_relu(x: torch.Tensor) -> torch.Tensor:
    return ref.squared_relu(x)


# ---------------------------------------------------------------------------
# RoPE  (K7)
# ---------------------------------------------------------------------------


class _RopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, cos, sin):
        ctx.save_for_backward(cos, sin)
        return _C.rope_fwd(x, cos, sin)

    @staticmethod
    def backward(ctx, dy):
        cos, sin = ctx.saved_tensors
        return _C.rope_bwd(dy.contiguous(), cos, sin), None, None


_rope_cache = {}


def rope_cos_sin(freqs: torch.Tensor):
    key = (freqs.data_ptr(), freqs.shape, freqs.stride())
    hit = _rope_cache.get(key)
    if hit is None:
        # the entry keeps `freqs` alive: a table gathered per step (inference
        # positions) is a temporary, and once freed the allocator hands its
        # address to the next step's table of the same shape, which must not
        # hit the previous step's cos/sin
        hit = (torch.cos(freqs).contiguous(), torch.sin(freqs).contiguous(), freqs)
        _rope_cache[key] = hit
        if len(_rope_cache) > 8:
            _rope_cache.pop(next(iter(_rope_cache)))
    return hit[:2]


def rope_apply(x: torch.Tensor, freqs: torch.Tensor) -> torch.Tensor:
    """x [s,b,h,d], freqs [s, d_rot/2] fp32 -> rotate-half RoPE.

    freqs may also be [s, b, d_rot/2] (per-row positions, dynamic-batching
    decode) — that path uses the torch implementation."""
    if freqs.dim() == 3:
        return ref.rope_apply_per_row(x, freqs)
    if _use_native(x):
        cos, sin = rope_cos_sin(freqs)
        return _RopeFn.apply(x.contiguous(), cos, sin)
    return ref.rope_apply(x, freqs)


class _QKVSplitRopeFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, cos, sin, rep):
        ctx.save_for_backward(cos, sin)
        q, k, v = _C.qkv_split_rope_fwd(qkv, cos, sin, rep)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        cos, sin = ctx.saved_tensors
        return _C.qkv_split_rope_bwd(dq, dk, dv, cos, sin), None, None, None


def qkv_split_rope_fused(qkv: torch.Tensor, freqs: Optional[torch.Tensor], rep: int) -> bool:
    """Whether qkv_split_rope takes the fused kernel for these inputs."""
    if freqs is None or freqs.dim() != 2 or qkv.dtype != torch.bfloat16 or unfused_glue():
        return False
    if freqs.dtype != torch.float32 or freqs.shape[0] != qkv.shape[0]:
        return False
    d = qkv.shape[-1] // (rep + 2)
    half = freqs.shape[-1]
    return d % 8 == 0 and half % 8 == 0 and 2 * half <= d and _use_native(qkv)


def qkv_split_rope(qkv: torch.Tensor, freqs: torch.Tensor, rep: int):
    """qkv [s,b,ng,(rep+2)*d] (per group: rep q heads | k | v), freqs [s, d_rot/2]
    -> contiguous q [s,b,ng*rep,d], k, v [s,b,ng,d] with rotate-half RoPE on q
    and k, in one pass; one pass back for the packed gradient.  Callers check
    qkv_split_rope_fused first."""
    cos, sin = rope_cos_sin(freqs)
    return _QKVSplitRopeFn.apply(qkv.contiguous(), cos, sin, rep)


# ---------------------------------------------------------------------------
# bias-dropout-add  (K6)
# ---------------------------------------------------------------------------


def bias_dropout_add(x, bias, residual, p: float, training: bool):
    # differentiable composition; fused HIP kernel is a later optimization —
    # llama-family has no bias and p=0 so the hot path is a single add.
    return ref.bias_dropout_add(x, bias, residual, p, training)


# ---------------------------------------------------------------------------
# fused attention  (K1)
# ---------------------------------------------------------------------------


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale, window):
        # q [s,b,hq,d] k/v [s,b,hkv,d]; kernel works in [b,h,s,d]
        out, lse = _C.attn_fwd(q, k, v, causal, scale, window if window is not None else 0)
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.causal, ctx.scale, ctx.window = causal, scale, window
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        dq, dk, dv = _C.attn_bwd(
            dout.contiguous(), q, k, v, out, lse, ctx.causal, ctx.scale, ctx.window if ctx.window is not None else 0
        )
        return dq, dk, dv, None, None, None


def flash_attention(q, k, v, causal=True, scale=None, window=None):
    if scale is None:
        scale = 1.0 / math.sqrt(q.shape[-1])
    # the MFMA kernel tiles for d in {64, 128}; other (test-size) head dims
    # take the plain-PyTorch path
    if _use_native(q) and q.shape[-1] in (64, 128):
        return _FlashAttnFn.apply(q.contiguous(), k.contiguous(), v.contiguous(), causal, scale, window)
    return ref.attention(q, k, v, causal=causal, scale=scale, window=window)


class _FlashAttnVarlenFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, cu_seqlens, causal, scale):
        out, lse = _C.attn_varlen_fwd(q, k, v, cu_seqlens, causal, scale)
        ctx.save_for_backward(q, k, v, out, lse, cu_seqlens)
        ctx.causal, ctx.scale = causal, scale
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse, cu_seqlens = ctx.saved_tensors
        dq, dk, dv = _C.attn_varlen_bwd(dout.contiguous(), q, k, v, out, lse, cu_seqlens, ctx.causal, ctx.scale)
        return dq, dk, dv, None, None, None


def flash_attention_varlen(q, k, v, cu_seqlens, causal=True, scale=None):
    """Packed (THD) attention: q [t, 1, hq, d], k/v [t, 1, hkv, d], documents
    at cu_seqlens [n_docs + 1]; each token attends inside its own document.
    cu_seqlens stays on the device (no host read, graph-capturable)."""
    d = q.shape[-1]
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    # the MFMA kernels tile for bf16, d in {64, 128} and one head dim for q/k/v
    # (MLA with dqk != dv, test-size heads and fp32 take the plain-PyTorch path)
    if _use_native(q) and q.dtype == torch.bfloat16 and d in (64, 128) and v.shape[-1] == d:
        cu = cu_seqlens.to(device=q.device, dtype=torch.int32).contiguous()
        return _FlashAttnVarlenFn.apply(q.contiguous(), k.contiguous(), v.contiguous(), cu, causal, scale)
    return ref.attention_varlen(q, k, v, cu_seqlens.to(q.device), causal=causal, scale=scale)


def paged_decode_attention(q, k_cache, v_cache, block_tables, context_lens, scale=None,
                           k_scale=None, v_scale=None):
    """Decode attention straight off a paged KV cache: q [b, hq, d], k/v cache
    [num_blocks, block_size, hkv, d] (bf16, or float8_e4m3fn with fp32
    k/v_scale [num_blocks * block_size, hkv]), block_tables [b, width] int64,
    context_lens [b] int64 (kv length including the newest token) -> [b, hq, d].
    Tables and lengths are read on the device only (graph-capturable)."""
    b, hq, d = q.shape
    bs, hkv = k_cache.shape[1], k_cache.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    # the MFMA kernel tiles for a bf16 query, d in {64, 128}, at most 16 query
    # heads per kv head and blocks of whole 16-token halves; everything else
    # (test-size heads, fp32, CPU) takes the plain-PyTorch path
    if (
        _use_native(q)
        and q.dtype == torch.bfloat16
        and d in (64, 128)
        and hq % hkv == 0 and hq // hkv <= 16
        and bs % 16 == 0
        and v_cache.dtype == k_cache.dtype
        and (k_cache.dtype == torch.bfloat16 or (fp8 and k_scale is not None and v_scale is not None))
        and block_tables.dtype == torch.int64 and block_tables.stride(-1) == 1
        and context_lens.dtype == torch.int64
    ):
        return _C.attn_paged_decode(q.contiguous(), k_cache, v_cache, block_tables,
                                    context_lens.contiguous(), scale,
                                    k_scale if fp8 else None, v_scale if fp8 else None)
    return ref.paged_decode_attention(q, k_cache, v_cache, block_tables, context_lens, scale,
                                      k_scale, v_scale)


def paged_prefill_attention(q, k_cache, v_cache, block_table, prior_len, scale=None, window=None,
                            k_scale=None, v_scale=None):
    """Prefill attention of one request straight off a paged KV cache: q
    [s, hq, d] at positions prior_len .. prior_len + s - 1, k/v cache
    [num_blocks, block_size, hkv, d] (bf16, or float8_e4m3fn with fp32
    k/v_scale [num_blocks * block_size, hkv]) already holding positions
    0 .. prior_len + s - 1, block_table [width] int64 -> [s, hq, d].  Causal
    with offset, optional sliding window.  prior_len is a host int."""
    s, hq, d = q.shape
    bs, hkv = k_cache.shape[1], k_cache.shape[2]
    if scale is None:
        scale = 1.0 / math.sqrt(d)
    fp8 = k_cache.dtype == torch.float8_e4m3fn
    # the MFMA kernel tiles for a bf16 query, d in {64, 128} and blocks of
    # whole 16-token halves; everything else (test-size heads, fp32, CPU)
    # takes the plain-PyTorch path
    if (
        _use_native(q)
        and q.dtype == torch.bfloat16
        and d in (64, 128)
        and hq % hkv == 0
        and bs % 16 == 0
        and v_cache.dtype == k_cache.dtype
        and (k_cache.dtype == torch.bfloat16 or (fp8 and k_scale is not None and v_scale is not None))
        and block_table.dtype == torch.int64 and block_table.dim() == 1
        and prior_len + s <= block_table.shape[0] * bs
        and (window is None or window >= 1)
    ):
        return _C.attn_paged_prefill(q.contiguous(), k_cache, v_cache, block_table.contiguous(),
                                     int(prior_len), scale, window if window is not None else 0,
                                     k_scale if fp8 else None, v_scale if fp8 else None)
    return ref.paged_prefill_attention(q, k_cache, v_cache, block_table, prior_len, scale, window,
                                       k_scale, v_scale)


# ---------------------------------------------------------------------------
# wgrad GEMM with fp32 accumulation  (K9)
# ---------------------------------------------------------------------------


def wgrad_gemm_accum(main_grad: torch.Tensor, grad_output_2d: torch.Tensor, input_2d: torch.Tensor):
    """main_grad(fp32) += grad_output^T @ input  (bf16 inputs, fp32 D, beta=1)."""
    if _C is not None and main_grad.is_cuda and hasattr(_C, "wgrad_gemm_accum"):
        _C.wgrad_gemm_accum(main_grad, grad_output_2d.contiguous(), input_2d.contiguous())
    else:
        main_grad.add_(torch.matmul(grad_output_2d.t(), input_2d).to(main_grad.dtype))


# ---------------------------------------------------------------------------
# Mamba causal conv1d + SiLU  (K14)
# ---------------------------------------------------------------------------


class _CausalConv1dSiluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias):
        out, pre = _C.causal_conv1d_fwd(x, weight, bias)
        ctx.save_for_backward(x, pre, weight)
        return out

    @staticmethod
    def backward(ctx, dy):
        x, pre, weight = ctx.saved_tensors
        dx, dw, db = _C.causal_conv1d_bwd(dy, x, pre, weight)
        return dx, dw.view(weight.shape).to(weight.dtype), db.to(weight.dtype)


def causal_conv1d_silu(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor) -> torch.Tensor:
    """silu(depthwise causal conv) over channel-last x [b, l, C];
    weight [C, 1, K], bias [C].  HIP kernel for K=4 bf16; torch fallback
    (F.conv1d + silu) otherwise."""
    if (
        _use_native(x)
        and x.dtype == torch.bfloat16
        and weight.shape[-1] == 4
        and x.shape[-1] % 8 == 0
    ):
        return _CausalConv1dSiluFn.apply(x.contiguous(), weight, bias)
    import torch.nn.functional as F

    y = F.conv1d(x.transpose(1, 2), weight, bias, groups=x.shape[-1],
                 padding=weight.shape[-1] - 1)[..., : x.shape[1]]
    return F.silu(y.transpose(1, 2))


# ---------------------------------------------------------------------------
# Mamba2 SSD scan, forward only  (K14)
# ---------------------------------------------------------------------------


def _ssd_native(x, B, C, D, *others) -> bool:
    """The HIP scan serves bf16 x/B/C on the GPU with head and state dims in
    {64, 128}, a per-head D, and no gradient: it has no backward."""
    tensors = [t for t in (x, B, C, D, *others) if t is not None]
    return (
        _use_native(x)
        and all(t.is_cuda for t in tensors)
        and x.dtype == B.dtype == C.dtype == torch.bfloat16
        and x.shape[-1] in (64, 128) and B.shape[-1] in (64, 128)
        and (D is None or D.dim() == 1)
        and not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))
    )


def ssd_chunked_scan(x, dt, A, B, C, D=None, chunk_size=128, initial_state=None,
                     return_final_state=False):
    """Chunked SSD scan, same contract as ssm.ssd.ssd_chunked_scan: x [b, l, h, p],
    dt [b, l, h] (softplus'ed), A [h], B/C [b, l, g, n] -> y [b, l, h, p] (and the
    final state [b, h, p, n] fp32).  The result does not depend on the chunk
    length, and the HIP kernels always use chunks of 128 rows: `chunk_size`
    only steers the torch path.  That path also serves everything the kernels
    do not: CPU, fp32, other sizes, D [h, p], and any input that needs a
    gradient."""
    if _ssd_native(x, B, C, D, dt, A, initial_state) and dt.dtype in (torch.bfloat16, torch.float32):
        y, final = _C.ssd_scan_fwd(
            x, dt, A.float(), B, C, None if D is None else D.float(),
            None if initial_state is None else initial_state.float())
        return (y, final) if return_final_state else y
    from megatron_amd.ssm import ssd

    return ssd.ssd_chunked_scan(x, dt, A, B, C, D=D, chunk_size=chunk_size,
                                initial_state=initial_state, return_final_state=return_final_state)


def ssd_step(x, dt, A, B, C, state, D=None):
    """Single-token SSD update, same contract as ssm.ssd.ssd_step: x [b, h, p],
    dt [b, h], B/C [b, g, n], state [b, h, p, n] fp32 updated in place ->
    (y [b, h, p], state).  One HIP kernel reads and writes the state once."""
    if (
        _ssd_native(x, B, C, D, dt, A, state)
        and dt.dtype in (torch.bfloat16, torch.float32)
        and state.dtype == torch.float32 and state.is_contiguous()
    ):
        y = _C.ssd_step_fwd(x, dt, A.float(), B, C, state, None if D is None else D.float())
        return y, state
    from megatron_amd.ssm import ssd

    return ssd.ssd_step(x, dt, A, B, C, state, D=D)


# ---------------------------------------------------------------------------
# grouped GEMM for MoE experts  (K11)
# ---------------------------------------------------------------------------


_USE_TORCH_GROUPED = (
    hasattr(torch, "_grouped_mm")
    and os.environ.get("MEGATRON_AMD_NO_TORCH_GROUPED", "0") != "1"
)


class _GroupedLinearFn(torch.autograd.Function):
    """y_e = x_e @ w_e^T over variable-size expert batches: one grouped-GEMM
    launch (torch._grouped_mm -> CK/hipBLASLt kernels; this image's
    hipblaslt-ext C++ grouped path is broken — every algo reports internal
    error — so the torch op is the native route).  Backward: grouped dgrad +
    grouped wgrad; wgrad accumulates fp32 into weight.main_grad when the DDP
    fused path is active (mirrors the dense _ParallelLinearFn contract)."""

    @staticmethod
    def forward(ctx, a, weight, sizes):
        a = a.contiguous()
        offs = torch.tensor(sizes, device=a.device, dtype=torch.int32).cumsum(0, dtype=torch.int32)
        out = torch._grouped_mm(a, weight.transpose(1, 2), offs=offs)
        ctx.save_for_backward(a, weight, offs)
        return out

    @staticmethod
    def backward(ctx, dy):
        a, weight, offs = ctx.saved_tensors
        dy = dy.contiguous()
        da = torch._grouped_mm(dy, weight, offs=offs)
        main_grad = getattr(weight, "main_grad", None)
        if main_grad is not None and main_grad.is_cuda and main_grad.dtype == torch.float32:
            # this build's _grouped_mm requires out dtype == input dtype; the
            # in-GEMM accumulation is still fp32, only the output rounds to
            # bf16 before the fp32 main_grad add
            dw = torch._grouped_mm(dy.t(), a, offs=offs)
            main_grad.view(weight.shape).add_(dw)
            weight.grad_added_to_main_grad = True
            cb = getattr(weight, "_ddp_grad_ready_cb", None)
            if cb is not None:
                cb()
            dw = None
        else:
            dw = torch._grouped_mm(dy.t(), a, offs=offs).to(weight.dtype)
        return da, dw, None


class _GroupedLinearFnHipblaslt(torch.autograd.Function):
    """hipBLASLt-ext variant (kept for environments where the ext grouped
    path works; MEGATRON_AMD_NO_TORCH_GROUPED=1 selects it)."""

    @staticmethod
    def forward(ctx, a, weight, sizes):
        out = _C.grouped_gemm(a.contiguous(), weight, list(sizes), True)
        ctx.save_for_backward(a, weight)
        ctx.sizes = sizes
        return out

    @staticmethod
    def backward(ctx, dy):
        a, weight = ctx.saved_tensors
        dy = dy.contiguous()
        sizes = list(ctx.sizes)
        da = _C.grouped_gemm(dy, weight, sizes, False)
        main_grad = getattr(weight, "main_grad", None)
        if main_grad is not None and main_grad.is_cuda and main_grad.dtype == torch.float32:
            _C.grouped_gemm_wgrad(dy, a.contiguous(), sizes, main_grad.view(weight.shape))
            weight.grad_added_to_main_grad = True
            cb = getattr(weight, "_ddp_grad_ready_cb", None)
            if cb is not None:
                cb()
            dw = None
        else:
            dw32 = torch.zeros(weight.shape, dtype=torch.float32, device=weight.device)
            _C.grouped_gemm_wgrad(dy, a.contiguous(), sizes, dw32)
            dw = dw32.to(weight.dtype)
        return da, dw, None


class _GroupedLinearFnHip(torch.autograd.Function):
    """The same product through the project's own grouped GEMM kernels
    (csrc/grouped_gemm_hip.hip): `sizes` is an [E] int32/int64 device tensor
    that is never read on the host, rows at or past sum(sizes) come out as
    zeros, and wgrad accumulates in fp32 straight into weight.main_grad."""

    @staticmethod
    def forward(ctx, a, weight, sizes):
        a = a.contiguous()
        out = _C.grouped_gemm_hip(a, weight.contiguous(), sizes, True)
        ctx.save_for_backward(a, weight, sizes)
        return out

    @staticmethod
    def backward(ctx, dy):
        a, weight, sizes = ctx.saved_tensors
        dy = dy.contiguous()
        da = _C.grouped_gemm_hip(dy, weight.contiguous(), sizes, False) if ctx.needs_input_grad[0] else None
        main_grad = getattr(weight, "main_grad", None)
        if main_grad is not None and main_grad.is_cuda and main_grad.dtype == torch.float32:
            mg = main_grad.view(weight.shape)
            if mg.data_ptr() % 16 == 0:
                _C.grouped_gemm_hip_wgrad(dy, a, sizes, mg, True)
            else:
                # a slice of a flat grad buffer that starts off a 16-byte boundary: the
                # kernel's 16-byte read-modify-write cannot address it; still an fp32 sum
                dw32 = torch.zeros_like(mg)
                _C.grouped_gemm_hip_wgrad(dy, a, sizes, dw32, True)
                mg.add_(dw32)
            weight.grad_added_to_main_grad = True
            cb = getattr(weight, "_ddp_grad_ready_cb", None)
            if cb is not None:
                cb()
            dw = None
        else:
            dw = torch.empty_like(weight, memory_format=torch.contiguous_format)
            _C.grouped_gemm_hip_wgrad(dy, a, sizes, dw, False)
        return da, dw, None


def _grouped_hip_serves(a: torch.Tensor, weight: torch.Tensor) -> bool:
    return (
        a.dtype == torch.bfloat16 and weight.dtype == torch.bfloat16
        and weight.shape[0] <= 256 and weight.shape[1] % 64 == 0 and weight.shape[2] % 64 == 0
        and a.shape[0] < 2**31 - 512
    )


def grouped_linear(a: torch.Tensor, weight: torch.Tensor, sizes, kernel: str = "torch") -> torch.Tensor:
    """a [M, k] bf16 rows grouped by expert; weight [E, n, k]; sizes: host
    ints per expert summing to M.  Returns [M, n].

    kernel="hip" runs the project's own grouped GEMM kernels: `sizes` may then
    be an [E] integer device tensor, used as it is with no host read (a list is
    uploaded), and may sum to less than M: the rows past the sum come out as
    zeros.  Other dtypes than bf16, n or k that is no multiple of 64, more than
    256 experts, 2^31 - 512 rows or more and CPU tensors take the path of
    kernel="torch", which reads the sizes on the host; the zero rows past the
    sum are kept there, the kernels' clamping of negative or too large sizes
    is not."""
    if kernel not in ("torch", "hip"):
        raise ValueError(f"grouped_linear kernel must be 'torch' or 'hip', got {kernel!r}")
    if kernel == "hip" and _use_native(a) and _grouped_hip_serves(a, weight):
        if not torch.is_tensor(sizes):
            sizes = torch.tensor([int(s) for s in sizes], dtype=torch.int64)
        if sizes.dtype not in (torch.int32, torch.int64):
            sizes = sizes.long()
        sizes = sizes.to(a.device).contiguous()
        return _GroupedLinearFnHip.apply(a, weight, sizes)
    if torch.is_tensor(sizes):
        sizes = sizes.tolist()
    if kernel == "hip":
        live = sum(int(s) for s in sizes)
        if live < a.shape[0]:
            out = grouped_linear(a[:live], weight, sizes)
            return torch.cat([out, out.new_zeros(a.shape[0] - live, out.shape[1])], dim=0)
    if _use_native(a):
        fn = _GroupedLinearFn if _USE_TORCH_GROUPED else _GroupedLinearFnHipblaslt
        return fn.apply(a, weight, tuple(int(s) for s in sizes))
    outs, start = [], 0
    for e, n_e in enumerate(sizes):
        n_e = int(n_e)
        outs.append(a[start : start + n_e] @ weight[e].t())
        start += n_e
    return torch.cat(outs, dim=0) if len(outs) > 1 else outs[0]


# ---------------------------------------------------------------------------
# MXFP8 quantise and block-scaled GEMM  (K15)
# ---------------------------------------------------------------------------


def _mx_aligned(*tensors) -> bool:
    return all(t.is_contiguous() and t.data_ptr() % 16 == 0 for t in tensors)


def mx_quantize(t: torch.Tensor, dual: bool = False):
    """t [R, K] -> (q e4m3 [R, K], s uint8 [R, K/32]): e8m0 scale bytes per
    block of 32 along K (format in ops/mxfp8.py).  dual=True also returns
    (qT [K, R], sT [K, R/32]), the quantisation of t^T, from the same read.
    HIP kernel for bf16 on the GPU; anything else takes the torch reference."""
    from megatron_amd.ops import mxfp8

    t = t.contiguous()
    if (
        _use_native(t) and t.dtype == torch.bfloat16 and t.dim() == 2 and t.shape[0] > 0
        and t.shape[1] % 32 == 0 and (not dual or t.shape[0] % 32 == 0) and _mx_aligned(t)
    ):
        return tuple(_C.mx_quantize(t, dual))
    return mxfp8.quantize_mxfp8_dual(t) if dual else mxfp8.quantize_mxfp8(t)


def mx_gemm_nt(aq: torch.Tensor, a_s: torch.Tensor, bq: torch.Tensor, b_s: torch.Tensor) -> torch.Tensor:
    """bf16 [M, N] = dequant(aq [M, K], a_s) @ dequant(bq [N, K], b_s)^T with
    fp32 accumulation.  HIP kernel for K % 128 == 0, N % 16 == 0 and 16-byte
    aligned contiguous operands on the GPU; anything else takes the reference
    (dequantise, matmul in fp32, round to bf16)."""
    from megatron_amd.ops import mxfp8

    if (
        _use_native(aq) and aq.dim() == 2 and bq.dim() == 2 and aq.shape[0] >= 1
        and aq.shape[1] % 128 == 0 and bq.shape[0] % 16 == 0 and bq.shape[0] > 0
        and aq.shape[1] < 2**24 and _mx_aligned(aq, a_s, bq, b_s)
    ):
        return _C.mx_gemm_nt(aq, a_s, bq, b_s)
    return mxfp8.gemm_nt_reference(aq, a_s, bq, b_s)


# ---------------------------------------------------------------------------
# multi-tensor optimizer kernels  (K10)
# ---------------------------------------------------------------------------


def fused_adamw(
    params_fp32, grads, exp_avgs, exp_avg_sqs, lr, beta1, beta2, eps, weight_decay, step,
    model_params_bf16=None,
):
    """AdamW on flat fp32 shards; optionally writes updated bf16 model params.

    On GPU with native ext: one multi-tensor HIP kernel over all shards.
    Fallback: torch._foreach ops (still batched).
    """
    if _C is not None and len(params_fp32) > 0 and params_fp32[0].is_cuda and hasattr(_C, "multi_tensor_adamw"):
        _C.multi_tensor_adamw(
            params_fp32, grads, exp_avgs, exp_avg_sqs,
            model_params_bf16 if model_params_bf16 is not None else [],
            lr, beta1, beta2, eps, weight_decay, step,
        )
        return
    bias_correction1 = 1 - beta1**step
    bias_correction2 = 1 - beta2**step
    torch._foreach_mul_(params_fp32, 1 - lr * weight_decay)
    torch._foreach_mul_(exp_avgs, beta1)
    torch._foreach_add_(exp_avgs, grads, alpha=1 - beta1)
    torch._foreach_mul_(exp_avg_sqs, beta2)
    torch._foreach_addcmul_(exp_avg_sqs, grads, grads, value=1 - beta2)
    denom = torch._foreach_sqrt(torch._foreach_div(exp_avg_sqs, bias_correction2))
    torch._foreach_add_(denom, eps)
    step_size = lr / bias_correction1
    torch._foreach_addcdiv_(params_fp32, exp_avgs, denom, value=-step_size)
    if model_params_bf16 is not None:
        for mp, p in zip(model_params_bf16, params_fp32):
            mp.copy_(p)


def l2_norm(tensors) -> torch.Tensor:
    """sqrt(sum of squares) across a tensor list (fp32 accumulate)."""
    if _C is not None and len(tensors) > 0 and tensors[0].is_cuda and hasattr(_C, "multi_tensor_l2norm"):
        return _C.multi_tensor_l2norm(list(tensors))
    if len(tensors) == 0:
        return torch.zeros((), dtype=torch.float32)
    norms = torch._foreach_norm(list(tensors))
    return torch.norm(torch.stack([n.float() for n in norms]))
