"""HIP grouped GEMM (ops.grouped_linear(kernel="hip")) against a per-expert fp64
reference.

Products of bf16 values are exact in fp32, so the error of a result is the fp32
accumulation over the reduction length r plus one final rounding:
    |x - ref| <= eps * |ref| + r * 2^-22 * (|A| @ |B|)
with eps = 2^-8 for a bf16 result and 2^-23 for an fp32 one; 2^-22 is four times
the sequential round-to-nearest bound, the margin for the summation order
inside an MFMA."""

import pytest
import torch

from megatron_amd import ops
from megatron_amd.config import TransformerConfig
from tests.utils import init_single

pytestmark = pytest.mark.gpu


def _case(sizes, M, n, k, dtype=torch.int64, eps=2.0**-8):
    """bf16 inputs on the GPU and, for Y, dX and dW, (fp64 reference, bound)."""
    g = torch.Generator().manual_seed(n + k + len(sizes))
    M = sum(sizes) if M is None else M
    a, dy = torch.randn(M, k, generator=g).bfloat16(), torch.randn(M, n, generator=g).bfloat16()
    w = torch.randn(len(sizes), n, k, generator=g).bfloat16()
    a64, dy64, w64 = a.double(), dy.double(), w.double()
    ref = {name: [torch.zeros(shape, dtype=torch.float64) for _ in range(2)]
           for name, shape in (("y", (M, n)), ("dx", (M, k)), ("dw", tuple(w.shape)))}
    r0 = 0
    for e, m in enumerate(sizes):
        rows = slice(r0, r0 + m)
        for name, idx, left, right, r in (("y", rows, a64[rows], w64[e].t(), k), ("dx", rows, dy64[rows], w64[e], n),
                                          ("dw", e, dy64[rows].t(), a64[rows], m)):
            prod, acc_err = left @ right, r * 2.0**-22 * (left.abs() @ right.abs())
            # the bound itself: an fp32 matmul rounded to bf16 stays inside it
            cpu = (left.float() @ right.float()).bfloat16().double()
            assert ((cpu - prod).abs() <= 2.0**-8 * prod.abs() + acc_err).all()
            ref[name][0][idx] = prod
            ref[name][1][idx] = eps * prod.abs() + acc_err
        r0 += m
    sz = torch.tensor(sizes, dtype=dtype, device="cuda")
    return a.cuda(), w.cuda(), dy.cuda(), sz, {k_: (v[0].cuda(), v[1].cuda()) for k_, v in ref.items()}


def _run(a, w, dy, sz, main_grad=None):
    a = a.clone().requires_grad_(True)
    w = torch.nn.Parameter(w.clone())
    if main_grad is not None:
        w.main_grad = main_grad
    y = ops.grouped_linear(a, w, sz, kernel="hip")
    y.backward(dy)
    return y.detach(), a.grad, w


@pytest.mark.parametrize("sizes,M,n,k,dtype", [
    ([128, 64, 0, 300], None, 256, 512, torch.int64),
    ([1, 2, 3, 4], None, 64, 64, torch.int32),
    ([257, 0, 0, 255], None, 192, 192, torch.int64),
    ([0, 0, 7], None, 128, 128, torch.int32),
    ([100, 60], 200, 320, 128, torch.int32),
    (list(range(1, 33)), None, 2304, 64, torch.int64),  # more than 256 blocks: second chunk of the block order
])
def test_matches_fp64_reference(sizes, M, n, k, dtype):
    a, w, dy, sz, ref = _case(sizes, M, n, k, dtype)
    y, dx, wp = _run(a, w, dy, sz)
    for name, got in (("y", y), ("dx", dx), ("dw", wp.grad)):
        want, bound = ref[name]
        err = (got.double() - want).abs()
        assert got.dtype == torch.bfloat16 and (err <= bound).all(), name
    tail = sum(sizes)
    assert (y[tail:] == 0).all() and (dx[tail:] == 0).all()


@pytest.mark.parametrize("offset", [0, 1])  # 1: a main_grad view off the 16-byte boundary of its flat buffer
def test_wgrad_accumulates_fp32_into_main_grad(offset):
    a, w, dy, sz, ref = _case([64, 0, 192], None, 128, 256, eps=2.0**-23)
    init = torch.randn(w.shape, device="cuda", dtype=torch.float32)
    flat = torch.zeros(w.numel() + 1, device="cuda", dtype=torch.float32)
    _, _, wp = _run(a, w, dy, sz, main_grad=flat[offset:offset + w.numel()].view(w.shape).copy_(init))
    assert wp.grad is None and wp.grad_added_to_main_grad
    want, bound = ref["dw"]
    err = (wp.main_grad.double() - init.double() - want).abs()
    assert (err <= bound).all()
    assert torch.equal(wp.main_grad[1], init[1])
    # the bf16-rounded route would not meet this bound
    assert not ((want.bfloat16().double() - want).abs() <= bound).all()


def test_independent_of_rows_outside_group():
    a, w, dy, sz, _ = _case([100, 60], 200, 320, 128, torch.int32)
    y, dx, wp = _run(a, w, dy, sz)
    a2, dy2 = a.clone(), dy.clone()
    a2[160:], dy2[160:] = float("nan"), float("nan")
    y2, dx2, wp2 = _run(a2, w, dy2, sz)
    for clean, dirty in ((y, y2), (dx, dx2), (wp.grad, wp2.grad)):
        assert torch.isfinite(dirty).all() and torch.equal(clean, dirty)
    a3, dy3 = a.clone(), dy.clone()
    a3[100:160], dy3[100:160] = a3[100:160] * 2 + 1, dy3[100:160] * 2 + 1
    y3, dx3, wp3 = _run(a3, w, dy3, sz)
    assert torch.equal(y3[:100], y[:100]) and torch.equal(dx3[:100], dx[:100]) and torch.equal(wp3.grad[0], wp.grad[0])
    assert not torch.equal(y3[100:160], y[100:160])


def test_grouped_mlp_graph_replay_with_new_sizes():
    from megatron_amd.moe.experts import GroupedMLP

    init_single()
    torch.manual_seed(0)
    cfg = dict(num_layers=1, hidden_size=128, num_attention_heads=4, vocab_size=64, ffn_hidden_size=128,
               num_experts=4, moe_ffn_hidden_size=128, activation="swiglu", params_dtype=torch.bfloat16,
               init_method_std=0.1)
    mlp = GroupedMLP(TransformerConfig(**cfg, moe_grouped_gemm_kernel="hip")).cuda()
    torch_mlp = GroupedMLP(TransformerConfig(**cfg)).cuda()
    torch_mlp.load_state_dict(mlp.state_dict())
    M = 300
    tokens = torch.randn(M, 128, device="cuda", dtype=torch.bfloat16)
    tpe = torch.tensor([70, 80, 90, 60], device="cuda")
    with torch.no_grad():
        eager = mlp(tokens, tpe)
        want = torch_mlp(tokens, tpe)
        # against the torch kernel, element by element.  Each GEMM of each route meets the
        # bf16 bound against fp64 on that route's own bf16 input.  fc1 has one reference for
        # both routes, so they lie within twice its bound of each other; the fc2 references
        # differ by exactly (h_hip - h_torch) @ W2^T, which adds to the two fc2 bounds.
        sizes, f64 = tpe.tolist(), lambda t: t.detach().double().cpu()
        fc1, h, fc2, bounds = {}, {}, {}, {}
        for kern, sz in (("hip", tpe), ("torch", sizes)):
            fc1[kern] = ops.grouped_linear(tokens, mlp.weight1, sz, kernel=kern)
            h[kern] = mlp._act(fc1[kern])
            fc2[kern] = ops.grouped_linear(h[kern], mlp.weight2, sz, kernel=kern)
            for x, w, got in ((tokens, mlp.weight1, fc1[kern]), (h[kern], mlp.weight2, fc2[kern])):
                ref = ops.grouped_linear(f64(x), f64(w), sizes)
                acc_err = x.shape[1] * 2.0**-22 * ops.grouped_linear(f64(x).abs(), f64(w).abs(), sizes)
                bounds[kern, got is fc2[kern]] = 2.0**-8 * ref.abs() + acc_err
                assert ((f64(got) - ref).abs() <= bounds[kern, got is fc2[kern]]).all(), kern
        assert torch.equal(eager, fc2["hip"]) and torch.equal(want, fc2["torch"])
        assert ((f64(fc1["hip"]) - f64(fc1["torch"])).abs() <= 2 * bounds["hip", False]).all()
        h_gap = ops.grouped_linear((f64(h["hip"]) - f64(h["torch"])).abs(), f64(mlp.weight2).abs(), sizes)
        assert ((f64(eager) - f64(want)).abs() <= bounds["hip", True] + bounds["torch", True] + h_gap).all()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = mlp(tokens, tpe)
        new_tokens, new_tpe = torch.randn_like(tokens), torch.tensor([150, 0, 30, 120], device="cuda")
        tokens.copy_(new_tokens)
        tpe.copy_(new_tpe)
        for _ in range(2):
            graph.replay()
            assert torch.equal(out, mlp(new_tokens, new_tpe))
    assert out.abs().sum() > 0
