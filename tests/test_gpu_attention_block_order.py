"""Attention kernels behind the block map (attention_sched.h): grids with
fewer heads than XCDs, padded grids with empty slots, uneven group ranges, an
exact multiple of 8, d = 64, non-causal, sq != skv, a window, and the packed
kernels.  A block the map sends to the wrong place, or never runs, shows as a
gross error or as NaN: before every native call tensors of the output sizes are
allocated, filled with NaN and freed, so the caching allocator hands the
kernels poisoned memory instead of stale, correct values.

Every case compares out, dq, dk and dv with ops.reference in fp32: the
backward with the metric and bound of test_gpu_attention_bwd_tiles
(_rel_err < 3e-2), the forward with the bound of test_attention_fwd in
test_gpu_kernels (_rel_err < 2e-2).  Inputs are the seeded, asymmetric inputs
of test_gpu_attention_bwd_tiles.  The exhaustive check of the map itself is
test_attention_block_map.py.
"""

import pytest
import torch

from megatron_amd import ops
from megatron_amd.ops import reference as ref
from tests.test_gpu_attention_bwd_tiles import _inputs, _rel_err

pytestmark = pytest.mark.gpu

FWD_BOUND, BWD_BOUND = 2e-2, 3e-2
NAMES = ("out", "dq", "dk", "dv")


def _poison(*like):
    """Leave NaN in the blocks the allocator will hand out next."""
    junk = [torch.full_like(t, float("nan")) for t in like]
    junk.append(torch.full((like[0].shape[1], like[0].shape[2], like[0].shape[0]), float("nan"),
                           device="cuda", dtype=torch.float32))  # lse / drow
    del junk


def _native(q, k, v, dy, causal, window):
    scale = q.shape[-1] ** -0.5
    _poison(q)
    out, lse = ops._C.attn_fwd(q, k, v, causal, scale, window)
    assert not torch.isnan(lse).any(), "lse holds NaN"
    _poison(q, k, v)
    dq, dk, dv = ops._C.attn_bwd(dy, q, k, v, out, lse, causal, scale, window)
    return out, dq, dk, dv


def _reference(attn, q, k, v, dy):
    q, k, v = (t.detach().float().requires_grad_(True) for t in (q, k, v))
    out = attn(q, k, v)
    out.backward(dy.float())
    return out.detach(), q.grad, k.grad, v.grad


def _check(name, got, want):
    errs = {n: _rel_err(g, w) for n, g, w in zip(NAMES, got, want)}
    print(name, errs)
    for n, e in errs.items():
        assert e < (FWD_BOUND if n == "out" else BWD_BOUND), f"{name}: {n} rel err {e}"


CASES = {
    # name: (sq, skv, b, hq, hkv, d, causal, window)
    "fewer_than_8_heads": (384, 384, 1, 2, 1, 128, True, 0),
    "padded_grid_odd_blocks": (320, 320, 1, 6, 3, 128, True, 0),
    "more_than_8_groups_uneven": (256, 256, 3, 6, 3, 128, True, 0),
    "multiple_of_8": (512, 512, 2, 8, 4, 128, True, 0),
    "d64": (320, 320, 1, 6, 3, 64, True, 0),
    "non_causal": (192, 192, 1, 4, 4, 128, False, 0),
    "sq_ne_skv": (64, 192, 1, 4, 2, 128, True, 0),
    "window_64": (256, 256, 1, 4, 2, 128, True, 64),
}


@pytest.mark.parametrize("name", list(CASES))
def test_attention_block_order(name):
    assert ops.has_native()
    sq, skv, b, hq, hkv, d, causal, window = CASES[name]
    q, k, v, dy = _inputs(sq, skv, b, hq, hkv, d)
    got = _native(q, k, v, dy, causal, window)
    want = _reference(lambda q, k, v: ref.attention(q, k, v, causal=causal, window=window or None), q, k, v, dy)
    _check(name, got, want)


def test_attention_block_order_repeat_bitwise():
    sq, skv, b, hq, hkv, d, causal, window = CASES["padded_grid_odd_blocks"]
    q, k, v, dy = _inputs(sq, skv, b, hq, hkv, d)
    first = _native(q, k, v, dy, causal, window)
    second = _native(q, k, v, dy, causal, window)
    for n, a, c in zip(NAMES, first, second):
        assert torch.equal(a.view(torch.int16), c.view(torch.int16)), f"{n} differs between two runs"


def _native_packed(q, k, v, dy, cu, causal):
    scale = q.shape[-1] ** -0.5
    _poison(q)
    out, lse = ops._C.attn_varlen_fwd(q, k, v, cu, causal, scale)
    assert not torch.isnan(lse).any(), "lse holds NaN"
    _poison(q, k, v)
    dq, dk, dv = ops._C.attn_varlen_bwd(dy, q, k, v, out, lse, cu, causal, scale)
    return out, lse, dq, dk, dv


def test_packed_block_order_two_documents():
    t, hq, hkv, d = 300, 6, 3, 128
    q, k, v, dy = _inputs(t, t, 1, hq, hkv, d)
    cu = torch.tensor([0, 100, 300], device="cuda", dtype=torch.int32)
    out, _, dq, dk, dv = _native_packed(q, k, v, dy, cu, True)
    want = _reference(lambda q, k, v: ref.attention_varlen(q, k, v, cu, causal=True), q, k, v, dy)
    _check("packed_100_200", (out, dq, dk, dv), want)


def test_packed_single_document_is_dense_bwd_bitwise():
    t, hq, hkv, d = 640, 8, 8, 128
    q, k, v, dy = _inputs(t, t, 1, hq, hkv, d)
    cu = torch.tensor([0, t], device="cuda", dtype=torch.int32)
    out, lse, *packed = _native_packed(q, k, v, dy, cu, True)
    _poison(q, k, v)
    dense = ops._C.attn_bwd(dy, q, k, v, out, lse.view(1, hq, t), True, d ** -0.5, 0)
    for n, a, c in zip(NAMES[1:], dense, packed):
        diff = (a.view(torch.int16) != c.view(torch.int16)).sum().item()
        print(n, "differing elements:", diff)
        assert diff == 0, f"{n}: packed and dense backward differ in {diff} elements"
