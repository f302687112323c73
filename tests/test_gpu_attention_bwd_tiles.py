"""Attention backward: the smallest shapes that reach every tile path of the
dq and dkv kernels (ragged tail, d=64, GQA head loop, 256-row dq blocks,
causal offset, sliding window, non-causal), bitwise repeatability, and the
hardware bf16 pack.

Every case compares dq/dk/dv with ops.reference.attention in fp32 using the
metric and bound of test_attention_bwd (_rel_err < 3e-2).  Inputs are seeded
and asymmetric (a per-row/per-column ramp on top of the noise) so a wrong
lane-to-element mapping is a gross error, not a small one.
"""

import pytest
import torch

from megatron_amd import ops
from megatron_amd.ops import reference as ref

pytestmark = pytest.mark.gpu


def _rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _inputs(sq, skv, b, hq, hkv, d, seed=0):
    g = torch.Generator(device="cuda").manual_seed(seed)

    def mk(s, h, slope):
        x = torch.randn(s, b, h, d, device="cuda", generator=g)
        # break every symmetry between rows, heads and columns
        x += slope * torch.linspace(-1, 1, s, device="cuda").view(s, 1, 1, 1)
        x += 0.25 * torch.linspace(-1, 1, d, device="cuda").view(1, 1, 1, d)
        x += 0.1 * torch.arange(h, device="cuda").view(1, 1, h, 1)
        return x.to(torch.bfloat16)

    q, k, v = mk(sq, hq, 0.5), mk(skv, hkv, -0.4), mk(skv, hkv, 0.3)
    dy = mk(sq, hq, 0.2)
    return q, k, v, dy


def _native_grads(q, k, v, dy, causal, window):
    q, k, v = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    out = ops.flash_attention(q, k, v, causal=causal, window=window)
    out.backward(dy)
    return q.grad, k.grad, v.grad


def _ref_grads(q, k, v, dy, causal, window):
    q, k, v = (t.detach().clone().float().requires_grad_(True) for t in (q, k, v))
    out = ref.attention(q, k, v, causal=causal, window=window)
    out.backward(dy.float())
    return q.grad, k.grad, v.grad


CASES = {
    # name: (sq, skv, b, hq, hkv, d, causal, window)
    "ragged_d128": (100, 100, 1, 2, 2, 128, True, None),
    "ragged_d64": (96, 96, 1, 2, 1, 64, True, None),
    "gqa_head_loop": (192, 192, 2, 8, 2, 128, True, None),
    "long_dq_blocks": (320, 320, 1, 4, 2, 128, True, None),
    "sq_ne_skv": (64, 192, 1, 4, 2, 128, True, None),
    "sliding_window": (256, 256, 1, 4, 2, 128, True, 64),
    "non_causal": (192, 192, 1, 4, 4, 128, False, None),
}


@pytest.mark.parametrize("name", list(CASES))
def test_attention_bwd_tile_paths(name):
    assert ops.has_native()
    sq, skv, b, hq, hkv, d, causal, window = CASES[name]
    q, k, v, dy = _inputs(sq, skv, b, hq, hkv, d)
    got = _native_grads(q, k, v, dy, causal, window)
    want = _ref_grads(q, k, v, dy, causal, window)
    errs = {n: _rel_err(g, w) for n, g, w in zip(("dq", "dk", "dv"), got, want)}
    print(name, errs)
    for n, e in errs.items():
        assert e < 3e-2, f"{name}: attn bwd {n} rel err {e}"


def test_attention_bwd_repeat_bitwise():
    sq, skv, b, hq, hkv, d, causal, window = CASES["long_dq_blocks"]
    q, k, v, dy = _inputs(sq, skv, b, hq, hkv, d)
    first = _native_grads(q, k, v, dy, causal, window)
    second = _native_grads(q, k, v, dy, causal, window)
    for n, a, c in zip(("dq", "dk", "dv"), first, second):
        assert torch.equal(a.view(torch.int16), c.view(torch.int16)), f"{n} differs between two runs"


def test_pack_bf16x2_rounds_like_torch():
    """dS of the dkv kernel is packed with pack_bf16x2.  With K = 0 (S = 0),
    lse = 0 (P = 1), O = 0 (drow = 0) and scale = 1, dS[q][kv] = dO[q] . V[kv]
    exactly; V rows carry a three-way bf16 split of a chosen fp32 value x[kv]
    and dO picks the three pieces, so dS = x[kv] bit for bit.  Q = identity
    then makes dk[kv][d] = bf16(dS[d][kv]): the pack's rounding, nothing else.

    Covered: exact ties (both parities), values next to ties, values next to
    the bf16 maximum, negative values.  fp32 subnormals are not covered: the
    packed value is always consumed as an MFMA operand next, and the matrix
    unit's own subnormal handling cannot be separated from the pack's."""
    s, d = 128, 128
    bf16_max = torch.finfo(torch.bfloat16).max
    base = torch.tensor(
        [
            1.0 + 2.0**-8,                # tie, rounds down to even
            1.0 + 2.0**-7 + 2.0**-8,      # tie, rounds up to even
            1.0 + 2.0**-8 + 2.0**-23,     # just above a tie
            1.0 + 2.0**-8 - 2.0**-23,     # just below a tie
            -(1.0 + 2.0**-8),
            -(1.0 + 2.0**-7 + 2.0**-8),
            3.0 + 2.0**-7,                # tie one binade up
            bf16_max,
            bf16_max * (1.0 - 2.0**-10),  # rounds up to the maximum
            -bf16_max * (1.0 - 2.0**-10),
            bf16_max * (1.0 - 2.0**-8),   # tie just under the maximum
            2.0**-100 * (1.0 + 2.0**-8),  # tie at a small exponent
            0.0,
            0.3333333432674408,
            123456.7890625,
            -7.0e-12,
        ],
        dtype=torch.float32,
    )
    x = base.repeat(s // base.numel())
    hi = x.to(torch.bfloat16)
    r1 = x - hi.float()
    mid = r1.to(torch.bfloat16)
    lo = (r1 - mid.float()).to(torch.bfloat16)
    assert torch.equal(hi.float() + mid.float() + lo.float(), x), "three-way bf16 split must be exact"

    dev = "cuda"
    q = torch.eye(s, d, dtype=torch.bfloat16, device=dev).view(s, 1, 1, d).contiguous()
    k = torch.zeros(s, 1, 1, d, dtype=torch.bfloat16, device=dev)
    v = torch.zeros(s, 1, 1, d, dtype=torch.bfloat16, device=dev)
    v[:, 0, 0, 0], v[:, 0, 0, 1], v[:, 0, 0, 2] = hi.to(dev), mid.to(dev), lo.to(dev)
    dout = torch.zeros(s, 1, 1, d, dtype=torch.bfloat16, device=dev)
    dout[:, 0, 0, :3] = 1.0
    out = torch.zeros_like(dout)
    lse = torch.zeros(1, 1, s, dtype=torch.float32, device=dev)
    _, dk, _ = ops._C.attn_bwd(dout, q, k, v, out, lse, False, 1.0, 0)
    want = x.to(torch.bfloat16).to(dev).view(s, 1).expand(s, d)
    got = dk.view(s, d)
    assert torch.equal(got.view(torch.int16), want.contiguous().view(torch.int16)), (
        got[:16, 0].float().tolist(), want[:16, 0].float().tolist())
