"""Attention kernel microbenchmark at the Llama-3-8B bench shape.

  python tools/bench_attn.py [--s 4096] [--b 1] [--hq 32] [--hkv 8] [--iters 20] [--no-causal]
  python tools/bench_attn.py --varlen 1024,1024,1024,1024 [--torch-path]

Prints achieved TFLOP/s for fwd and bwd (causal-halved flop count; the full
count with --no-causal, where every block does the same work, so that run is
balanced across the GPU by construction).
--varlen packs documents of the given lengths into one [t, 1, h, d] stream and
runs ops.flash_attention_varlen; --torch-path times the plain-PyTorch packed
attention on the same input instead.
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from megatron_amd import ops


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def bench_varlen(args):
    lengths = [int(x) for x in args.varlen.split(",")]
    t, hq, hkv, d = sum(lengths), args.hq, args.hkv, args.d
    torch.manual_seed(0)
    q = torch.randn(t, 1, hq, d, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(t, 1, hkv, d, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(t, 1, hkv, d, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    cu = torch.tensor([0] + lengths, device="cuda").cumsum(0).to(torch.int32)
    attn = ops.reference.attention_varlen if args.torch_path else ops.flash_attention_varlen
    name = "torch" if args.torch_path else "hip"

    # causal-halved per document, same gemm counts as the dense path
    fwd_flops = 2 * 2 * sum(n * n / 2 for n in lengths) * d * hq
    bwd_flops = fwd_flops / 2 * 7

    with torch.no_grad():
        dt = _time(lambda: attn(q, k, v, cu, causal=True, scale=d**-0.5), args.iters)
    print(f"varlen {name} t={t} docs={len(lengths)} fwd: {dt*1e3:.3f} ms  {fwd_flops/dt/1e12:.1f} TF (useful-flop basis)")
    if not args.no_bwd:
        out = attn(q, k, v, cu, causal=True, scale=d**-0.5)
        dy = torch.randn_like(out)
        dt = _time(lambda: torch.autograd.grad(out, (q, k, v), dy, retain_graph=True), args.iters)
        print(f"varlen {name} t={t} docs={len(lengths)} bwd: {dt*1e3:.3f} ms  {bwd_flops/dt/1e12:.1f} TF (issued-flop basis)")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--s", type=int, default=4096)
    p.add_argument("--b", type=int, default=1)
    p.add_argument("--hq", type=int, default=32)
    p.add_argument("--hkv", type=int, default=8)
    p.add_argument("--d", type=int, default=128)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--no-bwd", action="store_true")
    p.add_argument("--no-causal", action="store_true", help="dense path: full attention, equal work per block")
    p.add_argument("--varlen", type=str, default=None, help="comma-separated document lengths, packed")
    p.add_argument("--torch-path", action="store_true", help="with --varlen: time the plain-PyTorch path")
    args = p.parse_args()
    if args.varlen:
        return bench_varlen(args)
    s, b, hq, hkv, d = args.s, args.b, args.hq, args.hkv, args.d

    q = torch.randn(s, b, hq, d, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    k = torch.randn(s, b, hkv, d, device="cuda", dtype=torch.bfloat16, requires_grad=True)
    v = torch.randn(s, b, hkv, d, device="cuda", dtype=torch.bfloat16, requires_grad=True)

    causal = not args.no_causal
    # causal-halved: fwd = 2 gemms, bwd = 5 gemm-equivalents (2 recomputed)
    fwd_flops = 2 * 2 * (s * s / (2 if causal else 1)) * d * hq * b
    bwd_flops = fwd_flops / 2 * 7  # ST,dPT,dq + ST,dPT(dkv recompute),dV,dK

    out, lse = ops._C.attn_fwd(q, k, v, causal, d**-0.5, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iters):
        out, lse = ops._C.attn_fwd(q, k, v, causal, d**-0.5, 0)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / args.iters
    print(f"fwd: {dt*1e3:.3f} ms  {fwd_flops/dt/1e12:.1f} TF (useful-flop basis)")

    if not args.no_bwd:
        dy = torch.randn_like(out)
        ops._C.attn_bwd(dy, q, k, v, out, lse, causal, d**-0.5, 0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            ops._C.attn_bwd(dy, q, k, v, out, lse, causal, d**-0.5, 0)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / args.iters
        print(f"bwd: {dt*1e3:.3f} ms  {bwd_flops/dt/1e12:.1f} TF (issued-flop basis)")


if __name__ == "__main__":
    main()
