"""MXFP8 GEMM microbenchmark at the Llama-3-8B linear shapes.

  python tools/bench_mxfp8.py [--tokens 16384] [--iters 20] [--rounds 5]

Per shape (forward y = x w^T and its dgrad dx = dy w) it times, alternating
in one process: bf16 torch.matmul, tensorwise fp8 torch._scaled_mm,
ops.mx_gemm_nt alone, and ops.mx_gemm_nt with the quantise launches of a
training step (rowwise activation + dual weight in forward, rowwise gradient
in dgrad).  Device events around `iters` calls, `rounds` rounds; prints the
median time, TF/s on 2 M N K flops and the min..max spread over the rounds.
The quantise kernels are reported alone in GB/s over the bytes they must move.
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import torch

from megatron_amd import ops

# name, in features, out features of the Llama-3-8B linears
SHAPES = [("qkv", 4096, 6144), ("proj", 4096, 4096), ("fc1", 4096, 28672), ("fc2", 14336, 4096)]


def _round(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) / iters  # ms


def _bench(variants, iters, rounds):
    """variants: {name: fn}; alternates them round by round after a warm-up."""
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(_round(fn, iters))
    return times


def _report(tag, times, work, unit):
    for name, ts in times.items():
        med = statistics.median(ts)
        print(f"{tag:12s} {name:14s} {med:8.3f} ms  {work / (med * 1e-3):8.1f} {unit}  "
              f"(min {min(ts):.3f} max {max(ts):.3f})")


def gemm_variants(a, b):
    """The GEMM-only variants of out [M, N] = a [M, K] @ b [N, K]^T, and b's MX pair."""
    aq, a_s = ops.mx_quantize(a)
    bq, b_s = ops.mx_quantize(b)
    one = torch.ones((), device="cuda")
    a8, b8 = a.to(torch.float8_e4m3fn), b.to(torch.float8_e4m3fn)
    return bq, b_s, {
        "bf16 matmul": lambda: torch.matmul(a, b.t()),
        "fp8 scaled_mm": lambda: torch._scaled_mm(a8, b8.t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16),
        "mx_gemm_nt": lambda: ops.mx_gemm_nt(aq, a_s, bq, b_s),
    }


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--tokens", type=int, default=16384)
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--rounds", type=int, default=5)
    args = p.parse_args()
    assert torch.cuda.is_available() and ops.has_native(), "bench_mxfp8 needs the GPU and the native extension"
    torch.manual_seed(0)
    M = args.tokens
    for name, fin, fout in SHAPES:
        x = torch.randn(M, fin, device="cuda", dtype=torch.bfloat16)
        dy = torch.randn(M, fout, device="cuda", dtype=torch.bfloat16)
        w = torch.randn(fout, fin, device="cuda", dtype=torch.bfloat16) * 0.02
        wT = w.t().contiguous()
        flops = 2.0 * M * fin * fout

        # forward: x [M, in] . w [out, in]^T
        _, _, variants = gemm_variants(x, w)

        def fwd_with_quant():
            xq, xs = ops.mx_quantize(x)
            q, s, _, _ = ops.mx_quantize(w, dual=True)
            return ops.mx_gemm_nt(xq, xs, q, s)

        variants["mx + quantise"] = fwd_with_quant
        _report(f"{name} fwd", _bench(variants, args.iters, args.rounds), flops / 1e12, "TF/s")

        # dgrad: dy [M, out] . wT [in, out]^T, wT quantised once in forward
        wqT, wsT, variants = gemm_variants(dy, wT)

        def dgrad_with_quant():
            dyq, dys = ops.mx_quantize(dy)
            return ops.mx_gemm_nt(dyq, dys, wqT, wsT)

        variants["mx + quantise"] = dgrad_with_quant
        _report(f"{name} dgrad", _bench(variants, args.iters, args.rounds), flops / 1e12, "TF/s")

        # quantise kernels alone: read bf16, write e4m3 (+ 1/32 scales), dual writes twice
        quant = {
            "rowwise x": (lambda: ops.mx_quantize(x), x.numel() * (2 + 1 + 1 / 32)),
            "dual w": (lambda: ops.mx_quantize(w, dual=True), w.numel() * (2 + 2 + 2 / 32)),
        }
        for qname, (fn, nbytes) in quant.items():
            _report(f"{name} quant", _bench({qname: fn}, args.iters, args.rounds), nbytes / 1e9, "GB/s")


if __name__ == "__main__":
    main()
