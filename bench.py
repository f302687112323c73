"""Flagship training benchmark (driver contract).

  python bench.py --gpus N --steps K --warmup W [--model llama3-8b]
                  [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes the last step's
outputs if --dump-outputs is given and prints one JSON result line; anything
measured beyond that headline figure belongs behind --full.

Measures the BASELINE.json metric: whole-node tokens/s (+ MFU) for
Llama-3-8B / 70B on synthetic data of the benchmark shape with random-init
weights, bf16, seq 4096.  For N>1 the driver launches this under
torch.distributed.run with one rank per GPU over RCCL; per-GPU work is fixed
(weak scaling).
"""

from __future__ import annotations

import argparse
import json
import os
import time

import torch

from megatron_amd.config import DDPConfig, OptimizerConfig, TransformerConfig
from megatron_amd.datasets.mock import MockGPTDataIterator
from megatron_amd.models.gpt import GPTModel
from megatron_amd.parallel import grid as G
from megatron_amd.parallel.random import model_parallel_seed
from megatron_amd.training.flops import MI355X_BF16_DENSE_PEAK_TFLOPS, num_floating_point_operations
from megatron_amd.training.training import setup_model_and_optimizer, train_step

MODELS = {
    # llama-3 8B (BASELINE.json "Llama-3 8B DP=8 bf16")
    "llama3-8b": dict(
        num_layers=32, hidden_size=4096, num_attention_heads=32, num_query_groups=8,
        ffn_hidden_size=14336, vocab_size=128256, rotary_base=500000.0,
    ),
    # llama-3 70B (BASELINE.json "Llama-3 70B TP=8 over xGMI")
    "llama3-70b": dict(
        num_layers=80, hidden_size=8192, num_attention_heads=64, num_query_groups=8,
        ffn_hidden_size=28672, vocab_size=128256, rotary_base=500000.0,
    ),
    # Mixtral 8x7B (BASELINE.json "Mixtral 8x7B expert-parallel (all-to-all over xGMI)")
    "mixtral-8x7b": dict(
        num_layers=32, hidden_size=4096, num_attention_heads=32, num_query_groups=8,
        ffn_hidden_size=14336, vocab_size=32000, rotary_base=1000000.0,
        num_experts=8, moe_router_topk=2, moe_ffn_hidden_size=14336,
        moe_aux_loss_coeff=0.01,
    ),
    # tiny shape for CI plumbing
    "tiny": dict(
        num_layers=2, hidden_size=256, num_attention_heads=4, num_query_groups=2,
        ffn_hidden_size=512, vocab_size=1024,
    ),
}


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", default="llama3-8b")
    p.add_argument("--seq-len", type=int, default=4096)
    p.add_argument("--micro-batch-size", type=int, default=4)
    p.add_argument("--grad-accum", type=int, default=2, help="microbatches per step per DP rank")
    p.add_argument("--tp", type=int, default=None, help="tensor parallel size (default: model-dependent)")
    p.add_argument("--pp", type=int, default=1)
    p.add_argument("--ep", type=int, default=None, help="expert parallel size (default: world for MoE)")
    p.add_argument("--balanced-routing", action="store_true",
                   help="force round-robin balanced MoE routing (stable tok/s, uniform a2a)")
    p.add_argument("--vpp", type=int, default=None)
    p.add_argument("--recompute", action="store_true")
    p.add_argument("--no-dist-opt", action="store_true")
    p.add_argument("--hip-graphs", action="store_true",
                   help="capture per-layer fwd/bwd hipGraphs after warmup (dense models, dp-only)")
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--fp8", action="store_true",
                   help="fp8 (e4m3/e5m2 hybrid, delayed scaling) GEMMs; attention/softmax stay bf16")
    p.add_argument("--num-layers", type=int, default=None,
                   help="override layer count (reduced-depth evidence runs; the JSON "
                        "config records the override so the line is never mistaken "
                        "for the full model)")
    p.add_argument("--tune-gemm", action="store_true",
                   help="run hipBLASLt TunableOp algo search and save profiles/tunableop_gfx950.csv")
    p.add_argument("--no-tunableop", action="store_true",
                   help="skip loading the committed TunableOp GEMM selections")
    p.add_argument("--dump-outputs", metavar="DIR", default=None,
                   help="after the timed steps, write what the last timed step computed "
                        "(loss, grad norm, seeded samples of the gradients and of the "
                        "updated parameters) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline figure; there are "
                        "none yet (a plain run is set-up, warm-up, the timed steps and the "
                        "result line), so this is where further ones belong")
    return p.parse_args()


# elements sampled per parameter tensor by --dump-outputs: ~300 tensors in the
# 8B model -> a few MB per array, far under the 64 MB a dump may take
DUMP_SAMPLE_PER_TENSOR = 4096
DUMP_SAMPLE_SEED = 20240229


def dump_outputs(out_dir, chunks, last):
    """Write the last timed step's results as float32/float64 .npy arrays.

    A caller of train_step receives the loss and the grad norm and finds the
    gradients (main_grad) and the updated parameters in the model; the latter
    two are too large to store whole, so a fixed seeded sample of each tensor
    is kept, concatenated in named_parameters() order.  The indices depend
    only on the tensor sizes, so two builds run with the same arguments are
    compared element for element.
    """
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "loss.npy"), np.asarray([last["lm_loss"]], dtype=np.float64))
    if last.get("grad_norm") is not None:
        np.save(os.path.join(out_dir, "grad_norm.npy"),
                np.asarray([last["grad_norm"]], dtype=np.float64))
    gen = torch.Generator(device="cpu").manual_seed(DUMP_SAMPLE_SEED)
    params, grads = [], []
    for ch in chunks:
        for _, p in ch.named_parameters():
            n = p.numel()
            if n <= DUMP_SAMPLE_PER_TENSOR:
                idx = torch.arange(n)
            else:
                idx = torch.randint(0, n, (DUMP_SAMPLE_PER_TENSOR,), generator=gen)
            idx = idx.to(p.device)
            params.append(p.detach().reshape(-1)[idx].float().cpu())
            g = getattr(p, "main_grad", None)
            if g is not None:
                grads.append(g.detach().reshape(-1)[idx].float().cpu())
    np.save(os.path.join(out_dir, "params_sample.npy"), torch.cat(params).numpy())
    if grads:
        np.save(os.path.join(out_dir, "main_grad_sample.npy"), torch.cat(grads).numpy())


def setup_tunableop(args, rank):
    """hipBLASLt GEMM algorithm selection (PyTorch TunableOp).

    The committed profiles/tunableop_gfx950.csv holds the best hipBLASLt algo
    per GEMM shape, found once on MI355X with --tune-gemm; every later run
    (including the driver's) just loads it -- no tuning cost in the timed
    region.  Reference analog: Tensile solution selection inside TE.
    """
    if not torch.cuda.is_available() or args.no_tunableop:
        return None
    import torch.cuda.tunable as tunable

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                        "profiles", "tunableop_gfx950.csv")
    if args.tune_gemm:
        tunable.enable(True)
        tunable.tuning_enable(True)
        # cap per-candidate search cost so one pass covers fwd+dgrad shapes
        tunable.set_max_tuning_duration(10)
        tunable.set_max_tuning_iterations(10)
        tunable.set_filename(path, insert_device_ordinal=False)
        if os.path.exists(path):
            tunable.read_file(path)  # extend prior results instead of redoing
        return path if rank == 0 else None
    if os.path.exists(path):
        tunable.enable(True)
        tunable.tuning_enable(False)
        tunable.set_filename(path, insert_device_ordinal=False)
        tunable.read_file(path)
    return None


def main():
    args = parse_args()
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    use_dist = world > 1 or "RANK" in os.environ

    if torch.cuda.is_available():
        local_rank = int(os.environ.get("LOCAL_RANK", rank))
        torch.cuda.set_device(local_rank)
        device = torch.device("cuda", local_rank)
    else:
        device = torch.device("cpu")

    if use_dist and not torch.distributed.is_initialized():
        G.init_distributed()

    tune_out = setup_tunableop(args, rank)

    tp = args.tp
    if tp is None:
        tp = min(world, 8) if args.model == "llama3-70b" else 1
    if args.model == "llama3-70b" and world < 2 and args.tp is None:
        tp = 1  # single-GPU measurement of the 70B shape is impossible; caller sets --tp
    sp = tp > 1

    is_moe = "num_experts" in MODELS[args.model]
    ep = args.ep if args.ep is not None else (min(world, 8) if is_moe else 1)
    if use_dist:
        G.initialize_model_parallel(tensor_parallel_size=tp, pipeline_parallel_size=args.pp,
                                    virtual_pipeline_parallel_size=args.vpp,
                                    expert_parallel_size=ep)
    else:
        G.initialize_model_parallel(tensor_parallel_size=1, world_size=1, rank=0)
        ep = 1
    model_parallel_seed(args.seed)
    grid = G.get_grid()
    dp = grid.dp

    mdl = dict(MODELS[args.model])
    layers_overridden = False
    if args.num_layers is not None and args.num_layers != mdl["num_layers"]:
        mdl["num_layers"] = args.num_layers
        layers_overridden = True
    # 70B at 1 GPU cannot fit; scale layer count for sub-node smoke unless full node
    cfg = TransformerConfig(
        **mdl,
        bf16=True if device.type == "cuda" else False,
        max_position_embeddings=args.seq_len,
        tensor_parallel_size=tp,
        pipeline_parallel_size=args.pp,
        virtual_pipeline_parallel_size=args.vpp,
        sequence_parallel=sp,
        expert_parallel_size=ep,
        recompute_granularity="full" if args.recompute else None,
        moe_router_force_load_balancing=args.balanced_routing,
        gradient_accumulation_fusion=device.type == "cuda",
        fp8="hybrid" if args.fp8 else None,
    )
    opt_cfg = OptimizerConfig(
        lr=3e-4, weight_decay=0.1, clip_grad=1.0, bf16=cfg.bf16,
        use_distributed_optimizer=not args.no_dist_opt,
    )
    ddp_cfg = DDPConfig(
        grad_reduce_in_fp32=True,
        use_distributed_optimizer=not args.no_dist_opt, bucket_size=40_000_000,
        # graphs + overlap coexist: graphed backward fires the DDP grad-ready
        # callbacks after each layer replay (hip_graphs.py)
        overlap_grad_reduce=True,
    )

    def provider(config, pre_process=True, post_process=True, vp_stage=None):
        return GPTModel(config, pre_process=pre_process, post_process=post_process, vp_stage=vp_stage)

    chunks, optimizer = setup_model_and_optimizer(provider, cfg, opt_cfg, ddp_cfg, device=device)

    data = MockGPTDataIterator(args.micro_batch_size, args.seq_len, cfg.vocab_size,
                               seed=args.seed, device=str(device), dp_rank=grid.rank_in("dp_cp"))
    data_it = iter(data)

    def forward_step(it, model):
        batch = next(data_it)

        def loss_func(loss_sb):
            s = loss_sb.sum()
            return s, torch.tensor(loss_sb.numel(), device=loss_sb.device), {"loss_sum": s.detach()}

        out = model(batch["tokens"], labels=batch["labels"])
        return out, loss_func

    def one_step():
        return train_step(forward_step, None, chunks, optimizer, cfg,
                          args.grad_accum, args.seq_len, args.micro_batch_size)

    def barrier_sync():
        if torch.distributed.is_initialized():
            torch.distributed.barrier()
        if device.type == "cuda":
            torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_step()
    barrier_sync()
    if args.hip_graphs:
        # capture after warmup at a step boundary (no live autograd graphs);
        # under no_sync so capture-time ready-callbacks cannot launch reduces
        import contextlib as _ctx

        from megatron_amd.transformer.hip_graphs import capture_block_hip_graphs

        core = chunks[0].module if hasattr(chunks[0], "module") else chunks[0]
        sample = torch.randn(args.seq_len, args.micro_batch_size, cfg.hidden_size,
                             device=device, dtype=cfg.params_dtype)
        freqs = core._rotary_freqs(args.seq_len, device)
        with _ctx.ExitStack() as stack:
            for ch in chunks:
                if hasattr(ch, "no_sync"):
                    stack.enter_context(ch.no_sync())
            n = capture_block_hip_graphs(core.decoder, sample, rotary_freqs=freqs)
        if rank == 0:
            print(f"# captured {n} layer hipGraphs", flush=True)
        one_step()  # one replay-path warmup step
        barrier_sync()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = one_step()
    barrier_sync()
    elapsed = time.perf_counter() - t0

    # max over ranks
    if torch.distributed.is_initialized():
        t = torch.tensor([elapsed], dtype=torch.float64)
        if device.type == "cuda":
            t = t.to(device)
        torch.distributed.all_reduce(t, op=torch.distributed.ReduceOp.MAX)
        elapsed = float(t.item())

    if tune_out is not None:
        import torch.cuda.tunable as tunable

        tunable.write_file(tune_out)
        print(f"# wrote TunableOp results to {tune_out}", flush=True)

    if args.dump_outputs and rank == 0 and last is not None:
        dump_outputs(args.dump_outputs, chunks, last)

    ms_per_step = elapsed / args.steps * 1000.0
    global_batch = args.micro_batch_size * args.grad_accum * dp
    tokens_per_step = global_batch * args.seq_len
    tokens_per_s = tokens_per_step / (elapsed / args.steps)
    n_gpus = world if device.type == "cuda" else world
    flops_per_step = num_floating_point_operations(cfg, global_batch, args.seq_len)
    tflops_per_gpu = flops_per_step / (elapsed / args.steps) / max(n_gpus, 1) / 1e12
    # fp8 MFU prices against the 5 PF dense fp8 peak (2x bf16); note gfx950
    # non-block-scaled fp8 MFMA issues at the bf16 rate - fp8's realizable
    # win is operand bandwidth, so fp8 MFU is conservative by construction
    peak = MI355X_BF16_DENSE_PEAK_TFLOPS * (2 if args.fp8 else 1)
    mfu = tflops_per_gpu / peak

    if rank == 0:
        par = f"tp{tp}" + (f"pp{args.pp}" if args.pp > 1 else "") + f"dp{dp}" + (f"ep{ep}" if ep > 1 else "")
        print(json.dumps({
            "metric": "tokens/s",
            "value": round(tokens_per_s, 1),
            "unit": "tokens/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 2),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "fp8" if args.fp8 else ("bf16" if cfg.bf16 else "fp32"),
            "data": "synthetic",
            "tflops_per_gpu": round(tflops_per_gpu, 1),
            "mfu": round(mfu, 4),
            "mem_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1) if device.type == "cuda" else None,
            "loss": None if last is None else round(last["lm_loss"], 4),
            "config": {
                "model": args.model if not layers_overridden else f"{args.model}@{mdl['num_layers']}L",
                "num_layers": mdl["num_layers"],
                "global_batch": global_batch,
                "seq_len": args.seq_len,
                "parallelism": par,
                "micro_batch_size": args.micro_batch_size,
                "distributed_optimizer": not args.no_dist_opt,
            },
        }))


if __name__ == "__main__":
    main()
