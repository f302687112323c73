"""Aux subsystem tests: rerun state machine (transient vs deterministic
classification, data replay), straggler detector, metrics logger, param-hash
DP check, theoretical memory. Reference analogs: core/rerun_state_machine.py,
core/utils.py StragglerDetector / check_param_hashes_across_dp_replicas."""

import json
import os

import pytest
import torch

from megatron_amd.utils.rerun_state_machine import (
    EXIT_CODE_FAILED_ON_RESULT_VALIDATION,
    EXIT_CODE_SUCCESS_ON_RESULT_VALIDATION,
    RerunDataIterator,
    RerunMode,
    RerunStateMachine,
)
from tests.utils import init_single, spawn_dist


def test_rerun_disabled_runs_once():
    rsm = RerunStateMachine(RerunMode.DISABLED)
    it = RerunDataIterator(iter(range(10)))
    runs = 0
    while rsm.should_run_forward_backward(it):
        runs += 1
        next(it)
    assert runs == 1
    assert rsm.should_checkpoint_and_exit() is None


def test_rerun_replays_same_data_and_classifies_deterministic():
    rsm = RerunStateMachine(RerunMode.VALIDATE_RESULTS)
    it = RerunDataIterator(iter([torch.tensor([1.0]), torch.tensor([2.0]), torch.tensor([3.0])]))
    seen = []
    while rsm.should_run_forward_backward(it):
        b = next(it)
        seen.append(float(b))
        # deterministic NaN: same result both runs
        rsm.validate_result(torch.tensor(float("nan")), lambda t: not torch.isfinite(t).all())
    assert seen == [1.0, 1.0]  # second run replayed the SAME batch
    assert rsm.should_checkpoint_and_exit() == EXIT_CODE_FAILED_ON_RESULT_VALIDATION
    assert rsm.stats["persistent"] == 1


def test_rerun_classifies_transient():
    rsm = RerunStateMachine(RerunMode.VALIDATE_RESULTS)
    it = RerunDataIterator(iter([0, 0, 0]))
    vals = iter([float("nan"), 5.0])  # bad first run, clean replay
    while rsm.should_run_forward_backward(it):
        next(it)
        rsm.validate_result(torch.tensor(next(vals)), lambda t: not torch.isfinite(t).all())
    assert rsm.should_checkpoint_and_exit() == EXIT_CODE_SUCCESS_ON_RESULT_VALIDATION
    assert rsm.stats["transient"] == 1


def test_rerun_clean_iterations_no_rerun():
    rsm = RerunStateMachine(RerunMode.VALIDATE_RESULTS)
    it = RerunDataIterator(iter(range(6)))
    for _ in range(3):
        runs = 0
        while rsm.should_run_forward_backward(it):
            runs += 1
            next(it)
            rsm.validate_result(torch.tensor(1.0), lambda t: not torch.isfinite(t).all())
        assert runs == 1
        assert rsm.should_checkpoint_and_exit() is None
    assert rsm.stats["reruns"] == 0


def test_straggler_detector_single():
    from megatron_amd.utils.straggler import StragglerDetector

    d = StragglerDetector(enabled=True)
    for _ in range(3):
        d.start()
        torch.randn(64, 64) @ torch.randn(64, 64)
        d.stop()
    rep = d.report()
    assert rep is not None and rep.max_time_ms >= rep.min_time_ms >= 0.0


def test_metrics_logger(tmp_path):
    from megatron_amd.utils.metrics import MetricsLogger

    m = MetricsLogger(str(tmp_path), rank=0)
    m.log(1, lm_loss=2.5, lr=1e-4)
    m.log(2, lm_loss=2.4, lr=1e-4)
    m.close()
    lines = open(tmp_path / "metrics.jsonl").read().strip().splitlines()
    assert len(lines) == 2
    assert json.loads(lines[0])["lm_loss"] == 2.5


def _run_hash_check(rank, world):
    from megatron_amd.distributed.checks import check_param_hashes_across_dp_replicas
    from megatron_amd.parallel import grid as G

    G.initialize_model_parallel()
    torch.manual_seed(7)  # same params everywhere
    m = torch.nn.Linear(8, 8)
    assert check_param_hashes_across_dp_replicas([m])
    if rank == 1:  # desync one replica
        with torch.no_grad():
            m.weight += 1.0
    assert not check_param_hashes_across_dp_replicas([m])


def test_param_hash_across_dp():
    spawn_dist(_run_hash_check, world_size=2)


def test_theoretical_memory_llama8b():
    from megatron_amd.config import TransformerConfig
    from megatron_amd.training.theoretical_memory import num_parameters, report

    init_single()
    cfg = TransformerConfig(num_layers=32, hidden_size=4096, num_attention_heads=32,
                            num_query_groups=8, ffn_hidden_size=14336, vocab_size=128256,
                            max_position_embeddings=4096)
    n = num_parameters(cfg)
    assert 7.5e9 < n < 8.5e9  # Llama-3-8B
    r = report(cfg, micro_batch_size=4, num_microbatches=2)
    assert 0 < r["total_gb"] < 288


def test_pretrain_with_rerun_and_metrics(tmp_path):
    from megatron_amd.training.pretrain import pretrain

    def provider(config, pre_process=True, post_process=True, vp_stage=None):
        from megatron_amd.models.gpt import GPTModel

        return GPTModel(config, pre_process=pre_process, post_process=post_process)

    it = pretrain(provider, [
        "--num-layers", "1", "--hidden-size", "32", "--num-attention-heads", "2",
        "--num-query-groups", "2", "--ffn-hidden-size", "64", "--seq-length", "32",
        "--micro-batch-size", "1", "--global-batch-size", "1", "--vocab-size", "64",
        "--mock-data", "--train-iters", "2", "--log-interval", "1",
        "--rerun-mode", "validate_results", "--tensorboard-dir", str(tmp_path),
        "--log-straggler", "--straggler-report-interval", "1",
    ])
    assert it == 2
    assert os.path.exists(tmp_path / "metrics.jsonl")


def test_gpu_sniff_test_cpu_passes():
    from megatron_amd.utils.gpu_health import gpu_sniff_test

    assert gpu_sniff_test() == []


def test_profile_annotations():
    import torch

    from megatron_amd.utils.annotations import annotated, enable_annotations, profile_range

    calls = []

    @annotated("test:fn")
    def fn(x):
        calls.append(x)
        return x * 2

    assert fn(3) == 6  # disabled: plain call
    enable_annotations(True)
    try:
        with profile_range("test:range"):
            assert fn(4) == 8
        # ranges visible in a torch.profiler trace
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CPU]) as p:
            with profile_range("marked-region"):
                torch.randn(8) @ torch.randn(8)
        names = {e.name for e in p.events()}
        assert any("marked-region" in n for n in names)
    finally:
        enable_annotations(False)


def test_symmetric_allreduce_fallback_cpu():
    """Without CUDA/IPC the wrapper must transparently fall back (identity
    at world 1); the kernel itself needs a multi-GPU node (driver tier)."""
    import torch

    from megatron_amd.parallel.symm_collectives import SymmetricAllReduce

    ar = SymmetricAllReduce()
    assert not ar.enabled
    t = torch.randn(8)
    out = ar.all_reduce(t.clone())
    assert torch.equal(out, t)


def test_straggler_control_port_toggle():
    import socket

    from megatron_amd.utils.straggler import StragglerDetector

    det = StragglerDetector(enabled=False, control_port=0)  # 0 -> ephemeral
    try:
        for expect in (True, False, True):
            with socket.create_connection(("127.0.0.1", det.control_port), timeout=5) as c:
                c.sendall(b"GET / HTTP/1.0\r\n\r\n")
                resp = c.recv(256)
            assert b"straggler detection" in resp
            assert det.enabled is expect
    finally:
        det.close()


def test_debug_dumper(tmp_path):
    import json

    import torch

    from megatron_amd.config import TransformerConfig
    from megatron_amd.models.gpt import GPTModel
    from megatron_amd.utils.debug_dumps import DebugDumper
    from tests.utils import init_single

    init_single()
    torch.manual_seed(0)
    model = GPTModel(TransformerConfig(
        num_layers=2, hidden_size=32, num_attention_heads=4, num_query_groups=2,
        vocab_size=64, ffn_hidden_size=48, gradient_accumulation_fusion=False))
    path = str(tmp_path / "dumps.jsonl")
    d = DebugDumper(path)
    n = d.watch(model, ["decoder.layers.*.self_attention", "decoder.layers.*.mlp"], grads=True)
    assert n == 4
    toks = torch.randint(0, 64, (2, 8))
    out = model(toks, position_ids=None, attention_mask=None)
    out.float().square().mean().backward()
    d.next_step()
    acts = [r for r in d.records if r["kind"] == "activation"]
    dgrads = [r for r in d.records if r["kind"] == "dgrad"]
    assert len(acts) == 4 and len(dgrads) == 4
    assert all(r["n_nonfinite"] == 0 for r in d.records)
    assert d.nonfinite_modules() == []
    d.close()
    lines = [json.loads(l) for l in open(path)]
    assert len(lines) == len(d.records)
    assert {"norm", "absmax", "module"} <= set(lines[0])


def test_evaluate_ppl_and_cloze():
    import math

    import torch

    from megatron_amd.config import TransformerConfig
    from megatron_amd.models.gpt import GPTModel
    from tests.utils import init_single
    from tools.evaluate import evaluate_cloze, evaluate_perplexity

    init_single()
    torch.manual_seed(0)
    model = GPTModel(TransformerConfig(
        num_layers=2, hidden_size=32, num_attention_heads=4, num_query_groups=2,
        vocab_size=64, ffn_hidden_size=48, gradient_accumulation_fusion=False)).eval()
    g = torch.Generator().manual_seed(1)
    batches = []
    for _ in range(3):
        t = torch.randint(0, 64, (2, 17), generator=g)
        batches.append({"tokens": t[:, :-1], "labels": t[:, 1:]})
    r = evaluate_perplexity(model, batches)
    assert r["tokens"] == 3 * 2 * 16
    # random-init model on random tokens: loss near ln(V)
    assert abs(r["loss"] - math.log(64)) < 1.0
    assert r["ppl"] > 1.0

    # cloze: build samples where the target is the model's own greedy pick ->
    # accuracy 1.0; then shift targets -> accuracy 0.0
    samples = []
    for _ in range(4):
        ctx = torch.randint(0, 64, (9,), generator=g).tolist()
        with torch.no_grad():
            pred = int(model(torch.tensor([ctx]))[-1, 0].float().argmax())
        samples.append(ctx + [pred])
    assert evaluate_cloze(model, samples)["accuracy"] == 1.0
    wrong = [s[:-1] + [(s[-1] + 1) % 64] for s in samples]
    assert evaluate_cloze(model, wrong)["accuracy"] == 0.0


def test_tools_import_surface():
    """Every CLI tool parses/imports (no syntax or import rot)."""
    import importlib
    import sys

    sys.path.insert(0, ".")
    for mod in ["tools.evaluate", "tools.preprocess_data", "tools.profile_model",
                "tools.bench_inference", "tools.run_text_generation_server",
                "tools.checkpoint.convert_hf", "tools.checkpoint.export_hf"]:
        importlib.import_module(mod)


def test_bench_model_catalog_shapes():
    """bench.py model catalog matches the BASELINE architectures (llama3-8b
    / llama3-70b dims, mixtral expert count) and parses its flags."""
    import importlib
    import sys

    sys.path.insert(0, ".")
    bench = importlib.import_module("bench")
    m8 = bench.MODELS["llama3-8b"]
    assert (m8["num_layers"], m8["hidden_size"], m8["ffn_hidden_size"]) == (32, 4096, 14336)
    assert m8["vocab_size"] == 128256
    m70 = bench.MODELS["llama3-70b"]
    assert (m70["num_layers"], m70["hidden_size"]) == (80, 8192)
    mx = bench.MODELS["mixtral-8x7b"]
    assert mx["num_experts"] == 8 and mx["moe_router_topk"] == 2


def test_bench_dump_outputs_repeatable(tmp_path):
    """bench.py --dump-outputs: --steps sets the timed step count, the result
    line carries ms_per_step, and two runs with the same arguments write the
    same float32/float64 arrays (seeded inputs).  Tiny model on the CPU path
    so the comparison is exact."""
    import subprocess
    import sys

    import numpy as np

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONPATH=root, HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env.pop("RANK", None)
    env.pop("WORLD_SIZE", None)

    def run(out_dir, *extra):
        r = subprocess.run(
            [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2",
             "--warmup", "1", "--model", "tiny", "--seq-len", "32", "--micro-batch-size", "1",
             "--grad-accum", "1", "--dump-outputs", str(out_dir), *extra],
            cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        line = json.loads(r.stdout.strip().splitlines()[-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0
        for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert key in line
        return {f: np.load(os.path.join(out_dir, f)) for f in sorted(os.listdir(out_dir))}

    a = run(tmp_path / "a")
    b = run(tmp_path / "b", "--full")
    assert {"loss.npy", "params_sample.npy", "main_grad_sample.npy"} <= set(a)
    assert set(a) == set(b)
    for name, arr in a.items():
        assert arr.dtype in (np.float32, np.float64), name
        assert np.isfinite(arr).all(), name
        assert np.array_equal(arr, b[name]), name
    assert sum(arr.nbytes for arr in a.values()) <= 64 * 2**20
