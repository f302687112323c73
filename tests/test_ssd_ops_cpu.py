"""ops.ssd_chunked_scan / ops.ssd_step and the mamba_ssd_kernel option without
a GPU: CPU tensors take the ssm.ssd functions unchanged."""

import pytest
import torch

from megatron_amd import ops
from megatron_amd.config import TransformerConfig
from megatron_amd.ssm import ssd
from tests.utils import init_single


def _inputs(l, dtype):
    g = torch.Generator().manual_seed(l)
    b, h, p, grp, n = 2, 4, 16, 2, 8
    x = torch.randn(b, l, h, p, generator=g).to(dtype)
    dt = (torch.rand(b, l, h, generator=g) * 0.1 + 1e-3).to(dtype)
    A = -1.0 - torch.rand(h, generator=g)
    B, C = (torch.randn(b, l, grp, n, generator=g).to(dtype) for _ in range(2))
    return x, dt, A, B, C, torch.randn(h, generator=g), torch.randn(b, h, p, n, generator=g)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cpu_scan_and_step_are_the_ssd_functions(dtype):
    x, dt, A, B, C, D, init = _inputs(37, dtype)
    want = ssd.ssd_chunked_scan(x, dt, A, B, C, D=D, chunk_size=16, initial_state=init, return_final_state=True)
    got = ops.ssd_chunked_scan(x, dt, A, B, C, D=D, chunk_size=16, initial_state=init, return_final_state=True)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert torch.equal(ops.ssd_chunked_scan(x, dt, A, B, C), ssd.ssd_chunked_scan(x, dt, A, B, C))

    s_want, s_got = init.clone(), init.clone()
    y_want, _ = ssd.ssd_step(x[:, 0], dt[:, 0], A, B[:, 0], C[:, 0], s_want, D=D)
    y_got, out = ops.ssd_step(x[:, 0], dt[:, 0], A, B[:, 0], C[:, 0], s_got, D=D)
    assert out is s_got and torch.equal(y_got, y_want) and torch.equal(s_got, s_want)


def _mamba(kernel):
    from megatron_amd.models.mamba import MambaModel

    init_single()
    torch.manual_seed(0)
    cfg = TransformerConfig(num_layers=2, hidden_size=32, num_attention_heads=2, vocab_size=64,
                            max_position_embeddings=32, mamba_state_dim=8, mamba_head_dim=16,
                            mamba_num_groups=2, mamba_chunk_size=8, hybrid_override_pattern="MM",
                            mamba_ssd_kernel=kernel)
    return MambaModel(cfg).eval()


def test_config_hip_on_cpu_model_gives_identical_output():
    ids = torch.arange(24).view(2, 12)
    with torch.no_grad():
        assert torch.equal(_mamba("hip")(input_ids=ids), _mamba("torch")(input_ids=ids))


def test_unknown_kernel_name_raises():
    with pytest.raises(ValueError, match="mamba_ssd_kernel"):
        _mamba("triton")
