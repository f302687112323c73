"""Mamba2 SSD scan kernels (ssd_scan.hip) on the GPU against a float64
per-token recurrence: chunked scan, decode step, and the mixer option.

Largest errors measured on an MI355X (max abs error over max abs reference,
bound 2e-2) are listed in profiles/README.md."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from megatron_amd import ops  # noqa: E402
from megatron_amd.config import TransformerConfig  # noqa: E402
from tests.utils import init_single  # noqa: E402

TOL = 2e-2  # test_gpu_paged_decode.py: same measure, same bound
G = 2


def _rel_err(a, b):
    return ((a.float() - b.float()).abs().max() / (b.float().abs().max() + 1e-6)).item()


def _recurrence(x, dt, A, B, C, D=None, state=None):
    """h_t = exp(dt_t A) h_{t-1} + dt_t x_t (x) B_t, y_t = C_t . h_t + D x_t, float64 on the CPU."""
    x, dt, A, B, C = (t.double().cpu() for t in (x, dt, A, B, C))
    b, l, h, p = x.shape
    B, C = (t.repeat_interleave(h // t.shape[2], dim=2) for t in (B, C))
    s = torch.zeros(b, h, p, B.shape[-1], dtype=torch.float64) if state is None else state.double().cpu()
    ys = []
    for t in range(l):
        s = s * torch.exp(dt[:, t] * A)[..., None, None] + (dt[:, t, :, None] * x[:, t])[..., None] * B[:, t, :, None]
        ys.append((s * C[:, t, :, None]).sum(-1) + (0 if D is None else D.double().cpu()[:, None] * x[:, t]))
    return torch.stack(ys, 1), s


def _inputs(l, p, n, rep, with_d, with_init, dt_max=0.1, a=None, dt_dtype=torch.bfloat16, b=2):
    """dt log-uniform in [1e-3, dt_max] and A uniform in [-16, -1] as the mixer initialises them, or A = a."""
    g = torch.Generator().manual_seed(l * 1000 + p + n + rep)
    h = G * rep
    x = torch.randn(b, l, h, p, generator=g).bfloat16()
    dt = torch.exp(torch.rand(b, l, h, generator=g) * (math.log(dt_max) - math.log(1e-3)) + math.log(1e-3)).to(dt_dtype)
    A = -16.0 + 15.0 * torch.rand(h, generator=g) if a is None else torch.full((h,), a)
    B, C = (torch.randn(b, l, G, n, generator=g).bfloat16() for _ in range(2))
    D = torch.randn(h, generator=g) if with_d else None
    init = torch.randn(b, h, p, n, generator=g) if with_init else None
    return [None if t is None else t.cuda() for t in (x, dt, A, B, C, D, init)]


def _check_scan(args):
    x, dt, A, B, C, D, init = args
    want_y, want_s = _recurrence(x, dt, A, B, C, D, init)
    y, s = ops.ssd_chunked_scan(x, dt, A, B, C, D=D, initial_state=init, return_final_state=True)
    y2, s2 = ops.ssd_chunked_scan(x, dt, A, B, C, D=D, initial_state=init, return_final_state=True)
    assert y.dtype == torch.bfloat16 and s.dtype == torch.float32
    assert torch.isfinite(y).all() and torch.isfinite(s).all()
    ey, es = _rel_err(y.cpu(), want_y), _rel_err(s.cpu(), want_s)
    print(f"y err {ey:.2e} state err {es:.2e}")
    assert ey < TOL and es < TOL, (ey, es)
    assert torch.equal(y, y2) and torch.equal(s, s2)


# all l at one (p, n), all (p, n) at l = 129; rep, D and initial state vary along the way
CASES = (
    [(l, 64, 128, (1, 4)[i % 2], i % 3 != 0, i % 2 == 1) for i, l in enumerate((1, 63, 64, 65, 128, 129, 300))]
    + [(129, p, n, rep, rep == 1, rep == 4) for (p, n), rep in
       zip(((64, 64), (64, 128), (128, 64), (128, 128)), (4, 1, 1, 4))]
)


@pytest.mark.parametrize("l,p,n,rep,with_d,with_init", CASES)
def test_scan_matches_float64_recurrence(l, p, n, rep, with_d, with_init):
    _check_scan(_inputs(l, p, n, rep, with_d, with_init, dt_dtype=torch.float32 if l % 2 else torch.bfloat16))


@pytest.mark.parametrize("p,n", [(64, 128), (128, 64)])
def test_scan_strong_decay_stays_finite(p, n):
    # cs_i - cs_j reaches the thousands above the diagonal: the mask must select
    _check_scan(_inputs(300, p, n, 4, True, True, dt_max=1.0, a=-16.0))


def test_scan_takes_the_mixer_row_strided_views():
    x, dt, A, B, C, D, _ = _inputs(129, 64, 64, 4, True, False)
    b, l, h, p = x.shape
    packed = torch.cat([x.reshape(b, l, -1), B.reshape(b, l, -1), C.reshape(b, l, -1)], dim=-1)
    xs, Bs, Cs = torch.split(packed, [h * p, G * 64, G * 64], dim=-1)
    got = ops.ssd_chunked_scan(xs.view(b, l, h, p), dt, A, Bs.view(b, l, G, 64), Cs.view(b, l, G, 64), D=D)
    assert torch.equal(got, ops.ssd_chunked_scan(x, dt, A, B, C, D=D))


@pytest.mark.parametrize("n", [64, 128])
def test_step_continues_the_scan(n):
    x, dt, A, B, C, D, _ = _inputs(32, 64, n, 4, True, False)
    want_y, want_s = _recurrence(x, dt, A, B, C, D)
    y0, state = ops.ssd_chunked_scan(x[:, :24], dt[:, :24], A, B[:, :24], C[:, :24], D=D, return_final_state=True)
    ptr, ys = state.data_ptr(), [y0]
    for t in range(24, 32):
        y, out = ops.ssd_step(x[:, t], dt[:, t], A, B[:, t], C[:, t], state, D=D)
        assert out.data_ptr() == ptr and y.dtype == torch.bfloat16
        ys.append(y.unsqueeze(1))
    assert _rel_err(torch.cat(ys, 1).cpu(), want_y) < TOL
    assert _rel_err(state.cpu(), want_s) < TOL


@pytest.fixture(scope="module")
def mamba_pair():
    """MambaModel at the sizes of test_mamba_gpu_bf16_train_and_decode with the
    torch scan and with the HIP scan, same weights."""
    from megatron_amd.models.mamba import MambaModel

    init_single()
    torch.manual_seed(3)
    cfg = TransformerConfig(num_layers=3, hidden_size=256, num_attention_heads=4,
                            vocab_size=512, max_position_embeddings=256, bf16=True,
                            mamba_state_dim=64, mamba_head_dim=64, mamba_num_groups=2,
                            mamba_chunk_size=32, hybrid_override_pattern="MMM")
    ref_model = MambaModel(cfg).cuda().eval()
    hip_model = MambaModel(cfg.replace(mamba_ssd_kernel="hip")).cuda().eval()
    hip_model.load_state_dict(ref_model.state_dict())
    return ref_model, hip_model


def _prefill_and_decode(model, ids):
    states = model.decoder.allocate_inference_states(ids.shape[0], ids.device, torch.bfloat16)
    outs = [model(input_ids=ids[:, :24], inference_states=states)]
    outs += [model(input_ids=ids[:, t : t + 1], inference_states=states) for t in range(24, 32)]
    return torch.cat(outs, dim=0)


@pytest.mark.parametrize("run", [lambda m, ids: m(input_ids=ids), _prefill_and_decode], ids=["forward", "decode"])
def test_model_hip_scan_matches_torch_scan(mamba_pair, run):
    init_single()
    ids = torch.randint(0, 512, (2, 32), device="cuda", generator=torch.Generator("cuda").manual_seed(5))
    with torch.no_grad():
        want, got = (run(m, ids).float() for m in mamba_pair)
    assert _rel_err(got, want) < 0.05  # bound of test_mamba_gpu_bf16_train_and_decode


def test_model_hip_scan_trains_through_torch(mamba_pair):
    init_single()
    model = mamba_pair[1].train()
    ids = torch.randint(0, 512, (2, 64), device="cuda")
    loss = model(input_ids=ids, labels=ids).float().mean()
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert torch.isfinite(loss) and grads and all(torch.isfinite(g).all() for g in grads)
    model.eval().zero_grad(set_to_none=True)
