"""FlatAdam's CPU path against the fp64 Adam oracle (objective_cases.adam_oracle64): global-norm
clipping, weight decay, the folded grad_scale, the bf16 shadow and the state round trip. The
oracle itself is checked once against fp64 torch.optim.Adam + clip_grad_norm_."""
import pytest
import torch

from microbeast_amd.ops.optim import FlatAdam, FlatParams
from objective_cases import adam_oracle64

LR, EPS = 1e-2, 1e-5
CASES = [(0.0, 0.0, 1.0), (0.5, 0.0, 1.0), (0.5, 0.01, 0.25), (1e6, 0.0, 0.5)]


def _model():
    torch.manual_seed(0)
    return torch.nn.Sequential(torch.nn.Linear(33, 17), torch.nn.Linear(17, 5))


def _run(max_grad_norm, wd, grad_scale, steps=5, shadow=True):
    """``steps`` FlatAdam steps on the two-Linear model beside the fp64 oracle fed the same
    gradients. Returns (flat, opt, oracle, [(last_grad_norm, oracle norm, clip factor)])."""
    m = _model()
    flat = FlatParams(m, "cpu")
    opt = FlatAdam(flat, lr=LR, eps=EPS, weight_decay=wd, max_grad_norm=max_grad_norm,
                   bf16_shadow=shadow)
    ora = adam_oracle64(flat.data, lr=LR, eps=EPS, wd=wd, max_grad_norm=max_grad_norm)
    g = torch.Generator().manual_seed(1)
    norms = []
    for _ in range(steps):
        x = torch.randn(8, 33, generator=g)
        flat.zero_grad()
        m(x).pow(2).sum().backward()
        ora.step(flat.grad, grad_scale)
        opt.step(grad_scale=grad_scale)
        norms.append((opt.last_grad_norm, ora.last_grad_norm, ora.last_clip))
    return flat, opt, ora, norms


def test_oracle_matches_fp64_torch_adam_with_clip_grad_norm():
    torch.manual_seed(3)
    p0 = torch.randn(257, dtype=torch.float64)
    p = torch.nn.Parameter(p0.clone())
    wd, mx, gs = 0.01, 0.5, 0.25
    ta = torch.optim.Adam([p], lr=LR, eps=EPS, weight_decay=wd)
    ora = adam_oracle64(p0, lr=LR, eps=EPS, wd=wd, max_grad_norm=mx)
    clips = []
    for _ in range(4):
        g = torch.randn(257, dtype=torch.float64) * 3
        p.grad = g * gs
        total = torch.nn.utils.clip_grad_norm_([p], mx)
        ta.step()
        ora.step(g, gs)
        clips.append(ora.last_clip)
        torch.testing.assert_close(torch.tensor(ora.last_grad_norm, dtype=torch.float64), total,
                                   rtol=1e-12, atol=0)
    assert max(clips) < 0.9  # the clip was active
    torch.testing.assert_close(ora.p, p.detach(), rtol=1e-12, atol=1e-14)


@pytest.mark.parametrize("max_grad_norm,wd,grad_scale", CASES)
def test_flat_adam_cpu_vs_oracle64(max_grad_norm, wd, grad_scale):
    flat, opt, ora, norms = _run(max_grad_norm, wd, grad_scale)
    torch.testing.assert_close(flat.data.double(), ora.p, rtol=1e-4, atol=1e-5)
    assert opt.step_count == 5
    for got, want, clip in norms:
        if max_grad_norm > 0:
            torch.testing.assert_close(got.double(), torch.tensor(want, dtype=torch.float64),
                                       rtol=1e-5, atol=0)
        else:
            assert got is None
    if max_grad_norm == 0.5:
        assert all(c < 0.9 for _, _, c in norms)  # the clip binds in these cases
    assert opt.shadow.dtype == torch.bfloat16
    assert torch.equal(opt.shadow, flat.data.bfloat16())
    for _, o, n, _ in flat.slices:  # padding is never touched (wd: it is 0 and stays 0)
        pad_end = (o + n + 63) // 64 * 64
        assert float(flat.data[o + n:pad_end].abs().sum()) == 0.0


def test_huge_max_grad_norm_is_bit_equal_to_no_clipping():
    a = _run(1e6, 0.0, 0.5)
    b = _run(0.0, 0.0, 0.5)
    assert all(c == 1.0 for _, _, c in a[3])
    assert torch.equal(a[0].data, b[0].data)
    assert torch.equal(a[1].m, b[1].m) and torch.equal(a[1].v, b[1].v)


def test_state_dict_round_trip_next_step_bit_equal():
    flat, opt, _, _ = _run(0.5, 0.01, 0.25, steps=3)
    sd = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state_dict().items()}
    m2 = _model()
    flat2 = FlatParams(m2, "cpu")
    flat2.data.copy_(flat.data)
    opt2 = FlatAdam(flat2, lr=LR, eps=EPS, weight_decay=0.01, max_grad_norm=0.5, bf16_shadow=True)
    opt2.load_state_dict(sd)
    assert opt2.step_count == 3
    g = torch.randn(flat.numel, generator=torch.Generator().manual_seed(9))
    for f, o in ((flat, opt), (flat2, opt2)):
        f.grad.copy_(g)
        o.step(grad_scale=0.25)
    assert torch.equal(flat.data, flat2.data)
    assert torch.equal(opt.m, opt2.m) and torch.equal(opt.v, opt2.v)
    assert torch.equal(opt.shadow, opt2.shadow) and opt2.step_count == 4
