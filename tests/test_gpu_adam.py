"""adam.hip on the MI355X against the fp64 Adam oracle (objective_cases.adam_oracle64): the
grid-stride loop (a flat buffer above 2048 * 256 elements), global-norm clipping through
``mbk_grad_clip_scale`` -> ``gscale``, the folded ``gmul``, weight decay, late-step bias
correction, the bf16 shadow bit for bit, untouched padding; the clip-scale launcher and the two
bf16 converters called directly at their edge sizes; and one real HIP learner update with
clipping, checked on the learner's own gradient."""
import copy

import pytest
import torch

from microbeast_amd import _native as N
from microbeast_amd.ops.optim import FlatAdam, FlatParams
from objective_cases import adam_oracle64

pytestmark = pytest.mark.gpu

LR, EPS = 1e-2, 1e-5
NUMELS = (700001, 300003, 5, 1)   # flat: 1000192 elements with padding after every slice
SCALES = (1e-3, 1.0, 30.0, 1.0)   # per-parameter gradient scales


class _Bag(torch.nn.Module):
    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(0)
        self.ps = torch.nn.ParameterList(
            [torch.nn.Parameter(torch.randn(n, generator=g)) for n in NUMELS])


def _flat(dev):
    flat = FlatParams(_Bag(), dev)
    assert flat.numel == 1000192 and flat.numel > 2048 * 256
    return flat


def _grad(flat, seed):
    """Flat gradient on the CPU: N(0, 1) * s per parameter, about 1 % exact zeros, padding 0."""
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(flat.numel)
    for (_, o, n, _), s in zip(flat.slices, SCALES):
        x = torch.randn(n, generator=g) * s
        x[torch.rand(n, generator=g) < 0.01] = 0.0
        out[o:o + n] = x
    return out


def _pad_mask(flat):
    pad = torch.ones(flat.numel, dtype=torch.bool)
    for _, o, n, _ in flat.slices:
        pad[o:o + n] = False
    return pad


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _run(dev, clip_factor, wd, grad_scale, shadow, steps=3, max_grad_norm=None):
    """``steps`` device steps beside the oracle on the same gradients. ``clip_factor``: the
    clip bound is that fraction of the first gradient's fp64 norm (after grad_scale)."""
    flat = _flat(dev)
    grads = [_grad(flat, 10 + i) for i in range(steps)]
    if max_grad_norm is None:
        norm0 = float((grads[0].double() * grad_scale).norm())
        max_grad_norm = clip_factor * norm0 if clip_factor else 0.0
    opt = FlatAdam(flat, lr=LR, eps=EPS, weight_decay=wd, max_grad_norm=max_grad_norm,
                   bf16_shadow=shadow)
    ora = adam_oracle64(flat.data, lr=LR, eps=EPS, wd=wd, max_grad_norm=max_grad_norm)
    norms = []
    for g in grads:
        flat.grad.copy_(g)
        opt.step(grad_scale=grad_scale)
        ora.step(g, grad_scale)
        norms.append((None if opt.last_grad_norm is None else float(opt.last_grad_norm),
                      ora.last_grad_norm, ora.last_clip))
    torch.cuda.synchronize()
    return flat, opt, ora, norms


@pytest.mark.parametrize("shadow", [True, False])
@pytest.mark.parametrize("clip_factor,wd,grad_scale", [
    (0.0, 0.0, 1.0), (0.05, 0.0, 1.0), (0.5, 0.01, 0.25), (1e6, 0.0, 0.5)])
def test_flat_adam_kernel_vs_oracle64(cuda, clip_factor, wd, grad_scale, shadow):
    flat, opt, ora, norms = _run(cuda, clip_factor, wd, grad_scale, shadow)
    print(f"norms (kernel, fp64, clip factor): {norms}")
    torch.testing.assert_close(flat.data.cpu().double(), ora.p, rtol=1e-4, atol=1e-5)
    for got, want, clip in norms:
        if clip_factor:
            assert abs(got - want) <= 1e-5 * want
            if clip_factor < 1:  # the clip binds, well away from 1
                assert abs(clip - clip_factor) < 0.1 * clip_factor
            else:
                assert clip == 1.0
        else:
            assert got is None
    pad = _pad_mask(flat)
    assert float(flat.data.cpu()[pad].abs().sum()) == 0.0
    if wd == 0.0:
        assert float(opt.m.cpu()[pad].abs().sum()) == 0.0
        assert float(opt.v.cpu()[pad].abs().sum()) == 0.0
    if shadow:
        assert torch.equal(_bits(opt.shadow).cpu(), _bits(flat.data.cpu().bfloat16()))
    else:
        assert opt.shadow is None


def test_unreachable_clip_bound_is_bit_equal_to_no_clipping(cuda):
    a = _run(cuda, None, 0.0, 0.5, True, max_grad_norm=1e30)
    b = _run(cuda, None, 0.0, 0.5, True, max_grad_norm=0.0)
    assert all(c == 1.0 for _, _, c in a[3]) and a[3][0][0] is not None
    assert torch.equal(a[0].data, b[0].data)
    assert torch.equal(a[1].m, b[1].m) and torch.equal(a[1].v, b[1].v)
    assert torch.equal(_bits(a[1].shadow), _bits(b[1].shadow))


@pytest.mark.parametrize("step", [1, 999, 100000])
def test_bias_correction_at_later_steps(cuda, step):
    flat = _flat(cuda)
    g = torch.Generator().manual_seed(step)
    m0 = torch.randn(flat.numel, generator=g) * 0.1
    v0 = torch.rand(flat.numel, generator=g) * 0.5
    v0[torch.rand(flat.numel, generator=g) < 0.01] = 0.0
    opt = FlatAdam(flat, lr=LR, eps=EPS, bf16_shadow=True)
    opt.load_state_dict({"m": m0, "v": v0, "step": step})
    ora = adam_oracle64(flat.data, lr=LR, eps=EPS, m=m0, v=v0, step=step)
    gr = _grad(flat, 77)
    flat.grad.copy_(gr)
    opt.step()
    ora.step(gr)
    assert opt.step_count == step + 1 == ora.step_count
    torch.testing.assert_close(flat.data.cpu().double(), ora.p, rtol=1e-4, atol=1e-5)
    # the moments, at the parameters' rtol: fp32 holds 1 - b2 = 1 - 0.999f only to about 3e-5
    # relative (2^-25 * 0.999 / 0.001), so the g^2 term of v cannot match fp64 more closely;
    # atol: a few fp32 roundings at the largest |m| (3) and |v| (0.5 + 900 * 0.001) here
    torch.testing.assert_close(opt.m.cpu().double(), ora.m, rtol=1e-4, atol=1e-6)
    torch.testing.assert_close(opt.v.cpu().double(), ora.v, rtol=1e-4, atol=1e-7)
    assert torch.equal(_bits(opt.shadow).cpu(), _bits(flat.data.cpu().bfloat16()))


def _clip_scale(g, max_norm, gmul):
    """mbk_grad_clip_scale with ``partials`` and ``scale`` poisoned first; returns scale [2]."""
    partials = torch.full((1024,), float("nan"), device=g.device)
    scale = torch.full((2,), float("nan"), device=g.device)
    assert g.data_ptr() % 16 == 0 and g.dtype == torch.float32 and g.is_contiguous()
    N.check(N.kernels().mbk_grad_clip_scale(g.data_ptr(), g.numel(), max_norm, gmul,
                                            partials.data_ptr(), scale.data_ptr(),
                                            N.stream_ptr()), "grad_clip_scale")
    return scale.cpu()


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1023, 262147, 1048577])
def test_grad_clip_scale_direct(cuda, n):
    """n % 4 != 0 runs the scalar tail of the square-norm (FlatAdam never does: its buffer is a
    multiple of 64). The tail elements are made large so that dropping them shows at any n."""
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    if n % 4 and n > 4:
        g[n - n % 4:] = torch.tensor([40.0, -50.0, 60.0])[:n % 4] * (n ** 0.5) / 30
    norm = float(g.double().norm())
    tail = float(g[n - n % 4:].double().norm()) if n % 4 else 0.0
    assert n % 4 == 0 or tail > 0.3 * norm
    gd = g.to(cuda)
    tol = 1e-5
    for gmul in (1.0, 0.125):
        want = gmul * norm
        s = _clip_scale(gd, 0.3 * want, gmul)
        assert abs(float(s[1]) - want) <= tol * want, (float(s[1]), want)
        clip = min(1.0, 0.3 * want / (want + 1e-6))
        assert abs(float(s[0]) - clip) <= tol * clip, (float(s[0]), clip)
        assert float(s[0]) < 0.31
        assert torch.equal(s, _clip_scale(gd, 0.3 * want, gmul))  # bit-reproducible
        s0 = _clip_scale(gd, 0.0, gmul)
        assert float(s0[0]) == 1.0 and float(s0[1]) == float(s[1])
        s1 = _clip_scale(gd, 7.0 * want, gmul)  # a bound above the norm: no clipping
        assert float(s1[0]) == 1.0
    a, b = _clip_scale(gd, 0.0, 1.0), _clip_scale(gd, 0.0, 0.125)
    assert float(b[1]) == 0.125 * float(a[1])  # gmul scales the norm exactly once


def _f32_from_bits(bits):
    signed = [b - (1 << 32) if b >= (1 << 31) else b for b in bits]
    return torch.tensor(signed, dtype=torch.int32).view(torch.float32)


@pytest.mark.parametrize("n", [1, 255, 600001])
def test_bf16_converters_direct(cuda, n):
    """mbk_to_bf16 == round-to-nearest-even (.bfloat16()), mbk_from_bf16 == the exact widening
    (.float()), bit for bit, on ties, signed zeros, the largest finite fp32 (rounds to inf),
    infinities, subnormals and random bit patterns (NaNs left out: their payload is free)."""
    special = _f32_from_bits([
        0x3F808000,              # 1 + 2^-8: half-way, ties to even -> 0x3F80
        0x3F818000,              # half-way the other way: ties to even -> 0x3F82
        0x3F808001, 0x3F807FFF,  # just above / just below half-way
        0x00000000, 0x80000000,  # +0, -0
        0x7F7FFFFF, 0xFF7FFFFF,  # the largest finite fp32, both signs -> +-inf
        0x7F800000, 0xFF800000,  # +-inf
        0xBF808000, 0xBF818000,  # the two ties, negative
        0x7F7F7FFF, 0x7F7F8000,  # just below the largest bf16's upper half-way point / on it
    ])
    g = torch.Generator().manual_seed(n)
    x = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    x = x.view(torch.float32).clone()
    x[torch.isnan(x)] = 1.0
    k = min(n, special.numel())
    x[:k] = special[:k]
    want = x.bfloat16()
    k_ = N.kernels()
    pad = 64
    y = torch.full((n + 2 * pad,), 123.0, dtype=torch.bfloat16, device=cuda)
    xd = x.to(cuda)
    N.check(k_.mbk_to_bf16(xd.data_ptr(), n, y[pad:].data_ptr(), N.stream_ptr()), "to_bf16")
    yc = y.cpu()
    assert torch.equal(_bits(yc[pad:pad + n]), _bits(want))
    assert bool((yc[:pad] == 123.0).all()) and bool((yc[pad + n:] == 123.0).all())
    # and back: every non-NaN bf16 pattern widens exactly
    h = torch.randint(-2 ** 15, 2 ** 15 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int16)
    h = h.view(torch.bfloat16).clone()
    h[torch.isnan(h)] = 1.0
    h[:k] = want[:k]
    z = torch.full((n + 2 * pad,), 123.0, dtype=torch.float32, device=cuda)
    hd = h.to(cuda)
    N.check(k_.mbk_from_bf16(hd.data_ptr(), n, z[pad:].data_ptr(), N.stream_ptr()), "from_bf16")
    zc = z.cpu()
    assert torch.equal(_bits(zc[pad:pad + n]), _bits(h.float()))
    assert bool((zc[:pad] == 123.0).all()) and bool((zc[pad + n:] == 123.0).all())


def test_hip_learner_update_with_grad_clipping(cuda):
    """One learn() of the HIP learner (the S = 8 setup of
    test_gpu_learner_parity.py::test_learn_hip_matches_fp32_torch) with ``max_grad_norm`` at
    half the observed norm: the gradient buffer's padding is exactly 0 (no direct-gradient
    kernel writes past its slot), ``last_grad_norm`` is the norm of the learner's own gradient,
    and the update is the fp64 oracle's on that gradient -- the optimiser alone, away from the
    bf16 floor of the backward pass."""
    from helpers import engine_batches
    from microbeast_amd.learner import Learner, LearnerHParams
    from microbeast_amd.models.agent import Agent

    S = 8
    b = engine_batches(cuda, S, 2, groups=4, envs=64, T=8, seed=S)[1]
    torch.manual_seed(7)
    base = Agent((S, S, 27))
    with torch.no_grad():
        base.actor.weight.normal_(0, 0.02)
        base.actor.bias.normal_(0, 0.02)
    L0 = Learner(copy.deepcopy(base), LearnerHParams(), cuda)
    L0.learn(b)
    norm0 = float(L0.flat.grad.cpu().double().norm())
    assert norm0 > 0 and L0.opt.last_grad_norm is None
    hp = LearnerHParams(max_grad_norm=0.5 * norm0)
    L = Learner(copy.deepcopy(base), hp, cuda)
    p0 = L.flat.data.cpu().clone()
    L.learn(b)
    torch.cuda.synchronize()
    g = L.flat.grad.cpu()
    pad = _pad_mask(L.flat)
    assert bool(pad.any()) and float(g[pad].abs().max()) == 0.0
    sl = torch.cat([g[o:o + n] for _, o, n, _ in L.flat.slices]).double()
    want = float(sl.norm())
    got = float(L.opt.last_grad_norm)
    print(f"grad norm: kernel {got!r} fp64 {want!r} (unclipped run: {norm0!r})")
    assert abs(got - want) <= 1e-5 * want
    ora = adam_oracle64(p0, lr=hp.lr, eps=hp.adam_eps, max_grad_norm=hp.max_grad_norm)
    ora.step(g)
    assert 0.4 < ora.last_clip < 0.6
    torch.testing.assert_close(L.flat.data.cpu().double(), ora.p, rtol=1e-4, atol=1e-5)
    assert not torch.equal(L.flat.data.cpu(), p0)
