"""The stage-0 weight gradient summed over the non-empty cells (conv.hip wgrad0_sparse_kernel,
``HipEncoder.sparse_wgrad0``) against the dense pool-fused kernel it replaces by default.

Both scatter the same bf16 dY tile, so the stage-0 weight and bias gradients differ in fp32
summation order only (the project's order-only bound, 1e-5 relative, as
test_gpu_conv.py::test_wgrad_queue_matches_static); every other gradient is untouched."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_WGRAD_QUEUE = 4  # common.h kQueueWgrad (off for the suite: conftest.py)
ORDER_ONLY = 1e-5
S = 256


def _rel(a, b):
    return ((a.float() - b.float()).norm() / (b.float().norm() + 1e-12)).item()


def _random_words(g, shape):
    from microbeast_amd.ops.encoder import PLANE_GROUPS
    w = torch.zeros(shape, dtype=torch.int64)
    for off, k in PLANE_GROUPS:
        w |= 1 << (off + torch.randint(0, k, shape, generator=g))
    return w


def _nonempty_words(g, n):
    """n random one-hot words, none of them the empty word."""
    from microbeast_amd.ops.encoder import EMPTY_WORD
    w = _random_words(g, (n,))
    return torch.where(w == EMPTY_WORD, torch.full_like(w, EMPTY_WORD ^ 0x3), w)


def _mixed_obs(n, seed):
    """Image i is of kind i % 6: non-empty cells on every border row and column (and a few
    inside); none; exactly 1, at a corner (the four corners in turn); exactly 32; exactly 33 (one
    full block and one more cell); all 256 random words."""
    from microbeast_amd.ops.encoder import EMPTY_WORD
    g = torch.Generator().manual_seed(seed)
    obs = torch.full((n, S), EMPTY_WORD, dtype=torch.int64)
    border = [y * 16 + x for y in range(16) for x in range(16) if y in (0, 15) or x in (0, 15)]
    corners = [0, 15, 240, 255]
    for i in range(n):
        kind = i % 6
        if kind == 0:
            cells = torch.tensor(border + [17, 100, 238])
        elif kind == 1:
            continue
        elif kind == 2:
            cells = torch.tensor([corners[(i // 6) % 4]])
        elif kind in (3, 4):
            cells = torch.randperm(S, generator=g)[:32 if kind == 3 else 33]
        else:
            obs[i] = _random_words(g, (S,))
            continue
        obs[i, cells] = _nonempty_words(g, len(cells))
    return obs.to(torch.int32)


def _setup(cuda, n, seed):
    from microbeast_amd.models.agent import Agent
    from microbeast_amd.ops.encoder import encoder_params
    torch.manual_seed(2)
    m = Agent((16, 16, 27)).to(cuda)
    obs = _mixed_obs(n, seed).to(cuda)
    m.features(obs[:1])
    return m, m._hip_enc, encoder_params(m.network, 3), obs


def _grads(enc, params, obs, cuda, sparse):
    from microbeast_amd.ops.encoder import encode
    enc.sparse_wgrad0 = sparse
    try:
        for p in params:
            p.grad = None
        y = encode(obs, enc, params, True).float()
        r = torch.randn(y.shape, generator=torch.Generator().manual_seed(7)).to(cuda)
        (y * r).sum().backward()
        torch.cuda.synchronize()
        return [p.grad.detach().clone() for p in params]
    finally:
        enc.sparse_wgrad0 = True


def _check_pair(dense, sparse):
    for i in (0, 1):  # stage-0 weight and bias
        assert torch.isfinite(sparse[i]).all(), i
        assert float(sparse[i].abs().sum()) > 0, i
        rel = _rel(sparse[i], dense[i])
        print(f"param {i}: rel {rel:.3e} max|diff| {float((sparse[i] - dense[i]).abs().max()):.3e}"
              f" max|dense| {float(dense[i].abs().max()):.3e}")
        assert rel < ORDER_ONLY, (i, rel)
    for i in range(2, len(dense)):
        assert torch.equal(dense[i], sparse[i]), i


@pytest.mark.parametrize("n", [1, 3, 67, 300])
def test_sparse_matches_dense(cuda, n):
    """n = 1: a border image; 3: border, empty, one corner cell; 67 and 300: every kind of
    _mixed_obs (0, 1, 32, 33, 256 non-empty cells, borders), 300 over more than one image per
    wave."""
    m, enc, params, obs = _setup(cuda, n, seed=n)
    assert enc.sparse_wgrad0 and enc.fused_pool_wgrad0
    dense = _grads(enc, params, obs, cuda, False)
    sparse = _grads(enc, params, obs, cuda, True)
    _check_pair(dense, sparse)


def test_queue_matches_static_and_static_repeats(cuda):
    """The per-wave image queue (16-image chunks) against the static stride: each image summed
    exactly once, so equal up to fp32 summation order; the static stride twice: bit-identical."""
    from microbeast_amd import _native as N
    m, enc, params, obs = _setup(cuda, 300, seed=31)
    s0 = _grads(enc, params, obs, cuda, True)
    s1 = _grads(enc, params, obs, cuda, True)
    for a, b in zip(s0, s1):
        assert torch.equal(a, b)
    N.check(N.kernels().mbk_set_work_queue_site(_WGRAD_QUEUE, 1), "queue site")
    try:
        q = _grads(enc, params, obs, cuda, True)
        q2 = _grads(enc, params, obs, cuda, True)  # the counters reset themselves
    finally:
        N.check(N.kernels().mbk_set_work_queue_site(_WGRAD_QUEUE, 0), "queue site")
    for g in (q, q2):
        for i, (a, b) in enumerate(zip(s0, g)):
            assert torch.isfinite(b).all(), i
            assert _rel(b, a) < ORDER_ONLY, (i, _rel(b, a))
        assert float(g[0].abs().sum()) > 0


_CAP_CHILD = """
import sys
sys.path.insert(0, {root!r}); sys.path.insert(0, {root!r} + '/tests')
import torch
from microbeast_amd import _native as N
K = N.kernels()
N.check(K.mbk_set_learner_occupancy(0, 1), 'occupancy')
N.check(K.mbk_set_work_queue_site(4, 0), 'queue site')
import test_gpu_wgrad0_sparse as T
cuda = torch.device('cuda', 0)
n = 1700
parts = K.mbk_conv_wgrad0_sparse_parts(n)
cus = torch.cuda.get_device_properties(0).multi_processor_count
assert 1 <= parts <= 2 * cus < (n + 2) // 3, (parts, cus)
m, enc, params, obs = T._setup(cuda, n, seed=5)
T._check_pair(T._grads(enc, params, obs, cuda, False), T._grads(enc, params, obs, cuda, True))
print('CAP_OK', parts)
"""


def test_small_grid_many_images_per_wave(cuda):
    """A grid capped at 5 workgroups (15 waves, 20 images each, the prefetch and the image loop
    at length) against the dense kernel, static stride and queue."""
    from microbeast_amd import _native as N
    m, enc, params, obs = _setup(cuda, 300, seed=17)
    K = N.kernels()
    try:
        K.mbk_conv_set_grid_cap(5)
        assert K.mbk_conv_wgrad0_sparse_parts(300) == 5
        dense = _grads(enc, params, obs, cuda, False)
        _check_pair(dense, _grads(enc, params, obs, cuda, True))
        N.check(K.mbk_set_work_queue_site(_WGRAD_QUEUE, 1), "queue site")
        _check_pair(dense, _grads(enc, params, obs, cuda, True))
    finally:
        N.check(K.mbk_set_work_queue_site(_WGRAD_QUEUE, 0), "queue site")
        K.mbk_conv_set_grid_cap(0)


def test_under_the_backward_cap(cuda):
    """mbk_set_learner_occupancy(0, 1), set before the first grid is sized and so in a process
    of its own: at most two workgroups per CU (the kernel's 208 registers already hold it to two,
    so the cap bounds the grid without shrinking it), 1700 images, several per wave."""
    r = subprocess.run([sys.executable, "-c", _CAP_CHILD.format(root=ROOT)], cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "CAP_OK" in r.stdout, r.stdout[-2000:]
