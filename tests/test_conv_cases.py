"""The conv oracles of tests/conv_cases.py checked on the CPU: the tap sums against fp64
F.conv2d / max_pool2d and autograd, the exact case's representability at every shape of the GPU
matrix, and oracle-side mutations (a mutant the bounds could not tell from the oracle would mean
a kernel with that defect passes tests/test_gpu_conv_layers.py)."""
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


@pytest.mark.parametrize("n,H,W,cin,cout", [(3, 1, 1, 32, 32), (2, 5, 8, 16, 32), (2, 6, 6, 32, 16)])
def test_tap_sums_match_conv2d_and_autograd(n, H, W, cin, cout):
    c = cc.Case("round", 100 + H * W)
    x, add, dy, mask = (c.acts((n, H, W, ch)) for ch in (cin, cout, cout, cin))
    w, b = c.weights(cout, cin), c.bias(cout)
    wq = w.bfloat16().double()
    tol = dict(rtol=1e-12, atol=1e-12)
    for relu in (False, True):
        xt = _nchw(x.double()).clone().requires_grad_(True)
        wt = wq.clone().requires_grad_(True)
        bt = b.double().clone().requires_grad_(True)
        yt = F.conv2d(F.relu(xt) if relu else xt, wt, bt, padding=1)
        y, A = cc.conv_fwd_ref(x, w, b, relu, add)
        torch.testing.assert_close(y, _nhwc(yt.detach()) + add.double(), **tol)
        assert bool((A >= y.abs() - 1e-12).all())
        yt.backward(_nchw(dy.double()))
        dW, db, Aw, Ab = cc.conv_wgrad_ref(x, dy, relu)
        torch.testing.assert_close(dW, wt.grad, **tol)
        torch.testing.assert_close(db, bt.grad, **tol)
        assert bool((Aw >= dW.abs() - 1e-12).all()) and bool((Ab >= db.abs() - 1e-12).all())
        if not relu:  # dx of the plain conv; the mask and the residual are the caller's
            dx, Ad = cc.conv_dgrad_ref(dy, w)
            torch.testing.assert_close(dx, _nhwc(xt.grad), **tol)
            dxm, _ = cc.conv_dgrad_ref(dy, w, mask_src=mask, add=x)
            torch.testing.assert_close(dxm, dx * (mask.double() > 0) + x.double(), **tol)
            assert bool((Ad >= dx.abs() - 1e-12).all())


@pytest.mark.parametrize("n,H,W,C", [(2, 1, 1, 16), (3, 5, 8, 16), (2, 6, 6, 32), (2, 3, 3, 32)])
@pytest.mark.parametrize("kind", ["exact", "round"])
def test_pool_matches_max_pool2d(kind, n, H, W, C):
    """Values always; the window byte against ATen's flat index (its first maximum in scan order
    too), on the exact case's constant ties as well; the backward against autograd."""
    c = cc.Case(kind, 7 + H)
    x = c.acts((n, H, W, C))
    v, idx = cc.pool_ref(x)
    xt = _nchw(x.double()).clone().requires_grad_(True)
    vt, it = F.max_pool2d(xt, 3, 2, 1, return_indices=True)
    assert torch.equal(v, _nhwc(vt.detach()))
    Ho, Wo = v.shape[1:3]
    oy = torch.arange(Ho).view(1, Ho, 1, 1)
    ox = torch.arange(Wo).view(1, 1, Wo, 1)
    ky, kx = (idx // 3).long(), (idx % 3).long()
    flat = (2 * oy - 1 + ky) * W + (2 * ox - 1 + kx)
    assert torch.equal(flat, _nhwc(it))
    dp = c.acts((n, Ho, Wo, C))
    vt.backward(_nchw(dp.double()))
    dc, A, hits = cc.pool_bwd_ref(dp, idx, H, W)
    torch.testing.assert_close(dc, _nhwc(xt.grad), rtol=1e-12, atol=1e-12)
    assert float(hits.sum()) == dp.numel() and float(hits.max()) <= 4
    assert bool((A >= dc.abs() - 1e-12).all())
    if kind == "exact" and H > 1:
        assert int((cc.pool_ref(x, last=True)[1] != idx).sum()) > 0  # the ties are there


def _layer_operands(c, n, cin, cout, H, W, bits):
    x = cc.planes_nhwc(c.obs(n, H, W), H, W) if bits else c.acts((n, H, W, cin)).double()
    w = c.weights(cout, x.shape[-1])
    return x, w, c.bias(cout), c.acts((n, H, W, cout)), c.acts((n, H, W, cout))


@pytest.mark.parametrize("enc,li", cc.distinct_layers({**cc.ENCODERS, **cc.NONSQUARE}))
def test_exact_case_is_representable(enc, li):
    """Forward (plain and relu + add), data gradient and weight gradient of every layer of the
    GPU matrix on the exact case: exact in fp32 in any order, and the bf16 outputs exactly
    representable, so the GPU tests may ask for torch.equal."""
    h, w_, ch = {**cc.ENCODERS, **cc.NONSQUARE}[enc]
    _, cin, cout, H, W, bits, relu, pool = cc.trunk_layers(h, w_, ch)[li]
    worst = 0.0
    for seed in range(3):
        c = cc.Case("exact", 1000 * seed + li)
        n = max(3, 64 // (H * W))
        x, w, b, add, dy = _layer_operands(c, n, cin, cout, H, W, bits)
        for r, a in ((False, None), (relu, None if pool else add)):
            y, A = cc.conv_fwd_ref(x, w, b, r, a)
            cc.assert_fp32_exact(A, x, w)
            cc.assert_bf16_exact(y)
            worst = max(worst, float(y.abs().max()))
        if not bits:
            dx, A = cc.conv_dgrad_ref(dy, w, mask_src=x, add=x)
            cc.assert_fp32_exact(A, dy, w)
            cc.assert_bf16_exact(dx)
        dW, db, Aw, Ab = cc.conv_wgrad_ref(x, dy, relu)
        cc.assert_fp32_exact(Aw, x, dy)
        assert torch.equal(dW, dW.float().double()) and torch.equal(db, db.float().double())
    assert worst < 128  # bf16 holds halves exactly up to 128


# the factors below are asserted as floors well under what this file measures (README, Tests)
def _mutation_case():
    c = cc.Case("round", 77)
    n, H, W, cin, cout = 4, 6, 10, 16, 32
    x, add = c.acts((n, H, W, cin)), c.acts((n, H, W, cout))
    w, b = c.weights(cout, cin), c.bias(cout)
    y, A = cc.conv_fwd_ref(x, w, b, True, add)
    return c, x, add, w, b, y, A, cc.bf16_bound(y, A, 9 * cin + 2)


def test_mutant_shifted_tap_and_dropped_relu_exceed_the_bound(capsys):
    c, x, add, w, b, y, A, bound = _mutation_case()
    taps = list(cc.TAPS)
    taps[0] = (-1, 0)  # tap (ky, kx) = (0, 0) reads the pixel of tap (0, 1)
    shifted = cc.worst_ratio(cc.conv_fwd_ref(x, w, b, True, add, taps)[0], y, bound)
    norelu = cc.worst_ratio(cc.conv_fwd_ref(x, w, b, False, add)[0], y, bound)
    with capsys.disabled():
        print(f"\nmutation factors: shifted tap {shifted:.0f}, dropped relu {norelu:.0f}")
    assert shifted > 50 and norelu > 50


def test_mutant_swapped_h_w_exceeds_the_bound(capsys):
    """The same buffer walked as a W x H map (what swapped launcher arguments would compute)."""
    c, x, add, w, b, y, A, bound = _mutation_case()
    n, H, W, cin = x.shape
    ys = cc.conv_fwd_ref(x.reshape(n, W, H, cin), w, b, True, add.reshape(n, W, H, -1))[0]
    f = cc.worst_ratio(ys.reshape(y.shape), y, bound)
    with capsys.disabled():
        print(f"\nmutation factor: swapped H and W {f:.0f}")
    assert f > 50
    # the weight gradient too (fp32 bound)
    dy = c.acts(y.shape)
    dW, _, Aw, _ = cc.conv_wgrad_ref(x, dy, True)
    dWs = cc.conv_wgrad_ref(x.reshape(n, W, H, cin), dy.reshape(n, W, H, -1), True)[0]
    assert cc.worst_ratio(dWs, dW, cc.f32_bound(Aw, n * H * W)) > 50


def test_mutant_truncating_store_exceeds_the_bound(capsys):
    """Truncation errs by up to one bf16 ulp, 2^-7 |ref| at the bottom of a binade, against the
    store term's 2^-8 |ref|: a factor that approaches 2 from below, and no more than that, so a
    truncating kernel fails on the elements near the bottom of their binade."""
    c, x, add, w, b, y, A, bound = _mutation_case()
    assert cc.worst_ratio(y.bfloat16().double(), y, bound) < 1.0  # round to nearest passes
    f = cc.worst_ratio(cc.round_trunc_bf16(y), y, bound)
    frac = float(((cc.round_trunc_bf16(y) - y).abs() > bound).double().mean())
    with capsys.disabled():
        print(f"\nmutation factor: truncating store {f:.2f} ({100 * frac:.0f} % of elements)")
    assert f > 1.7 and frac > 0.1


def test_mutant_last_maximum_moves_the_bytes(capsys):
    """Exact case: windows tie constantly, so the last-maximum rule moves a large share of the
    argmax bytes while every pooled value stays the same (values alone could not see it)."""
    c = cc.Case("exact", 5)
    x = c.acts((4, 8, 8, 16))
    w, b = c.weights(32, 16), c.bias(32)
    y = cc.conv_fwd_ref(x, w, b)[0]
    v0, i0 = cc.pool_ref(y)
    v1, i1 = cc.pool_ref(y, last=True)
    frac = float((i0 != i1).double().mean())
    with capsys.disabled():
        print(f"\nmutation: last maximum moves {100 * frac:.1f} % of the argmax bytes")
    assert torch.equal(v0, v1) and frac > 0.02
    # and the backward through the moved bytes differs from the true one
    dp = c.acts(v0.shape)
    assert not torch.equal(cc.pool_bwd_ref(dp, i0, 8, 8)[0], cc.pool_bwd_ref(dp, i1, 8, 8)[0])
