"""The trunk-tail oracles of tests/tail_cases.py checked on the CPU: against fp64 nn.Linear +
relu + critic with autograd on the reference's NCHW flatten (through ops/tail.py's three index
maps, at square and non-square maps), the exact case's exactness at every shape of the GPU
matrix, and oracle-side mutants on the GPU tests' own inputs (a mutant the bounds could not
tell from the oracle would mean a kernel with that defect passes tests/test_gpu_tail.py)."""
import pytest
import torch

import tail_cases as tc
from microbeast_amd.ops.linear import nhwc_weight
from microbeast_amd.ops.tail import nhwc_linear_maps

TOL = dict(rtol=1e-12, atol=1e-12)


def _report(capsys, text):
    with capsys.disabled():
        print("\n" + text)


# ------------------------------------------------------------------ oracles vs autograd
@pytest.mark.parametrize("c,ho,wo", tc.MAP_SHAPES)
def test_oracles_match_linear_autograd_through_the_maps(c, ho, wo):
    """relu -> Linear (NCHW flatten, parameter-layout weight) -> relu -> critic, plus a head-like
    second consumer of the first rows of f, in fp64 autograd; against fc_fwd_ref / critic_ref /
    value_bwd_ref / gemm_nt_ref / wgrad_ref on the NHWC flatten with the weight gathered through
    the fwd and dgrad maps, and the NHWC dW scattered back through the grad map."""
    k1, n, rows = 24, 37, 29
    g = torch.Generator().manual_seed(100 * ho + wo)
    f_in = c * ho * wo
    y = torch.randn(n, ho, wo, c, generator=g, dtype=torch.float64)       # NHWC trunk output
    w = (torch.randn(k1, f_in, generator=g) * 0.2).bfloat16().double()    # parameter layout
    b, wc, bc = (torch.randn(s, generator=g, dtype=torch.float64) for s in (k1, k1, 1))
    dv = torch.randn(n, generator=g, dtype=torch.float64)
    gadd = torch.randn(rows, k1, generator=g, dtype=torch.float64)
    # independent: the reference model's layout
    x = y.permute(0, 3, 1, 2).reshape(n, -1).clone().requires_grad_(True)
    wt_, bt, wct, bct = (t.clone().requires_grad_(True) for t in (w, b, wc, bc))
    ft = torch.relu(torch.nn.functional.linear(torch.relu(x), wt_, bt))
    vt = ft @ wct + bct
    ((vt * dv).sum() + (ft[:rows] * gadd).sum()).backward()
    # the oracles on the kernels' operands
    fwd, dgrad, grad = (m.long() for m in nhwc_linear_maps(k1, c, ho, wo))
    wp, wT = w.reshape(-1)[fwd], w.reshape(-1)[dgrad]
    assert wp.shape == (k1, f_in) and wT.shape == (f_in, k1)
    y2 = y.reshape(n, -1)
    f, A = tc.fc_fwd_ref(y2, wp, b, True)
    torch.testing.assert_close(f, ft.detach(), **TOL)
    assert bool((A >= f - 1e-12).all())
    v, Av = tc.critic_ref(f, wc, bc)
    torch.testing.assert_close(v, vt.detach(), **TOL)
    dh, Ah, dW2, Aw2, db2, Ab2 = tc.value_bwd_ref(dv, f, wc, gadd, rows)
    torch.testing.assert_close(dW2, wct.grad, **TOL)
    torch.testing.assert_close(db2.reshape(1), bct.grad, **TOL)
    assert bool((Ah >= dh.abs() - 1e-12).all()) and bool((Aw2 >= dW2.abs() - 1e-12).all())
    dy, Ay = tc.gemm_nt_ref(dh, wT, mask=y2)
    torch.testing.assert_close(dy.view(n, ho, wo, c).permute(0, 3, 1, 2).reshape(n, -1), x.grad,
                               **TOL)
    dW, db, Aw, Ab = tc.wgrad_ref(dh, y2, True)
    torch.testing.assert_close(tc.map_gather_ref(dW, grad).view(k1, f_in), wt_.grad, **TOL)
    torch.testing.assert_close(db, bt.grad, **TOL)
    assert bool((Aw >= dW.abs() - 1e-12).all()) and bool((Ab >= db.abs() - 1e-12).all())
    # ops/linear.py's permutation is the fwd map
    assert torch.equal(nhwc_weight(w, (c, ho, wo)), wp)
    # and chain_ref (what the GPU chain test compares with) is this computation
    fr, dyr, dwr, dbr = tc.chain_ref(y, w, b, dh)
    torch.testing.assert_close(fr, f, **TOL)
    torch.testing.assert_close(dyr, dy, **TOL)
    torch.testing.assert_close(dwr, wt_.grad, **TOL)
    torch.testing.assert_close(dbr, db, **TOL)


def test_gemm_and_gather_oracles_by_hand():
    a = torch.tensor([[1.0, -2.0], [0.5, 3.0]])
    b = torch.tensor([[2.0, 1.0], [-1.0, 0.0], [0.0, 1.0]])
    bias = torch.tensor([1.0, -1.0, 0.25])
    mask = torch.tensor([[1.0, 0.0, -0.0], [-3.0, 2.0, 1e-30]])
    c0 = torch.full((2, 3), 10.0)
    y, A = tc.gemm_nt_ref(a, b, bias, True, mask, c0)
    # a b^T + bias = [[1, -2, -1.75], [5, -1.5, 3.25]] -> relu -> mask -> + 10
    assert y.tolist() == [[11.0, 10.0, 10.0], [10.0, 10.0, 13.25]]
    assert A.tolist() == [[15.0, 10.0, 10.0], [10.0, 11.5, 13.25]]
    src = torch.arange(6.0).view(2, 3)
    assert tc.map_gather_ref(src, torch.tensor([5, -1, 0, 2])).tolist() == [5.0, 0.0, 0.0, 2.0]
    s, As = tc.colsum_ref(torch.tensor([[1.0, -1.0, 7.0], [2.0, -3.0, 7.0]]), 2)
    assert s.tolist() == [3.0, -4.0] and As.tolist() == [3.0, 4.0]
    assert tc.colsum_ref(torch.zeros(0, 3), 2)[0].tolist() == [0.0, 0.0]
    assert tc.gemm_terms(32) == 33 and tc.gemm_terms(32, True, True) == 35


def test_part_lists_take_the_paths_they_name():
    for n in tc.WGRAD_N + tc.WIDE_N:
        for ps in (tc.wgrad_nparts(n), tc.wide_nparts(n)):
            assert 1 in ps and tc.stages(n) in ps and any(p > tc.stages(n) for p in ps)
            assert 65 in ps and 97 in ps  # > 64: the two-level reduce, 65 % 32 = 97 % 32 = 1
    assert 2 in tc.wgrad_nparts(129) and 2 in tc.wgrad_nparts(300)
    for nparts, n in tc.LONG_PARTS.items():  # the last part, alone in its split, has rows
        assert nparts > 64 and nparts % 32 == 1 and tc.stages(n) == nparts and n % tc.STAGE == 5
    Ms, Ns, Ks = ({t[i] for t in tc.GEMM_CASES} for i in range(3))
    assert Ms == {1, 127, 128, 129, 255, 256, 257, 513}
    assert Ns == {1, 8, 31, 32, 33, 64, 65, 72, 128, 129, 136, 264}
    assert Ks == {8, 24, 32, 40, 64, 256, 288}
    for lo, hi in ((1, 32), (33, 64), (65, 1 << 30)):  # every tile meets every epilogue
        tile = [t for t in tc.GEMM_CASES if lo <= t[1] <= hi]
        vec = [t for t in tile if t[3] == "bf16" and t[1] % 8 == 0 and t[7] % 8 == 0 and not t[8]]
        assert vec and any(t[6] for t in vec) and any(t[7] == 8 for t in vec)
        assert any(t[3] == "bf16" and t[1] % 8 for t in tile)
        assert any(t[3] == "bf16" and t[7] == 3 for t in tile)
        assert any(t[3] == "bf16" and t[8] == 1 and t[6] for t in tile)
        assert any(t[3] == "f32" for t in tile) and any(t[3] == "acc" for t in tile)
        for opt in (4, 5, 6):  # bias, relu, mask: with and without
            assert {bool(t[opt]) for t in tile} == {True, False}


# ------------------------------------------------------------------ the exact case is exact
@pytest.mark.parametrize("O,I", tc.FC_RB + tc.FC_GENERIC)
def test_exact_fc_forward(O, I):
    x, w5, b5, wc, bc = tc.fc_operands("exact", O, I)
    pz, nz = tc.signed_zero_counts(x)
    assert pz > 0.05 * x.numel() and nz > 0.05 * x.numel()
    for relu_in in (0, 1):
        f, A = tc.fc_fwd_ref(x, w5, b5, relu_in)
        tc.assert_fp32_exact(A, x, w5, plus=(b5,))
        fb = f.bfloat16()
        v, Av = tc.critic_ref(fb, wc, bc)
        tc.assert_fp32_exact(Av, fb, wc, plus=(bc,))
        assert torch.equal(v, v.float().double())
        # f is rounded for real: values that are no bf16 numbers, ties among them
        moved = fb.double() != f
        assert int(moved.sum()) > 50 and float(f.max()) > 256
        ulp = 2.0 ** (torch.floor(torch.log2(f.clamp_min(1.0))) - 7)
        ties = moved & ((f / ulp - torch.floor(f / ulp)) == 0.5)
        assert int(ties.sum()) > 50
        assert bool((f == 0).any()) and bool((f > 0).any())  # the output relu gates both ways


@pytest.mark.parametrize("idx", range(len(tc.GEMM_CASES)))
def test_exact_gemm(idx):
    M, N, K, out, bias, relu, mask, _, _ = tc.GEMM_CASES[idx]
    a, b, bv, mk, c0 = tc.gemm_operands("exact", idx)
    y, A = tc.gemm_nt_ref(a, b, bv, relu, mk, c0)
    tc.assert_fp32_exact(tc.gemm_nt_ref(a, b, bv, relu, None, c0)[1], a, b,
                         plus=tuple(t for t in (bv, c0) if t is not None))
    if out != "bf16":
        assert torch.equal(y, y.float().double())
    if mask and M * N >= 256:
        pz, nz = tc.signed_zero_counts(mk)
        assert pz > 0 and nz > 0


def test_exact_weight_gradients_and_sums():
    """At the longest row counts used (sums only grow with the rows)."""
    for O, I in tc.WGRAD_OI + [(256, i) for i in tc.WIDE_I]:
        n = max(tc.LONG_PARTS.values())
        assert n > max(tc.WGRAD_N + tc.WIDE_N)
        g, x, out0 = tc.wgrad_operands("exact", O, I, n)
        for relu in (0, 1):
            dW, db, Aw, Ab = tc.wgrad_ref(g, x, relu)
            tc.assert_fp32_exact(Aw + out0.abs().double(), g, x, plus=(out0,))
            tc.assert_fp32_exact(Ab, g)
    for K in tc.VALUE_K:
        R = max(tc.VALUE_R)
        dv, h, w2, gadd = tc.value_operands("exact", K, R)
        dh, Ah, dW2, Aw, db2, Ab = tc.value_bwd_ref(dv, h, w2, gadd, R)
        tc.assert_fp32_exact(Ah, dv, w2, plus=(gadd,))
        tc.assert_bf16_exact(dh)
        tc.assert_fp32_exact(Aw, dv, h)
        assert tc.signed_zero_counts(h)[1] > 0
    for name, C, ld, f32, off in tc.COLSUM_CASES:
        x = tc.colsum_operands("exact", name)
        tc.assert_fp32_exact(tc.colsum_ref(x, C)[1], x)


@pytest.mark.parametrize("ho,wo", tc.CHAIN_SHAPES)
def test_exact_chain(ho, wo):
    y, w5, b5, wc, bc, dh = tc.chain_operands("exact", ho, wo)
    n = y.shape[0]
    fwd, dgrad, grad = (m.long() for m in nhwc_linear_maps(256, 32, ho, wo))
    y2 = y.reshape(n, -1)
    f, A = tc.fc_fwd_ref(y2, w5.reshape(-1)[fwd], b5, True)
    tc.assert_fp32_exact(A, y2, w5, plus=(b5,))
    dy, Ay = tc.gemm_nt_ref(dh, w5.reshape(-1)[dgrad])
    tc.assert_fp32_exact(Ay, dh, w5)
    dW, db, Aw, Ab = tc.wgrad_ref(dh, y2, True)
    tc.assert_fp32_exact(Aw, dh, y2)
    tc.assert_fp32_exact(Ab, dh)


# ------------------------------------------------------------------ mutants
# Each on the GPU test's own inputs of the case named, against the bound that test applies. The
# floors asserted are far below what is measured (README, Tests).
def _fc_case(kind, O=256, I=288):
    x, w5, b5, wc, bc = tc.fc_operands(kind, O, I)
    f, A = tc.fc_fwd_ref(x, w5, b5, True)
    return x, w5, b5, wc, bc, f, tc.bf16_bound(f, A, I + 1)


def test_mutants_of_the_forward_exceed_the_bound(capsys):
    x, w5, b5, wc, bc, f, bound = _fc_case("round")
    wq = w5.double()
    norelu = tc.worst_ratio(tc.fc_fwd_ref(x, w5, b5, False)[0], f, bound)
    late_bias = tc.worst_ratio((x.double().clamp_min(0) @ wq.t()).clamp_min(0) + b5.double(), f,
                               bound)
    xk = x.clone()
    xk[:, 32:64] = 0
    kblock = tc.worst_ratio(tc.fc_fwd_ref(xk, w5, b5, True)[0], f, bound)
    _report(capsys, f"mutation factors, forward: dropped input relu {norelu:.0f}, bias after the "
                    f"relu {late_bias:.0f}, one K block of 32 dropped {kblock:.0f}")
    assert norelu > 50 and late_bias > 5 and kblock > 50
    # the same K block in the GEMM (case 16: 513 x 264 x 288, bias, relu, mask)
    M, N, K, *_ = tc.GEMM_CASES[16]
    a, b, bv, mk, c0 = tc.gemm_operands("round", 16)
    y, A = tc.gemm_nt_ref(a, b, bv, True, mk)
    ak = a.clone()
    ak[:, K - 32:] = 0
    gk = tc.worst_ratio(tc.gemm_nt_ref(ak, b, bv, True, mk)[0], y,
                        tc.bf16_bound(y, A, tc.gemm_terms(K, True)))
    _report(capsys, f"mutation factor, GEMM: last K block dropped {gk:.0f}")
    assert gk > 50


def test_mutant_truncating_store_stays_between_one_and_two_bounds(capsys):
    """Truncation errs by up to one bf16 ulp, 2^-7 |ref| at the bottom of a binade, against the
    store term's 2^-8 |ref|: above the bound, and never twice it."""
    x, w5, b5, wc, bc, f, bound = _fc_case("round")
    assert tc.worst_ratio(f.bfloat16().double(), f, bound) < 1.0  # round to nearest passes
    t = tc.worst_ratio(tc.round_trunc_bf16(f), f, bound)
    frac = float(((tc.round_trunc_bf16(f) - f).abs() > bound).double().mean())
    _report(capsys, f"mutation factor: truncating store {t:.2f} ({100 * frac:.0f} % of elements)")
    assert 1.5 < t < 2.0 and frac > 0.05


def test_mutants_of_the_weight_gradient_exceed_the_bound(capsys):
    O, I, N = 256, 128, 300
    g, x, out0 = tc.wgrad_operands("round", O, I, N)
    dW, db, Aw, Ab = tc.wgrad_ref(g, x, True)
    bw, bb = tc.f32_bound(Aw, N), tc.f32_bound(Ab, N)
    last = N - N % 16  # rows 288..299: the last, partial 16-row block
    drop = tc.worst_ratio(tc.wgrad_ref(g[:last], x[:last], True)[0], dW, bw)
    drop_b = tc.worst_ratio(tc.wgrad_ref(g[:last], x[:last], True)[1], db, bb)
    # two parts: rows 0..255 | 256..299; part 0 runs on into its neighbour's stage
    nb = tc.wgrad_ref(g[256:], x[256:], True)
    neigh = tc.worst_ratio(dW + nb[0], dW, bw)
    neigh_b = tc.worst_ratio(db + nb[1], db, bb)
    norelu = tc.worst_ratio(tc.wgrad_ref(g, x, False)[0], dW, bw)
    db_x = x.double().clamp_min(0).sum(0)[torch.arange(O) % I]  # the ones-MFMA on the x fragment
    from_x = tc.worst_ratio(db_x, db, bb)
    _report(capsys, f"mutation factors, weight gradient: last partial 16-row block dropped "
                    f"{drop:.0f} (db {drop_b:.0f}), a neighbour's rows included {neigh:.0f} (db "
                    f"{neigh_b:.0f}), dropped relu {norelu:.0f}, db from x {from_x:.0f}")
    assert min(drop, drop_b, neigh, neigh_b, norelu, from_x) > 1000
    # the column sums lose their last rows the same way
    xs = tc.colsum_operands("round", "vec78_80")[:1025]
    s, As = tc.colsum_ref(xs, 78)
    cdrop = tc.worst_ratio(tc.colsum_ref(xs[:1024], 78)[0], s, tc.f32_bound(As, 1025))
    _report(capsys, f"mutation factor, column sums: last row dropped {cdrop:.0f}")
    assert cdrop > 5  # one row of 1025 against a bound that grows with R^2


def test_mutant_gadd_past_its_rows_exceeds_the_bound(capsys):
    K, R = 96, 1025
    dv, h, w2, gadd = tc.value_operands("round", K, R)
    dh, Ah, *_ = tc.value_bwd_ref(dv, h, w2, gadd, R - 5)
    f = tc.worst_ratio(tc.value_bwd_ref(dv, h, w2, gadd, R)[0], dh, tc.bf16_bound(dh, Ah, 2))
    _report(capsys, f"mutation factor: gadd added at rows >= gadd_rows {f:.0f}")
    assert f > 50


def _transposed_maps(k1, c, hh, ww):
    """nhwc_linear_maps with the spatial index walked column-major (p = x hh + y): the maps of a
    kernel that took the [n, ho, wo, c] activations for [n, wo, ho, c]."""
    fwd, dgrad, grad = nhwc_linear_maps(k1, c, hh, ww)
    perm = torch.arange(hh * ww).view(hh, ww).t().reshape(-1)        # p' -> p
    fwd_t = fwd.view(k1, hh * ww, c)[:, perm].reshape(k1, -1)
    inv = torch.argsort(perm)
    kf = torch.arange(k1).view(-1, 1, 1) * (c * hh * ww)  # dst (k, c', p) <- k f + p' c + c'
    grad_t = kf + inv.view(1, 1, -1) * c + torch.arange(c).view(1, -1, 1)
    return fwd_t.contiguous(), fwd_t.t().contiguous(), grad_t.reshape(-1).int()


@pytest.mark.parametrize("c,ho,wo", tc.MAP_SHAPES)
def test_mutant_swapped_ho_wo_is_seen_where_it_can_be(capsys, c, ho, wo):
    """NCHW and NHWC both flatten the map row-major, so the three maps depend on ho wo only:
    built for a wo x ho map they are the same maps at every shape (asserted), and passing the two
    sizes the wrong way round cannot be wrong. What can be wrong is the walk: the spatial index
    taken column-major. A map with a single row or column has one walk only, so 1x1, 1x2 and 2x1
    cannot see it either (asserted equal); 2x2 and 3x3 do, far above the bound."""
    k1, n = 256, 47
    t = tc.TailCase("round", 300 + 10 * ho + wo)
    y, w5, b5 = t.gated((n, ho * wo * c)), t.mat(k1, c * ho * wo), t.vec(k1)
    maps = nhwc_linear_maps(k1, c, ho, wo)
    assert all(torch.equal(a, b) for a, b in zip(maps, nhwc_linear_maps(k1, c, wo, ho)))
    mt = _transposed_maps(k1, c, ho, wo)
    f, A = tc.fc_fwd_ref(y, w5.reshape(-1)[maps[0].long()], b5, True)
    r = tc.worst_ratio(tc.fc_fwd_ref(y, w5.reshape(-1)[mt[0].long()], b5, True)[0], f,
                       tc.bf16_bound(f, A, c * ho * wo + 1))
    _report(capsys, f"mutation factor: the map walked column-major, {ho}x{wo}: {r:.0f}")
    if min(ho, wo) == 1:
        assert all(torch.equal(a, b) for a, b in zip(maps, mt)) and r == 0.0
    else:
        assert r > 50
        dW = t.f32((k1, ho * wo * c))  # the gradient map scatters to other slots too
        assert not torch.equal(tc.map_gather_ref(dW, maps[2]), tc.map_gather_ref(dW, mt[2]))
        # (and the transposed maps are consistent among themselves: a transposed weight)
        assert torch.equal(tc.map_gather_ref(w5.reshape(-1)[mt[0].long()], mt[2]), w5.reshape(-1))


def test_mutant_mask_ge_breaks_exact_zeros(capsys):
    """Exact case: mask >= 0 lets the +0 and -0 entries through; both must stay exactly zero."""
    idx = 16
    M, N, K, *_ = tc.GEMM_CASES[idx]
    a, b, bv, mk, c0 = tc.gemm_operands("exact", idx)
    y, A = tc.gemm_nt_ref(a, b, bv, True, mk)
    ge = (a.double() @ b.double().t() + bv.double()).clamp_min(0) * (mk.double() >= 0)
    bits = mk.contiguous().view(torch.int16)
    wrong_p = int(((ge != y) & (bits == 0)).sum())
    wrong_n = int(((ge != y) & (bits == -32768)).sum())
    _report(capsys, f"mutation: mask >= 0 makes {wrong_p} entries at +0 and {wrong_n} at -0.0 "
                    f"non-zero (of {M * N})")
    assert wrong_p > 1000 and wrong_n > 1000
    assert tc.worst_ratio(ge, y, tc.bf16_bound(y, A, tc.gemm_terms(K, True))) == float("inf")
    # the sign-bit test of the packed relu (-0.0 has it set) and the value test agree: what a
    # "bits != 0" test would let through is caught the same way on the forward's input
    x, w5, b5, wc, bc, f, bound = _fc_case("exact", 256, 128)
    xb = x.contiguous().view(torch.int16)
    assert torch.equal(torch.where(xb < 0, torch.zeros_like(x), x).double(),
                       x.double().clamp_min(0))


def test_mutant_critic_on_the_unrounded_f_breaks_the_exact_value(capsys):
    x, w5, b5, wc, bc, f, bound = _fc_case("exact", 256, 288)
    v, Av = tc.critic_ref(f.bfloat16(), wc, bc)
    vu = tc.critic_ref(f, wc, bc)[0]
    wrong = int((vu.float() != v.float()).sum())
    _report(capsys, f"mutation: the critic on the unrounded f changes {wrong} of {v.numel()} "
                    f"exact values")
    assert wrong > v.numel() // 2
    # and on the rounding case it leaves the bound
    x, w5, b5, wc, bc, f, bound = _fc_case("round", 256, 288)
    v, Av = tc.critic_ref(f.bfloat16(), wc, bc)
    r = tc.worst_ratio(tc.critic_ref(f, wc, bc)[0], v, tc.f32_bound(Av, 257))
    _report(capsys, f"mutation factor: the critic on the unrounded f, rounding case {r:.0f}")
    assert r > 5
