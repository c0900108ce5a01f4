"""Every per-layer launcher of the conv trunk (conv.hip: forward / data gradient, weight
gradient, pool backward) against the fp64 oracles of tests/conv_cases.py, at every distinct
layer shape the supported maps produce and at the smallest batches that can still go wrong:
one image, one more than a workgroup's group (a partial last group) and, under a grid cap of 2,
four groups and one image (every workgroup walks several groups, the last one partial).

Every case runs twice. Exact case: torch.equal against the oracle rounded once to the output
type, no tolerance. Rounding case: the derived element-wise bounds of conv_cases; the worst
error / bound ratio of each family is printed (pytest -s) and must stay below 1.

Every output the launchers write lies inside a larger buffer filled with 0xFF bytes (a NaN in
bf16 and fp32, no window byte): afterwards no such value is left inside an output and the bytes
around it are unchanged.

The fused forward kernels that return their intermediates (resblock.hip, stage2.hip) run on the
exact case at the end of the file; the fused backward kernels keep du / dc in LDS and stay
anchored through tests/test_gpu_conv.py's fused-vs-per-layer tests (README, Tests)."""
import dataclasses

import pytest
import torch

import conv_cases as cc
from guarded import GuardedTorch as _GuardedTorch, filled

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue


@pytest.fixture
def gt(monkeypatch):
    from microbeast_amd.ops import encoder
    g = _GuardedTorch()
    monkeypatch.setattr(encoder, "torch", g)
    return g


_ENC = {}


def _encoder(cuda, name, kind):
    """(HipEncoder with packed weights, fp32 weights, fp32 biases on the CPU), one per kind."""
    from microbeast_amd.ops.encoder import HipEncoder
    if (name, kind) not in _ENC:
        h, w, ch = {**cc.ENCODERS, **cc.NONSQUARE}[name]
        enc = HipEncoder(h, w, 27, ch, cuda)
        c = cc.Case(kind, 31)
        ws = [c.weights(L.cout, L.cin_real) for L in enc.layers]
        bs = [c.bias(L.cout) for L in enc.layers]
        enc.pack([t.to(cuda).contiguous() for t in ws], with_bwd=True)
        # _wgrad reduces its partial rows at once (no backward pass is deferring them)
        enc.defer_reduce = False
        assert enc._rjobs is None
        _ENC[name, kind] = (enc, ws, bs)
    enc, ws, bs = _ENC[name, kind]
    enc._pbufs = {}  # the partial-row workspace is allocated again, inside this test's guards
    return enc, ws, bs


def _kernels():
    from microbeast_amd import _native as N
    return N.kernels()


def _batches(g):
    """(images, grid cap): one, a partial last group, several groups per workgroup."""
    return [(1, 0), (g + 1, 0), (4 * g + 1, 2)]


class _Ratios:
    """Worst error / bound per family of the rounding case (reported, never an input)."""

    def __init__(self, tag):
        self.tag, self.r = tag, {}

    def add(self, family, got, ref, bound):
        r = cc.worst_ratio(got, ref, bound)
        self.r[family] = max(self.r.get(family, 0.0), r)
        assert r < 1.0, (self.tag, family, r)

    def report(self):
        for f, r in self.r.items():
            print(f"ratio {self.tag} {f} {r:.3f}")


def _cmp_bf16(rt, family, exact, got, ref, A, n):
    got = got.cpu()
    if exact:
        cc.assert_bf16_exact(ref)
        assert torch.equal(got, ref.bfloat16()), (rt.tag, family)
    else:
        rt.add(family, got, ref, cc.bf16_bound(ref, A, n))


def _cmp_pooled(rt, exact, p, y_full, pidx, ref, A, n):
    """Pre-pool values against the oracle, then the pool. In both cases the pooled values and
    the window bytes must be exactly the first-maximum pool of the kernel's OWN bf16 pre-pool
    values, which pins every byte, ties included. Against the fp64 oracle the bytes are compared
    where the window maximum of the oracle rounded to bf16 is unique; a difference there is
    accepted only where one of the window's pre-pool values is not the rounded oracle's (a value
    the fp32 sum put across a bf16 rounding boundary, inside the bound, can move the maximum),
    and then the first check has already pinned the byte. The count of such windows is printed;
    none of 423 359 was moved when this was written."""
    p, y_full, pidx = p.cpu(), y_full.cpu(), pidx.cpu()
    _cmp_bf16(rt, "fwd pre-pool", exact, y_full, ref, A, n)
    vk, ik = cc.pool_ref(y_full)
    assert torch.equal(p.double(), vk) and torch.equal(pidx, ik), (rt.tag, "pool of own values")
    rb = ref.bfloat16()
    vr, ir = cc.pool_ref(rb)
    if exact:
        assert torch.equal(p, vr.bfloat16()) and torch.equal(pidx, ir), (rt.tag, "pool")
        return
    rt.add("fwd pooled", p, cc.pool_ref(ref)[0], cc.pool_ref(cc.bf16_bound(ref, A, n))[0])
    Ho, Wo = vr.shape[1:3]
    ninf = float("-inf")
    rp = torch.nn.functional.pad(rb.double(), (0, 0, 1, 1, 1, 1), value=ninf)
    same = torch.nn.functional.pad((y_full == rb).double(), (0, 0, 1, 1, 1, 1), value=1.0)
    count = torch.zeros_like(vr)
    clean = torch.ones_like(vr)
    for t in range(9):
        ky, kx = t // 3, t % 3
        count += rp[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] == vr
        clean *= same[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2]
    differ = (count == 1) & (pidx != ir)
    assert not bool((differ & (clean == 1)).any()), (rt.tag, "argmax byte")
    print(f"argmax {rt.tag}: {int((count == 1).sum())} unique windows, {int(differ.sum())} moved "
          f"by a pre-pool value across a rounding boundary")


def _run_forward(cuda, gt, rt, enc, L, w, b, case, row_modes):
    k = _kernels()
    n_terms = 9 * L.cin + 2
    # (the pooled launch stages its pre-pool values too, so its groups may be smaller)
    gs = sorted({k.mbk_conv_fwd_imgs(int(L.bits), L.cin, L.cout, L.H, L.W, pool, 0)
                 for pool in {0, int(L.pool)}})
    assert gs[0] >= 1
    batches = sorted({b for g in gs for b in _batches(g)})
    nmax = batches[-1][0]
    if L.bits:
        xin = case.obs(nmax, L.H, L.W)
        x64 = cc.planes_nhwc(xin, L.H, L.W)
    else:
        xin = case.acts((nmax, L.H, L.W, L.cin))
        x64 = xin.double()
    add = case.acts((nmax, L.H, L.W, L.cout))
    plain = dataclasses.replace(L, relu_in=False, pool=False)
    variants = [("fwd plain", plain, None)]
    if not L.pool:
        variants.append(("fwd relu+add", dataclasses.replace(L, relu_in=True), add))
    refs = {name: cc.conv_fwd_ref(x64, w, b, Lv.relu_in, a) for name, Lv, a in variants}
    if L.pool:
        refs["pool"] = cc.conv_fwd_ref(x64, w, b, L.relu_in, None)
    if case.exact:
        for y, A in refs.values():
            cc.assert_fp32_exact(A, x64, w, plus=(b, add))
            cc.assert_bf16_exact(y)
    xg, bg, addg = xin.to(cuda), b.to(cuda), add.to(cuda)
    Ho, Wo = (L.H + 1) // 2, (L.W + 1) // 2
    for row in row_modes:
        for n, cap in batches:
            k.mbk_conv0_row_set(row)
            k.mbk_conv_set_grid_cap(cap)
            try:
                outs = [(name, enc._fwd(Lv, xg[:n], bg, add=None if a is None else addg[:n]))
                        for name, Lv, a in variants]
                if L.pool:
                    yf = gt.empty(n, L.H, L.W, L.cout, dtype=torch.bfloat16, device=cuda)
                    pi = gt.empty(n, Ho, Wo, L.cout, dtype=torch.uint8, device=cuda)
                    p = enc._fwd(L, xg[:n], bg, y_full=yf, pool_idx=pi)
            finally:
                k.mbk_conv_set_grid_cap(0)
                k.mbk_conv0_row_set(1)
            gt.check()
            for name, y in outs:
                _cmp_bf16(rt, name, case.exact, y, refs[name][0][:n], refs[name][1][:n], n_terms)
            if L.pool:
                _cmp_pooled(rt, case.exact, p, yf, pi, refs["pool"][0][:n], refs["pool"][1][:n],
                            n_terms)


def _run_dgrad(cuda, gt, rt, enc, L, w, case):
    k = _kernels()
    g = k.mbk_conv_fwd_imgs(0, L.cout, L.cin, L.H, L.W, 0, 0)
    assert g >= 1
    nmax = 4 * g + 1
    dy = case.acts((nmax, L.H, L.W, L.cout))
    mask, add = (case.acts((nmax, L.H, L.W, L.cin)) for _ in range(2))
    refs = {"dgrad mask": cc.conv_dgrad_ref(dy, w, mask, None),
            "dgrad mask+add": cc.conv_dgrad_ref(dy, w, mask, add)}
    if case.exact:
        for y, A in refs.values():
            cc.assert_fp32_exact(A, dy, w, plus=(add,))
            cc.assert_bf16_exact(y)
    dyg, mg, ag = dy.to(cuda), mask.to(cuda), add.to(cuda)
    for n, cap in _batches(g):
        k.mbk_conv_set_grid_cap(cap)
        try:
            d0 = enc._fwd(L, dyg[:n], None, mask_src=mg[:n], dgrad=True)
            d1 = enc._fwd(L, dyg[:n], None, mask_src=mg[:n], add=ag[:n], dgrad=True)
        finally:
            k.mbk_conv_set_grid_cap(0)
        gt.check()
        for name, d in (("dgrad mask", d0), ("dgrad mask+add", d1)):
            _cmp_bf16(rt, name, case.exact, d, refs[name][0][:n], refs[name][1][:n], 9 * L.cout + 2)


def _cmp_wgrad(rt, family, exact, dw, db, ref, extra_w=None):
    dW, dB, Aw, Ab, terms = ref
    dw, db = dw.cpu(), db.cpu()
    filled(dw)
    filled(db)
    if exact:
        assert torch.equal(dw.double(), dW) and torch.equal(db.double(), dB), (rt.tag, family)
    else:
        bw = cc.f32_bound(Aw, terms)
        rt.add(family + " dW", dw, dW, bw if extra_w is None else bw + extra_w)
        rt.add(family + " db", db, dB, cc.f32_bound(Ab, terms))


def _run_wgrad(cuda, gt, rt, enc, L, case):
    k = _kernels()
    g = k.mbk_conv_wgrad_imgs(int(L.bits), L.cin, L.cout, L.H, L.W, 0)
    assert g >= 1
    nmax = 4 * g + 1
    if L.bits:
        xin = case.obs(nmax, L.H, L.W)
        x64 = cc.planes_nhwc(xin, L.H, L.W)
    else:
        xin = case.acts((nmax, L.H, L.W, L.cin))
        x64 = xin.double()
    dy = case.acts((nmax, L.H, L.W, L.cout))
    xg, dyg = xin.to(cuda), dy.to(cuda)
    for n, cap in _batches(g):
        dW, dB, Aw, Ab = cc.conv_wgrad_ref(x64[:n], dy[:n], L.relu_in)
        if case.exact:
            cc.assert_fp32_exact(Aw, x64, dy)
        dw = gt.empty(L.cout, L.cin_real, 3, 3, dtype=torch.float32, device=cuda)
        db = gt.empty(L.cout, dtype=torch.float32, device=cuda)
        k.mbk_conv_set_grid_cap(cap)
        try:
            enc._wgrad(L, xg[:n], dyg[:n], dw, db)
        finally:
            k.mbk_conv_set_grid_cap(0)
        gt.check()
        _cmp_wgrad(rt, "wgrad", case.exact, dw, db, (dW, dB, Aw, Ab, n * L.H * L.W))


def _run_layer(cuda, gt, name, li, kind):
    enc, ws, bs = _encoder(cuda, name, kind)
    L = enc.layers[li]
    rt = _Ratios(f"{name}[{li}] {L.cin}->{L.cout} {L.H}x{L.W}{' pool' if L.pool else ''}")
    case = cc.Case(kind, 1000 + 17 * li + L.H)
    # bit-plane layers: the row kernels (16-wide and 17..32-wide maps) and the generic kernel
    _run_forward(cuda, gt, rt, enc, L, ws[li], bs[li], case, (1, 0) if L.bits else (1,))
    if not L.bits:
        _run_dgrad(cuda, gt, rt, enc, L, ws[li], case)
    _run_wgrad(cuda, gt, rt, enc, L, case)
    rt.report()


@pytest.mark.parametrize("kind", ["exact", "round"])
@pytest.mark.parametrize("name,li", cc.distinct_layers(cc.ENCODERS))
def test_layer_against_oracle(cuda, gt, name, li, kind):
    """Forward (plain; relu + residual; pooled with the pre-pool values and argmax bytes; the
    bit-plane layers on the row kernels and on the generic one), data gradient (relu mask, with
    and without the residual gradient) and weight gradient of one layer shape."""
    _run_layer(cuda, gt, name, li, kind)


def _pool_shapes(encoders):
    seen = []
    for name, li in cc.distinct_layers(encoders):
        h, w, ch = encoders[name]
        _, _, cout, H, W, _, _, pool = cc.trunk_layers(h, w, ch)[li]
        if pool and (H, W, cout) not in seen:
            seen.append((H, W, cout))
    return seen


def _run_pool_bwd(cuda, gt, H, W, C, kind):
    from microbeast_amd import _native as N
    k = _kernels()
    rt = _Ratios(f"pool_bwd {H}x{W}x{C}")
    case = cc.Case(kind, 50 + H * W + C)
    for n in (1, 5):
        c = case.acts((n, H, W, C))
        _, idx = cc.pool_ref(c)
        dp = case.acts(idx.shape)
        ref, A, _ = cc.pool_bwd_ref(dp, idx, H, W)
        cg, ig, dg = c.to(cuda), idx.to(cuda), dp.to(cuda)
        d_idx = gt.empty(n, H, W, C, dtype=torch.bfloat16, device=cuda)
        d_val = gt.empty(n, H, W, C, dtype=torch.bfloat16, device=cuda)
        N.check(k.mbk_pool_bwd_idx(ig.data_ptr(), dg.data_ptr(), n, H, W, C, d_idx.data_ptr(),
                                   N.stream_ptr()), "pool_bwd_idx")
        N.check(k.mbk_pool_bwd(cg.data_ptr(), dg.data_ptr(), n, H, W, C, d_val.data_ptr(),
                               N.stream_ptr()), "pool_bwd")
        gt.check()
        # at most 4 windows feed a cell: 4 summed terms
        _cmp_bf16(rt, "pool_bwd_idx", case.exact, d_idx, ref, A, 4)
        _cmp_bf16(rt, "pool_bwd", case.exact, d_val, ref, A, 4)
    rt.report()


@pytest.mark.parametrize("kind", ["exact", "round"])
@pytest.mark.parametrize("H,W,C", _pool_shapes(cc.ENCODERS))
def test_pool_backward_against_oracle(cuda, gt, H, W, C, kind):
    """mbk_pool_bwd_idx (stored argmax bytes) and mbk_pool_bwd (argmax recomputed from the
    pre-pool values, first maximum) against the scatter-add; the exact case ties constantly."""
    _run_pool_bwd(cuda, gt, H, W, C, kind)


@pytest.mark.parametrize("kind", ["exact", "round"])
@pytest.mark.parametrize("form", ["dense1", "dense2", "sparse"])
def test_stage0_pool_fused_wgrad_against_oracle(cuda, gt, form, kind):
    """The stage-0 weight gradient of a 16x16 map with the pool backward inside: the dense
    pool-fused kernel at 1 and 2 images per round and the sparse kernel, each against
    dW = wgrad(X, pool_bwd(dp, pidx)).

    Rounding case. Both kernels build dY in a bf16 tile by adding one window's dp at a time
    (fp32 add, bf16 store), so a cell that k windows chose carries up to k - 1 roundings of a
    partial sum: |dY - ref| <= (k - 1) 2^-8 (1 + 2^-8)^2 sum |dp|, which enters dW through the
    planes as wgrad(X, that). The sparse kernel sums E S_t + D dY (conv.hip) instead of X dY, so
    its magnitude is A(E, |dY|) + A(|X - E|, |dY|)."""
    from microbeast_amd.ops.encoder import EMPTY_WORD
    k = _kernels()
    enc, ws, bs = _encoder(cuda, "s16", kind)
    L = enc.layers[0]
    rt = _Ratios(f"stage-0 pool-fused wgrad {form}")
    case = cc.Case(kind, 900 + len(form))
    per = {"dense1": 1, "dense2": 2, "sparse": 3}[form]  # images per round / waves per workgroup
    nmax = 4 * per + 1
    obs = case.obs(nmax, 16, 16)
    x64 = cc.planes_nhwc(obs, 16, 16)
    _, pidx = cc.pool_ref(case.acts((nmax, 16, 16, 16)))
    dp = case.acts(pidx.shape)
    og, pg, dg = obs.to(cuda), pidx.to(cuda), dp.to(cuda)
    e64 = cc.planes_nhwc(torch.full((1, 256), EMPTY_WORD, dtype=torch.int32), 16, 16)
    saved = enc.wgrad0_imgs
    try:
        for n, cap in _batches(per):
            dY, AdY, hits = cc.pool_bwd_ref(dp[:n], pidx[:n], 16, 16)
            dW, dB, Aw, Ab = cc.conv_wgrad_ref(x64[:n], dY)
            if case.exact:
                cc.assert_bf16_exact(dY)
                cc.assert_fp32_exact(Aw, x64, dY)
            eY = (hits - 1).clamp_min(0) * cc.U_BF16 * (1 + cc.U_BF16) ** 2 * AdY
            extra = cc.conv_wgrad_ref(x64[:n], eY)
            if form == "sparse":
                Aw = (cc.conv_wgrad_ref(e64.expand(n, -1, -1, -1), dY.abs())[2]
                      + cc.conv_wgrad_ref((x64[:n] - e64).abs(), dY.abs())[2])
            dw = gt.empty(16, 27, 3, 3, dtype=torch.float32, device=cuda)
            db = gt.empty(16, dtype=torch.float32, device=cuda)
            k.mbk_conv_set_grid_cap(cap)
            try:
                if form == "sparse":
                    enc._wgrad0_sparse(L, og[:n], dg[:n], pg[:n], dw, db)
                else:
                    enc.wgrad0_imgs = per
                    enc._wgrad(L, og[:n], None, dw, db, dp=dg[:n], pidx=pg[:n])
            finally:
                k.mbk_conv_set_grid_cap(0)
            gt.check()
            terms = n * 256
            dw, db = dw.cpu(), db.cpu()
            filled(dw)
            filled(db)
            if case.exact:
                assert torch.equal(dw.double(), dW) and torch.equal(db.double(), dB), (form, n)
            else:
                rt.add("dW", dw, dW, cc.f32_bound(Aw, terms) + extra[0])
                rt.add("db", db, dB, cc.f32_bound(Ab, terms) + extra[1])
    finally:
        enc.wgrad0_imgs = saved
    rt.report()


# ------------------------------------------------------------------ fused forward kernels
def _exact_layer(x, w, b, relu, add=None):
    """One layer of the exact case on the kernel's own bf16 input: the bf16 the kernel must
    store (the fp32 sum is exact, so it is the oracle rounded once)."""
    y, A = cc.conv_fwd_ref(x, w, b, relu, add)
    cc.assert_fp32_exact(A, x, w, plus=(b,) if add is None else (b, add))
    return y.bfloat16()


@pytest.mark.parametrize("name", ["s8", "s10", "s16", "s24"])
def test_fused_forward_kernels_exact(cuda, gt, name):
    """res_fwd16 (with the next stage's conv + pool where the launcher takes the shape),
    res_blk32 in its round and wave forms and pool_conv_fwd4, on the exact case, at one image
    and at a batch with a partial last group. Every stored intermediate must equal the oracle of
    its layer applied to the kernel's own stored input, bit for bit."""
    k = _kernels()
    enc, ws, bs = _encoder(cuda, name, "exact")
    bg = [b.to(cuda) for b in bs]
    case = cc.Case("exact", 400 + enc.layers[0].H)
    L1, L6, L10 = enc.layers[1], enc.layers[6], enc.layers[10]
    stage = bool(k.mbk_res_fwd16_stage_ok(enc.layers[5].H, enc.layers[5].W))
    for n in (1, 5):
        p = case.acts((n, L1.H, L1.W, 16))
        outs = enc._res_fwd16(0, p.to(cuda), bg, stage=True if stage else None)
        gt.check()
        u0, y0, u1, y1 = (t.cpu() for t in outs[:4])
        assert torch.equal(u0, _exact_layer(p, ws[1], bs[1], True))
        assert torch.equal(y0, _exact_layer(u0, ws[2], bs[2], True, p))
        assert torch.equal(u1, _exact_layer(y0, ws[3], bs[3], True))
        assert torch.equal(y1, _exact_layer(u1, ws[4], bs[4], True, y0))
        if stage:
            pn, pi = (t.cpu() for t in outs[4])
            v, i = cc.pool_ref(_exact_layer(y1, ws[5], bs[5], False))
            assert torch.equal(pn, v.bfloat16()) and torch.equal(pi, i)
    g32 = k.mbk_res_blk32_fwd_imgs(L6.H, L6.W)
    saved = enc.fused_res_blk32_wave
    try:
        for wave in ((True, False) if L6.H in (2, 4) else (False,)):
            enc.fused_res_blk32_wave = wave
            for n in (1, (21 if wave else g32 + 1)):
                x = case.acts((n, L6.H, L6.W, 32))
                u, y = (t.cpu() for t in enc._res_blk32(6, x.to(cuda), bg))
                gt.check()
                assert torch.equal(u, _exact_layer(x, ws[6], bs[6], True)), (wave, n)
                assert torch.equal(y, _exact_layer(u, ws[7], bs[7], True, x)), (wave, n)
    finally:
        enc.fused_res_blk32_wave = saved
    if (L10.H, L10.W) == (4, 4):
        for n in (1, 9):
            x = case.acts((n, 4, 4, 32))
            pi = gt.empty(n, 2, 2, 32, dtype=torch.uint8, device=cuda)
            y = enc._pool_conv_fwd4(L10, x.to(cuda), bg[10], pi)
            gt.check()
            v, i = cc.pool_ref(_exact_layer(x, ws[10], bs[10], False))
            assert torch.equal(y.cpu(), v.bfloat16()) and torch.equal(pi.cpu(), i)


# ------------------------------------------------------------------ non-square maps
class TestNonSquare:
    """H != W (8x16, 16x8, 10x16 and the maps their stages produce). Read first, conv.hip: the
    forward / data-gradient kernel, pool_tile, both pool backward kernels and the plain and band
    weight-gradient layouts index rows by W and images by H * W throughout; the 16-wide row
    kernel takes the height at run time. The pool-fused stage-0 weight gradient walks 8 x 8
    windows per image whatever H is, so its launcher refuses every map but 16x16."""

    @pytest.mark.parametrize("kind", ["exact", "round"])
    @pytest.mark.parametrize("name,li", cc.distinct_layers(cc.NONSQUARE))
    def test_layer_against_oracle(self, cuda, gt, name, li, kind):
        _run_layer(cuda, gt, name, li, kind)

    @pytest.mark.parametrize("kind", ["exact", "round"])
    @pytest.mark.parametrize("H,W,C", _pool_shapes(cc.NONSQUARE))
    def test_pool_backward_against_oracle(self, cuda, gt, H, W, C, kind):
        _run_pool_bwd(cuda, gt, H, W, C, kind)

    @pytest.mark.parametrize("H,W", [(8, 16), (10, 16), (16, 8), (20, 16)])
    def test_pool_fused_wgrad_refuses_all_but_16x16(self, cuda, H, W):
        k = _kernels()
        assert k.mbk_conv_wgrad_parts(1, 32, 16, 3, 16, 16, 1) > 0
        assert k.mbk_conv_wgrad_parts(1, 32, 16, 3, H, W, 1) == -INVALID
        from microbeast_amd import _native as N
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        obs = torch.zeros(3, H * W, dtype=torch.int32, device=cuda)
        dp = torch.zeros(3, Ho, Wo, 16, dtype=torch.bfloat16, device=cuda)
        pidx = torch.full((3, Ho, Wo, 16), 4, dtype=torch.uint8, device=cuda)
        part = torch.zeros(1 << 16, dtype=torch.float32, device=cuda)
        assert k.mbk_conv_wgrad(obs.data_ptr(), 1, 32, 16, None, dp.data_ptr(), pidx.data_ptr(),
                                part.data_ptr(), 1, 3, H, W, 1, 0, N.stream_ptr()) == INVALID
        torch.cuda.synchronize()
        assert float(part.abs().sum()) == 0

    def test_wave_block_refuses_non_square(self, cuda):
        """res_blk32's wave form is for 4x4 / 2x2 maps: 2x4 is refused, nothing is launched."""
        import ctypes
        from microbeast_amd import _native as N
        enc, ws, bs = _encoder(cuda, "8x16", "exact")
        x = torch.zeros(3, 2, 4, 32, dtype=torch.bfloat16, device=cuda)
        u, y = torch.full_like(x, 7.0), torch.full_like(x, 7.0)
        base = enc.packed_fwd.data_ptr()
        wp = (ctypes.c_void_p * 2)(*[base + 2 * enc.layers[6 + j].w_off for j in range(2)])
        bg = [bs[6 + j].to(cuda) for j in range(2)]
        bp = (ctypes.c_void_p * 2)(*[b.data_ptr() for b in bg])
        rc = _kernels().mbk_res_blk32_fwd_wave(
            x.data_ptr(), u.data_ptr(), y.data_ptr(), ctypes.cast(wp, ctypes.c_void_p),
            ctypes.cast(bp, ctypes.c_void_p), 3, 2, 4, N.stream_ptr())
        torch.cuda.synchronize()
        assert rc == INVALID and bool((u == 7).all()) and bool((y == 7).all())
