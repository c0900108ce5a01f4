"""The trunk tail's launchers -- mbk_fc_fwd, mbk_gemm_nt / mbk_gemm_nt_mask, mbk_fc_wgrad /
mbk_fc_wgrad_ex / mbk_fc_wgrad_wide (fc.hip, gemm.hip), mbk_value_bwd, mbk_colsum and
mbk_map_gather (gridnet.hip) -- against the fp64 oracles of tests/tail_cases.py, at the smallest
shapes where each path can go wrong: every fc_fwd instance at F around 16 and 32 rows and at a
second trip of the persistent loop, the three GEMM tiles through each epilogue with partial
tiles on every axis, hand-passed part counts (part boundaries, empty parts, the two-level
reduce), row counts around the 1024-row parts of the column sums.

Every case runs twice. Exact case: torch.equal against the oracle rounded once to the output
type, no tolerance. Rounding case: the derived element-wise bounds of tail_cases; the worst
error / bound ratio of each family is printed (pytest -s) and must stay below 1.

Every output (and every scratch buffer) lies inside a larger buffer of 0xFF bytes (a NaN in bf16
and fp32): afterwards the bytes around it are unchanged, no output element holds the fill, and
the row gaps of an output with ldc > N still do. Input row gaps (lda, ldb > K) hold NaN."""
import ctypes

import pytest
import torch

import tail_cases as tc
from guarded import GuardedTorch, filled, untouched

pytestmark = pytest.mark.gpu

INVALID = 1  # hipErrorInvalidValue
KINDS = ["exact", "round"]
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture
def gt():
    return GuardedTorch()


def _k():
    from microbeast_amd import _native as N
    return N, N.kernels()


class _Ratios:
    """Worst error / bound per family of the rounding case (reported, never an input)."""

    def __init__(self, tag):
        self.tag, self.r = tag, {}

    def add(self, family, got, ref, bound):
        r = tc.worst_ratio(got.cpu(), ref, bound)
        self.r[family] = max(self.r.get(family, 0.0), r)
        assert r < 1.0, (self.tag, family, r)

    def report(self):
        for f, r in self.r.items():
            print(f"ratio {self.tag} | {f} | {r:.3f}")


def _cmp(rt, family, exact, got, ref, bound, note=None):
    """Exact: the oracle rounded once to got's type, bit for bit. Round: inside the bound."""
    got = got.cpu()
    filled(got)
    if exact:
        assert torch.equal(got, ref.to(got.dtype)), (rt.tag, family, note)
    else:
        rt.add(family, got, ref, bound)


def _padded(t, ld, cuda, gap=float("nan")):
    """t [R, C] inside a [R, ld] device buffer whose gap columns hold `gap`."""
    buf = torch.full((t.shape[0], ld), gap, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf.to(cuda)


# ------------------------------------------------------------------ mbk_fc_fwd
def _fc_launch(x, relu_in, w5, b5, wc, bc, F, I, O, f, v):
    N, k = _k()
    return k.mbk_fc_fwd(x.data_ptr(), relu_in, w5.data_ptr(), b5.data_ptr(), wc.data_ptr(),
                        bc.data_ptr(), F, I, O, f.data_ptr(), v.data_ptr(), N.stream_ptr())


def _run_fc(cuda, gt, kind, O, I, Fs):
    rt = _Ratios(f"fc_fwd O={O} I={I}")
    x, w5, b5, wc, bc = tc.fc_operands(kind, O, I, max(Fs))
    xg, wg, bg, wcg, bcg = (t.to(cuda) for t in (x, w5.bfloat16(), b5, wc, bc))
    for relu_in in (0, 1):
        ref, A = tc.fc_fwd_ref(x, w5, b5, relu_in)
        bound = tc.bf16_bound(ref, A, I + 1)
        if kind == "exact":
            tc.assert_fp32_exact(A, x, w5, plus=(b5,))
        for F in Fs:
            f = gt.empty(F, O, dtype=BF, device=cuda)
            v = gt.empty(F, dtype=F32, device=cuda)
            assert _fc_launch(xg, relu_in, wg, bg, wcg, bcg, F, I, O, f, v) == 0
            gt.check()
            _cmp(rt, "f", kind == "exact", f, ref[:F], bound[:F], (relu_in, F))
            # the critic on the kernel's own stored activations
            vr, Av = tc.critic_ref(f.cpu(), wc, bc)
            _cmp(rt, "v", kind == "exact", v, vr, tc.f32_bound(Av, O + 1), (relu_in, F))
    rt.report()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("O,I", tc.FC_RB + tc.FC_GENERIC)
def test_fc_fwd_small_row_counts(cuda, gt, O, I, kind):
    """All four fc_fwd_rb_kernel<256, NKS> instances, two of <128, .>, and the generic kernel at
    O = 128 / 256 / 512: F = 1 .. 47 (one row, partial and full 16-row blocks, a half-valid and
    a full 32-row group, a second group), relu_in 0 and 1."""
    _run_fc(cuda, gt, kind, O, I, tc.FC_F)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("O,I", tc.FC_LONG)
def test_fc_fwd_second_trip_of_the_persistent_loop(cuda, gt, O, I, kind):
    """F = 2 CUs 32 + 49: the launcher's grid is 2 CUs workgroups of 32-row groups, so the first
    two workgroups take a second group, the others none, and the last group is half valid."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _run_fc(cuda, gt, kind, O, I, [2 * cus * 32 + 49])


def test_fc_fwd_empty_and_refused(cuda, gt):
    x, w5, b5, wc, bc = (t.to(cuda) for t in tc.fc_operands("exact", 256, 64))
    w5 = w5.bfloat16()
    f = gt.empty(47, 256, dtype=BF, device=cuda, interior=False)
    v = gt.empty(47, dtype=F32, device=cuda)
    assert _fc_launch(x, 1, w5, b5, wc, bc, 0, 64, 256, f, v) == 0      # F = 0
    assert _fc_launch(x, 1, w5, b5, wc, bc, 47, 48, 256, f, v) == INVALID  # I % 32
    assert _fc_launch(x, 1, w5, b5, wc, bc, 47, 40, 256, f, v) == INVALID
    assert _fc_launch(x, 1, w5, b5, wc, bc, 47, 64, 64, f, v) == INVALID   # O = 64
    assert _fc_launch(x, 1, w5, b5, wc, bc, 47, 160, 64, f, v) == INVALID
    gt.check()
    assert untouched(f) and untouched(v)


# ------------------------------------------------------------------ mbk_gemm_nt(_mask)
def _gemm_launch(a, b, C, bias, M, N_, K, lda, ldb, ldc, relu, out_bf16, acc, mask_ptr, masked):
    N, k = _k()
    if masked:
        return k.mbk_gemm_nt_mask(a.data_ptr(), b.data_ptr(), C.data_ptr(), N.ptr(bias), M, N_, K,
                                  lda, ldb, ldc, relu, out_bf16, mask_ptr, N.stream_ptr())
    return k.mbk_gemm_nt(a.data_ptr(), b.data_ptr(), C.data_ptr(), N.ptr(bias), M, N_, K, lda,
                         ldb, ldc, relu, out_bf16, acc, N.stream_ptr())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("idx", range(len(tc.GEMM_CASES)))
def test_gemm_nt_tiles_and_epilogues(cuda, gt, idx, kind):
    """One row of tail_cases.GEMM_CASES: lda = K + 8 and ldb = K + 16 with NaN in the gaps, the
    output in a 0xFF buffer whose row gaps (ldc > N) must survive, the mask in the output's
    layout with positive values in its gaps, masked entries exactly zero (their bound is 0)."""
    M, N_, K, out, bias, relu, mask, dldc, moff = tc.GEMM_CASES[idx]
    rt = _Ratios(f"gemm {M}x{N_}x{K} {out}")
    a, b, bv, mk, c0 = tc.gemm_operands(kind, idx)
    lda, ldb, ldc = K + 8, K + 16, N_ + dldc
    ag, bg = _padded(a, lda, cuda), _padded(b, ldb, cuda)
    bias_g = None if bv is None else bv.to(cuda)
    C = gt.empty(M, ldc, dtype=BF if out == "bf16" else F32, device=cuda, interior=False)
    if out == "acc":
        C[:, :N_] = c0.to(cuda)
    mask_ptr, keep = None, None
    if mask:
        keep = torch.ones(M * ldc + 8, dtype=BF)
        keep[moff:moff + M * ldc].view(M, ldc)[:, :N_] = mk
        keep = keep.to(cuda)
        mask_ptr = keep.data_ptr() + 2 * moff
        assert (mask_ptr % 16 != 0) == bool(moff)
    vec = out == "bf16" and N_ % 8 == 0 and ldc % 8 == 0 and not moff
    assert C.data_ptr() % 16 == 0 and ag.data_ptr() % 16 == 0 and bg.data_ptr() % 16 == 0
    rc = _gemm_launch(ag, bg, C, bias_g, M, N_, K, lda, ldb, ldc, relu, int(out == "bf16"),
                      int(out == "acc"), mask_ptr, bool(mask))
    assert rc == 0
    gt.check()
    if dldc:
        assert untouched(C[:, N_:]), "row gap overwritten"
    ref, A = tc.gemm_nt_ref(a, b, bv, relu, mk, c0)
    n = tc.gemm_terms(K, bool(bias), out == "acc")
    if kind == "exact":
        tc.assert_fp32_exact(tc.gemm_nt_ref(a, b, bv, relu, None, c0)[1], a, b,
                             plus=tuple(t for t in (bv, c0) if t is not None))
    bound = tc.bf16_bound(ref, A, n) if out == "bf16" else tc.f32_bound(A, n)
    got = C[:, :N_].contiguous()
    fam = ("bf16 vectorised" if vec else "bf16 per element") if out == "bf16" else "fp32 " + out
    _cmp(rt, fam, kind == "exact", got, ref, bound)
    if mask:
        assert bool((got.cpu()[~(mk.double() > 0)] == 0).all()), "masked entry not zero"
    rt.report()


@pytest.mark.parametrize("masked", [False, True])
def test_gemm_nt_refusals(cuda, gt, masked):
    a = torch.ones(16, 64, dtype=BF, device=cuda)
    b = torch.ones(16, 64, dtype=BF, device=cuda)
    C = gt.empty(16, 16, dtype=BF, device=cuda, interior=False)
    mp = a.data_ptr() if masked else None
    for K, lda, ldb in ((12, 16, 16), (4, 8, 8), (16, 20, 16), (16, 16, 28), (0, 16, 16)):
        assert _gemm_launch(a, b, C, None, 16, 16, K, lda, ldb, 16, 0, 1, 0, mp, masked) == INVALID
    assert _gemm_launch(a, b, C, None, 0, 16, 16, 16, 16, 16, 0, 1, 0, mp, masked) == 0  # empty
    assert _gemm_launch(a, b, C, None, 16, 0, 16, 16, 16, 16, 0, 1, 0, mp, masked) == 0
    gt.check()
    assert untouched(C)


# ------------------------------------------------------------------ weight gradients
def _wgrad_scratch(gt, cuda, nparts, row):
    """NaN-prefilled (0xFF) scratch: nparts partial rows and the two-level reduce's split rows."""
    return gt.empty((nparts + (nparts + 31) // 32) * row, dtype=F32, device=cuda)


def _wgrad_launch(g, x, n, O, I, scratch, nparts, out, acc, relu, plain):
    N, k = _k()
    if plain:  # mbk_fc_wgrad: the entry point without relu_x
        assert not relu
        return k.mbk_fc_wgrad(g.data_ptr(), x.data_ptr(), n, O, I, scratch.data_ptr(), nparts,
                              out.data_ptr(), acc, N.stream_ptr())
    return k.mbk_fc_wgrad_ex(g.data_ptr(), x.data_ptr(), n, O, I, scratch.data_ptr(), nparts,
                             out.data_ptr(), acc, relu, N.stream_ptr())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("O,I", tc.WGRAD_OI)
def test_fc_wgrad_parts_by_hand(cuda, gt, O, I, kind):
    """mbk_fc_wgrad / mbk_fc_wgrad_ex: N from one row to 300 with nparts passed by hand (one,
    two across a part boundary, the stage count, more parts than stages whose empty parts must
    write exact zeros over the NaN scratch, 65 and 97 for the two-level reduce), accumulate and
    relu_x cycling through their four combinations under every part count; where nparts is the
    stage count a second call must be bit-identical. Then N = 8197 at 65 parts and 12 293 at 97,
    where the last part, alone in the reduce's last split, has rows (tail_cases.LONG_PARTS)."""
    rt = _Ratios(f"fc_wgrad O={O} I={I}")
    seen = set()
    for ni, n in enumerate(tc.WGRAD_N):
        g, x, out0 = tc.wgrad_operands(kind, O, I, n)
        gg, xg, o0g = g.to(cuda), x.to(cuda), out0.to(cuda)
        refs = {r: tc.wgrad_ref(g, x, r) for r in (0, 1)}
        for pi, nparts in enumerate(tc.wgrad_nparts(n)):
            acc, relu = (ni + pi) & 1, ((ni + pi) >> 1) & 1
            label = "one" if nparts == 1 else "empty" if nparts == tc.stages(n) + 2 else nparts
            seen.add((label, acc, relu))
            dW, _, Aw, _ = refs[relu]
            ref, A, terms = (dW + out0.double(), Aw + out0.double().abs(), n + 1) if acc else \
                (dW, Aw, n)
            if kind == "exact":
                tc.assert_fp32_exact(A, g, x, plus=(out0,))
            outs = []
            for rep in range(2 if nparts == tc.stages(n) else 1):
                out = gt.empty(O, I, dtype=F32, device=cuda)
                if acc:
                    out.copy_(o0g)
                scratch = _wgrad_scratch(gt, cuda, nparts, O * I)
                rc = _wgrad_launch(gg, xg, n, O, I, scratch, nparts, out, acc, relu,
                                   plain=not relu and pi % 2 == 0)
                assert rc == 0
                gt.check()
                outs.append(out)
            _cmp(rt, "dW", kind == "exact", outs[0], ref, tc.f32_bound(A, terms), (n, nparts))
            if len(outs) == 2:
                assert torch.equal(outs[0], outs[1]), (n, nparts)
    for label in ("one", "empty", 65, 97):  # each under every accumulate x relu_x
        assert len({s for s in seen if s[0] == label}) == 4, label
    # the two-level reduce with rows in its partial last split (tail_cases.LONG_PARTS)
    for (nparts, n), (acc, relu) in zip(tc.LONG_PARTS.items(), ((1, 1), (0, 0))):
        g, x, out0 = tc.wgrad_operands(kind, O, I, n)
        dW, _, Aw, _ = tc.wgrad_ref(g, x, relu)
        ref, A, terms = (dW + out0.double(), Aw + out0.double().abs(), n + 1) if acc else \
            (dW, Aw, n)
        if kind == "exact":
            tc.assert_fp32_exact(A, g, x, plus=(out0,))
        out = gt.empty(O, I, dtype=F32, device=cuda)
        if acc:
            out.copy_(out0.to(cuda))
        scratch = _wgrad_scratch(gt, cuda, nparts, O * I)
        assert _wgrad_launch(g.to(cuda), x.to(cuda), n, O, I, scratch, nparts, out, acc, relu,
                             plain=False) == 0
        gt.check()
        _cmp(rt, "dW", kind == "exact", out, ref, tc.f32_bound(A, terms), (n, nparts))
    rt.report()


def test_fc_wgrad_refusals(cuda, gt):
    g = torch.ones(64, 16, dtype=BF, device=cuda)
    x = torch.ones(64, 16, dtype=BF, device=cuda)
    out = gt.empty(16, 16, dtype=F32, device=cuda)
    scratch = gt.empty(4 * 256, dtype=F32, device=cuda)
    for n, O, I, nparts in ((64, 16, 12, 1), (64, 16, 4, 1), (0, 16, 16, 1), (64, 16, 16, 0)):
        for plain in (True, False):
            assert _wgrad_launch(g, x, n, O, I, scratch, nparts, out, 0, 0, plain) == INVALID
    gt.check()
    assert untouched(out) and untouched(scratch)


def _wide_launch(g, x, n, O, I, relu, scratch, nparts, dw, db):
    N, k = _k()
    return k.mbk_fc_wgrad_wide(g.data_ptr(), x.data_ptr(), n, O, I, relu, scratch.data_ptr(),
                               nparts, dw.data_ptr(), db.data_ptr(), N.stream_ptr())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("I", tc.WIDE_I)
def test_fc_wgrad_wide_parts_by_hand(cuda, gt, I, kind):
    """mbk_fc_wgrad_wide: dW and db each against its oracle at N = 1 .. 1300, nparts one, the
    stage count, three more (empty parts), 65 and 97, relu_x 0 and 1; at the stage count a second
    call bit-identical; on the exact case bit-equal to mbk_fc_wgrad_ex + mbk_colsum; then the
    two long cases of tail_cases.LONG_PARTS."""
    from microbeast_amd.ops.pixconv import colsum
    N, k = _k()
    O = 256
    rt = _Ratios(f"fc_wgrad_wide I={I}")
    for n in tc.WIDE_N:
        g, x, _ = tc.wgrad_operands(kind, O, I, n)
        gg, xg = g.to(cuda), x.to(cuda)
        assert k.mbk_fc_wgrad_wide_parts(n, O, I) >= 1
        for relu in (0, 1):
            dW, dB, Aw, Ab = tc.wgrad_ref(g, x, relu)
            if kind == "exact":
                tc.assert_fp32_exact(Aw, g, x)
                tc.assert_fp32_exact(Ab, g)
            first = None
            for nparts in tc.wide_nparts(n):
                outs = []
                for rep in range(2 if nparts == tc.stages(n) else 1):
                    dw = gt.empty(O, I, dtype=F32, device=cuda)
                    db = gt.empty(O, dtype=F32, device=cuda)
                    scratch = _wgrad_scratch(gt, cuda, nparts, O * I + O)
                    assert _wide_launch(gg, xg, n, O, I, relu, scratch, nparts, dw, db) == 0
                    gt.check()
                    outs.append((dw, db))
                dw, db = outs[0]
                _cmp(rt, "dW", kind == "exact", dw, dW, tc.f32_bound(Aw, n), (n, nparts, relu))
                _cmp(rt, "db", kind == "exact", db, dB, tc.f32_bound(Ab, n), (n, nparts, relu))
                if len(outs) == 2:
                    assert torch.equal(dw, outs[1][0]) and torch.equal(db, outs[1][1])
                first = first or (dw, db)
            if kind == "exact":  # the fallback of _ImpalaTail.backward gives the same bits
                nparts = k.mbk_fc_wgrad_parts(n, O, I)
                dw2 = gt.empty(O, I, dtype=F32, device=cuda)
                db2 = gt.empty(O, dtype=F32, device=cuda)
                scratch = _wgrad_scratch(gt, cuda, nparts, O * I)
                assert _wgrad_launch(gg, xg, n, O, I, scratch, nparts, dw2, 0, relu, False) == 0
                colsum(gg, O, db2)
                gt.check()
                assert torch.equal(first[0], dw2) and torch.equal(first[1], db2), (n, relu)
    # the two-level reduce with rows in its partial last split (tail_cases.LONG_PARTS)
    for (nparts, n), relu in zip(tc.LONG_PARTS.items(), (1, 0)):
        g, x, _ = tc.wgrad_operands(kind, O, I, n)
        dW, dB, Aw, Ab = tc.wgrad_ref(g, x, relu)
        if kind == "exact":
            tc.assert_fp32_exact(Aw, g, x)
        dw = gt.empty(O, I, dtype=F32, device=cuda)
        db = gt.empty(O, dtype=F32, device=cuda)
        scratch = _wgrad_scratch(gt, cuda, nparts, O * I + O)
        assert _wide_launch(g.to(cuda), x.to(cuda), n, O, I, relu, scratch, nparts, dw, db) == 0
        gt.check()
        _cmp(rt, "dW", kind == "exact", dw, dW, tc.f32_bound(Aw, n), (n, nparts, relu))
        _cmp(rt, "db", kind == "exact", db, dB, tc.f32_bound(Ab, n), (n, nparts, relu))
    rt.report()


def test_fc_wgrad_wide_uncovered_shapes(cuda, gt):
    N, k = _k()
    for O, I in ((128, 128), (512, 64), (255, 32), (256, 96), (256, 288), (256, 16), (256, 256)):
        assert k.mbk_fc_wgrad_wide_parts(1300, O, I) == 0, (O, I)
    assert k.mbk_fc_wgrad_wide_parts(0, 256, 128) == 0
    g = torch.ones(128, 256, dtype=BF, device=cuda)
    x = torch.ones(128, 288, dtype=BF, device=cuda)
    dw = gt.empty(256, 288, dtype=F32, device=cuda)
    db = gt.empty(256, dtype=F32, device=cuda)
    scratch = gt.empty(2 * (256 * 288 + 256), dtype=F32, device=cuda)
    for I in (96, 288):
        assert _wide_launch(g, x, 128, 256, I, 1, scratch, 1, dw, db) == INVALID
    assert _wide_launch(g, x, 128, 256, 128, 1, scratch, 0, dw, db) == INVALID  # nparts < 1
    gt.check()
    assert untouched(dw) and untouched(db) and untouched(scratch)


# ------------------------------------------------------------------ mbk_value_bwd
def _value_launch(dv, h, w2, R, K, dh, partial, gadd, rows):
    N, k = _k()
    return k.mbk_value_bwd(dv.data_ptr(), h.data_ptr(), w2.data_ptr(), R, K, dh.data_ptr(),
                           partial.data_ptr(), N.ptr(gadd), rows,
                           int(gadd is not None and gadd.dtype == F32), N.stream_ptr())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K", tc.VALUE_K)
def test_value_bwd(cuda, gt, K, kind):
    """dh, dW2 and db2 for R = 1 .. 2049 (one, two and three 1024-row parts), gadd null, fp32 or
    bf16 over 1, R - 5 or R rows (the gadd buffer always holds R rows: the rows past gadd_rows
    are there to be wrongly added); the partial rows reduced by mbk_colsum split at c0 = K, as
    ops/pixconv.py does."""
    from microbeast_amd.ops.pixconv import colsum
    N, k = _k()
    rt = _Ratios(f"value_bwd K={K}")
    for R in tc.VALUE_R:
        dv, h, w2, gadd = tc.value_operands(kind, K, R)
        dvg, hg, w2g = dv.to(cuda), h.to(cuda), w2.to(cuda)
        variants = [(None, 0)] + [(dt, rows) for dt in (F32, BF) for rows in tc.value_gadd_rows(R)]
        for dt, rows in variants:
            ga = None if dt is None else gadd.to(dt).to(cuda)
            dh_r, Ah, dW2, Aw, db2, Ab = tc.value_bwd_ref(dv, h, w2, gadd, rows)
            if kind == "exact":
                tc.assert_fp32_exact(Ah, dv, w2, plus=(gadd,))
                tc.assert_fp32_exact(Aw, dv, h)
            P = k.mbk_value_bwd_parts(R)
            assert P == (R + 1023) // 1024
            dh = gt.empty(R, K, dtype=BF, device=cuda)
            partial = gt.empty(P, K + 1, dtype=F32, device=cuda)
            gw2 = gt.empty(K, dtype=F32, device=cuda)
            gb2 = gt.empty(1, dtype=F32, device=cuda)
            assert _value_launch(dvg, hg, w2g, R, K, dh, partial, ga, rows) == 0
            colsum(partial, K + 1, gw2, K, gb2)
            gt.check()
            filled(partial)
            note = (R, dt, rows)
            _cmp(rt, "dh", kind == "exact", dh, dh_r, tc.bf16_bound(dh_r, Ah, 2), note)
            assert bool((dh.cpu()[~(h.double() > 0)] == 0).all()), note
            _cmp(rt, "dW2", kind == "exact", gw2, dW2, tc.f32_bound(Aw, R), note)
            _cmp(rt, "db2", kind == "exact", gb2, db2.reshape(1), tc.f32_bound(Ab.reshape(1), R),
                 note)
    rt.report()


def test_value_bwd_refusals(cuda, gt):
    R = 16
    dv = torch.ones(R, device=cuda)
    h = torch.ones(R, 2056, dtype=BF, device=cuda)
    w2 = torch.ones(2056, device=cuda)
    ga = torch.ones(R + 1, 2056, device=cuda)
    dh = gt.empty(R, 2056, dtype=BF, device=cuda, interior=False)
    partial = gt.empty(2057, dtype=F32, device=cuda)
    assert _value_launch(dv, h, w2, R, 12, dh, partial, None, 0) == INVALID      # K % 8
    assert _value_launch(dv, h, w2, R, 2056, dh, partial, None, 0) == INVALID    # K > 2048
    assert _value_launch(dv, h, w2, R, 256, dh, partial, ga, R + 1) == INVALID   # gadd_rows > R
    assert _value_launch(dv, h, w2, 0, 256, dh, partial, None, 0) == 0           # no rows
    gt.check()
    assert untouched(dh) and untouched(partial)


# ------------------------------------------------------------------ mbk_colsum
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name,C,ld,f32,off", tc.COLSUM_CASES)
def test_colsum(cuda, gt, name, C, ld, f32, off, kind):
    """The bf16 vector path (C = 256; C = 78 inside ld = 80 and 96), the bf16 scalar path
    (C > 256, ld % 8 != 0, a base pointer one element off 16 bytes) and fp32 input, at R = 0 (exact
    zeros), 1 and around one and five 1024-row parts, into out0 alone (c0 = C, out1 null) and
    split at c0 = C - 1."""
    N, k = _k()
    rt = _Ratios(f"colsum {name}")
    x = tc.colsum_operands(kind, name)
    rmax = x.shape[0]
    flat = torch.zeros(rmax * ld + 8, dtype=x.dtype)
    flat[off:off + rmax * ld] = x.reshape(-1)
    flat = flat.to(cuda)
    ptr = flat.data_ptr() + off * flat.element_size()
    vec = not f32 and ld % 8 == 0 and C <= 256 and ptr % 16 == 0
    assert vec == name.startswith("vec")
    for R in tc.COLSUM_R:
        ref, A = tc.colsum_ref(x[:R], C)
        if kind == "exact":
            tc.assert_fp32_exact(A.clamp_min(1.0), x)
        P = k.mbk_colsum_parts(R)
        assert P == max(1, (R + 1023) // 1024)
        for c0 in (C, C - 1):
            partial = gt.empty(P * C, dtype=F32, device=cuda)
            out0 = gt.empty(c0, dtype=F32, device=cuda)
            out1 = gt.empty(C - c0, dtype=F32, device=cuda) if c0 < C else None
            rc = k.mbk_colsum(ptr, f32, R, C, ld, partial.data_ptr(), out0.data_ptr(), c0,
                              N.ptr(out1), N.stream_ptr())
            assert rc == 0
            gt.check()
            filled(partial)
            got = out0 if out1 is None else torch.cat([out0, out1])
            _cmp(rt, "sum", kind == "exact", got, ref, tc.f32_bound(A, max(R, 1)), (R, c0))
            if R == 0:
                assert bool((got == 0).all())
    # ld < C is refused
    out0 = gt.empty(C, dtype=F32, device=cuda)
    partial = gt.empty(C, dtype=F32, device=cuda)
    assert k.mbk_colsum(ptr, f32, 1, C, C - 1, partial.data_ptr(), out0.data_ptr(), C, None,
                        N.stream_ptr()) == INVALID
    gt.check()
    assert untouched(out0) and untouched(partial)
    rt.report()


# ------------------------------------------------------------------ mbk_map_gather
def _gather_launch(segs):
    """segs: [(src fp32, dst, map int32)] through the raw launcher; returns its code."""
    N, k = _k()
    n = len(segs)
    srcs = (ctypes.c_void_p * n)(*[s.data_ptr() for s, _, _ in segs])
    dsts = (ctypes.c_void_p * n)(*[d.data_ptr() for _, d, _ in segs])
    maps = (ctypes.c_void_p * n)(*[m.data_ptr() for _, _, m in segs])
    ns = (ctypes.c_int * n)(*[d.numel() for _, d, _ in segs])
    bf = (ctypes.c_int * n)(*[int(d.dtype == BF) for _, d, _ in segs])
    for s, d, m in segs:
        assert s.dtype == F32 and m.dtype == torch.int32 and m.numel() == d.numel()
        assert m.numel() == 0 or (int(m.max()) < s.numel() and int(m.min()) >= -1)
    return k.mbk_map_gather(n, srcs, dsts, maps, ns, bf, N.stream_ptr())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def _gather_check(src_cpu, dst, m_cpu):
    ref = tc.map_gather_ref(src_cpu, m_cpu).to(dst.dtype)
    assert torch.equal(_bits(dst.cpu().reshape(-1)), _bits(ref))


@pytest.mark.parametrize("c,ho,wo", tc.MAP_SHAPES)
def test_map_gather(cuda, gt, c, ho, wo):
    """The fwd, dgrad and grad maps of ops/tail.py at k1 = 256 into fp32 and bf16 destinations
    (a copy: bit for bit; the source holds full fp32 values, so a bf16 destination is rounded),
    maps holding -1, 24 segments of unequal length with an empty one, 25 segments refused."""
    from microbeast_amd.ops.tail import nhwc_linear_maps
    k1 = 256
    g = torch.Generator().manual_seed(ho * 10 + wo)
    src = torch.randn(k1, c * ho * wo, generator=g)
    src[0, :4] = torch.tensor([0.0, -0.0, 1.00390625, -1.01171875])  # signed zeros, bf16 ties
    srcg = src.to(cuda)
    maps = list(nhwc_linear_maps(k1, c, ho, wo))
    holes = maps[0].reshape(-1).clone()
    holes[::7] = -1
    holes[-1] = -1
    maps.append(holes)
    for m in maps:  # one segment
        for dt in (F32, BF):
            dst = gt.empty(m.numel(), dtype=dt, device=cuda)
            assert _gather_launch([(srcg, dst, m.reshape(-1).to(cuda))]) == 0
            gt.check()
            filled(dst)
            _gather_check(src, dst, m)
    # 24 segments cut from the grad map at uneven points, the 6th empty, dtypes alternating
    flat = maps[2].reshape(-1)
    L = flat.numel()
    cuts = sorted({0, L} | {(L * (j * j + 3 * j)) // (23 * 23 + 3 * 23 + 40) for j in range(1, 23)})
    cuts = cuts[:6] + [cuts[5]] + cuts[6:]
    assert len(cuts) == 25 and cuts[-1] == L
    segs = []
    for j in range(24):
        m = flat[cuts[j]:cuts[j + 1]].contiguous()
        dst = gt.empty(m.numel(), dtype=BF if j % 2 else F32, device=cuda)
        segs.append((srcg, dst, m.to(cuda), m))
    assert any(s[3].numel() == 0 for s in segs) and len({s[3].numel() for s in segs}) > 12
    assert _gather_launch([s[:3] for s in segs]) == 0
    gt.check()
    for s in segs:
        filled(s[1])
        _gather_check(src, s[1], s[3])
    # 25 segments: refused, nothing written
    dsts = [gt.empty(8, dtype=F32, device=cuda) for _ in range(25)]
    m8 = flat[:8].contiguous().to(cuda)
    assert _gather_launch([(srcg, d, m8) for d in dsts]) == INVALID
    gt.check()
    assert all(untouched(d) for d in dsts)


# ------------------------------------------------------------------ the chain, as plumbing
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ho,wo", tc.CHAIN_SHAPES)
def test_chain_matches_reference_layout_autograd(cuda, gt, ho, wo, kind):
    """TailMaps.pack -> mbk_fc_fwd -> mbk_gemm_nt_mask on a given dh -> the weight gradient as
    _ImpalaTail.backward selects it (mbk_fc_wgrad_wide at I = 64 and 128, mbk_fc_wgrad_ex +
    mbk_colsum at I = 288) -> mbk_map_gather with maps.grad, against fp64 autograd of the
    reference-layout nn.Linear on the NCHW flatten with the bf16-rounded weights."""
    from microbeast_amd.ops.pixconv import colsum, map_gather
    from microbeast_amd.ops.tail import TailMaps
    N, k = _k()
    O, c = 256, 32
    I = c * ho * wo
    rt = _Ratios(f"chain {ho}x{wo}")
    exact = kind == "exact"
    y, w5, b5, wc, bc, dh = tc.chain_operands(kind, ho, wo)
    n = y.shape[0]
    y2 = y.reshape(n, I)
    maps = TailMaps(O, c, ho, wo, cuda)
    fwd, dgrad, grad = (m.cpu().long() for m in (maps.fwd, maps.dgrad, maps.grad))
    wp, wt = maps.pack(w5.to(cuda))
    assert torch.equal(wp.cpu(), w5.reshape(-1)[fwd].bfloat16())
    assert torch.equal(wt.cpu(), w5.reshape(-1)[dgrad].bfloat16())
    f_r, dy_r, dw_r, db_r = tc.chain_ref(y, w5, b5, dh)
    yg, dhg, b5g, wcg, bcg = (t.to(cuda) for t in (y2, dh, b5, wc, bc))
    st = N.stream_ptr()
    # forward
    f = gt.empty(n, O, dtype=BF, device=cuda)
    v = gt.empty(n, dtype=F32, device=cuda)
    assert _fc_launch(yg, 1, wp, b5g, wcg, bcg, n, I, O, f, v) == 0
    # dy = (dh . W5) [y > 0]
    dy = gt.empty(n, I, dtype=BF, device=cuda)
    assert k.mbk_gemm_nt_mask(dhg.data_ptr(), wt.data_ptr(), dy.data_ptr(), None, n, I, O, O, O,
                              I, 0, 1, yg.data_ptr(), st) == 0
    # dW5 (NHWC columns) and db5, as _ImpalaTail.backward chooses
    dw5 = gt.empty(O, I, dtype=F32, device=cuda)
    gb5 = gt.empty(O, dtype=F32, device=cuda)
    wparts = k.mbk_fc_wgrad_wide_parts(n, O, I)
    assert (wparts > 0) == (I in (64, 128))
    if wparts > 0:
        scratch = _wgrad_scratch(gt, cuda, wparts, O * I + O)
        assert _wide_launch(dhg, yg, n, O, I, 1, scratch, wparts, dw5, gb5) == 0
    else:
        nparts = k.mbk_fc_wgrad_parts(n, O, I)
        scratch = _wgrad_scratch(gt, cuda, nparts, O * I)
        assert _wgrad_launch(dhg, yg, n, O, I, scratch, nparts, dw5, 0, 1, False) == 0
        colsum(dhg, O, gb5)
    gw5 = gt.empty(O, I, dtype=F32, device=cuda)
    map_gather([(dw5, gw5, maps.grad)])
    gt.check()
    A_f = tc.fc_fwd_ref(y2, w5.reshape(-1)[fwd], b5, True)[1]
    _cmp(rt, "f", exact, f, f_r, tc.bf16_bound(f_r, A_f, I + 1))
    vr, Av = tc.critic_ref(f.cpu(), wc, bc)
    _cmp(rt, "v", exact, v, vr, tc.f32_bound(Av, O + 1))
    A_y = tc.gemm_nt_ref(dh, w5.reshape(-1)[dgrad], mask=y2)[1]
    _cmp(rt, "dy", exact, dy, dy_r, tc.bf16_bound(dy_r, A_y, tc.gemm_terms(O)))
    _, _, Aw, Ab = tc.wgrad_ref(dh, y2, True)
    Aw_p = tc.map_gather_ref(Aw, grad).view(O, I)
    if exact:
        tc.assert_fp32_exact(Aw, dh, y2)
    _cmp(rt, "dW5", exact, gw5, dw_r, tc.f32_bound(Aw_p, n))
    _cmp(rt, "db5", exact, gb5, db_r, tc.f32_bound(Ab, n))
    rt.report()
