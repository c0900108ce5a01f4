"""Every kernel on the learner's path through the sparse action head (head.hip) against the fp64
oracles of tests/head_cases.py, at the edges of its tiles and chunks: cells with exactly 0, 1,
15..17, 63..65, 127..129, 255..257, 511..513, 640 and 1025 pairs on a 10x10 map (S % 32 != 0),
a 32x32 map (MAX_S), the frame-block scan's carry (F = 70 001) and the backward's chunk-run rule
at grids of 3 and 1 workgroups.

Integer outputs (the compaction) and the exact cases are compared bit for bit; the rounding cases
against the derived element-wise bounds of head_cases, whose worst error / bound ratio per family
is printed (pytest -s) and must stay below 1. Every output lies inside a larger buffer of 0xFF
bytes (-1 as int32, a NaN in fp32 and bf16): afterwards the bytes around it are unchanged, no
element that must be written holds the fill, and every element that must not be written still
does."""
import types

import pytest
import torch

import head_cases as hc
from microbeast_amd.ops.cell_head import OFFS

pytestmark = pytest.mark.gpu

GUARD = 4096
INVALID = 1  # hipErrorInvalidValue


class Guards:
    """Outputs in the middle of larger 0xFF-filled buffers."""

    def __init__(self, device):
        self.device, self.bufs = device, []

    def new(self, *shape, dtype):
        nbytes = torch.empty((), dtype=dtype).element_size()
        for s in shape:
            nbytes *= int(s)
        raw = torch.full((2 * GUARD + (nbytes + 255) // 256 * 256,), 0xFF, dtype=torch.uint8,
                         device=self.device)
        self.bufs.append((raw, nbytes, shape))
        return raw[GUARD:GUARD + nbytes].view(dtype).view(*shape)

    def check(self):
        torch.cuda.synchronize()
        for raw, nbytes, shape in self.bufs:
            assert bool((raw[:GUARD] == 0xFF).all()) and bool((raw[GUARD + nbytes:] == 0xFF).all()), \
                f"write outside an output of shape {tuple(shape)}"


def untouched(t):
    """Every byte of t still holds the fill."""
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


def _k():
    from microbeast_amd import _native as N
    return N, N.kernels()


class _Ratios:
    """Worst error / bound per family (reported, never an input)."""

    def __init__(self, tag):
        self.tag, self.r = tag, {}

    def add(self, family, got, ref, bound, limit=1.0):
        r = hc.worst_ratio(got.cpu(), ref, bound)
        self.r[family] = max(self.r.get(family, 0.0), r)
        assert r < limit, (self.tag, family, r)

    def report(self):
        for f, r in self.r.items():
            print(f"ratio {self.tag} {f} {r:.3f}")


# ------------------------------------------------------------------ compaction
def _counts(S, F, seed):
    """Random counts 0..F with both extremes present; cells 0 and S-1 active."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, F + 1, (S,), generator=g)
    c[torch.rand(S, generator=g) < 0.5] = 0
    c[0], c[S - 1] = F, max(1, F - 1)
    if S > 2:
        c[1] = 0
    return c.tolist()


def _run_compact(cuda, active, mask_bits, abits_given, dense):
    """mbk_head_compact into guarded outputs, checked against the oracle bit for bit."""
    N, k = _k()
    F, S = active.shape
    comp = hc.compaction_ref(active)
    P, U, Q = comp.totals
    fb = min(256, max(8, F // 64))  # mbk_head_fb
    nfb = (F + fb - 1) // fb
    g = Guards(cuda)
    i32 = torch.int32
    cnt, off = g.new(S * nfb, dtype=i32), g.new(S * nfb, dtype=i32)
    gs, gc, cs = g.new(S, dtype=i32), g.new(S, dtype=i32), g.new(S, dtype=i32)
    nu, nq = F * S // 16 + S + 1, F * S // 512 + S + 1
    uc, ur = g.new(nu, dtype=i32), g.new(nu, dtype=i32)
    qc, qr = g.new(nq, dtype=i32), g.new(nq, dtype=i32)
    tot = g.new(3, dtype=i32)
    pairs, pidx = g.new(F * S, dtype=i32), g.new(F, S, dtype=i32)
    SW = (S + 31) // 32
    abits = g.new(F, SW, dtype=i32)
    abits_ref = comp.abits.clone()
    if abits_given:  # a given bitmap may hold anything in the last word's bits S % 32 ..
        if S % 32:
            abits_ref[:, -1] |= -(1 << (S % 32))
        abits.copy_(abits_ref.to(cuda))
    az = lp = en = None
    if dense:
        az = g.new(F, S, 7, dtype=torch.uint8)
        lp, en = g.new(F, S, dtype=torch.float32), g.new(F, S, dtype=torch.float32)
    mb = None if abits_given else mask_bits.to(cuda)  # given bitmap: the masks are not read
    rc = k.mbk_head_compact(N.ptr(mb), F, S, cnt.data_ptr(), off.data_ptr(), gs.data_ptr(),
                            gc.data_ptr(), uc.data_ptr(), ur.data_ptr(), qc.data_ptr(),
                            qr.data_ptr(), cs.data_ptr(), tot.data_ptr(), pairs.data_ptr(),
                            pidx.data_ptr(), abits.data_ptr(), int(abits_given), N.ptr(az),
                            N.ptr(lp), N.ptr(en), N.stream_ptr())
    g.check()
    outs = dict(cnt=cnt, off=off, gs=gs, gc=gc, cs=cs, uc=uc, ur=ur, qc=qc, qr=qr, tot=tot,
                pairs=pairs, pidx=pidx, abits=abits, az=az, lp=lp, en=en)
    if S > 1024:
        return rc, outs, comp
    assert rc == 0
    assert tuple(tot.tolist()) == comp.totals
    assert torch.equal(abits.cpu(), abits_ref)
    assert torch.equal(gs.cpu(), comp.grp_start) and torch.equal(gc.cpu(), comp.grp_count)
    assert torch.equal(cs.cpu(), comp.chunk_start)
    assert torch.equal(pairs[:P].cpu(), comp.pairs) and untouched(pairs[P:])
    assert torch.equal(uc[:U].cpu(), comp.unit_cell) and torch.equal(ur[:U].cpu(), comp.unit_row)
    assert torch.equal(qc[:Q].cpu(), comp.chunk_cell) and torch.equal(qr[:Q].cpu(), comp.chunk_row)
    assert untouched(uc[U:]) and untouched(ur[U:]) and untouched(qc[Q:]) and untouched(qr[Q:])
    # pidx: the pair slot at active cells, the fill (-1, which is also the oracle's) elsewhere
    assert torch.equal(pidx.cpu().long(), comp.pidx)
    if dense:
        act = active.to(cuda)
        assert untouched(az[act]) and untouched(lp[act]) and untouched(en[act])
        assert bool((az[~act] == 0).all()) and bool((lp[~act] == 0).all()) and bool((en[~act] == 0).all())
    return rc, outs, comp


COMPACT_SHAPES = [(4, 1), (4, 7), (100, 1), (100, 7), (256, 7), (1024, 1), (1024, 7), (100, 513)]


@pytest.mark.parametrize("abits_given", [0, 1])
@pytest.mark.parametrize("S,F", COMPACT_SHAPES)
def test_compaction_small(cuda, S, F, abits_given):
    active = hc.place(_counts(S, F, S + F), F, S * 31 + F)
    assert bool(active[0, 0]) and bool(active[F - 1, S - 1])
    mask, _, _ = hc.build_masks(active, 5, plain=True)
    _run_compact(cuda, active, hc.pack_bits(mask), abits_given, dense=bool(abits_given))
    if F == 513:
        assert (F + 8 - 1) // 8 == 65  # fb = 8, 65 frame blocks


@pytest.mark.parametrize("abits_given", [0, 1])
@pytest.mark.parametrize("dense", [False, True])
def test_compaction_edge_problem(cuda, abits_given, dense):
    pb = _problem("edge", "exact")
    _run_compact(cuda, pb.active, pb.mask_bits, abits_given, dense)


@pytest.mark.parametrize("abits_given", [0, 1])
def test_compaction_scan_carry(cuda, abits_given):
    """F = 70 001 frames at S = 4: 274 frame blocks of 256, so head_cell_scan's carry over
    256-block tiles runs (production updates have 2048 blocks)."""
    F, S = 70001, 4
    fb = min(256, max(8, F // 64))
    nfb = (F + fb - 1) // fb
    assert fb == 256 and nfb == 274 and nfb > 256
    active = hc.place([F, 0, 35000, 3], F, 77)
    # the blocks beyond the first tile hold pairs of both cells (the carry matters)
    assert int(active[256 * 256:, 2].sum()) > 0
    mask, _, _ = hc.build_masks(active, 6, plain=True)
    _run_compact(cuda, active, hc.pack_bits(mask), abits_given, dense=False)


@pytest.mark.parametrize("abits_given", [0, 1])
def test_compaction_all_inactive(cuda, abits_given):
    active = torch.zeros(7, 100, dtype=torch.bool)
    _, outs, comp = _run_compact(cuda, active, torch.zeros(7, 100, 3, dtype=torch.int32),
                                 abits_given, dense=True)
    assert comp.totals == (0, 0, 0) and outs["tot"].tolist() == [0, 0, 0]


def test_compaction_refuses_more_than_1024_cells(cuda):
    active = torch.zeros(2, 1025, dtype=torch.bool)
    active[0, 0] = active[1, 1024] = True
    mask, _, _ = hc.build_masks(active, 6, plain=True)
    rc, outs, _ = _run_compact(cuda, active, hc.pack_bits(mask), 0, dense=True)
    assert rc == INVALID
    for name, t in outs.items():
        assert untouched(t), name


# ------------------------------------------------------------------ problems on the device
_PB, _ST = {}, {}
_BUILD = {"edge": hc.edge_problem, "s1024": hc.s1024_problem,
          "inactive": lambda kind: hc.build_problem([0] * 100, 7, kind, 41)}


def _problem(name, kind):
    if (name, kind) not in _PB:
        _PB[name, kind] = _BUILD[name](kind)
    return _PB[name, kind]


def _state(cuda, name, kind):
    """The problem on the device: packed weights, compaction (SparseHead), operands, oracles."""
    from microbeast_amd.ops.head import SparseHead
    if (name, kind) not in _ST:
        pb = _problem(name, kind)
        head = SparseHead(pb.S, cuda)
        head.pack(pb.W.to(cuda), pb.b.to(cuda), with_t=True)
        mb = pb.mask_bits.to(cuda)
        head.compact(mb, pb.F, None, dense_out=False)
        torch.cuda.synchronize()
        st = types.SimpleNamespace(
            pb=pb, comp=hc.compaction_ref(pb.active), head=head, mb=mb, X=pb.X.to(cuda),
            action=pb.action.to(cuda), gl=pb.g_logp.to(cuda), ge=pb.g_ent.to(cuda), oracles={},
            stats=None)
        assert tuple(head.totals.tolist()) == st.comp.totals
        _ST[name, kind] = st
    return _ST[name, kind]


def _oracle(st, g_ent=True):
    if g_ent not in st.oracles:
        st.oracles[g_ent] = hc.pair_oracle(st.pb, st.comp, g_ent=g_ent)
    return st.oracles[g_ent]


def _score(st, plp, pent, stats):
    N, k = _k()
    h = st.head
    N.check(k.mbk_head_score(st.X.data_ptr(), h.Wp.data_ptr(), h.bp.data_ptr(), st.mb.data_ptr(),
                             st.action.data_ptr(), h.pairs.data_ptr(), h.grp_start.data_ptr(),
                             h.grp_count.data_ptr(), h.chunk_cell.data_ptr(),
                             h.chunk_row.data_ptr(), h.totals.data_ptr(), st.pb.S,
                             plp.data_ptr(), N.ptr(pent), N.ptr(stats), N.stream_ptr()), "score")


def _fwd_pairs(st, plp, pent):
    N, k = _k()
    h = st.head
    N.check(k.mbk_head_fwd(st.X.data_ptr(), h.Wp.data_ptr(), h.bp.data_ptr(), st.mb.data_ptr(),
                           st.action.data_ptr(), None, 0, h.pairs.data_ptr(),
                           h.unit_cell.data_ptr(), h.unit_row.data_ptr(), h.grp_start.data_ptr(),
                           h.grp_count.data_ptr(), h.totals.data_ptr(), st.pb.S, h.fwd_grid,
                           plp.data_ptr(), N.ptr(pent), 1, N.stream_ptr()), "head_fwd")


def _bitmaps(st):
    """The compaction's bitmap, and (S % 32 != 0) a copy whose last word's unused bits are set:
    the per-frame consumers must not look at them."""
    out = [st.head.abits]
    if st.pb.S % 32:
        dirty = st.head.abits[:st.pb.F * ((st.pb.S + 31) // 32)].clone().view(st.pb.F, -1)
        dirty[:, -1] |= -(1 << (st.pb.S % 32))
        out.append(dirty)
    return out


# ------------------------------------------------------------------ scoring
@pytest.mark.parametrize("name,kind", [("edge", "exact"), ("edge", "round"), ("edge", "wide"),
                                       ("s1024", "exact"), ("s1024", "round"), ("s1024", "wide")])
def test_scoring_per_pair(cuda, name, kind):
    st = _state(cuda, name, kind)
    o = _oracle(st)
    P = st.comp.totals[0]
    rt = _Ratios(f"{name}/{kind}")
    f32 = torch.float32
    first = None
    for want_ent, want_stats in ((True, True), (False, False), (True, False), (False, True)):
        g = Guards(cuda)
        plp, pent, stats = g.new(P + 3, dtype=f32), g.new(P + 3, dtype=f32), g.new(P + 3, 16, dtype=f32)
        _score(st, plp, pent if want_ent else None, stats if want_stats else None)
        g.check()
        assert untouched(plp[P:]) and untouched(pent[P:] if want_ent else pent)
        assert untouched(stats[P:] if want_stats else stats)
        rt.add("score lp", plp[:P], o.lp, o.e_lp)
        if want_ent:
            rt.add("score ent", pent[:P], o.ent, o.e_ent)
        if want_stats:
            s = stats[:P].cpu()
            rt.add("score stats lse", s[:, :7], o.lse, o.e_lse)
            rt.add("score stats H", s[:, 7:14], o.H, o.e_H)
            assert bool((s[:, 14:] == 0).all())
            empty = torch.stack([~o.M[:, OFFS[j]:OFFS[j + 1]].any(-1) for j in range(7)], 1)
            assert bool(empty.any())
            assert bool((s[:, :7][empty] == 0).all()) and bool((s[:, 7:14][empty] == 0).all())
        if first is None:
            first = plp[:P].clone()
        assert torch.equal(first, plp[:P])  # the optional outputs change nothing
    for want_ent in (True, False):  # head_fwd's 16-pair units in pair-indexed scoring mode
        g = Guards(cuda)
        plp, pent = g.new(P + 3, dtype=f32), g.new(P + 3, dtype=f32)
        _fwd_pairs(st, plp, pent if want_ent else None)
        g.check()
        assert untouched(plp[P:]) and untouched(pent[P:] if want_ent else pent)
        rt.add("fwd lp", plp[:P], o.lp, o.e_lp)
        if want_ent:
            rt.add("fwd ent", pent[:P], o.ent, o.e_ent)
    bad = st.pb.bad[st.comp.pairs.long(), st.comp.pcell]
    assert bool(bad.any()) and bool((first.cpu()[bad] < -9e7).all())  # -1e8 - lse
    rt.report()


@pytest.mark.parametrize("name", ["edge", "s1024", "inactive"])
def test_pair_rowsum_exact(cuda, name):
    """Small-integer pair values: the per-frame sums are exact in fp32, so bit equality; a frame
    with no active cell gives 0, and the S % 32 tail word (S = 100) hides nothing."""
    N, k = _k()
    st = _state(cuda, name, "round")
    pb, comp, h = st.pb, st.comp, st.head
    P = comp.totals[0]
    gen = torch.Generator().manual_seed(P)
    a = torch.randint(-3, 4, (max(P, 1),), generator=gen).float()
    b = torch.randint(-3, 4, (max(P, 1),), generator=gen).float()
    assert int(pb.active.sum(1).min()) == 0
    ad, bd = a.to(cuda), b.to(cuda)
    for want_ent, bits in [(e, m) for e in (True, False) for m in _bitmaps(st)]:
        g = Guards(cuda)
        lp, en = g.new(pb.F, dtype=torch.float32), g.new(pb.F, dtype=torch.float32)
        N.check(k.mbk_head_pair_rowsum(h.pidx.data_ptr(), bits.data_ptr(), pb.F, pb.S,
                                       ad.data_ptr(), bd.data_ptr() if want_ent else None,
                                       lp.data_ptr(), en.data_ptr() if want_ent else None,
                                       N.stream_ptr()), "rowsum")
        g.check()
        assert torch.equal(lp.cpu().double(), hc.frame_sums(comp, a[:P])[0])
        if want_ent:
            assert torch.equal(en.cpu().double(), hc.frame_sums(comp, b[:P])[0])
        else:
            assert untouched(en)


# ------------------------------------------------------------------ backward
def _bwd(st, grid, stats, g_ent):
    """mbk_head_bwd into guarded, NaN-prefilled outputs: (dXp, dW, db)."""
    N, k = _k()
    h, pb = st.head, st.pb
    P, _, nch = st.comp.totals
    g = Guards(st.X.device)
    dXp = g.new(max(P, 1) + 2, 256, dtype=torch.bfloat16)
    dWp = g.new(max(nch, 1), 78, 256, dtype=torch.float32)
    dbp = g.new(max(nch, 1), 78, dtype=torch.float32)
    dW = g.new(pb.S, 78, 256, dtype=torch.float32)
    db = g.new(pb.S, 78, dtype=torch.float32)
    N.check(k.mbk_head_bwd(st.X.data_ptr(), h.Wp.data_ptr(), h.WpT.data_ptr(), h.bp.data_ptr(),
                           st.mb.data_ptr(), st.action.data_ptr(), h.pairs.data_ptr(),
                           h.grp_start.data_ptr(), h.grp_count.data_ptr(),
                           h.chunk_cell.data_ptr(), h.chunk_row.data_ptr(),
                           h.chunk_start.data_ptr(), h.totals.data_ptr(), st.gl.data_ptr(),
                           st.ge.data_ptr() if g_ent else None, pb.S, grid, dXp.data_ptr(),
                           dWp.data_ptr(), dbp.data_ptr(), dW.data_ptr(), db.data_ptr(),
                           N.ptr(stats), N.stream_ptr()), "head_bwd")
    g.check()
    assert untouched(dXp[P:])
    return dXp[:P], dW, db


BWD_PROBLEMS = [("edge", "round"), ("edge", "wide"), ("s1024", "round"), ("inactive", "round")]


@pytest.mark.parametrize("grid", [0, 3, 1])
@pytest.mark.parametrize("g_ent", [True, False])
@pytest.mark.parametrize("name,kind", BWD_PROBLEMS)
def test_backward(cuda, name, kind, g_ent, grid):
    """grid 0: the default (one workgroup per chunk up to the CUs); 3 and 1: a workgroup owns
    runs of several chunks and a cell's chunks split across workgroups (hb_run_end's rule)."""
    st = _state(cuda, name, kind)
    pb, comp = st.pb, st.comp
    o = _oracle(st, g_ent)
    P, _, nch = comp.totals
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    wgs = max(1, min(nch if grid == 0 else grid, cus))
    if grid and nch:
        qn = (nch + wgs - 1) // wgs
        assert qn > 1  # the multi-chunk run rule is reached
        q0, q1 = comp.chunk_start.long(), comp.chunk_start.long() + (comp.grp_count.long() - 1) // 512
        split = [c for c in o.cells.tolist() if int(q0[c]) // qn != int(q1[c]) // qn]
        if name == "edge" and grid == 3:
            print(f"qn {qn}, cells whose chunks split across workgroups: {split}")
            assert hc.EDGE_CELL[1025] in split and hc.EDGE_CELL[513] in split
    if st.stats is None:
        st.stats = torch.empty(max(P, 1), 16, dtype=torch.float32, device=cuda)
        if P:
            _score(st, torch.empty(P, device=cuda), None, st.stats)
    rt = _Ratios(f"{name}/{kind} g_ent={int(g_ent)} grid={grid}")
    cells = o.cells.to(cuda)
    idle = torch.ones(pb.S, dtype=torch.bool, device=cuda)
    idle[cells] = False
    res = {}
    garg = grid if grid else max(nch, 1)  # (SparseHead.backward's default: the launcher caps it)
    for use_stats in (True, False):
        dXp, dW, db = _bwd(st, garg, st.stats if use_stats else None, g_ent)
        fam = "ST" if use_stats else "own"
        assert not bool(torch.isnan(dW).any()) and not bool(torch.isnan(db).any())
        assert bool((dW[idle] == 0).all()) and bool((db[idle] == 0).all())  # cells without pairs
        if P:
            rt.add(f"{fam} dXp", dXp.float(), o.dXp, o.b_dXp)
            # (a zero bound demands equality: the dW rows of logits never legal in a cell)
            never = (o.b_dW.amax(-1) == 0)
            assert bool(never.any())
            assert bool((dW[cells].cpu()[never] == 0).all())
            rt.add(f"{fam} dW", dW[cells], o.dW, o.b_dW)
            rt.add(f"{fam} db", db[cells], o.db, o.b_db)
        dXp2, dW2, db2 = _bwd(st, garg, st.stats if use_stats else None, g_ent)
        assert torch.equal(dXp.view(torch.int16), dXp2.view(torch.int16))
        assert torch.equal(dW, dW2) and torch.equal(db, db2)  # deterministic
        res[use_stats] = tuple(t.cpu().double() for t in (dXp.float(), dW[cells], db[cells]))
    if P:  # the two templates agree within twice the bound
        for i, (fam, bound) in enumerate((("dXp", o.b_dXp), ("dW", o.b_dW), ("db", o.b_db))):
            rt.add(f"ST-own {fam}", res[True][i], res[False][i], bound, limit=2.0)
        if name == "edge" and grid == 0:
            for c in hc.EDGE_SINGLE + hc.EDGE_ONLY0:
                # (a row whose action sits on a masked logit has dz = -g_logp on its legal one)
                g0, n = int(comp.grp_start[c]), int(comp.grp_count[c])
                ok = ~pb.bad[comp.pairs[g0:g0 + n].long(), c]
                z = [bool((res[s][0][g0:g0 + n][ok] == 0).all()) for s in (True, False)]
                print(f"single-legal cell {c} ({int(ok.sum())} of {n} pairs with a legal action): "
                      f"pair rows exactly zero ST {z[0]} own {z[1]}")
    rt.report()


# ------------------------------------------------------------------ gathers
def _small_state(cuda, F):
    """An S = 100 problem of F frames (compaction only)."""
    from microbeast_amd.ops.head import SparseHead
    if ("small", F) not in _ST:
        counts = _counts(100, F, 3 * F)
        pb = hc.build_problem(counts, F, "round", 50 + F)
        head = SparseHead(100, cuda)
        mb = pb.mask_bits.to(cuda)
        head.compact(mb, F, None, dense_out=False)
        _ST["small", F] = types.SimpleNamespace(pb=pb, comp=hc.compaction_ref(pb.active), head=head)
    return _ST["small", F]


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("which", [1, 5, "edge", "s1024"])
def test_dx_gather(cuda, which, exact):
    N, k = _k()
    st = _small_state(cuda, which) if isinstance(which, int) else _state(cuda, which, "round")
    pb, comp, h = st.pb, st.comp, st.head
    P = comp.totals[0]
    gen = torch.Generator().manual_seed(P + 1)
    rows = (torch.randint(-3, 4, (P, 256), generator=gen) if exact
            else torch.randn(P, 256, generator=gen)).bfloat16()
    rd = rows.to(cuda)
    ref, A, n = hc.gather_ref(comp, rows)
    rt = _Ratios(f"gather {which}")
    for bits in _bitmaps(st):
        g = Guards(cuda)
        dX = g.new(pb.F, 256, dtype=torch.float32)
        N.check(k.mbk_head_dx_gather(rd.data_ptr(), h.pidx.data_ptr(), bits.data_ptr(),
                                     pb.F, pb.S, dX.data_ptr(), N.stream_ptr()), "dx_gather")
        g.check()
        if exact:
            assert torch.equal(dX.cpu().double(), ref)
        else:
            rt.add("dX", dX, ref, hc.f32_bound(A, n.double()[:, None]))
    rt.report()


def _dx_value(cuda, st, rows, dv, h, wc, F, R, parts, bits=None):
    N, k = _k()
    bits = st.head.abits if bits is None else bits
    g = Guards(cuda)
    dh = g.new(R, 256, dtype=torch.bfloat16)
    partial = g.new(max(parts, 1), 257, dtype=torch.float32)
    ops = [t.to(cuda) for t in (rows, dv, h, wc)]  # (kept alive until the check's synchronize)
    rc = k.mbk_head_dx_value(ops[0].data_ptr(), st.head.pidx.data_ptr(),
                             bits.data_ptr(), F, st.pb.S, ops[1].data_ptr(),
                             ops[2].data_ptr(), ops[3].data_ptr(), R, dh.data_ptr(),
                             partial.data_ptr(), parts, N.stream_ptr())
    g.check()
    return rc, dh, partial


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("extra", [0, 5])
@pytest.mark.parametrize("name", ["edge", "s1024"])
def test_dx_value(cuda, name, extra, exact):
    """S = 100: two 64-cell slots, the second partial; S = 1024: all 16 slots of the kernel."""
    N, k = _k()
    st = _state(cuda, name, "round")
    pb, comp = st.pb, st.comp
    P, F, R = comp.totals[0], pb.F, pb.F + extra
    gen = torch.Generator().manual_seed(R)
    if exact:
        rows = torch.randint(-3, 4, (P, 256), generator=gen).bfloat16()
        dv = (torch.randint(-2, 3, (R,), generator=gen) / 2).float()
        wc = (torch.randint(-2, 3, (256,), generator=gen) / 2).float()
        h = torch.randint(-2, 3, (R, 256), generator=gen).bfloat16()
    else:
        rows = torch.randn(P, 256, generator=gen).bfloat16()
        dv, wc = torch.randn(R, generator=gen), torch.randn(256, generator=gen)
        h = torch.randn(R, 256, generator=gen).bfloat16()
    parts = k.mbk_head_dx_value_parts(R)
    assert 1 <= parts <= (R + 3) // 4
    rc, dh, partial = _dx_value(cuda, st, rows, dv, h, wc, F, R, parts)
    assert rc == 0
    for bits in _bitmaps(st)[1:]:  # unused bits of the bitmap's last word change nothing
        rc2, dh2, partial2 = _dx_value(cuda, st, rows, dv, h, wc, F, R, parts, bits)
        assert rc2 == 0 and torch.equal(dh.view(torch.int16), dh2.view(torch.int16))
        assert torch.equal(partial, partial2)
    ref, A, terms, dWc, dbc = hc.dx_value_ref(comp, rows, dv, h, wc, R)
    assert not bool(torch.isnan(dh).any()) and not bool(torch.isnan(partial).any())
    assert bool((dh.float().cpu()[h.float() <= 0] == 0).all())
    col = partial.cpu().double().sum(0)
    if exact:
        hc_ref = ref.bfloat16()
        assert torch.equal(hc_ref.double(), ref)  # exact before its single bf16 store
        assert torch.equal(dh.cpu(), hc_ref)
        assert torch.equal(col[:256], dWc) and float(col[256]) == float(dbc)
    else:
        rt = _Ratios(f"dx_value {name} R=F+{extra}")
        rt.add("dh", dh.float(), ref, hc.bf16_bound(ref, A, (terms + 1)[:, None]))
        Aw = (dv.double().abs()[:, None] * h.double().abs()).sum(0)
        rt.add("dWc", col[:256], dWc, hc.f32_bound(Aw, R + parts))
        rt.add("dbc", col[256:], dbc.reshape(1), hc.f32_bound(dv.double().abs().sum().reshape(1), R + parts))
        rt.report()
    if exact and extra:  # refusals: nothing is written
        for Fx, px in ((R + 1, parts), (F, 0)):
            rc, dh, partial = _dx_value(cuda, st, rows, dv, h, wc, Fx, R, px)
            assert rc == INVALID and untouched(dh) and untouched(partial)


# ------------------------------------------------------------------ pack
@pytest.mark.parametrize("with_t", [True, False])
@pytest.mark.parametrize("S", [4, 100])
def test_pack(cuda, S, with_t):
    N, k = _k()
    gen = torch.Generator().manual_seed(S)
    W = torch.randn(S * 78, 256, generator=gen)
    b = torch.randn(S * 78, generator=gen)
    g = Guards(cuda)
    Wp = g.new(S, 80, 256, dtype=torch.bfloat16)
    WpT = g.new(S, 256, 96, dtype=torch.bfloat16)
    bp = g.new(S, 80, dtype=torch.float32)
    Wd, bd = W.to(cuda), b.to(cuda)
    N.check(k.mbk_head_pack(Wd.data_ptr(), bd.data_ptr(), S, Wp.data_ptr(),
                            bp.data_ptr(), WpT.data_ptr() if with_t else None, N.stream_ptr()),
            "pack")
    g.check()
    rWp, rWpT, rbp = hc.pack_ref(W, b, S)
    assert torch.equal(Wp.cpu().view(torch.int16), rWp.view(torch.int16))
    assert torch.equal(bp.cpu().view(torch.int32), rbp.view(torch.int32))
    assert bool((Wp[:, 78:] == 0).all()) and bool((bp[:, 78:] == 0).all())
    if with_t:
        assert torch.equal(WpT.cpu().view(torch.int16), rWpT.view(torch.int16))
        assert bool((WpT[:, :, 78:] == 0).all())
    else:
        assert untouched(WpT)


# ------------------------------------------------------------------ sampling frequencies
def test_sampling_frequencies(cuda):
    """head_fwd's sampling mode on 8192 frames that share one X row and one active cell: per
    segment the counts follow the fp64 masked softmax (Philox: deterministic); masked logits are
    never drawn."""
    from microbeast_amd.ops.head import SparseHead, sparse_sample
    x, W, b, m, p = hc.sampling_case()
    n, S, c = hc.SAMPLE_N, hc.SAMPLE_S, hc.SAMPLE_CELL
    mask = torch.zeros(n, S, 78, dtype=torch.bool)
    mask[:, c] = m
    head = SparseHead(S, cuda)
    rng = torch.tensor([2024, 0], dtype=torch.int64, device=cuda)
    a, _ = sparse_sample(x.repeat(n, 1).to(cuda), W.to(cuda), b.to(cuda),
                         hc.pack_bits(mask).to(cuda), rng, head)
    a = a.cpu()
    assert bool((a[:, [0, 1, 3]] == 0).all())
    hc.assert_in_band(a[:, c], m, p)


# ------------------------------------------------------------------ count-mode units (acting)
# Pairs per cell at the edges of head_fwd's 16-pair unit and head_act's 64-pair job; the first
# cell, the last two and the runs 4..6 and 13..96 are empty (an empty cell shares the next one's
# prefix: the tie of the unit search)
UNIT_CELLS = {1: 1, 2: 15, 3: 16, 7: 17, 8: 63, 9: 0, 10: 64, 11: 65, 12: 128, 97: 129}
UNIT_F, UNIT_S, UNIT_E = 131, 100, 130  # frames, cells, bucket stride (>= the largest count)


def _unit_state(cuda):
    """Hand-built buckets (cell c's frames, ascending, at bucket[c * E ..]) and the sorted path's
    actions / per-cell log-probs of modes 1 and 2, computed once."""
    from guarded import GuardedTorch
    from microbeast_amd.ops.head import SparseHead
    if "units" in _ST:
        return _ST["units"]
    N, k = _k()
    F, S, E = UNIT_F, UNIT_S, UNIT_E
    counts = [UNIT_CELLS.get(c, 0) for c in range(S)]
    assert counts[0] == 0 and counts[-1] == 0 and max(counts) <= E
    assert sorted(set(counts)) == [0, 1, 15, 16, 17, 63, 64, 65, 128, 129]
    active = hc.place(counts, F, 91, special={0: []})  # frame 0: no active cell
    mask, _, _ = hc.build_masks(active, 92)
    gen = torch.Generator().manual_seed(93)
    head = SparseHead(S, cuda)
    head.pack((torch.randn(S * 78, 256, generator=gen) * 0.05).to(cuda),
              (torch.randn(S * 78, generator=gen) * 0.1).to(cuda), with_t=False)
    # unused bucket slots name frame 0: a slot read by mistake writes an inactive cell's output
    bucket = torch.zeros(S, E, dtype=torch.int32)
    for c in range(S):
        fr = active[:, c].nonzero().flatten()
        assert not (counts[c] == 0 and len(fr)) and not bool(active[0, c])
        bucket[c, :len(fr)] = fr.int()
    st = types.SimpleNamespace(
        F=F, S=S, E=E, head=head, active=active.to(cuda), mb=hc.pack_bits(mask).to(cuda),
        X=(torch.randn(F, 256, generator=gen) * 0.5).bfloat16().to(cuda), bucket=bucket.to(cuda),
        cnt=torch.tensor(counts, dtype=torch.int32, device=cuda),
        rng=torch.tensor([4711, 5], dtype=torch.int64, device=cuda), ref={})
    head.compact(st.mb, F, None, dense_out=False)
    for mode in (1, 2):
        g = GuardedTorch()
        a = g.empty(F, S, 7, dtype=torch.uint8, device=cuda, interior=False)
        lp = g.empty(F, S, dtype=torch.float32, device=cuda, interior=False)
        N.check(k.mbk_head_fwd(st.X.data_ptr(), head.Wp.data_ptr(), head.bp.data_ptr(),
                               st.mb.data_ptr(), a.data_ptr(), st.rng.data_ptr(), mode,
                               head.pairs.data_ptr(), head.unit_cell.data_ptr(),
                               head.unit_row.data_ptr(), head.grp_start.data_ptr(),
                               head.grp_count.data_ptr(), head.totals.data_ptr(), S, head.fwd_grid,
                               lp.data_ptr(), None, 0, N.stream_ptr()), "head_fwd")
        g.check()
        assert untouched(a[~st.active]) and untouched(lp[~st.active])
        assert not bool(torch.isnan(lp[st.active]).any()) and bool((a[st.active] <= 48).all())
        st.ref[mode] = (a[st.active].clone(), lp[st.active].view(torch.int32).clone())
    assert not torch.equal(st.ref[1][0], st.ref[2][0])  # sampling and arg-max differ somewhere
    _ST["units"] = st
    return st


@pytest.mark.parametrize("grid", [0, 3, 1])
@pytest.mark.parametrize("greedy", [0, 1])
def test_count_mode_units_match_sorted_path(cuda, greedy, grid):
    """mbk_head_fwd_counts derives its 16-pair units from the per-cell bucket counts in every
    workgroup (unit_prefix + cell_of, the derivation head_act's jobs share): on counts at every
    unit and job edge, with empty cells first, last and in runs, its actions and per-cell
    log-probs equal the sorted path's (mbk_head_compact + mbk_head_fwd) bit for bit. grid 1 and
    3: one workgroup's four waves stride over all 35 units. The counters are left alone and
    nothing is written for an inactive cell."""
    from guarded import GuardedTorch
    N, k = _k()
    st = _unit_state(cuda)
    F, S, E, head = st.F, st.S, st.E, st.head
    g = GuardedTorch()
    a = g.empty(F, S, 7, dtype=torch.uint8, device=cuda, interior=False)
    lp = g.empty(F, S, dtype=torch.float32, device=cuda, interior=False)
    cnt = g.empty(S, dtype=torch.int32, device=cuda, interior=False)
    cnt.copy_(st.cnt)
    N.check(k.mbk_head_fwd_counts(st.X.data_ptr(), head.Wp.data_ptr(), head.bp.data_ptr(),
                                  st.mb.data_ptr(), a.data_ptr(), st.rng.data_ptr(),
                                  st.bucket.data_ptr(), cnt.data_ptr(), E, S,
                                  grid if grid else head.fwd_grid, lp.data_ptr(), greedy,
                                  N.stream_ptr()), "head_fwd_counts")
    g.check()
    assert torch.equal(cnt, st.cnt)
    assert untouched(a[~st.active]) and untouched(lp[~st.active])
    ra, rlp = st.ref[2 if greedy else 1]
    assert torch.equal(a[st.active], ra)
    assert torch.equal(lp[st.active].view(torch.int32), rlp)
