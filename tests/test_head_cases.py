"""The sparse head's fp64 oracles (tests/head_cases.py) against the dense reference formulation
and a brute-force compaction, the exact / wide cases' preconditions, the measured transcendental
constant, and the oracle-side mutants: each wrong kernel the GPU suite is meant to catch is
applied to the oracle and shown to exceed the bound (or break the equality) it targets. The
factors are printed (pytest -s) and quoted in the README."""
import functools
import math

import torch

import head_cases as hc
from microbeast_amd.ops import cell_head
from microbeast_amd.ops.cell_head import NVEC, OFFS


@functools.lru_cache(maxsize=None)
def _edge(kind):
    pb = hc.edge_problem(kind)
    return pb, hc.compaction_ref(pb.active)


@functools.lru_cache(maxsize=None)
def _edge_oracle(kind):
    return hc.pair_oracle(*_edge(kind))


def _tiny(kind, seed=3):
    counts = [3, 0, 8, 1, 2, 5, 0, 4]
    pb = hc.build_problem(counts, 9, kind, seed, {1: [], 2: [2]}, single_cells=(4,),
                          only0_cells=(3,), bad_rate=0.5)
    return pb, hc.compaction_ref(pb.active)


# ------------------------------------------------------------------ oracle vs reference
def _dense_reference(pb):
    """lp, ent [F] and dX, dW, db of sum(g_logp lp + g_ent ent) through cell_head_torch on
    float64 logits = X W^T + b. A fully masked segment scores -log n in float64 (fp32 rounds it
    to the 0 the kernels define): its constant is added back."""
    X = pb.X.double().requires_grad_(True)
    W = pb.W.bfloat16().double().requires_grad_(True)
    b = pb.b.double().requires_grad_(True)
    _, lp, ent = cell_head.cell_head_torch(X @ W.t() + b, pb.mask, pb.action_ref())
    ((lp * pb.g_logp.double()).sum() + (ent * pb.g_ent.double()).sum()).backward()
    const = torch.zeros(pb.F, dtype=torch.float64)
    for k in range(7):
        empty = ~pb.mask[..., OFFS[k]:OFFS[k + 1]].any(-1)
        const += empty.sum(1) * math.log(NVEC[k])
    return (lp + const).detach(), ent.detach(), X.grad, W.grad.view(pb.S, 78, 256), b.grad.view(pb.S, 78)


def test_oracle_matches_dense_reference():
    for kind in ("round", "exact"):
        pb, comp = _tiny(kind)
        segs = torch.stack([pb.mask[..., OFFS[k]:OFFS[k + 1]].sum(-1) for k in range(7)], -1)
        act = pb.active
        assert 0 in pb.counts and bool((segs[act] == 0).any()) and bool((segs[act] == 1).any())
        assert bool(pb.bad.any())
        o = hc.pair_oracle(pb, comp, round_dz=False)
        lp, ent, dX, dW, db = _dense_reference(pb)
        tol = dict(rtol=1e-10, atol=1e-10)
        # (float64 at 1e8 rounds to 1.5e-8: every fully masked segment of the dense form costs that)
        torch.testing.assert_close(hc.frame_sums(comp, o.lp)[0], lp, rtol=1e-12, atol=1e-5)
        assert bool((lp < -1e7).any())  # an action on a masked logit: -1e8 - lse
        torch.testing.assert_close(hc.frame_sums(comp, o.ent)[0], ent, **tol)
        torch.testing.assert_close(hc.gather_ref(comp, o.dXp)[0], dX, **tol)
        ref_w, ref_b = torch.zeros_like(dW), torch.zeros_like(db)
        ref_w[o.cells], ref_b[o.cells] = o.dW, o.db
        torch.testing.assert_close(ref_w, dW, **tol)
        torch.testing.assert_close(ref_b, db, **tol)
        # the modelled bf16 dZ store moves dW (and dXp) by no more than their bounds
        r = hc.pair_oracle(pb, comp)
        assert hc.worst_ratio(o.dW, r.dW, r.b_dW) < 1
        assert hc.worst_ratio(o.dXp, r.dXp, r.b_dXp) < 1
        assert torch.equal(o.db, r.db)


def test_frame_oracles():
    pb, comp = _tiny("round")
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(comp.totals[0], 256, generator=g).bfloat16()
    dX, A, n = hc.gather_ref(comp, rows)
    for f in range(pb.F):
        want = sum((rows[int(comp.pidx[f, c])].double() for c in range(pb.S) if pb.active[f, c]),
                   torch.zeros(256, dtype=torch.float64))
        torch.testing.assert_close(dX[f], want, rtol=1e-12, atol=1e-12)
        assert int(n[f]) == int(pb.active[f].sum())
    R = pb.F + 2
    dv, wc = torch.randn(R, generator=g), torch.randn(256, generator=g)
    h = torch.randn(R, 256, generator=g).bfloat16()
    dh, _, _, dWc, dbc = hc.dx_value_ref(comp, rows, dv, h, wc, R)
    full = dv.double()[:, None] * wc.double()
    full[:pb.F] += dX
    torch.testing.assert_close(dh, full * (h.double() > 0), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(dWc, dv.double() @ h.double(), rtol=1e-12, atol=1e-12)
    assert float(dbc) == float(dv.double().sum())


# ------------------------------------------------------------------ compaction
def _brute_compaction(active):
    F, S = active.shape
    pairs, pcell, pidx = [], [], {}
    for c in range(S):
        for f in range(F):
            if active[f, c]:
                pidx[f, c] = len(pairs)
                pairs.append(f)
                pcell.append(c)
    return pairs, pcell, pidx


def _expand(cells, rows, comp, step):
    """The pair ranges a unit / chunk list covers, concatenated."""
    out = []
    for c, r in zip(cells.tolist(), rows.tolist()):
        end = int(comp.grp_start[c] + comp.grp_count[c])
        assert int(comp.grp_start[c]) <= r < end and (r - int(comp.grp_start[c])) % step == 0
        out += list(range(r, min(r + step, end)))
    return out


def test_compaction_oracle_matches_brute_force():
    for active in (_edge("exact")[0].active, _tiny("exact")[0].active,
                   torch.zeros(5, 3, dtype=torch.bool)):
        F, S = active.shape
        comp = hc.compaction_ref(active)
        pairs, pcell, pidx = _brute_compaction(active)
        P = len(pairs)
        assert comp.pairs.tolist() == pairs and comp.pcell.tolist() == pcell
        assert comp.grp_count.tolist() == active.sum(0).tolist()
        for c in range(S):
            g0, n = int(comp.grp_start[c]), int(comp.grp_count[c])
            assert pcell[g0:g0 + n] == [c] * n
        for f in range(F):
            for c in range(S):
                assert int(comp.pidx[f, c]) == pidx.get((f, c), -1)
                word = int(comp.abits[f, c >> 5]) & 0xFFFFFFFF
                assert ((word >> (c & 31)) & 1) == int(active[f, c])
        assert _expand(comp.unit_cell, comp.unit_row, comp, hc.UNIT) == list(range(P))
        assert _expand(comp.chunk_cell, comp.chunk_row, comp, hc.CHUNK) == list(range(P))
        assert comp.totals == (P, sum((n + 15) // 16 for n in active.sum(0).tolist()),
                               sum((n + 511) // 512 for n in active.sum(0).tolist()))
        for c in range(S):
            q = int(comp.chunk_start[c])
            if int(comp.grp_count[c]):
                assert int(comp.chunk_cell[q]) == c and int(comp.chunk_row[q]) == int(comp.grp_start[c])


def test_edge_problem_has_its_edges():
    pb, comp = _edge("exact")
    for n in (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 640, 1025):
        assert pb.counts[hc.EDGE_CELL[n]] == n
    # at a grid of 3 the 1025- and 513-pair cells' chunks split across workgroups
    qn = (comp.totals[2] + 2) // 3
    for n in (1025, 513):
        q0 = int(comp.chunk_start[hc.EDGE_CELL[n]])
        assert q0 // qn != (q0 + (n - 1) // 512) // qn
    assert bool(pb.active[0, 0]) and bool(pb.active[-1, -1])
    per_frame = pb.active.sum(1)
    assert [int(per_frame[f]) for f in (1, 2, 3, 4, 5)] == [0, 1, 4, 5, 9]
    for c in (31, 32, 63, 64, 95, 96):
        assert pb.counts[c] > 0
    assert bool(pb.active[3, 31] & pb.active[3, 32]) and bool(pb.active[4, 95] & pb.active[4, 96])
    rows = pb.mask[pb.active]
    segs = torch.stack([rows[:, OFFS[k]:OFFS[k + 1]].sum(-1) for k in range(7)], -1)
    assert bool(rows.all(-1).any())                      # all 78 legal
    assert bool((segs == 1).all(-1).any())               # one legal logit per segment
    assert bool(((segs == 0).any(-1) & (segs > 1).any(-1)).any())
    assert bool(((rows.sum(-1) == 1) & rows[:, 0]).any())  # only logit 0
    assert bool(pb.bad.any())
    c = hc.EDGE_CELL[513]  # 513 pairs, and logits no pair may use
    assert hc.never_legal(c) and not bool(pb.mask[:, c][:, hc.never_legal(c)].any())
    assert (pb.action[~pb.active] == hc.INACTIVE_BYTE).all()


# ------------------------------------------------------------------ exact / wide / c_t
def test_exact_case_is_exact_and_wide_case_reaches_its_range():
    o = _edge_oracle("exact")  # assert_fp32_exact inside
    assert float(o.eZ.abs().max()) == 0
    pb, comp = _edge("wide")
    Z, _, _ = hc.logits_ref(pb, comp)
    legal = Z[pb.mask[comp.pairs.long(), comp.pcell]]
    print(f"wide legal logits {float(legal.min()):.1f} .. {float(legal.max()):.1f}")
    assert float(legal.max()) >= 89 and float(legal.min()) <= -80  # exp(89) overflows fp32
    w = hc.pair_oracle(pb, comp)
    for t in (w.lp, w.ent, w.dXp, w.dW, w.db, w.b_dXp, w.b_dW):
        assert bool(torch.isfinite(t).all())


def test_cpu_transcendental_constant():
    we, wl = hc.measure_ct(*_edge("exact"))
    print(f"c_t: float32 CPU exp {we:.3f} log {wl:.3f} (units of 2^-23 (1 + |x|)); "
          f"C_CPU {hc.C_CPU} C_T {hc.C_T}")
    assert 0.9 * hc.C_CPU <= max(we, wl) <= hc.C_CPU and hc.C_T == 4 * hc.C_CPU


def test_fp32_cpu_form_is_inside_the_bounds():
    """The formulas in float32 on the CPU (the kernels' arithmetic, libm's exp / log) stay inside
    the bounds given C_CPU: the bounds are not too tight for a correct implementation."""
    for kind in ("exact", "round", "wide"):
        pb, comp = _edge(kind)
        o = hc.pair_oracle(pb, comp, backward=False, c_t=hc.C_CPU)
        Z = o.Z.float() if pb.exact else (
            pb.X[comp.pairs.long()].float()[:, None, :]
            * pb.W.bfloat16().float().view(pb.S, 78, 256)[comp.pcell]).sum(-1) \
            + pb.b.view(pb.S, 78)[comp.pcell]
        assert hc.worst_ratio(Z, o.Z, o.eZ) < 1
        for k in range(7):
            zs, ms = Z[:, OFFS[k]:OFFS[k + 1]], o.M[:, OFFS[k]:OFFS[k + 1]]
            has = ms.any(-1)
            mx = torch.where(ms, zs, torch.full_like(zs, float("-inf"))).max(-1).values
            mx = torch.where(has, mx, torch.zeros_like(mx))
            e = torch.where(ms, (zs - mx[:, None]).exp(), torch.zeros_like(zs))
            s = torch.where(has, e.sum(-1), torch.ones_like(mx))
            lse = torch.where(has, mx + s.log(), torch.zeros_like(mx))
            H = torch.where(has, lse - (e * zs).sum(-1) / s, torch.zeros_like(mx))
            assert hc.worst_ratio(lse, o.lse[:, k], o.e_lse[:, k]) < 1, (kind, k)
            assert hc.worst_ratio(H, o.H[:, k], o.e_H[:, k]) < 1, (kind, k)


# ------------------------------------------------------------------ mutants
def _cell_slice(comp, c):
    g0 = int(comp.grp_start[c])
    return g0, int(comp.grp_count[c])


def _dw_without(pb, comp, o, c, rows, scale=-1.0):
    """dW_c of cell c with the given rows of it dropped (scale -1) or doubled (+1)."""
    g0, _ = _cell_slice(comp, c)
    i = o.cells.tolist().index(c)
    r = slice(g0 + rows.start, g0 + rows.stop)
    x = pb.X[comp.pairs[r].long()].double()
    return i, o.dW[i] + scale * (o.dzb[r].t() @ x)


def test_mutants_exceed_their_bounds():
    pb, comp = _edge("round")
    o = _edge_oracle("round")
    f = {}
    # a tile's first row lost: the 129th row of the 129-pair cell
    i, m = _dw_without(pb, comp, o, hc.EDGE_CELL[129], slice(128, 129))
    f["row 129 dropped (dW)"] = hc.worst_ratio(m, o.dW[i], o.b_dW[i])
    # the last partial tile's rows doubled: rows 129.. of the 255-pair cell
    i, m = _dw_without(pb, comp, o, hc.EDGE_CELL[255], slice(128, 255), +1.0)
    f["partial tile doubled (dW)"] = hc.worst_ratio(m, o.dW[i], o.b_dW[i])
    # a run_end mismatch: the partial of the first chunk of the 1025-pair cell left out
    i, m = _dw_without(pb, comp, o, hc.EDGE_CELL[1025], slice(0, 512))
    f["first chunk's partial dropped (dW)"] = hc.worst_ratio(m, o.dW[i], o.b_dW[i])
    g0, n = _cell_slice(comp, hc.EDGE_CELL[1025])
    mb = o.db[i] - o.dz[g0:g0 + 512].sum(0)
    f["first chunk's partial dropped (db)"] = hc.worst_ratio(mb, o.db[i], o.b_db[i])
    for name, kw in (("entropy gradient sign flipped", dict(ent_sign=-1.0)),
                     ("H from the neighbouring segment", dict(h_shift=True)),
                     ("masked logit given gradient", dict(mask_grad=True)),
                     ("truncating dZ store", dict(trunc=True))):
        m = hc.pair_oracle(pb, comp, **kw)
        f[name + " (dXp)"] = hc.worst_ratio(m.dXp, o.dXp, o.b_dXp)
        f[name + " (dW)"] = hc.worst_ratio(m.dW, o.dW, o.b_dW)
    # the unaligned action-word path reading one byte early
    early = torch.roll(pb.action.flatten(), 1).view_as(pb.action)
    m = hc.pair_oracle(pb, comp, action=early)
    f["action byte one early (lp)"] = hc.worst_ratio(m.lp, o.lp, o.e_lp)
    f["action byte one early (dW)"] = hc.worst_ratio(m.dW, o.dW, o.b_dW)
    # stats-slot shift as the forward would write it
    sh = torch.roll(o.stats[:, 7:14], -1, 1)
    f["H slots shifted (stats)"] = hc.worst_ratio(sh, o.stats[:, 7:14], o.e_stats[:, 7:14])
    for k, v in f.items():
        print(f"mutant {k}: {v:.3g} x bound")
        assert v > 1 or k == "truncating dZ store (dXp)", k  # (its dW factor must exceed 1)
    assert f["masked logit given gradient (dW)"] == float("inf")  # an exact zero broken
    # pack with rows 78 / 79 non-zero: bit equality fails
    Wp, _, _ = hc.pack_ref(pb.W, pb.b, pb.S)
    Wm, _, _ = hc.pack_ref(pb.W, pb.b, pb.S, pads=1.0)
    diff = int((Wp.view(torch.int16) != Wm.view(torch.int16)).sum())
    print(f"mutant pack pads non-zero: {diff} elements differ")
    assert diff == pb.S * 2 * 256


def test_sampling_band_holds_for_cpu_draws():
    """torch.multinomial from the sampling case's probabilities stays inside the band the GPU
    test holds head_fwd's sampling mode to (so the band is no lottery for these inputs)."""
    _, _, _, m, p = hc.sampling_case()
    g = torch.Generator().manual_seed(7)
    acts = torch.stack([torch.multinomial(p[OFFS[k]:OFFS[k + 1]], hc.SAMPLE_N, True, generator=g)
                        for k in range(7)], 1)
    assert bool((m.sum() > 14)) and all(
        bool(m[OFFS[k]:OFFS[k + 1]].sum() >= 2) and not bool(m[OFFS[k]:OFFS[k + 1]].all())
        for k in range(7))
    hc.assert_in_band(acts, m, p)
