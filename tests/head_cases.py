"""fp64 oracles, case builders and derived bounds for the sparse action head (head.hip).

The oracles are written from the definitions, in plain torch float64 / int64, on the kernels'
bf16-rounded operands; tests/test_head_cases.py checks them against the dense reference
formulation (ops/cell_head.cell_head_torch in float64 with autograd) and a brute-force
compaction on the CPU, tests/test_gpu_head_edges.py holds every launcher of the learner's head
path to them.

Problems are built from a list of per-cell pair counts (``place``): the frames of every cell are
drawn so that each cell has exactly the requested number of active (frame, cell) pairs, a few
"special" frames have an exact set of active cells (none, 1, 4, 5, 9: the four-rows-in-flight
grouping of head_dx_value), and (0, 0) and (F-1, S-1) are active. ``edge_counts`` puts the counts
0, 1, 15, 16, 17 (a 16-pair unit), 63, 64, 65 (a scoring wave), 127, 128, 129 (HB_TM), 255, 256,
257 (HS_TM), 511, 512, 513 (CHUNK), 640 and 1025 (three chunks) on a 10x10 map (S % 32 != 0).
Active rows mix four kinds (all 78 logits legal / one legal logit per segment / some segments
fully masked / only logit 0 legal) with random ones; some cells hold only single-legal rows, some
never allow a few logits, and a marked subset of rows carries an action on a masked logit.

Two kinds of case, as in conv_cases:

* exact: X, W, b and the loss gradients are small multiples of 0.5, so every logit is exact in
  fp32 in any order (``assert_fp32_exact``) and eps_z = 0: the only error left in the forward is
  the device's exp / log.
* round: random-normal bf16 X (scale 0.5), W (scale 0.05); wide: the same with a few X rows
  scaled so that the legal logits reach beyond +-80 (a softmax without its max-subtraction
  overflows there).

Bounds (first order; U_SUM = 2^-23 per summed term is twice fp32's 2^-24, U_BF16 = 2^-8 one
round-to-nearest bf16 store; c_t: the transcendental constant, below). Per segment with legal
logits j, p = softmax, d_j = z_j - max z, zbar = sum p z:

  eps_z_j  = 256 U_SUM sum_k |x_k||w_jk| + U_SUM |b_j|      (the MFMA sum, the bias add; exact: 0)
  rho_j    = eps_z_j + 2^-24 |d_j| + c_t 2^-23 (1 + |d_j|)   relative error of e_j = exp(d_j)
  rho_s    = sum p_j rho_j + n U_SUM                         relative error of s = sum e_j
  eps_lse  = rho_s + c_t 2^-23 (1 + |log s|) + 2^-24 (|max z| + |lse|)
  eps_H    = eps_lse + sum p_j rho_j |z_j - zbar| + sum p_j eps_z_j
             + (n + 3) U_SUM sum p_j |z_j| + 2^-24 (|lse| + |zbar|)     (H = lse - sum e z / s:
             the normalised weights' errors sum to zero, hence z_j - zbar; the division / rcp)
  eps_lp   = sum_k (eps_z_a + eps_lse_k) + 14 U_SUM sum_k (|z_a or 1e8| + |lse_k|)
  eps_ent  = sum_k eps_H_k + 7 U_SUM sum_k |H_k|
  backward, lp_j = z_j - lse, p_j = exp(lp_j), dz_j = gl (1[j = a] - p_j) - ge p_j (lp_j + H):
  eps_lpj  = eps_z_j + eps_lse + 2^-24 |lp_j|
  rho_pj   = eps_lpj + c_t 2^-23 (1 + |lp_j|)
  eps_dz_j = |gl| p_j rho_pj + |ge| p_j (rho_pj |lp_j + H| + eps_lpj + eps_H + 2^-24 (|lp_j| + |H|))
             + 4 U_SUM (|gl| (1[j = a] + p_j) + |ge| p_j (|lp_j| + |H|))
  bf16 dZ store, modelled by the oracle (dzb = bf16(dz)):
  eps_dzb_j = eps_dz_j + U_BF16 |dz_j| + (bf16(dz_j + eps_dz_j) - bf16(dz_j - eps_dz_j))
             (the last term is zero unless dz_j lies within eps_dz_j of a bf16 rounding boundary:
             there the kernel's own dz may round to the neighbouring bf16 number, one bf16 ulp)
  dXp      : U_BF16 |ref| + sum_j eps_dzb_j |w_jd| + 96 U_SUM sum_j |dzb_j||w_jd|
  dW_c     : sum_pairs eps_dzb |x| + (n_c + partials) U_SUM sum_pairs |dzb||x|
  db_c     : sum_pairs eps_dz + (n_c + 16) U_SUM sum_pairs |dz|   (db sums the fp32 dz)
  dX / dh  : conv_cases.f32_bound / bf16_bound over a frame's active cells (+ the value term)

Flush to zero: the device may return 0 for any fp32 / bf16 result below the smallest normal
number TINY = 2^-126 (denormal flushing, v_exp_f32's underflow, the MFMA's denormal handling), so
wherever a bound is proportional to a probability (eps_dz and what is summed from it) it also
carries an absolute floor: TINY (4 + |gl| + |ge||lp_j + H|) per legal logit's dz (p itself lost,
times what multiplies it, and three products), one more for the bf16 store, and one per non-zero
product of the sums. Masked logits have no floor: their
zeros stay exact. (The wide case needs this: p = exp(-180) there.)

c_t is the error of one device exp / log call in units of 2^-23 (1 + |x|) relative for exp(x) and
2^-23 (1 + |log s|) absolute for log(s). The HIP documentation shipped with ROCm carries no ULP
table for __expf / __logf, so it is measured (``measure_ct``): the float32 CPU form of the formulas above
(torch.exp / torch.log in float32) against float64 on the exact case gives C_CPU = 0.31 (exp
0.113, log 0.303: half an ulp of libm, divided by 1 + |x|); the kernels get C_T = 4 C_CPU = 1.24.
(v_exp_f32 and v_log_f32 are 1-ulp instructions around one rounded multiply by log2 e / ln 2:
below 1 in these units; a logic error is thousands.) No bound is fitted to a kernel's output.
"""
import dataclasses

import torch

from conv_cases import (U_BF16, U_SUM, assert_fp32_exact, bf16_bound, f32_bound,  # noqa: F401
                        round_trunc_bf16, worst_ratio)
from microbeast_amd.ops.cell_head import NVEC, OFFS

KD, NP, NPT, CELL, COMPS, UNIT, CHUNK = 256, 80, 96, 78, 7, 16, 512
MASK_FILL = -1e8
C_CPU = 0.31         # measured by measure_ct on the exact case (test_head_cases pins it)
C_T = 4 * C_CPU      # the kernels' allowance
INACTIVE_BYTE = 200  # action bytes of inactive cells: never a valid action if read by mistake
U24 = 2.0 ** -24
TINY = 2.0 ** -126     # smallest normal fp32 / bf16: results below it may be flushed to zero


# ------------------------------------------------------------------ placement
EDGE_NAMED = (1, 0, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512)  # cells 0..15
# the multi-chunk cells sit where the backward's workgroup ranges end at a grid of 3 (81 chunks, 27
# per workgroup): cell 33's chunks are 26 | 27, 28 and cell 65's 53 | 54, split across workgroups
EDGE_BIG = {25: 640, 33: 1025, 65: 513}
EDGE_CELL = {**{n: c for c, n in enumerate(EDGE_NAMED)}, **{n: c for c, n in EDGE_BIG.items()}}


def edge_counts():
    """Per-cell pair counts of the edge problem (S = 100; needs F >= 1031)."""
    counts = list(EDGE_NAMED) + [0] * 6 + [[3, 0, 7, 2, 5, 0, 11, 1][c % 8] for c in range(22, 100)]
    for c in (31, 63, 95):
        counts[c] = 4
    for c, n in EDGE_BIG.items():
        counts[c] = n
    return counts


EDGE_F, EDGE_S = 1100, 100
EDGE_RANKS = (0, 15, 16, 63, 64, 127, 128, 255, 256, 511, 512, 639, 1023, 1024)
# frame -> its exact set of active cells: none, 1, 4 (31/32 and 63), 5 (64, 95/96), 9
EDGE_SPECIAL = {1: [], 2: [33], 3: [33, 31, 32, 63], 4: [33, 7, 64, 95, 96],
                5: [33, 4, 5, 6, 7, 8, 9, 10, 11]}
EDGE_SINGLE = (3, 27, 31)   # cells whose rows all have one legal logit per segment
EDGE_ONLY0 = (0, 23)        # cells whose rows have only logit 0 legal


def place(counts, F, seed, special=None):
    """bool [F, S]: cell c active in exactly counts[c] frames; frames in ``special`` have exactly
    the listed active cells; (0, 0) and (F-1, S-1) are active when their cells have pairs."""
    S = len(counts)
    special = special or {}
    g = torch.Generator().manual_seed(seed)
    active = torch.zeros(F, S, dtype=torch.bool)
    for f, cells in special.items():
        active[f, cells] = True
    keep = torch.ones(F, dtype=torch.bool)
    keep[list(special)] = False
    general = keep.nonzero().flatten()
    used = active.sum(0)
    for c, n in enumerate(counts):
        need = int(n - used[c])
        assert 0 <= need <= len(general), (c, n)
        if need == 0:
            continue
        sel = general[torch.randperm(len(general), generator=g)[:need]]
        if c == 0 and bool(keep[0]) and not bool((sel == 0).any()):
            sel[0] = 0
        if c == S - 1 and bool(keep[F - 1]) and not bool((sel == F - 1).any()):
            sel[-1] = F - 1
        active[sel, c] = True
    assert torch.equal(active.sum(0), torch.tensor(counts))
    for f, cells in special.items():
        assert int(active[f].sum()) == len(cells)
    return active


def never_legal(c):
    """Logits no pair of cell c may use (cells c % 4 == 1), else none."""
    return [5, 9, 30 + c % 48, 77] if c % 4 == 1 else []


def build_masks(active, seed, single_cells=(), only0_cells=(), plain=False, bad_rate=0.1):
    """(mask bool [F, S, 78], action uint8 [F, S, 7], bad bool [F, S]) for an activity pattern.
    plain: random rows only (the large compaction-only problems)."""
    F, S = active.shape
    g = torch.Generator().manual_seed(seed)
    fi, ci = active.nonzero(as_tuple=True)
    P = len(fi)
    ar = torch.arange(P)
    m = torch.rand(P, CELL, generator=g) < 0.5
    m[:, 0] = True
    bad = torch.zeros(P, dtype=torch.bool)
    act = torch.zeros(P, COMPS, dtype=torch.uint8)
    if not plain and P:
        kind = torch.randint(0, 8, (P,), generator=g)  # 0 all, 1 single, 2 segments, 3 only 0
        # the first and last rows of a cell's units, waves, tiles and chunks are random rows: a
        # single-legal row has no gradient, so losing it there would go unseen
        rank = (active.long().cumsum(0) - 1)[fi, ci]
        edge = torch.isin(rank, torch.tensor(EDGE_RANKS)) | (rank == active.sum(0)[ci] - 1)
        kind[edge] = 4
        for c in single_cells:
            kind[ci == c] = 1
        for c in only0_cells:
            kind[ci == c] = 3
        m[kind == 0] = True
        one = torch.zeros(P, CELL, dtype=torch.bool)
        for k in range(COMPS):
            one[ar, OFFS[k] + torch.randint(0, NVEC[k], (P,), generator=g)] = True
        m[kind == 1] = one[kind == 1]
        drop = torch.rand(P, COMPS, generator=g) < 0.5
        drop[ar, ar % COMPS] = False  # one segment stays
        dropped = torch.repeat_interleave(drop, torch.tensor(NVEC), dim=1)
        forced = torch.zeros(P, CELL, dtype=torch.bool)
        forced[ar, torch.tensor(OFFS[:COMPS])[ar % COMPS]] = True
        m2 = (m & ~dropped) | forced
        m[kind == 2] = m2[kind == 2]
        only0 = torch.zeros(P, CELL, dtype=torch.bool)
        only0[:, 0] = True
        m[kind == 3] = only0[kind == 3]
        for c in range(S):
            nv = never_legal(c)
            if nv and c not in single_cells and c not in only0_cells:
                rows = (ci == c).nonzero().flatten()
                if len(rows):
                    m[rows[:, None], torch.tensor(nv)[None, :]] = False
        assert bool(m.any(-1).all())
        marked = torch.rand(P, generator=g) < bad_rate
        for k in range(COMPS):
            seg = m[:, OFFS[k]:OFFS[k + 1]]
            pick = torch.multinomial(seg.float() + 1e-9, 1, generator=g).flatten()
            act[:, k] = torch.where(seg.any(-1), pick, torch.zeros_like(pick)).to(torch.uint8)
            cond = marked & (ar % COMPS == k) & seg.any(-1) & ~seg.all(-1)
            wrong = torch.multinomial((~seg).float() + 1e-9, 1, generator=g).flatten()
            act[:, k] = torch.where(cond, wrong, act[:, k].long()).to(torch.uint8)
            bad |= cond
    mask = torch.zeros(F, S, CELL, dtype=torch.bool)
    mask[fi, ci] = m
    action = torch.full((F, S, COMPS), INACTIVE_BYTE, dtype=torch.uint8)
    action[fi, ci] = act
    badfs = torch.zeros(F, S, dtype=torch.bool)
    badfs[fi, ci] = bad
    return mask, action, badfs


def pack_bits(mask):
    """bool [F, S, 78] -> int32 [F, S, 3] (ops.cell_head.pack_mask, in frame blocks)."""
    F, S, _ = mask.shape
    out = torch.empty(F, S, 3, dtype=torch.int32)
    sh = torch.arange(32)
    for f0 in range(0, F, 4096):
        blk = mask[f0:f0 + 4096]
        m = torch.zeros(*blk.shape[:2], 96, dtype=torch.int64)
        m[..., :CELL] = blk
        w = (m.view(*blk.shape[:2], 3, 32) << sh).sum(-1)
        out[f0:f0 + 4096] = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return out


@dataclasses.dataclass
class Problem:
    kind: str
    F: int
    S: int
    counts: list
    active: torch.Tensor     # bool [F, S]
    mask: torch.Tensor       # bool [F, S, 78]
    mask_bits: torch.Tensor  # int32 [F, S, 3]
    action: torch.Tensor     # uint8 [F, S, 7], INACTIVE_BYTE at inactive cells
    bad: torch.Tensor        # bool [F, S]: the action of one segment is on a masked logit
    X: torch.Tensor          # bf16 [F, 256]
    W: torch.Tensor          # fp32 [S * 78, 256]
    b: torch.Tensor          # fp32 [S * 78]
    g_logp: torch.Tensor     # fp32 [F]
    g_ent: torch.Tensor      # fp32 [F]

    @property
    def exact(self):
        return self.kind == "exact"

    def action_ref(self):
        """The actions with zeros at inactive cells (what a dense formulation may index with)."""
        return torch.where(self.active[..., None], self.action, torch.zeros_like(self.action))


def build_problem(counts, F, kind, seed, special=None, single_cells=(), only0_cells=(),
                  bad_rate=0.1):
    assert kind in ("exact", "round", "wide")
    S = len(counts)
    active = place(counts, F, seed, special)
    mask, action, bad = build_masks(active, seed + 1, single_cells, only0_cells, bad_rate=bad_rate)
    g = torch.Generator().manual_seed(seed + 2)
    if kind == "exact":
        X = (torch.randint(-2, 3, (F, KD), generator=g) / 2
             * (torch.rand(F, KD, generator=g) < 0.125)).bfloat16()
        W = (torch.tensor([-1.0, -0.5, 0.5, 1.0])[torch.randint(0, 4, (S * CELL, KD), generator=g)]
             * (torch.rand(S * CELL, KD, generator=g) < 0.5)).float()
        b = (torch.randint(-4, 5, (S * CELL,), generator=g) / 2).float()
        g_logp = (torch.randint(-2, 3, (F,), generator=g) / 2).float()
        g_ent = (torch.randint(-2, 3, (F,), generator=g) / 2).float()
    else:
        X = (torch.randn(F, KD, generator=g) * 0.5).bfloat16()
        W = torch.randn(S * CELL, KD, generator=g) * 0.05
        b = torch.randn(S * CELL, generator=g) * 0.1
        g_logp = torch.randn(F, generator=g)
        g_ent = torch.randn(F, generator=g)
    pb = Problem(kind, F, S, list(counts), active, mask, pack_bits(mask), action, bad, X, W, b,
                 g_logp, g_ent)
    if kind == "wide":
        _widen(pb)
    return pb


def _widen(pb):
    """Scale the X row of every 7th frame with active cells so its largest legal |logit| is
    about 95."""
    frames = pb.active.any(1).nonzero().flatten()[::7]
    Wq = pb.W.bfloat16().double().view(pb.S, CELL, KD)
    for f in frames.tolist():
        cells = pb.active[f].nonzero().flatten()
        z = torch.einsum("k,cjk->cj", pb.X[f].double(), Wq[cells])
        top = float(z[pb.mask[f, cells]].abs().max())
        if top > 0:
            pb.X[f] = (pb.X[f].float() * (95.0 / top)).bfloat16()


def edge_problem(kind, seed=11):
    return build_problem(edge_counts(), EDGE_F, kind, seed, EDGE_SPECIAL, EDGE_SINGLE, EDGE_ONLY0)


def s1024_counts():
    """A few hundred pairs on a 32x32 map (MAX_S): cells 0 and 1023, the 64-cell word edges of
    head_dx_value's 16 slots, one cell past a 128-pair tile."""
    counts = [0] * 1024
    for c, n in ((0, 5), (31, 2), (32, 3), (63, 1), (64, 17), (511, 130), (512, 16), (959, 1),
                 (960, 33), (1022, 2), (1023, 64)):
        counts[c] = n
    for c in range(100, 1000, 37):
        counts[c] = max(counts[c], 1 + c % 5)
    return counts


S1024_F = 140
S1024_SPECIAL = {1: [], 2: [1023], 3: [0, 511, 960, 1023], 4: [0, 64, 511, 512, 1023],
                 5: [0, 31, 32, 64, 511, 512, 960, 1022, 1023]}


def s1024_problem(kind, seed=23):
    return build_problem(s1024_counts(), S1024_F, kind, seed, S1024_SPECIAL, (64,), (63,))


# ------------------------------------------------------------------ compaction oracle
@dataclasses.dataclass
class Compaction:
    abits: torch.Tensor        # int32 [F, (S + 31) // 32]
    grp_start: torch.Tensor    # int32 [S]
    grp_count: torch.Tensor    # int32 [S]
    pairs: torch.Tensor        # int32 [P]: frame of every pair, grouped by cell, frames ascending
    pcell: torch.Tensor        # int64 [P]: cell of every pair
    pidx: torch.Tensor         # int64 [F, S]: pair slot, -1 at inactive cells
    unit_cell: torch.Tensor
    unit_row: torch.Tensor
    chunk_cell: torch.Tensor
    chunk_row: torch.Tensor
    chunk_start: torch.Tensor  # int32 [S]
    totals: tuple              # (P, units, chunks)


def _lists(start, count, step):
    cells, rows = [], []
    for c in range(len(count)):
        r = torch.arange(0, int(count[c]), step)
        cells.append(torch.full_like(r, c))
        rows.append(int(start[c]) + r)
    return torch.cat(cells).int(), torch.cat(rows).int()


def compaction_ref(active):
    """Stable counting sort of the active (frame, cell) pairs by cell."""
    F, S = active.shape
    fi, ci = active.nonzero(as_tuple=True)  # frame-major
    order = torch.sort(ci, stable=True).indices
    pairs, pcell = fi[order], ci[order]
    count = active.sum(0)
    start = torch.cumsum(count, 0) - count
    pidx = torch.full((F, S), -1, dtype=torch.int64)
    pidx[pairs, pcell] = torch.arange(len(pairs))
    SW = (S + 31) // 32
    bits = torch.zeros(F, SW * 32, dtype=torch.int64)
    bits[:, :S] = active
    w = (bits.view(F, SW, 32) << torch.arange(32)).sum(-1)
    abits = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    uc, ur = _lists(start, count, UNIT)
    qc, qr = _lists(start, count, CHUNK)
    nq = (count + CHUNK - 1) // CHUNK
    return Compaction(abits, start.int(), count.int(), pairs.int(), pcell, pidx, uc, ur, qc, qr,
                      (torch.cumsum(nq, 0) - nq).int(), (len(pairs), len(uc), len(qc)))


# ------------------------------------------------------------------ per-pair oracle
@dataclasses.dataclass
class Pairs:
    cells: torch.Tensor   # int64 [nc]: the cells that have pairs, ascending
    Z: torch.Tensor       # [P, 78] logits
    eZ: torch.Tensor
    M: torch.Tensor       # bool [P, 78]
    lse: torch.Tensor     # [P, 7]
    H: torch.Tensor
    e_lse: torch.Tensor
    e_H: torch.Tensor
    lp: torch.Tensor      # [P]
    ent: torch.Tensor
    e_lp: torch.Tensor
    e_ent: torch.Tensor
    stats: torch.Tensor   # [P, 16]
    e_stats: torch.Tensor
    dz: torch.Tensor = None     # [P, 78]
    e_dz: torch.Tensor = None
    dzb: torch.Tensor = None    # the bf16 dZ the GEMMs read
    e_dzb: torch.Tensor = None
    dXp: torch.Tensor = None    # [P, 256]
    b_dXp: torch.Tensor = None
    dW: torch.Tensor = None     # [nc, 78, 256]
    b_dW: torch.Tensor = None
    db: torch.Tensor = None     # [nc, 78]
    b_db: torch.Tensor = None


def _bf16(t):
    return t.float().bfloat16().double()


def logits_ref(pb, comp):
    """(Z, A, cells): Z[p][j] = x_f . bf16(w_cj) + b_cj per pair, A on absolute values."""
    P = comp.totals[0]
    Z = torch.zeros(P, CELL, dtype=torch.float64)
    A = torch.zeros_like(Z)
    cells = comp.grp_count.nonzero().flatten()
    for c in cells.tolist():
        g0, n = int(comp.grp_start[c]), int(comp.grp_count[c])
        x = pb.X[comp.pairs[g0:g0 + n].long()].double()
        w = pb.W[c * CELL:(c + 1) * CELL].bfloat16().double()
        bc = pb.b[c * CELL:(c + 1) * CELL].double()
        Z[g0:g0 + n] = x @ w.t() + bc
        A[g0:g0 + n] = x.abs() @ w.abs().t() + bc.abs()
    return Z, A, cells


def pair_oracle(pb, comp, backward=True, c_t=C_T, action=None, g_ent=True, round_dz=True,
                trunc=False, ent_sign=1.0, h_shift=False, mask_grad=False):
    """The scoring forward per pair and (backward) dz, dXp, dW_c, db_c with their bounds.
    action / trunc / ent_sign / h_shift / mask_grad: the oracle-side mutants of test_head_cases;
    round_dz False: no bf16 dZ store (the comparison with the dense reference)."""
    P = comp.totals[0]
    Z, A, cells = logits_ref(pb, comp)
    if pb.exact:
        if P:
            assert_fp32_exact(A, pb.X, pb.W, plus=(pb.b,))
        eZ = torch.zeros_like(Z)
    else:
        babs = pb.b.view(pb.S, CELL)[comp.pcell].double().abs()
        eZ = 256 * U_SUM * (A - babs) + U_SUM * babs
    fi, ci = comp.pairs.long(), comp.pcell
    M = pb.mask[fi, ci]
    act = (pb.action if action is None else action)[fi, ci].long()
    gl = pb.g_logp[fi].double()
    ge = pb.g_ent[fi].double() if g_ent else torch.zeros(P, dtype=torch.float64)
    z0 = torch.zeros(P, COMPS, dtype=torch.float64)
    lse, H, e_lse, e_H = z0.clone(), z0.clone(), z0.clone(), z0.clone()
    lp, ent, e_lp, e_ent = (torch.zeros(P, dtype=torch.float64) for _ in range(4))
    A_lp, A_ent = torch.zeros(P, dtype=torch.float64), torch.zeros(P, dtype=torch.float64)
    seg = []
    for k in range(COMPS):
        o0, o1 = OFFS[k], OFFS[k + 1]
        zs, ms, ez = Z[:, o0:o1], M[:, o0:o1], eZ[:, o0:o1]
        has = ms.any(-1)
        n = ms.sum(-1).double()
        mx = torch.where(ms, zs, torch.full_like(zs, float("-inf"))).max(-1).values
        mx = torch.where(has, mx, torch.zeros_like(mx))
        d = torch.where(ms, zs - mx[:, None], torch.zeros_like(zs))
        e = torch.where(ms, d.exp(), torch.zeros_like(zs))
        s = torch.where(has, e.sum(-1), torch.ones_like(mx))
        p = e / s[:, None]
        ls = torch.where(has, mx + s.log(), torch.zeros_like(mx))
        zbar = (p * zs).sum(-1)
        h = torch.where(has, ls - zbar, torch.zeros_like(mx))
        rho = torch.where(ms, ez + U24 * d.abs() + c_t * U_SUM * (1 + d.abs()),
                          torch.zeros_like(zs))
        rho_s = (p * rho).sum(-1) + n * U_SUM
        el = rho_s + c_t * U_SUM * (1 + s.log().abs()) + U24 * (mx.abs() + ls.abs())
        eh = (el + (p * rho * (zs - zbar[:, None]).abs()).sum(-1) + (p * ez).sum(-1)
              + (n + 3) * U_SUM * (p * zs.abs()).sum(-1) + U24 * (ls.abs() + zbar.abs()))
        el, eh = el * has, eh * has
        lse[:, k], H[:, k], e_lse[:, k], e_H[:, k] = ls, h, el, eh
        a = act[:, k]
        ain = a < (o1 - o0)
        ac = a.clamp(max=o1 - o0 - 1)
        valid = ain & ms.gather(1, ac[:, None]).squeeze(1)
        za = torch.where(valid, zs.gather(1, ac[:, None]).squeeze(1),
                         torch.full_like(mx, MASK_FILL))
        lp += torch.where(has, za - ls, torch.zeros_like(mx))
        A_lp += torch.where(has, za.abs() + ls.abs(), torch.zeros_like(mx))
        e_lp += torch.where(has, ez.gather(1, ac[:, None]).squeeze(1) * valid + el,
                            torch.zeros_like(mx))
        ent += h
        e_ent += eh
        A_ent += h.abs()
        seg.append((zs, ms, ez, p, ls, el, ac, ain))
    e_lp += 14 * U_SUM * A_lp
    e_ent += 7 * U_SUM * A_ent
    stats = torch.cat([lse, H, torch.zeros(P, 2, dtype=torch.float64)], 1)
    e_stats = torch.cat([e_lse, e_H, torch.zeros(P, 2, dtype=torch.float64)], 1)
    out = Pairs(cells, Z, eZ, M, lse, H, e_lse, e_H, lp, ent, e_lp, e_ent, stats, e_stats)
    if not backward:
        return out
    dz = torch.zeros(P, CELL, dtype=torch.float64)
    e_dz = torch.zeros_like(dz)
    for k in range(COMPS):
        o0, o1 = OFFS[k], OFFS[k + 1]
        zs, ms, ez, p, ls, el, ac, ain = seg[k]
        hk = H[:, (k + 1) % COMPS] if h_shift else H[:, k]
        ehk = e_H[:, k]
        lpj = torch.where(ms, zs - ls[:, None], torch.zeros_like(zs))
        onehot = torch.zeros_like(zs)
        onehot.scatter_(1, ac[:, None], ain.double()[:, None])
        g1, g2 = gl[:, None], ge[:, None]
        v = g1 * (onehot - p) - ent_sign * g2 * p * (lpj + hk[:, None])
        elpj = ez + el[:, None] + U24 * lpj.abs()
        rp = elpj + c_t * U_SUM * (1 + lpj.abs())
        Adz = g1.abs() * (onehot + p) + g2.abs() * p * (lpj.abs() + hk.abs()[:, None])
        ev = (g1.abs() * p * rp
              + g2.abs() * p * (rp * (lpj + hk[:, None]).abs() + elpj + ehk[:, None]
                                + U24 * (lpj.abs() + hk.abs()[:, None]))
              + 4 * U_SUM * Adz
              + TINY * (4 + g1.abs() + g2.abs() * (lpj + hk[:, None]).abs()))  # p flushed
        if mask_grad:  # the mutant: the action's one-hot passes through the mask
            dz[:, o0:o1] = torch.where(ms, v, g1 * onehot)
        else:
            dz[:, o0:o1] = torch.where(ms, v, torch.zeros_like(v))
        e_dz[:, o0:o1] = torch.where(ms, ev, torch.zeros_like(ev))
    if not round_dz:
        dzb = dz.clone()
        e_dzb = e_dz.clone()
    else:
        dzb = round_trunc_bf16(dz) if trunc else _bf16(dz)
        e_dzb = e_dz + U_BF16 * dz.abs() + (_bf16(dz + e_dz) - _bf16(dz - e_dz)) + TINY * (e_dz > 0)
    out.dz, out.e_dz, out.dzb, out.e_dzb = dz, e_dz, dzb, e_dzb
    nc = len(cells)
    out.dXp = torch.zeros(P, KD, dtype=torch.float64)
    out.b_dXp = torch.zeros_like(out.dXp)
    out.dW = torch.zeros(nc, CELL, KD, dtype=torch.float64)
    out.b_dW = torch.zeros_like(out.dW)
    out.db = torch.zeros(nc, CELL, dtype=torch.float64)
    out.b_db = torch.zeros_like(out.db)
    for i, c in enumerate(cells.tolist()):
        g0, n = int(comp.grp_start[c]), int(comp.grp_count[c])
        r = slice(g0, g0 + n)
        x = pb.X[comp.pairs[r].long()].double()
        w = pb.W[c * CELL:(c + 1) * CELL].bfloat16().double()
        ref = dzb[r] @ w
        legal = (e_dz[r] > 0).double()  # the elements that carry the flush floors
        out.dXp[r] = ref
        out.b_dXp[r] = (U_BF16 * ref.abs() + (1 + U_BF16) * (e_dzb[r] @ w.abs())
                        + NPT * U_SUM * (dzb[r].abs() @ w.abs())
                        + TINY * (1 + legal @ (w != 0).double()))
        parts = (n + CHUNK - 1) // CHUNK
        out.dW[i] = dzb[r].t() @ x
        out.b_dW[i] = (e_dzb[r].t() @ x.abs() + (n + parts) * U_SUM * (dzb[r].abs().t() @ x.abs())
                       + TINY * (legal.t() @ (x != 0).double()))
        out.db[i] = dz[r].sum(0)
        out.b_db[i] = (e_dz[r].sum(0) + (n + 16) * U_SUM * dz[r].abs().sum(0)
                       + TINY * legal.sum(0))
    return out


def measure_ct(pb, comp):
    """The float32 CPU form of the forward's exp / log against float64 on the exact case, in the
    units of the module docstring: (worst exp, worst log)."""
    assert pb.exact
    Z, _, _ = logits_ref(pb, comp)
    M = pb.mask[comp.pairs.long(), comp.pcell]
    we = wl = 0.0
    for k in range(COMPS):
        zs, ms = Z[:, OFFS[k]:OFFS[k + 1]], M[:, OFFS[k]:OFFS[k + 1]]
        has = ms.any(-1)
        zs, ms = zs[has], ms[has]
        mx = torch.where(ms, zs, torch.full_like(zs, float("-inf"))).max(-1).values
        d = (zs - mx[:, None])[ms]
        assert torch.equal(d.float().double(), d)
        e32 = d.float().exp().double()
        ok = d.exp() > 2.0 ** -120  # (below: fp32 denormals, an absolute matter)
        we = max(we, float(((e32 - d.exp()).abs() / d.exp() / (U_SUM * (1 + d.abs())))[ok].max()))
        s32 = torch.where(ms, (zs - mx[:, None]).float().exp(), torch.zeros_like(zs).float()).sum(-1)
        l64 = s32.double().log()
        wl = max(wl, float(((s32.log().double() - l64).abs() / (U_SUM * (1 + l64.abs()))).max()))
    return we, wl


# ------------------------------------------------------------------ per-frame oracles
def frame_sums(comp, vals):
    """out[f] = sum over f's active cells of vals[pidx[f][c]] (float64), and the same on |vals|."""
    act = comp.pidx >= 0
    if not len(vals):
        z = torch.zeros(comp.pidx.shape[0], dtype=torch.float64)
        return z, z.clone()
    v = torch.where(act, vals.double()[comp.pidx.clamp(min=0)], torch.zeros((), dtype=torch.float64))
    return v.sum(1), v.abs().sum(1)


def gather_ref(comp, dXp):
    """dX[f] = sum over f's active cells of the pair rows dXp [P, 256] (as stored: bf16), A, and
    the active cells per frame."""
    F, S = comp.pidx.shape
    dX = torch.zeros(F, KD, dtype=torch.float64)
    A = torch.zeros_like(dX)
    rows = dXp.double()
    fr = comp.pairs.long()
    dX.index_add_(0, fr, rows)
    A.index_add_(0, fr, rows.abs())
    return dX, A, (comp.pidx >= 0).sum(1)


def dx_value_ref(comp, dXp, dv, h, wc, R):
    """dh [R, 256] = (dv wc + dX) * (h > 0) with rows >= F taking the value term only, its A, the
    summed terms per row, and (dWc [256], dbc)."""
    F = comp.pidx.shape[0]
    dX, A, n = gather_ref(comp, dXp)
    val = dv.double()[:, None] * wc.double()[None, :]
    full = val.clone()
    full[:F] += dX
    Af = val.abs()
    Af[:F] += A
    pos = (h.double() > 0).double()
    terms = torch.ones(R, dtype=torch.float64)
    terms[:F] += n
    dWc = (dv.double()[:, None] * h.double()).sum(0)
    return full * pos, Af * pos, terms, dWc, dv.double().sum()


def pack_ref(W, b, S, pads=0.0):
    """(Wp [S, 80, 256] bf16, WpT [S, 256, 96] bf16, bp [S, 80] fp32); pads: the mutant's value in
    the rows 78, 79 of Wp."""
    Wq = W.view(S, CELL, KD).bfloat16()
    Wp = torch.full((S, NP, KD), pads, dtype=torch.bfloat16)
    Wp[:, :CELL] = Wq
    WpT = torch.zeros(S, KD, NPT, dtype=torch.bfloat16)
    WpT[:, :, :CELL] = Wq.transpose(1, 2)
    bp = torch.zeros(S, NP, dtype=torch.float32)
    bp[:, :CELL] = b.view(S, CELL)
    return Wp, WpT, bp


# ------------------------------------------------------------------ sampling frequencies
SAMPLE_N, SAMPLE_S, SAMPLE_CELL = 8192, 4, 2


def sampling_case(seed=5):
    """One X row, one active cell whose mask leaves every segment at least two legal and one
    masked logit: (x bf16 [256], W, b, mask bool [78], p float64 [78]: the masked softmax of
    every segment, 0 at masked logits)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(KD, generator=g) * 2).bfloat16()
    W = torch.randn(SAMPLE_S * CELL, KD, generator=g) * 0.05
    b = torch.randn(SAMPLE_S * CELL, generator=g) * 0.1
    m = torch.rand(CELL, generator=g) < 0.6
    for k in range(COMPS):
        m[OFFS[k]] = m[OFFS[k] + 1] = True
        m[OFFS[k + 1] - 1] = False
    c = SAMPLE_CELL
    z = W[c * CELL:(c + 1) * CELL].bfloat16().double() @ x.double() + b[c * CELL:(c + 1) * CELL].double()
    p = torch.zeros(CELL, dtype=torch.float64)
    for k in range(COMPS):
        o0, o1 = OFFS[k], OFFS[k + 1]
        zk = torch.where(m[o0:o1], z[o0:o1], torch.full((o1 - o0,), float("-inf"), dtype=torch.float64))
        p[o0:o1] = torch.softmax(zk, 0)
    return x, W, b, m, p


def assert_in_band(actions, m, p):
    """actions int [N, 7] drawn from p: per segment |n_j - N p_j| <= 5 sqrt(N p_j (1 - p_j)) + 1
    for every legal j, and no masked logit is ever drawn."""
    N = actions.shape[0]
    for k in range(COMPS):
        o0, o1 = OFFS[k], OFFS[k + 1]
        n = torch.bincount(actions[:, k].long(), minlength=o1 - o0).double()
        assert len(n) == o1 - o0, "an action outside its segment"
        pk, mk = p[o0:o1], m[o0:o1]
        assert float(n[~mk].sum()) == 0, "a masked logit was sampled"
        band = 5 * (N * pk * (1 - pk)).sqrt() + 1
        assert bool(((n - N * pk).abs() <= band)[mk].all()), (k, n.tolist(), (N * pk).tolist())
