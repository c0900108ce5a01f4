"""Greedy (arg-max) mode of the acting kernels: per segment the lowest legal index whose logit
equals the segment's legal maximum == ``cell_head.greedy`` (argmax of where(mask, z, -1e8),
first occurrence), no random numbers, the sampler's step counter advancing as for a sampled
step. Sparse head (head.hip, sorted and bucketed), the fused acting step (launch B) against
the graph step, and the three masked-cell samplers (masked_cell.hip)."""
import pytest
import torch

from microbeast_amd import _native as N
from microbeast_amd.ops import cell_head
from microbeast_amd.ops.cell_head import OFFS, pack_mask
from microbeast_amd.ops.head import SparseHead, sparse_sample, sparse_score

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ A: sparse head, exact
def _int_problem(F, S, seed, hot_cell=None, hot_frames=0):
    """Integer-valued operands: every logit is an exact fp32 integer (|z| <= 2 * 256 + 3) in
    any summation order, so the kernel's logits equal the dense fp32 ones bit for bit.
    Adjacent weight rows are duplicated inside segments: exact ties."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randint(-2, 3, (F, 256), generator=g).float()
    W = torch.randint(-1, 2, (S * 78, 256), generator=g).float()
    b = torch.randint(-3, 4, (S * 78,), generator=g).float()
    Wv, bv = W.view(S, 78, 256), b.view(S, 78)
    for j in (0, 2, 7, 11, 22, 23, 30, 31, 32, 60, 76):  # j and j + 1 share a segment
        Wv[:, j + 1] = Wv[:, j]
        bv[:, j + 1] = bv[:, j]
    active = torch.rand(F, S, generator=g) < 0.15
    if hot_cell is not None:  # one cell active in hot_frames frames: > one 64-pair job, and a
        active[:, hot_cell] = False                                      # ragged 16-pair unit
        active[torch.randperm(F, generator=g)[:hot_frames], hot_cell] = True
    m = (torch.rand(F, S, 78, generator=g) < 0.5) & active[..., None]
    m[..., 0] |= active
    fa = active.nonzero()
    # active cells with fully masked segments, and single-legal-bit segments
    for i, (f, c) in enumerate(fa.tolist()):
        if i % 5 == 0:
            m[f, c, 6:22] = False
        if i % 7 == 0:
            m[f, c, 29:78] = False
            m[f, c, 29 + (i % 49)] = True
        if i % 11 == 0:
            m[f, c, 22:29] = False
            m[f, c, 23], m[f, c, 24] = True, True   # a legal pair at tied logits
    assert bool((~m.any(-1)).any()) and bool((m.any(-1) & ~m[..., 6:10].any(-1)).any())
    return X.bfloat16(), W, b, m


def _fill_buckets(head, m, E):
    """What mbk_decode_obs_mask_bucket leaves for the head: per-cell frame lists + counts,
    zeroed per-cell log-probs."""
    S = head.S
    head.ensure_buckets(E)
    act = m.any(-1)
    bucket = torch.zeros(S, E, dtype=torch.int32)
    cnt = act.sum(0).to(torch.int32)
    for c in range(S):
        fr = act[:, c].nonzero().view(-1).to(torch.int32)
        bucket[c, :len(fr)] = fr
    head.bucket.copy_(bucket.view(-1))
    head.bucket_cnt.copy_(cnt)
    head.cell_lp.zero_()


@pytest.mark.parametrize("F,S,hot", [(150, 16, 100), (70, 256, 0)])
def test_sparse_head_greedy_exact(cuda, F, S, hot):
    X, W, b, m = _int_problem(F, S, seed=F, hot_cell=3 if hot else None, hot_frames=hot)
    if hot:
        assert int(m.any(-1)[:, 3].sum()) == hot
    logits = X.float() @ W.T + b          # exact
    mb = pack_mask(m)
    ref = cell_head.greedy(logits, mb)
    assert int(ref[~m.any(-1)].sum()) == 0
    Xg, Wg, bg, mbg = X.to(cuda), W.to(cuda), b.to(cuda), mb.to(cuda)
    head = SparseHead(S, cuda)
    rng = torch.tensor([7, 5], dtype=torch.int64, device=cuda)
    a, lp = sparse_sample(Xg, Wg, bg, mbg, rng, head, greedy=True)
    assert int(rng[1]) == 6, "the step counter advances by one"
    assert torch.equal(a.cpu(), ref), "sorted path: greedy actions differ from cell_head.greedy"
    lp2, _ = sparse_score(Xg, Wg, bg, mbg, a, head)
    torch.testing.assert_close(lp, lp2, rtol=1e-5, atol=1e-4)
    rng2 = torch.tensor([991, 0], dtype=torch.int64, device=cuda)
    a2, lpb = sparse_sample(Xg, Wg, bg, mbg, rng2, head, greedy=True)
    assert torch.equal(a2, a) and torch.equal(lpb, lp), "greedy must not depend on the seed"
    assert int(rng2[1]) == 1
    # a sampled step with the same weights differs somewhere
    a3, _ = sparse_sample(Xg, Wg, bg, mbg, rng2, head)
    assert not torch.equal(a3, a)
    # bucketed paths: head_units + head_fwd, and head_fwd deriving its units from the counts
    for counts in (False, True):
        _fill_buckets(head, m, F)
        ab = torch.zeros(F, S, 7, dtype=torch.uint8, device=cuda)
        lb = torch.empty(F, device=cuda)
        a16 = torch.zeros(F, S, dtype=torch.int16, device=cuda) if counts else None
        rng3 = torch.tensor([31 + counts, 9], dtype=torch.int64, device=cuda)
        sparse_sample(Xg, Wg, bg, mbg, rng3, head, action_out=ab, logp_out=lb, prepacked=True,
                      bucketed=True, act16_out=a16, greedy=True)
        torch.cuda.synchronize()
        assert int(rng3[1]) == 10
        assert torch.equal(ab.cpu(), ref), f"bucketed path (counts={counts}): actions differ"
        torch.testing.assert_close(lb, lp2, rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------ B: random-normal bf16
def test_sparse_head_greedy_near_max_bf16(cuda):
    F, S = 500, 256
    g = torch.Generator().manual_seed(3)
    X = (torch.randn(F, 256, generator=g) * 0.5).bfloat16()
    W = torch.randn(S * 78, 256, generator=g) * 0.05
    b = torch.randn(S * 78, generator=g) * 0.1
    active = torch.rand(F, S, generator=g) < 0.08
    m = (torch.rand(F, S, 78, generator=g) < 0.5) & active[..., None]
    m[..., 0] |= active
    head = SparseHead(S, cuda)
    rng = torch.tensor([7, 0], dtype=torch.int64, device=cuda)
    a, _ = sparse_sample(X.to(cuda), W.to(cuda), b.to(cuda), pack_mask(m).to(cuda), rng, head,
                         greedy=True)
    a = a.cpu().long()
    # fp32 oracle on the same bf16-rounded operands
    z = (X.float() @ W.bfloat16().float().T + b).view(F, S, 78)
    assert int(a[~m.any(-1)].sum()) == 0
    worst = 0.0
    for k in range(7):
        seg, zs = m[..., OFFS[k]:OFFS[k + 1]], z[..., OFFS[k]:OFFS[k + 1]]
        has = seg.any(-1)
        ak = a[..., k:k + 1]
        assert bool((seg.gather(-1, ak).squeeze(-1) | ~has).all()), "illegal greedy action"
        assert int(a[..., k][~has].sum()) == 0
        mx = torch.where(seg, zs, torch.full_like(zs, -float("inf"))).max(-1).values
        gap = (mx - zs.gather(-1, ak).squeeze(-1))[has]
        worst = max(worst, float(gap.max()))
    print(f"largest gap to the segment's legal maximum: {worst:.3e}")
    assert worst <= 2e-3


# ------------------------------------------------------------------ C: fused == graph, greedy
def _codes_stream(E, steps, seed):
    """Codes of E real 16x16 simulator envs over `steps` steps of random legal play."""
    from microbeast_amd.ops.cell_head import unpack_mask
    rt = N.runtime()
    S = 256
    env = rt.VecEnv(16, E, 300, seed, [0, 1, 2, 3, 5])
    obs = torch.zeros(E, S, dtype=torch.int32)
    mask = torch.zeros(E, S, 3, dtype=torch.int32)
    env.reset(obs.data_ptr(), mask.data_ptr())
    codes = torch.zeros(E, S, dtype=torch.int16)
    res = torch.zeros(E, dtype=torch.int32)
    rew, done = torch.zeros(E), torch.zeros(E, dtype=torch.uint8)
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(steps):
        env.obs_codes(codes.data_ptr(), res.data_ptr())
        out.append((codes.clone(), res.clone()))
        mb = unpack_mask(mask)
        a = torch.zeros(E, S, 7, dtype=torch.uint8)
        for k in range(7):
            seg = mb[..., OFFS[k]:OFFS[k + 1]].float() + 1e-6
            a[..., k] = torch.multinomial(seg.view(-1, seg.shape[-1]), 1,
                                          generator=gen).view(E, S)
        env.step(a.data_ptr(), obs.data_ptr(), mask.data_ptr(), rew.data_ptr(), done.data_ptr())
    return out


def _model(cuda, seed):
    from microbeast_amd.models.agent import Agent
    torch.manual_seed(seed)
    m = Agent((16, 16, 27))
    torch.nn.init.normal_(m.actor.weight, std=0.05)  # a non-uniform policy
    torch.nn.init.normal_(m.actor.bias, std=0.5)
    m = m.to(cuda).eval()
    m.pack_inference(cuda)
    return m


@pytest.mark.parametrize("E,sparse", [(96, False), (200, True)])
def test_fused_greedy_step_equals_graph_step(cuda, E, sparse):
    from microbeast_amd.ops.act import ActWorkspace, code_lists, dense_actions
    from microbeast_amd.runtime.gpu_actors import graph_policy_step, make_io

    S = 256
    m = _model(cuda, 3)
    rng_a = torch.tensor([12345, 7], dtype=torch.int64, device=cuda)   # graph step
    rng_b = torch.tensor([999, 7], dtype=torch.int64, device=cuda)     # fused step: other seed
    rng_c = torch.tensor([12345, 7], dtype=torch.int64, device=cuda)   # sampled graph step
    io, io_s = make_io(E, S, cuda), make_io(E, S, cuda)
    ws = ActWorkspace(m, E, rng_b, cuda)
    obs = torch.empty(E, S, dtype=torch.int32, device=cuda)
    mask = torch.empty(E, S, 3, dtype=torch.int32, device=cuda)
    action = torch.full((E, S, 7), 0xAB, dtype=torch.uint8, device=cuda)
    logp = torch.full((E,), float("nan"), device=cuda)
    value = torch.full((E,), float("nan"), device=cuda)
    act16 = torch.full((E, S), -1, dtype=torch.int16, device=cuda)
    stride = S + 4
    act_list = torch.full((E, stride), -1, dtype=torch.int32, device=cuda)
    differs = n_active = 0
    for i, (codes, res) in enumerate(_codes_stream(E, 8, seed=E)):
        io["in_codes"].copy_(codes)
        io["in_res"].copy_(res)
        graph_policy_step(io, m, rng_a, E, 16, cuda, greedy=True)
        if sparse:
            cl = code_lists(codes, res, stride)
            cl = cl.pin_memory() if i % 2 == 1 else cl.to(cuda)
            ws.step(None, None, obs, mask, action, logp, value, None, code_list=cl,
                    act_list=act_list, greedy=True)
            torch.cuda.synchronize()
            act16 = dense_actions(act_list, S).to(cuda)
        else:
            ws.step(io["in_codes"], io["in_res"], obs, mask, action, logp, value, act16,
                    greedy=True)
        torch.cuda.synchronize()
        assert torch.equal(mask, io["in_mask"]) and torch.equal(obs, io["in_obs"])
        assert torch.equal(action, io["out_action"]), f"actions differ at step {i}"
        assert torch.equal(act16, io["out_act16"]), f"packed actions differ at step {i}"
        assert torch.equal(logp.view(torch.int32), io["out_logp"].view(torch.int32)), \
            f"log-probs differ at step {i}"
        assert torch.equal(value.view(torch.int32), io["out_value"].view(torch.int32)), \
            f"values differ at step {i}"
        assert int(rng_a[1]) == int(rng_b[1]) == 8 + i, "step counter"
        assert int(ws.pending[:E].abs().sum()) == 0
        # the greedy actions are the arg-max of the dense logits' legal entries where those
        # are not within rounding of a tie: checked exactly in test_sparse_head_greedy_exact;
        # here: legal, and different from a sampled step of the same weights somewhere
        io_s["in_codes"].copy_(codes)
        io_s["in_res"].copy_(res)
        graph_policy_step(io_s, m, rng_c, E, 16, cuda)
        torch.cuda.synchronize()
        differs += int((io_s["out_action"] != action).sum())
        n_active += int((mask != 0).any(-1).sum())
    assert n_active > 0, "no active cell in 8 steps: the head never acted"
    assert differs > 0, "greedy steps equal sampled steps everywhere"


# ------------------------------------------------------------------ D: masked-cell kernels
def _tied_logits(n, S, ld, seed):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, S, ld, generator=g).bfloat16().float()   # exact in both dtypes
    for j in (0, 3, 7, 12, 23, 24, 29, 30, 50, 76):
        z[:, ::2, j + 1] = z[:, ::2, j]
    m = torch.rand(n, S, 78, generator=g) < 0.4
    m &= (torch.rand(n, S, generator=g) < 0.3)[..., None]       # sparse active cells
    m[0, 0] = True
    m[1, 1, :] = False
    m[1, 1, 23], m[1, 1, 24] = True, True                       # tied pair only
    return z, m


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_masked_cell_greedy_dense(cuda, dtype):
    n, S = 7, 100  # 700 cells: not a multiple of the 64-cell block
    z, m = _tied_logits(n, S, 78, 1)
    logits = z.reshape(n, S * 78).to(dtype).to(cuda)
    mb = pack_mask(m).to(cuda)
    rng = torch.tensor([3, 4], dtype=torch.int64, device=cuda)
    a, lp = cell_head.sample_gpu(logits, mb, rng, greedy=True)
    assert int(rng[1]) == 5
    assert torch.equal(a.cpu(), cell_head.greedy(logits.cpu(), mb.cpu()))
    lp0, _ = cell_head.score(logits, mb, a)   # mode 0 on those actions
    assert torch.equal(lp, lp0)
    a2, _ = cell_head.sample(logits, mb, torch.tensor([77, 0], dtype=torch.int64, device=cuda),
                             greedy=True)
    assert torch.equal(a2, a)


def test_masked_cell_greedy_pixel_major_and_rows(cuda):
    from microbeast_amd.ops import pixconv as pc
    n, S, ld = 7, 100, pc.LOGIT_LD
    z, m = _tied_logits(n, S, ld, 2)
    lg = z.permute(1, 0, 2).contiguous().bfloat16().to(cuda)     # [S][n][ld]
    mb = pack_mask(m).to(cuda)
    cm = z[..., :78].reshape(n, S * 78)
    ref = cell_head.greedy(cm, mb.cpu())
    rng = torch.tensor([3, 4], dtype=torch.int64, device=cuda)
    a, lp = cell_head.sample_pbc(lg, mb, rng, greedy=True)
    assert int(rng[1]) == 5
    assert torch.equal(a.cpu(), ref)
    lp0, _ = cell_head.score_pbc(lg, mb, a)
    assert torch.equal(lp, lp0)
    cells = pc.Cells(mb, n, S)
    nact = int(cells.totals[0])
    rc = cells.rowcell[:nact].long()
    Zc = torch.zeros(cells.cap, ld, dtype=torch.bfloat16, device=cuda)
    Zc[:nact] = lg.permute(1, 0, 2).reshape(n * S, -1)[rc]
    ar, lpr = cell_head.sample_rows(Zc, cells, mb, rng, greedy=True)
    assert int(rng[1]) == 6
    assert torch.equal(ar.cpu(), ref)
    lpr0, _ = cell_head.score_rows(Zc, cells, mb, ar)
    assert torch.equal(lpr, lpr0)
