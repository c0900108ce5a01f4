"""PPO row-block minibatches and target-KL early stopping on the MI355X: ppo.hip's
mbk_adv_stats_rows / mbk_ppo_loss_rows against the fp32 torch oracle per block, bit
reproducibility, the running epoch mean, the HIP learner's two block steps against the fp32 CPU
learner on a real engine rollout, the stop rule on the device and the CLI on the GPU runtime."""
import copy
import csv
import os

import pytest
import torch

from microbeast_amd.ops import ppo as P
from microbeast_amd.ops.vtrace import VTraceWorkspace
from ppo_cases import BC, CLIP, EC, GAMMA, LAM, VCLIP, autograd_oracle, recipe

pytestmark = pytest.mark.gpu

KW = dict(clip=CLIP, baseline_cost=BC, entropy_cost=EC)


def _run_gpu(c, cuda, ws, K, norm=True, value_clip=VCLIP, order=None):
    """GAE, the K stats pairs and one epoch of block losses (in ``order``) on the device;
    per step: (k, g_logp, g_value, losses) cloned, and the epoch mean after the last."""
    d = {k: v.to(cuda) for k, v in c.items()}
    T = c["lpn"].shape[0]
    Tm = T // K
    g = P.gae(d["v_old"], d["rew"], d["done"], GAMMA, LAM, norm_adv=norm, ws=ws)
    stats = P.adv_stats_rows(g.adv, K, norm, ws=ws)
    steps, mean = [], None
    for j, k in enumerate(order if order is not None else range(K)):
        r = slice(k * Tm, (k + 1) * Tm)
        o = P.ppo_loss_rows(d["lpn"][r], d["lpo"], d["values"][r], d["v_old"], g.adv, g.ret,
                            stats[k], k * Tm, d["ent"][r], value_clip=value_clip, step=j,
                            epoch_mean=mean, ws=ws, **KW)
        mean = o.epoch_mean
        assert o.g_ent == -EC / (Tm * c["lpn"].shape[1])
        steps.append((k, o.g_logp.clone(), o.g_value.clone(), o.losses.clone()))
    return g, stats, steps, mean


def _check(c, cuda, ws, K, norm=True, value_clip=VCLIP):
    """Per block against the fp32 torch oracle at tests/test_gpu_ppo.py::_check's tolerances;
    the gradients are compared away from their branch boundaries (fp64 margins below 1e-4 are
    left out, at most 0.5 % of a block's elements)."""
    T, B = c["lpn"].shape
    Tm = T // K
    M = Tm * B
    rg = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM, norm_adv=norm)
    rstats = P.adv_stats_rows_torch(rg.adv, K, norm)
    g, stats, steps, mean = _run_gpu(c, cuda, ws, K, norm, value_clip)
    adv, st = g.adv.cpu(), stats.cpu()
    assert st.shape == (K, 2)
    torch.testing.assert_close(adv, rg.adv, rtol=1e-4, atol=1e-4)
    if not norm:
        assert st.tolist() == [[0.0, 1.0]] * K
    for k, gl, gv, lg in steps:
        t0 = k * Tm
        r = slice(t0, t0 + Tm)
        torch.testing.assert_close(st[k], rstats[k], rtol=1e-4, atol=1e-5)
        torch.testing.assert_close((adv[r] - st[k, 0]) * st[k, 1],
                                   (rg.adv[r] - rstats[k, 0]) * rstats[k, 1], rtol=1e-4, atol=1e-4)
        ro = P.ppo_loss_rows_torch(c["lpn"][r], c["lpo"], c["values"][r], c["v_old"], rg.adv,
                                   rg.ret, rstats[k], t0, c["ent"][r], value_clip=value_clip, **KW)
        blk = dict(lpn=c["lpn"][r], lpo=c["lpo"][r], ent=c["ent"][r],
                   values=torch.cat([c["values"][r], c["v_old"][t0 + Tm:t0 + Tm + 1]]),
                   v_old=c["v_old"][t0:t0 + Tm + 1])
        f64 = autograd_oracle(blk, rg.adv[r], rg.ret[r], rstats[k], value_clip=value_clip)
        keep = (f64["m_ratio"] > 1e-4) & (f64["m_value"] > 1e-4)
        left = int((~keep).sum())
        print(f"T={T} B={B} K={K} block {k} norm={norm} value_clip={value_clip}: left out {left} "
              f"of {M}; losses gpu {lg.tolist()} ref {ro.losses.tolist()}")
        assert left <= 0.005 * M
        gl, gv, lg = gl.cpu(), gv.cpu(), lg.cpu()
        assert gl.shape == (Tm, B) and gv.shape == (Tm, B)
        torch.testing.assert_close(gl[keep], ro.g_logp[keep], rtol=1e-4, atol=1e-8)
        torch.testing.assert_close(gv[keep], ro.g_value[keep], rtol=1e-4, atol=1e-8)
        torch.testing.assert_close(lg[:6], ro.losses[:6], rtol=1e-4, atol=1e-5)
        assert abs(float(lg[6]) - float(ro.losses[6])) <= left / M + 1e-6
    # the epoch mean the finalize kernel keeps is the mean of the K per-step losses
    torch.testing.assert_close(mean.cpu(), torch.stack([s[3].cpu() for s in steps]).mean(0),
                               rtol=1e-6, atol=1e-6)
    return g, stats, steps, mean


@pytest.mark.parametrize("T,B,K,norm,value_clip", [
    (12, 300, 3, True, VCLIP),   # vector path, two blocks per minibatch, partial block and wave
    (6, 259, 2, True, VCLIP),    # B % 4 != 0: the scalar path
    (2, 1, 2, True, VCLIP),
    (12, 300, 3, False, VCLIP),  # normalisation off: every pair exactly (0, 1)
    (12, 300, 3, True, 0.0),     # plain (v - R)^2
])
def test_row_block_kernels_vs_torch(cuda, T, B, K, norm, value_clip):
    _check(recipe(T, B), cuda, VTraceWorkspace(), K, norm, value_clip)


def test_one_block_stats_agree_with_gae(cuda):
    """K = 1: the same statistics as mbk_gae's, through another merge tree."""
    c = recipe(12, 300)
    ws = VTraceWorkspace()
    g, stats, _, _ = _run_gpu(c, cuda, ws, 1)
    torch.testing.assert_close(stats[0], g.stats, rtol=1e-4, atol=1e-5)


def test_row_block_kernels_are_bit_reproducible(cuda):
    c = recipe(12, 300)
    ws = VTraceWorkspace()

    def snap():
        g, stats, steps, mean = _run_gpu(c, cuda, ws, 3, order=[2, 0, 1])
        out = [stats.clone(), mean.clone()]
        for _, gl, gv, lg in steps:
            out += [gl, gv, lg]
        return out

    a, b = snap(), snap()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # the same workspace at another shape (buffers re-sized), then back
    _check(recipe(6, 259), cuda, ws, 2)
    assert all(torch.equal(x, y) for x, y in zip(a, snap()))


def test_epoch_mean_restarts_at_step_zero(cuda):
    """Two epochs through one workspace: step 0 of the second overwrites the first's mean."""
    c = recipe(12, 300)
    ws = VTraceWorkspace()
    for order in ([0, 1, 2], [1, 2, 0]):
        _, _, steps, mean = _run_gpu(c, cuda, ws, 3, order=order)
        torch.testing.assert_close(mean.cpu(), torch.stack([s[3].cpu() for s in steps]).mean(0),
                                   rtol=1e-6, atol=1e-6)


# ----------------------------------------------------------------------------- learner
def _models():
    from microbeast_amd.models.agent import Agent
    S = 8
    torch.manual_seed(7)
    base = Agent((S, S, 27))
    with torch.no_grad():
        base.actor.weight.normal_(0, 0.02)
        base.actor.bias.normal_(0, 0.02)
    hip_model = copy.deepcopy(base)
    ref_model = copy.deepcopy(base)
    ref_model.hip_kernels = False
    ref_model.compute_dtype = torch.float32
    bf_model = copy.deepcopy(base)
    bf_model.hip_kernels = False  # torch ops under bf16 autocast on the GPU
    return hip_model, ref_model, bf_model


@pytest.fixture(scope="module")
def engine_batch(cuda):
    from helpers import engine_batches
    return engine_batches(cuda, 8, 2, groups=4, envs=64, T=8, seed=8)[1]


def step_losses(monkeypatch, learner, batch):
    """one learn(); the losses [7] of each optimiser step (host)"""
    from microbeast_amd import learner as learner_mod
    real = P.ppo_loss_rows
    seen = []

    def hook(*a, **k):
        o = real(*a, **k)
        seen.append(o.losses.clone())
        return o

    monkeypatch.setattr(learner_mod, "ppo_loss_rows", hook)
    out = learner.learn(batch)
    monkeypatch.setattr(learner_mod, "ppo_loss_rows", real)
    return [s.cpu() for s in seen], out.cpu()


# Step 1's floor: the largest entry of |torch-bf16 learner - fp32 learner| over step 1's seven
# losses on this batch (the torch path under bf16 autocast on the GPU, as
# tests/test_gpu_learner_parity.py builds it), measured once on one MI355X.
STEP1_FLOOR = 4.46e-6


def test_minibatch_learner_hip_matches_fp32_torch(cuda, engine_batch, monkeypatch):
    """K = 2, E = 1, blocks in order: the HIP learner against the fp32 CPU learner from the same
    weights on one engine rollout of 64 envs x T = 8 (set up as
    tests/test_gpu_ppo.py::test_ppo_learner_hip_matches_fp32_torch). Step 0's seven losses are
    within that test's rtol 2e-2 / atol 2e-3 (measured: <= 5.4e-5 on every entry). Step 1 starts
    from weights that already differ by one bf16-against-fp32 step, so its bound is measured:
    twice the floor, and the floor is the largest entry of |torch-bf16 learner - fp32 learner|
    over step 1's losses on the same batch. Measured per entry (pg, value, entropy, total, mean
    ratio, approx_kl, clip_frac):
      floor |bf16 - fp32|  4.46e-6  6.13e-7  2.2e-8  3.85e-6  3.6e-7  0       0
      HIP   |hip  - fp32|  3.10e-6  1.44e-6  4.8e-8  1.65e-6  8.3e-7  7.1e-8  0
    so the floor is 4.46e-6, the bound 8.92e-6 and the HIP value (its largest entry) 3.10e-6.
    The bound is one number for the seven losses, not one per entry: an entry's own torch-bf16
    deviation is a single draw that can be a few fp32 roundings of the loss or exactly 0 (the
    last three here), and the HIP learner is a few roundings off there as well."""
    from microbeast_amd.learner import Learner, LearnerHParams
    hip_model, ref_model, _ = _models()
    hp = LearnerHParams(algo="ppo", ppo_epochs=1, ppo_minibatches=2, ppo_shuffle=False)
    Lh = Learner(hip_model, hp, cuda)
    Lr = Learner(ref_model, hp, torch.device("cpu"))
    flat0 = Lr.flat.data.clone()
    assert torch.equal(Lh.flat.data.cpu(), flat0)
    sh, mh = step_losses(monkeypatch, Lh, engine_batch)
    sr, mr = step_losses(monkeypatch, Lr, {k: v.cpu() for k, v in engine_batch.items()})
    assert len(sh) == len(sr) == 2 and Lh.opt.step_count == 2 == Lh.last_opt_steps
    assert Lh.n_updates == 1 and not torch.equal(Lh.flat.data.cpu(), flat0)
    for j in range(2):
        print(f"step {j}: hip {sh[j].tolist()}\n        ref {sr[j].tolist()}\n"
              f"        |hip - ref| {(sh[j] - sr[j]).abs().tolist()}")
    assert all(torch.isfinite(x).all() for x in sh)
    torch.testing.assert_close(sh[0], sr[0], rtol=2e-2, atol=2e-3)
    torch.testing.assert_close(mh, torch.stack(sh).mean(0), rtol=1e-6, atol=1e-6)
    assert float((sh[1] - sr[1]).abs().max()) <= 2.0 * STEP1_FLOOR


def test_stop_rule_on_the_device(cuda, engine_batch):
    from microbeast_amd.learner import Learner, LearnerHParams
    b = dict(engine_batch)
    for target, steps in ((1e9, 4), (1e-12, 1)):
        hip_model = _models()[0]
        L = Learner(hip_model, LearnerHParams(algo="ppo", ppo_epochs=2, ppo_minibatches=2,
                                              ppo_target_kl=target), cuda)
        start = L.flat.data.clone()
        losses = L.learn(b).cpu()
        print(f"target_kl {target}: steps {L.last_opt_steps}, losses {losses.tolist()}")
        # the behaviour log-probs come from the bf16 acting kernels: step 0's KL is not zero
        # (K = 2: after one step the returned epoch mean is step 0's own losses)
        assert steps == 4 or float(losses[5]) > 1e-12
        assert L.opt.step_count == steps == L.last_opt_steps and L.n_updates == 1
        assert not torch.equal(L.flat.data, start)


def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def test_gpu_cli_minibatch_train_and_eval(cuda, tmp_path):
    from microbeast_amd.cli import main
    from microbeast_amd.utils.checkpoint import load_checkpoint
    from microbeast_amd.utils.metrics import LOSS_HEADER
    args = ["--exp_name", "p", "--runtime", "gpu", "--env_size", "8", "--groups", "2",
            "--envs_per_group", "32", "--unroll_length", "8", "--batch_size", "1",
            "--savedir", str(tmp_path), "--quiet", "--max_episode_steps", "10"]
    assert main(args + ["--algo", "ppo", "--ppo_minibatches", "2", "--ppo_epochs", "2",
                        "--max_updates", "3"]) == 0
    ck = load_checkpoint(os.path.join(tmp_path, "p.ckpt"))
    assert ck["n_update"] == 3 and ck["optimizer_state_dict"]["step"] == 12
    with open(tmp_path / "pLosses.csv") as f:
        assert f.readline().strip().split(",") == LOSS_HEADER + ["approx_kl", "clip_frac",
                                                                 "opt_steps"]
    loss = _rows(tmp_path / "pLosses.csv")
    assert [int(r["update"]) for r in loss] == [1, 2, 3]
    for r in loss:
        assert int(r["opt_steps"]) == 4
        for k in ("pg_loss", "value_loss", "entropy_loss", "total_loss", "mean_rho", "approx_kl",
                  "clip_frac"):
            v = float(r[k])
            assert v == v and abs(v) < 1e9, (k, r)
    assert main(args + ["--test", "--eval_envs", "16"]) == 0
    assert len(_rows(tmp_path / "p_eval.csv")) == 16
