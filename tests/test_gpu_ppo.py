"""PPO on the MI355X: ppo.hip (mbk_gae, mbk_ppo_loss) against the fp32 torch oracle, bit
reproducibility, the HIP PPO learner against the fp32 CPU learner on a real engine rollout, and
``--algo ppo`` end to end on the GPU runtime. (Reference: none -- its PPO_learn is V-trace and
its GAE helpers are dead code, libs/utils.py:104-163, 277-329.)"""
import copy
import csv
import os

import pytest
import torch

from microbeast_amd.ops import ppo as P
from microbeast_amd.ops.vtrace import VTraceWorkspace
from ppo_cases import BC, CLIP, EC, GAMMA, LAM, VCLIP, autograd_oracle, recipe

pytestmark = pytest.mark.gpu


def _run_gpu(c, cuda, ws, norm=True, value_clip=VCLIP, reward_clip=0.0):
    d = {k: v.to(cuda) for k, v in c.items()}
    g = P.gae(d["v_old"], d["rew"], d["done"], GAMMA, LAM, reward_clip=reward_clip, norm_adv=norm,
              ws=ws)
    o = P.ppo_loss(d["lpn"], d["lpo"], d["values"], d["v_old"], g.adv, g.ret, g.stats, d["ent"],
                   clip=CLIP, value_clip=value_clip, baseline_cost=BC, entropy_cost=EC, ws=ws)
    return g, o


def _check(c, cuda, ws, norm=True, value_clip=VCLIP, reward_clip=0.0):
    """Kernels vs the fp32 torch oracle at the V-trace kernel test's tolerances; the two
    gradients are compared away from their branch boundaries (fp64 margins below 1e-4 are left
    out, at most 0.5 % of the elements)."""
    T, B = c["lpn"].shape
    M = T * B
    rg = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM, reward_clip=reward_clip,
                     norm_adv=norm)
    ro = P.ppo_loss_torch(c["lpn"], c["lpo"], c["values"], c["v_old"], rg.adv, rg.ret, rg.stats,
                          c["ent"], clip=CLIP, value_clip=value_clip, baseline_cost=BC,
                          entropy_cost=EC)
    g, o = _run_gpu(c, cuda, ws, norm, value_clip, reward_clip)
    adv, ret, stats = g.adv.cpu(), g.ret.cpu(), g.stats.cpu()
    torch.testing.assert_close(adv, rg.adv, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(ret, rg.ret, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close((adv - stats[0]) * stats[1], (rg.adv - rg.stats[0]) * rg.stats[1],
                               rtol=1e-4, atol=1e-4)
    if not norm:
        assert stats.tolist() == [0.0, 1.0]
    f64 = autograd_oracle(c, rg.adv, rg.ret, rg.stats, value_clip=value_clip)
    keep = (f64["m_ratio"] > 1e-4) & (f64["m_value"] > 1e-4)
    left = int((~keep).sum())
    print(f"T={T} B={B} norm={norm} value_clip={value_clip}: left out {left} of {M}; "
          f"losses gpu {o.losses.tolist()} ref {ro.losses.tolist()}")
    assert left <= 0.005 * M
    gl, gv = o.g_logp.cpu(), o.g_value.cpu()
    assert gl.shape == (T, B) and gv.shape == (T + 1, B)
    torch.testing.assert_close(gl[keep], ro.g_logp[keep], rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(gv[:T][keep], ro.g_value[:T][keep], rtol=1e-4, atol=1e-8)
    assert float(gv[T].abs().max()) == 0.0
    lg = o.losses.cpu()
    torch.testing.assert_close(lg[:6], ro.losses[:6], rtol=1e-4, atol=1e-5)
    assert abs(float(lg[6]) - float(ro.losses[6])) <= left / M + 1e-6
    assert o.g_ent == -EC / M
    return g, o


@pytest.mark.parametrize("T,B,done_row,norm,value_clip", [
    (37, 300, None, True, VCLIP),   # two blocks, partial last block and wave, vector path + tail
    (5, 259, None, True, VCLIP),    # B % 4 != 0: scalar path, one lane in the second block
    (1, 1, None, True, VCLIP),
    (37, 300, 11, True, VCLIP),     # one done row all ones
    (37, 300, None, False, VCLIP),  # normalisation off: stats = (0, 1)
    (37, 300, None, True, 0.0),     # plain (v - R)^2
])
def test_ppo_kernels_vs_torch(cuda, T, B, done_row, norm, value_clip):
    _check(recipe(T, B, done_row), cuda, VTraceWorkspace(), norm, value_clip)


def test_gae_kernel_reward_clip(cuda):
    """mbk_gae's reward clamp against gae_torch(reward_clip=0.5) (about 62 % of the unit-normal
    rewards are clipped; on the CPU the fp64 margins of this recipe leave out 20 of the 11100
    elements, 0.18 %, inside the 0.5 % cap), and a clip above every |r| bit-equal to no clip."""
    c = recipe(37, 300)
    assert 0.5 < float((c["rew"].abs() > 0.5).float().mean()) < 0.7
    g, o = _check(c, cuda, VTraceWorkspace(), reward_clip=0.5)
    g0, o0 = _run_gpu(c, cuda, VTraceWorkspace())
    assert not torch.equal(g.adv, g0.adv)
    big = float(c["rew"].abs().max()) * 1.5
    g1, o1 = _run_gpu(c, cuda, VTraceWorkspace(), reward_clip=big)
    for a, b in zip((g1.adv, g1.ret, g1.stats, o1.g_logp, o1.g_value, o1.losses),
                    (g0.adv, g0.ret, g0.stats, o0.g_logp, o0.g_value, o0.losses)):
        assert torch.equal(a, b)


def test_ppo_kernels_are_bit_reproducible(cuda):
    c = recipe(37, 300)
    snaps = []
    ws = VTraceWorkspace()
    for _ in range(2):
        g, o = _run_gpu(c, cuda, ws)
        snaps.append([t.clone() for t in (o.g_logp, o.g_value, g.stats, o.losses, g.adv, g.ret)])
    for a, b in zip(*snaps):
        assert torch.equal(a, b)
    # the same workspace at another B (buffers re-sized), then back
    _check(recipe(5, 259), cuda, ws)
    g, o = _check(recipe(37, 300), cuda, ws)
    for a, b in zip(snaps[0], (o.g_logp, o.g_value, g.stats, o.losses, g.adv, g.ret)):
        assert torch.equal(a, b)


def test_ppo_learner_hip_matches_fp32_torch(cuda):
    """One PPO update (ppo_epochs=1) of the HIP learner against the fp32 CPU learner from the
    same weights on one engine rollout (models set up as tests/test_gpu_learner_parity.py):
    losses 0-4 within rtol 2e-2, atol 2e-3, what that test allows the V-trace losses on the
    same kind of batch. Measured on this batch: |hip - ref| <= 4.1e-6 on every entry (the
    torch-bf16 learner on the GPU, the floor that test uses: <= 5.7e-5), so the bound holds
    with a wide margin and is kept as set."""
    from helpers import engine_batches
    from microbeast_amd.learner import Learner, LearnerHParams
    from microbeast_amd.models.agent import Agent

    S = 8
    b_gpu = engine_batches(cuda, S, 2, groups=4, envs=64, T=8, seed=S)[1]
    torch.manual_seed(7)
    base = Agent((S, S, 27))
    with torch.no_grad():
        base.actor.weight.normal_(0, 0.02)
        base.actor.bias.normal_(0, 0.02)
    hip_model = copy.deepcopy(base)
    ref_model = copy.deepcopy(base)
    ref_model.hip_kernels = False
    ref_model.compute_dtype = torch.float32
    hp = LearnerHParams(algo="ppo", ppo_epochs=1)
    Lh = Learner(hip_model, hp, cuda)
    Lr = Learner(ref_model, hp, torch.device("cpu"))
    flat0 = Lr.flat.data.clone()
    assert torch.equal(Lh.flat.data.cpu(), flat0)
    lh = Lh.learn(b_gpu).cpu()
    lr = Lr.learn({k: v.cpu() for k, v in b_gpu.items()})
    print(f"losses hip {lh.tolist()}\nlosses ref {lr.tolist()}\n"
          f"|hip - ref| {(lh - lr).abs().tolist()}")
    assert lh.shape == (7,) and torch.isfinite(lh).all()
    torch.testing.assert_close(lh[:5], lr[:5], rtol=2e-2, atol=2e-3)
    assert Lh.opt.step_count == 1 and Lh.n_updates == 1
    assert not torch.equal(Lh.flat.data.cpu(), flat0)  # the update was applied


def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def test_gpu_cli_ppo_train_and_eval(cuda, tmp_path):
    from microbeast_amd.cli import main
    from microbeast_amd.utils.checkpoint import load_checkpoint
    from microbeast_amd.utils.metrics import LOSS_HEADER
    args = ["--exp_name", "p", "--runtime", "gpu", "--env_size", "8", "--groups", "2",
            "--envs_per_group", "32", "--unroll_length", "8", "--batch_size", "1",
            "--savedir", str(tmp_path), "--quiet", "--max_episode_steps", "10"]
    assert main(args + ["--algo", "ppo", "--ppo_epochs", "2", "--max_updates", "4",
                        "--checkpoint_every", "2"]) == 0
    ck = load_checkpoint(os.path.join(tmp_path, "p.ckpt"))
    assert ck["n_update"] == 4 and ck["step"] == 4 * 256
    assert ck["optimizer_state_dict"]["step"] == 8  # Adam steps once per epoch
    with open(tmp_path / "pLosses.csv") as f:
        assert f.readline().strip().split(",") == LOSS_HEADER + ["approx_kl", "clip_frac"]
    loss = _rows(tmp_path / "pLosses.csv")
    assert [int(r["update"]) for r in loss] == [1, 2, 3, 4]
    for r in loss:
        for k in ("pg_loss", "value_loss", "entropy_loss", "total_loss", "mean_rho", "approx_kl",
                  "clip_frac"):
            v = float(r[k])
            assert v == v and abs(v) < 1e9, (k, r)
        assert 0.0 <= float(r["clip_frac"]) <= 1.0 and int(r["policy_lag"]) >= 0
    assert all(float(r["fwd_ms"]) > 0 for r in loss[1:])  # both epochs' marks, summed
    assert main(args + ["--test", "--eval_envs", "16"]) == 0
    assert len(_rows(tmp_path / "p_eval.csv")) == 16
