"""V-trace-corrected PPO advantages on the MI355X: ppo.hip's mbk_vtrace_adv against the fp64
oracle (tests/ppo_vtrace_cases.py) in poisoned buffers, bit reproducibility, the on-policy
reduction to mbk_gae, the launcher's refusals, the HIP learner under ``ppo_adv="vtrace"``
against the fp32 CPU learner on a real engine rollout, and ``--ppo_adv vtrace`` end to end on
the GPU runtime."""
import copy
import csv
import os

import pytest
import torch

from microbeast_amd import _native as N
from microbeast_amd.ops import ppo as P
from microbeast_amd.ops.vtrace import VTraceWorkspace
from ppo_cases import GAMMA, LAM
from ppo_vtrace_cases import (SETTINGS, SHAPES, TOL, case, check_against_oracle, oracle_for,
                              settings)

pytestmark = pytest.mark.gpu

KEYS = ("ppo_vt_adv", "ppo_vt_ret", "ppo_vt_partials", "ppo_vt_stats", "ppo_vt_is_stats")


def _poison(ws, T, B, dev):
    """the scan's outputs and its partials pre-filled with NaN: every element must be written"""
    for key, shape in zip(KEYS, ((T, B), (T, B), (((B + 255) // 256) * 6,), (2,), (3,))):
        ws.get(key, shape, dev).fill_(float("nan"))


def _run(c, cuda, ws, s, pi="lpn"):
    d = {k: v.to(cuda) for k, v in c.items()}
    T, B = c["rew"].shape
    _poison(ws, T, B, cuda)
    return P.vtrace_adv(d[pi], d["lpo"], d["v_old"], d["rew"], d["done"], ws=ws, **s)


@pytest.mark.parametrize("name", list(SETTINGS))
@pytest.mark.parametrize("shape", SHAPES)
def test_vtrace_adv_kernel_vs_oracle(cuda, shape, name):
    """(37, 300): two blocks, a partial block and a partial wave; (5, 259): one lane in the
    second block; (1, 1); a done row; all dones."""
    c, o = oracle_for(shape, name)
    s = settings(name)
    ws = VTraceWorkspace()
    g, is_stats = _run(c, cuda, ws, s)
    assert g.adv.shape == c["rew"].shape and g.adv.dtype == torch.float32
    for t in (g.adv, g.ret, g.stats, is_stats, ws.get("ppo_vt_partials",
                                                      (((shape[1] + 255) // 256) * 6,), cuda)):
        assert torch.isfinite(t).all()
    check_against_oracle(g, is_stats, o, s["norm_adv"])


def test_vtrace_adv_kernel_is_bit_reproducible(cuda):
    c = case(37, 300)
    s = settings("mixed")
    ws = VTraceWorkspace()
    snaps = []
    for _ in range(2):
        g, is_stats = _run(c, cuda, ws, s)
        snaps.append([t.clone() for t in (g.adv, g.ret, g.stats, is_stats)])
    for a, b in zip(*snaps):
        assert torch.equal(a, b)
    # the same workspace at another B (buffers re-sized), then back
    c2, o2 = oracle_for(SHAPES[1], "mixed")
    check_against_oracle(*_run(c2, cuda, ws, s), o2, True)
    g, is_stats = _run(c, cuda, ws, s)
    for a, b in zip(snaps[0], (g.adv, g.ret, g.stats, is_stats)):
        assert torch.equal(a, b)
    # keys of its own: gae's outputs in the same workspace are untouched by the scan
    d = {k: v.to(cuda) for k, v in c.items()}
    ga = P.gae(d["v_old"], d["rew"], d["done"], GAMMA, LAM, ws=ws)
    keep = [t.clone() for t in (ga.adv, ga.ret, ga.stats)]
    _run(c, cuda, ws, s)
    for a, b in zip(keep, (ga.adv, ga.ret, ga.stats)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("shape", SHAPES[:4])
@pytest.mark.parametrize("bars", [1.0, 1e9])
def test_on_policy_scan_matches_gae_kernel(cuda, shape, bars):
    """logp_pi == logp_mu, bars >= 1: mbk_gae's outputs at the oracle checks' tolerance (the two
    kernels may contract their multiply-adds differently, so bit equality is not required)."""
    c = case(*shape)
    ws = VTraceWorkspace()
    s = {**settings("defaults"), "rho_bar": bars, "c_bar": bars}
    g, is_stats = _run(c, cuda, ws, s, pi="lpo")
    d = {k: v.to(cuda) for k, v in c.items()}
    ref = P.gae(d["v_old"], d["rew"], d["done"], GAMMA, LAM, ws=ws)
    torch.testing.assert_close(g.adv, ref.adv, rtol=TOL, atol=TOL)
    torch.testing.assert_close(g.ret, ref.ret, rtol=TOL, atol=TOL)
    torch.testing.assert_close((g.adv - g.stats[0]) * g.stats[1],
                               (ref.adv - ref.stats[0]) * ref.stats[1], rtol=TOL, atol=TOL)
    assert is_stats.tolist() == [1.0, 0.0, 0.0]
    print(f"{shape} bars {bars}: bit-equal adv {torch.equal(g.adv, ref.adv)} "
          f"ret {torch.equal(g.ret, ref.ret)} stats {torch.equal(g.stats, ref.stats)}")


def test_launcher_refusals(cuda):
    c = case(5, 259)
    d = {k: v.to(cuda) for k, v in c.items()}
    ws = VTraceWorkspace()
    for bars in (dict(rho_bar=0.0), dict(c_bar=-1.0), dict(rho_bar=float("nan"))):
        with pytest.raises(RuntimeError, match="vtrace_adv failed with hipError 1$"):
            P.vtrace_adv(d["lpn"], d["lpo"], d["v_old"], d["rew"], d["done"], ws=ws,
                         **{**settings("defaults"), **bars})
    # T = 0, B = 0: refused before any launch (no pointer is read)
    x = torch.zeros(8, device=cuda)
    p = x.data_ptr()
    for T, B in ((0, 4), (4, 0), (-1, 4)):
        rc = N.kernels().mbk_vtrace_adv(p, p, p, p, p, T, B, 0.99, 0.95, 1.0, 1.0, 0.0, 1, p, p,
                                        p, p, p, N.stream_ptr())
        assert rc == 1  # hipErrorInvalidValue
    torch.cuda.synchronize()


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
    return hip_model, ref_model


@pytest.fixture(scope="module")
def lagged_batch(cuda):
    """tests/test_gpu_ppo.py::test_ppo_learner_hip_matches_fp32_torch's engine rollout with the
    behaviour log-probs perturbed by a seeded N(0, 0.2): ratios well off 1"""
    from helpers import engine_batches
    b = engine_batches(cuda, 8, 2, groups=4, envs=64, T=8, seed=8)[1]
    noise = 0.2 * torch.randn(b["logp"].shape, generator=torch.Generator().manual_seed(11))
    b["logp"] = b["logp"] + noise.to(cuda)
    return b


def test_vtrace_learner_hip_matches_fp32_torch(cuda, lagged_batch):
    """One ``ppo_adv="vtrace"`` update (ppo_epochs=1) of the HIP learner against the fp32 CPU
    learner from the same weights on the lagged engine rollout: losses 0-4 within
    tests/test_gpu_ppo.py's rtol 2e-2 / atol 2e-3 and the importance statistics within 1e-3; the
    same batch under ``gae`` gives a pg or value loss further away than that bound, so the mode
    is shown to act. The measured |hip - ref| is printed, never used as a bound. Measured once
    on one MI355X: |hip - ref| <= 4.2e-6 on every loss and on mean w, 0 on the two shares
    (0.515625 each); value loss 0.10448 under ``vtrace`` against 0.13049 under ``gae``."""
    from microbeast_amd.learner import Learner, LearnerHParams
    cpu_batch = {k: v.cpu() for k, v in lagged_batch.items()}
    out = {}
    for mode in ("vtrace", "gae"):
        hip_model, ref_model = _models()
        hp = LearnerHParams(algo="ppo", ppo_epochs=1, ppo_adv=mode)
        Lh = Learner(hip_model, hp, cuda)
        Lr = Learner(ref_model, hp, torch.device("cpu"))
        flat0 = Lr.flat.data.clone()
        assert torch.equal(Lh.flat.data.cpu(), flat0)
        out[mode] = (Lh.learn(lagged_batch).cpu(), Lr.learn(cpu_batch), Lh, Lr)
        assert Lh.opt.step_count == 1 and Lh.n_updates == 1
        assert not torch.equal(Lh.flat.data.cpu(), flat0)
    lh, lr, Lh, Lr = out["vtrace"]
    ih, ir = Lh.last_is_stats.cpu(), Lr.last_is_stats
    print(f"losses hip {lh.tolist()}\nlosses ref {lr.tolist()}\n|hip - ref| "
          f"{(lh - lr).abs().tolist()}\nis_stats hip {ih.tolist()} ref {ir.tolist()} |hip - ref| "
          f"{(ih - ir).abs().tolist()}\ngae losses hip {out['gae'][0].tolist()}")
    assert lh.shape == (7,) and torch.isfinite(lh).all()
    assert Lh.last_is_stats.is_cuda and ih.shape == (3,)
    torch.testing.assert_close(lh[:5], lr[:5], rtol=2e-2, atol=2e-3)
    torch.testing.assert_close(ih, ir, rtol=0, atol=1e-3)
    assert 0.2 < float(ih[1]) < 0.8  # the bars bite on this batch
    lg = out["gae"][0]
    assert out["gae"][2].last_is_stats is None
    far = (lg[:2] - lr[:2]).abs() > 2e-3 + 2e-2 * lr[:2].abs()
    assert bool(far.any()), (lg.tolist(), lr.tolist())


def test_vtrace_minibatch_learner_hip_matches_fp32_torch(cuda, lagged_batch, monkeypatch):
    """K = 2, E = 1, blocks in order, ``ppo_adv="vtrace"``: both block steps of the HIP learner
    against the fp32 CPU learner, as tests/test_gpu_ppo_minibatch.py does for ``gae``. Step 0 is
    held to rtol 2e-2 / atol 2e-3. Step 1 starts from weights that already differ by one
    bf16-against-fp32 step; it is held to the same bound (that file's tighter step-1 bound is a
    measured floor of its own batch and mode and does not carry over). Measured once on one
    MI355X: |hip - ref| <= 4.9e-5 on step 0's losses and <= 2.2e-6 on step 1's."""
    from microbeast_amd import learner as learner_mod
    from microbeast_amd.learner import Learner, LearnerHParams
    hip_model, ref_model = _models()
    hp = LearnerHParams(algo="ppo", ppo_epochs=1, ppo_minibatches=2, ppo_shuffle=False,
                        ppo_adv="vtrace")
    Lh = Learner(hip_model, hp, cuda)
    Lr = Learner(ref_model, hp, torch.device("cpu"))
    real = P.ppo_loss_rows
    seen = []

    def hook(*a, **k):
        o = real(*a, **k)
        seen.append(o.losses.cpu().clone())
        return o

    monkeypatch.setattr(learner_mod, "ppo_loss_rows", hook)
    mh = Lh.learn(lagged_batch).cpu()
    Lr.learn({k: v.cpu() for k, v in lagged_batch.items()})
    sh, sr = seen[:2], seen[2:]
    assert len(sh) == len(sr) == 2 and Lh.opt.step_count == 2 == Lh.last_opt_steps
    for j in range(2):
        print(f"step {j}: hip {sh[j].tolist()}\n        ref {sr[j].tolist()}\n"
              f"        |hip - ref| {(sh[j] - sr[j]).abs().tolist()}")
        assert torch.isfinite(sh[j]).all()
        torch.testing.assert_close(sh[j][:5], sr[j][:5], rtol=2e-2, atol=2e-3)
    torch.testing.assert_close(mh, torch.stack(sh).mean(0), rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(Lh.last_is_stats.cpu(), Lr.last_is_stats, rtol=0, atol=1e-3)


# --------------------------------------------------------------------------------- CLI
def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def test_gpu_cli_vtrace_train_resume_and_eval(cuda, tmp_path):
    from microbeast_amd.cli import main
    from microbeast_amd.utils.checkpoint import load_checkpoint
    from microbeast_amd.utils.metrics import LOSS_HEADER
    args = ["--exp_name", "v", "--runtime", "gpu", "--env_size", "8", "--groups", "2",
            "--envs_per_group", "32", "--unroll_length", "8", "--batch_size", "1",
            "--savedir", str(tmp_path), "--quiet", "--max_episode_steps", "10"]
    train = args + ["--algo", "ppo", "--ppo_adv", "vtrace", "--ppo_epochs", "2",
                    "--checkpoint_every", "2"]
    assert main(train + ["--max_updates", "4"]) == 0
    ck = load_checkpoint(os.path.join(tmp_path, "v.ckpt"))
    assert ck["n_update"] == 4 and ck["optimizer_state_dict"]["step"] == 8
    header = LOSS_HEADER + ["approx_kl", "clip_frac", "rho_clip_frac", "c_clip_frac"]
    with open(tmp_path / "vLosses.csv") as f:
        assert f.readline().strip().split(",") == header
    loss = _rows(tmp_path / "vLosses.csv")
    assert [int(r["update"]) for r in loss] == [1, 2, 3, 4]
    for r in loss:
        for k in ("pg_loss", "value_loss", "entropy_loss", "total_loss", "mean_rho", "approx_kl",
                  "clip_frac", "rho_clip_frac", "c_clip_frac"):
            v = float(r[k])
            assert v == v and abs(v) < 1e9, (k, r)
        assert 0.0 <= float(r["rho_clip_frac"]) <= 1.0 and 0.0 <= float(r["c_clip_frac"]) <= 1.0
    # resume: two more updates appended under the same header
    assert main(train + ["--max_updates", "6", "--resume"]) == 0
    assert load_checkpoint(os.path.join(tmp_path, "v.ckpt"))["n_update"] == 6
    with open(tmp_path / "vLosses.csv") as f:
        assert f.readline().strip().split(",") == header
    loss = _rows(tmp_path / "vLosses.csv")
    assert [int(r["update"]) for r in loss] == [1, 2, 3, 4, 5, 6]
    assert all(0.0 <= float(r["c_clip_frac"]) <= 1.0 for r in loss)
    assert main(args + ["--test", "--eval_envs", "16"]) == 0
    assert len(_rows(tmp_path / "v_eval.csv")) == 16
