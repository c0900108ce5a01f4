"""V-trace-corrected PPO advantages on the CPU (ops/ppo.py vtrace_adv_torch,
LearnerHParams.ppo_adv, --ppo_adv): the fp64 oracle against GAE, V-trace and its lambda = 0
form, the fp32 torch form against the oracle, the unchanged ``gae`` path, the learner's first
step against fp64 autograd, the pre-pass and scan accounting, the refusals, the toy task on
stale behaviour log-probs and (slow) the CLI on the mono runtime."""
import copy
import csv

import pytest
import torch

from helpers import synthetic_batch
from microbeast_amd import learner as learner_mod
from microbeast_amd.learner import Learner, LearnerHParams, ppo_block_order
from microbeast_amd.models.agent import Agent
from microbeast_amd.ops import ppo as P
from objective_cases import vtrace_oracle64
from ppo_cases import BC, EC, GAMMA, LAM, autograd_oracle
from ppo_vtrace_cases import (SETTINGS, SHAPES, TOL, case, check_against_oracle, oracle64,
                              oracle_for, settings)

CPU = torch.device("cpu")
D = torch.float64


# ----------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("shape", SHAPES[:4])
def test_oracle_on_policy_is_gae(shape):
    c = case(*shape)
    for bars in (1.0, 1.7, 1e9):
        o = oracle64(c["lpo"], c["lpo"], c["v_old"], c["rew"], c["done"], GAMMA, LAM, bars, bars)
        g = P.gae_torch(c["v_old"].to(D), c["rew"].to(D), c["done"], GAMMA, LAM)
        assert g.adv.dtype == D
        torch.testing.assert_close(o["adv"], g.adv, rtol=0, atol=1e-12)
        torch.testing.assert_close(o["ret"], g.ret, rtol=0, atol=1e-12)
        torch.testing.assert_close(o["stats"], g.stats, rtol=1e-12, atol=1e-12)
        assert o["is_stats"].tolist() == [1.0, 0.0, 0.0]


@pytest.mark.parametrize("rho_bar,c_bar", [(1.0, 1.0), (1.3, 0.9)])
def test_oracle_at_lambda_one_is_vtrace(rho_bar, c_bar):
    c = case(37, 300)
    o = oracle64(c["lpn"], c["lpo"], c["v_old"], c["rew"], c["done"], GAMMA, 1.0, rho_bar, c_bar,
                 reward_clip=0.5)
    v = vtrace_oracle64(c["lpn"], c["lpo"], c["v_old"], c["rew"], c["done"], None, GAMMA, rho_bar,
                        c_bar, 1e30, BC, EC, 0.5)
    torch.testing.assert_close(o["ret"], v["vs"], rtol=0, atol=1e-12)
    torch.testing.assert_close(o["adv"] * o["w"], v["adv"], rtol=1e-12, atol=1e-12)


def test_oracle_at_lambda_zero_is_one_step():
    c = case(37, 300)
    o = oracle64(c["lpn"], c["lpo"], c["v_old"], c["rew"], c["done"], GAMMA, 0.0, 1.3, 0.9)
    assert torch.equal(o["adv"], o["td"])
    torch.testing.assert_close(o["ret"], c["v_old"][:37].to(D) + o["rho"] * o["td"], rtol=0,
                               atol=1e-14)
    assert float((o["rho"] < o["w"]).double().mean()) > 0.05  # the bar is active


def test_recipe_is_far_from_on_policy():
    """The recipe's behaviour log-probs move the advantages away from GAE's by far more than
    the bound the kernels are held to, so a scan that ignored them would fail every check."""
    c, o = oracle_for(SHAPES[0], "defaults")
    g = P.gae_torch(c["v_old"].to(D), c["rew"].to(D), c["done"], GAMMA, LAM)
    assert float((o["adv"] - g.adv).abs().max()) > 100 * TOL
    assert float((o["ret"] - g.ret).abs().max()) > 100 * TOL
    assert 0.4 < float(o["w"].min()) < 0.6 and 1.8 < float(o["w"].max()) < 2.5
    assert 0.4 < float(o["is_stats"][1]) < 0.6
    assert o["near"] <= 0.001  # (measured: 0.03 % of the 11100 elements)


# ------------------------------------------------------------------ torch form vs the oracle
@pytest.mark.parametrize("name", list(SETTINGS))
@pytest.mark.parametrize("shape", SHAPES)
def test_torch_form_matches_oracle(shape, name):
    c, o = oracle_for(shape, name)
    s = settings(name)
    g, is_stats = P.vtrace_adv_torch(c["lpn"], c["lpo"], c["v_old"], c["rew"], c["done"], **s)
    assert g.adv.dtype == torch.float32 and g.adv.shape == c["rew"].shape
    check_against_oracle(g, is_stats, o, s["norm_adv"])
    # the dispatcher takes CPU tensors to the same code
    g2, is2 = P.vtrace_adv(c["lpn"], c["lpo"], c["v_old"], c["rew"], c["done"], **s)
    assert torch.equal(g2.adv, g.adv) and torch.equal(g2.ret, g.ret) and torch.equal(is2, is_stats)


def test_torch_form_keeps_fp64_and_reduces_to_gae():
    c = case(37, 300)
    a = [c[k].to(D) for k in ("lpn", "lpo", "v_old", "rew")]
    g, is_stats = P.vtrace_adv_torch(*a, c["done"], GAMMA, LAM, 1.3, 0.9, reward_clip=0.5)
    o = oracle64(*a, c["done"], GAMMA, LAM, 1.3, 0.9, reward_clip=0.5)
    assert g.adv.dtype == D and is_stats.dtype == D
    torch.testing.assert_close(g.adv, o["adv"], rtol=0, atol=1e-12)
    torch.testing.assert_close(g.ret, o["ret"], rtol=0, atol=1e-12)
    assert torch.equal(is_stats[1:], o["is_stats"][1:])
    # fp32, on-policy: GAE's own numbers
    on, on_is = P.vtrace_adv_torch(c["lpo"], c["lpo"], c["v_old"], c["rew"], c["done"], GAMMA, LAM)
    ref = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM)
    torch.testing.assert_close(on.adv, ref.adv, rtol=TOL, atol=TOL)
    torch.testing.assert_close(on.ret, ref.ret, rtol=TOL, atol=TOL)
    assert on_is.tolist() == [1.0, 0.0, 0.0]


# ----------------------------------------------------------------------------- learner
def _learner(seed=0, **kw):
    torch.manual_seed(seed)
    m = Agent((4, 4, 27))
    return m, Learner(m, LearnerHParams(algo="ppo", **kw), CPU)


def _lagged(b, T, B, scale=0.2, seed=2):
    """the batch with behaviour log-probs off the learner's: ratios away from 1"""
    b = dict(b)
    b["logp"] = b["logp"] + scale * torch.randn(T + 1, B, generator=torch.Generator().manual_seed(seed))
    return b


@pytest.mark.parametrize("kw", [dict(), dict(ppo_minibatches=2, ppo_epochs=2),
                                dict(ppo_target_kl=1e9, ppo_epochs=2)])
def test_gae_mode_runs_no_new_code(monkeypatch, kw):
    def boom(*a, **k):
        raise AssertionError("V-trace advantage code ran under ppo_adv='gae'")

    outs = []
    for patched in (False, True):
        if patched:
            monkeypatch.setattr(learner_mod, "vtrace_adv", boom)
            monkeypatch.setattr(learner_mod, "multi_copy", boom)
            monkeypatch.setattr(P, "vtrace_adv", boom)
            monkeypatch.setattr(P, "vtrace_adv_torch", boom)
            monkeypatch.setattr(Learner, "_vtrace_adv", boom)
        m, L = _learner(ppo_adv="gae", **kw) if patched else _learner(**kw)
        b = _lagged(synthetic_batch(m, 8, 3, 16, seed=0), 8, 3)
        losses = L.learn(b).clone()
        assert L.last_is_stats is None
        outs.append((losses, L.flat.data.clone(), L.opt.step_count))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    assert outs[0][2] == outs[1][2]
    assert LearnerHParams().ppo_adv == "gae"


@pytest.mark.parametrize("steps_path", [False, True])
def test_first_step_matches_fp64_autograd(monkeypatch, steps_path):
    """K = 1 (``_learn_ppo``, and ``_learn_ppo_steps`` through a target KL that never stops):
    the seeds the first step back-propagates, dL/dlogp and dL/dV, against fp64 autograd of the
    clipped surrogate built on the ORACLE's adv / ret of the learner's own first pass. Elements
    within 1e-4 of a branch boundary are left out as ppo_cases.autograd_oracle marks them (at
    most 0.5 %). The learner's adv / ret are an fp32 evaluation, held to TOL elsewhere; through
    A^ = (adv - mean) rstd and R that bound reaches the seeds as the absolute terms below.
    (M = 1600 elements, so that the 0.5 % cap is 8 elements and not 1: with ratios spread
    N(0, 0.2) about 1 in the log, about 0.1 % of them lie that close to 1 -+ clip.)"""
    T, B, S = 8, 200, 16
    torch.manual_seed(3)
    m = Agent((4, 4, 27), hip_kernels=False)
    with torch.no_grad():
        m.actor.weight.normal_(0, 0.05)
    ref = copy.deepcopy(m)
    hp = LearnerHParams(algo="ppo", ppo_adv="vtrace", rho_bar=1.3, c_bar=0.9, gamma=0.97,
                        ppo_target_kl=1e9 if steps_path else 0.0)
    L = Learner(m, hp, CPU)
    b = _lagged(synthetic_batch(m, T, B, S, seed=1), T, B)
    b["done"] = (torch.rand(T + 1, B, generator=torch.Generator().manual_seed(5)) < 0.1).to(torch.uint8)
    seeds = []
    real = learner_mod.ppo_loss

    def rec(*a, **k):
        o = real(*a, **k)
        seeds.append((o.g_logp.clone(), o.g_value.clone()))
        return o

    monkeypatch.setattr(learner_mod, "ppo_loss", rec)
    start = L.flat.data.clone()
    L.learn(b)
    assert len(seeds) == 1 and L.opt.step_count == 1 and not torch.equal(L.flat.data, start)

    flat = lambda x, t: x[:t].reshape(t * B, *x.shape[2:])  # noqa: E731
    with torch.no_grad():
        logp, ent, value = ref.evaluate(flat(b["obs"], T + 1), flat(b["mask"], T),
                                        flat(b["action"], T), n_score=T * B)
    logp, ent, value = logp.view(T, B), ent.view(T, B), value.view(T + 1, B)
    o = oracle64(logp, b["logp"][:T], value, b["reward"][:T], b["done"][:T], hp.gamma,
                 hp.gae_lambda, hp.rho_bar, hp.c_bar)
    assert 0.05 < float(o["is_stats"][1]) < 0.5 and float(o["is_stats"][2]) > float(o["is_stats"][1])
    c = dict(lpn=logp, lpo=b["logp"][:T], values=value, v_old=value, ent=ent)
    f64 = autograd_oracle(c, o["adv"], o["ret"], o["stats"], clip=hp.ppo_clip,
                          value_clip=hp.ppo_value_clip, bc=hp.baseline_cost, ec=hp.entropy_cost)
    keep = (f64["m_ratio"] > 1e-4) & (f64["m_value"] > 1e-4)
    assert float((~keep).double().mean()) <= 0.005
    M = T * B
    atol_l = 2 * TOL * float(o["stats"][1]) * float(f64["ratio"].max()) / M
    atol_v = 2 * hp.baseline_cost * TOL / M
    gl, gv = seeds[0]
    torch.testing.assert_close(gl.double()[keep], f64["g_logp"][keep], rtol=1e-4, atol=atol_l)
    torch.testing.assert_close(gv.double()[:T][keep], f64["g_value"][:T][keep], rtol=1e-4,
                               atol=atol_v)
    assert float(gv[T].abs().max()) == 0.0
    # and GAE's seeds on the same batch are not these
    g = P.gae_torch(value, b["reward"][:T], b["done"][:T], hp.gamma, hp.gae_lambda)
    ga = autograd_oracle(c, g.adv, g.ret, g.stats, clip=hp.ppo_clip, value_clip=hp.ppo_value_clip,
                         bc=hp.baseline_cost, ec=hp.entropy_cost)
    assert float((ga["g_logp"] - f64["g_logp"]).abs().max()) > 100 * atol_l
    torch.testing.assert_close(L.last_is_stats.double()[0], o["is_stats"][0], rtol=TOL, atol=TOL)
    assert float((L.last_is_stats.double()[1:] - o["is_stats"][1:]).abs().max()) <= o["near"] + 1e-6


def _count(monkeypatch, names=("gae", "vtrace_adv", "adv_stats_rows")):
    calls = {n: 0 for n in names}
    for n in names:
        def counted(*a, _f=getattr(learner_mod, n), _n=n, **k):
            calls[_n] += 1
            return _f(*a, **k)
        monkeypatch.setattr(learner_mod, n, counted)
    return calls


def test_minibatch_prepass_scores_the_rollout(monkeypatch):
    """K = 4: the no-grad pre-pass is one ``evaluate`` over rows 0..T (never ``values``), the
    scan runs once per rollout, and the steps and block orders are those of ``gae``."""
    K, E, T, B = 4, 2, 8, 3
    calls = _count(monkeypatch)
    seen, evals = [], []
    real_rows, real_eval, real_values = learner_mod.ppo_loss_rows, Agent.evaluate, Agent.values

    def rows(logp_new, logp_old, values, v_old, adv, ret, stats, t0, *a, **k):
        seen.append(t0 // (T // K))
        return real_rows(logp_new, logp_old, values, v_old, adv, ret, stats, t0, *a, **k)

    def evaluate(self, obs, mask, action, **k):
        evals.append((obs.shape[0], mask.shape[0], torch.is_grad_enabled()))
        return real_eval(self, obs, mask, action, **k)

    def no_values(self, obs):
        raise AssertionError("the value-only pre-pass ran under ppo_adv='vtrace'")

    monkeypatch.setattr(learner_mod, "ppo_loss_rows", rows)
    monkeypatch.setattr(Agent, "evaluate", evaluate)
    monkeypatch.setattr(Agent, "values", no_values)
    m, L = _learner(ppo_minibatches=K, ppo_epochs=E, ppo_seed=5, ppo_adv="vtrace")
    b = _lagged(synthetic_batch(m, T, B, 16, seed=0), T, B)
    losses = L.learn(b)
    assert calls == {"gae": 0, "vtrace_adv": 1, "adv_stats_rows": 1}
    assert evals[0] == ((T + 1) * B, T * B, False)
    assert evals[1:] == [(T // K * B, T // K * B, True)] * (E * K)
    assert L.opt.step_count == E * K == L.last_opt_steps and L.n_updates == 1
    assert [seen[e * K:(e + 1) * K] for e in range(E)] == [ppo_block_order(5, 0, e, K)
                                                           for e in range(E)]
    assert losses.shape == (7,) and torch.isfinite(losses).all()
    assert L.last_is_stats.shape == (3,) and 0 < float(L.last_is_stats[1]) < 1
    # the scan's inputs are the pre-pass's own numbers: the same rollout under gae differs
    m2, L2 = _learner(ppo_minibatches=K, ppo_epochs=E, ppo_seed=5)
    monkeypatch.setattr(Agent, "values", real_values)
    assert not torch.equal(L2.learn(b), losses)


@pytest.mark.parametrize("kw", [dict(), dict(ppo_target_kl=1e9)])
def test_later_epochs_reuse_the_scan(monkeypatch, kw):
    calls = _count(monkeypatch)
    m, L = _learner(ppo_epochs=3, ppo_adv="vtrace", **kw)
    b = _lagged(synthetic_batch(m, 8, 3, 16, seed=0), 8, 3)
    for n in (1, 2):
        losses = L.learn(b)
        assert calls == {"gae": 0, "vtrace_adv": n, "adv_stats_rows": 0}
        assert L.opt.step_count == 3 * n and L.n_updates == n
    assert losses.shape == (7,) and torch.isfinite(losses).all()


def test_on_policy_vtrace_update_is_the_gae_update():
    """Behaviour log-probs equal to the learner's own (the synthetic batch is sampled from the
    learner's weights): w = 1 up to the rounding of two evaluations of one log-prob, and the
    update is GAE's to that rounding."""
    outs = []
    for mode in ("gae", "vtrace"):
        m, L = _learner(ppo_adv=mode, ppo_epochs=2)
        losses = L.learn(synthetic_batch(m, 8, 3, 16, seed=0))
        outs.append((losses.clone(), L.flat.data.clone()))
    torch.testing.assert_close(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-5)
    assert abs(float(L.last_is_stats[0]) - 1.0) < 1e-5


# ----------------------------------------------------------------------------- refusals
def test_refusals(tmp_path, monkeypatch):
    from microbeast_amd import train as train_mod
    from microbeast_amd.config import parse_flags
    with pytest.raises(ValueError, match="--ppo_adv 'retrace'.*gae \\| vtrace"):
        LearnerHParams(algo="ppo", ppo_adv="retrace")
    for bars in (dict(rho_bar=0.0), dict(c_bar=-1.0)):
        with pytest.raises(ValueError, match="--rho_bar .* --c_bar"):
            LearnerHParams(algo="ppo", ppo_adv="vtrace", **bars)
        LearnerHParams(algo="ppo", **bars)  # (gae never reads the bars)
    c = case(5, 259)
    for bars in ((0.0, 1.0), (1.0, -1.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="expected > 0"):
            P.vtrace_adv_torch(c["lpn"], c["lpo"], c["v_old"], c["rew"], c["done"], GAMMA, LAM,
                               *bars)

    def started(*a, **k):
        raise AssertionError("train() got as far as starting a runtime")

    monkeypatch.setattr(train_mod.D, "init_distributed", started)
    base = ["--algo", "ppo", "--savedir", str(tmp_path), "--exp_name", "x", "--device", "cpu",
            "--unroll_length", "8"]
    for extra, match in ((["--ppo_adv", "retrace"], "--ppo_adv 'retrace'"),
                         (["--ppo_adv", "vtrace", "--rho_bar", "0"], "--rho_bar")):
        with pytest.raises(ValueError, match=match):
            train_mod.train(parse_flags(base + extra, interactive=False))
    assert parse_flags([], interactive=False).ppo_adv == "gae"
    hp = train_mod._hparams(parse_flags(base + ["--ppo_adv", "vtrace", "--rho_bar", "1.3",
                                                "--c_bar", "0.9"], interactive=False))
    assert (hp.ppo_adv, hp.rho_bar, hp.c_bar) == ("vtrace", 1.3, 0.9)


# ----------------------------------------------------------------------------- toy task
def test_vtrace_ppo_learns_from_a_stale_behaviour_policy():
    """tests/test_ppo.py::test_ppo_learns_to_prefer_rewarded_action (its task, its 40 rollouts
    and its threshold: p0 < 0.2 and p1 > p0 + 0.3), with every rollout acted by a copy of the
    policy that is refreshed only every 4th update: behaviour log-probs up to 3 updates old."""
    torch.manual_seed(0)
    m = Agent((4, 4, 27))
    L = Learner(m, LearnerHParams(lr=3e-3, entropy_cost=0.0, algo="ppo", ppo_epochs=2,
                                  ppo_adv="vtrace"), CPU)
    S = 16
    obs = torch.randint(0, 2**26, (1, S), dtype=torch.int32)

    def prob():
        with torch.no_grad():
            logits, _ = m.policy_value(obs)
            return torch.softmax(logits[0, :6], 0)[2].item()

    p0 = prob()
    off = []
    for it in range(40):
        if it % 4 == 0:
            actor = copy.deepcopy(m)
        T, B = 8, 8
        b = synthetic_batch(actor, T, B, S, seed=it, obs=obs.repeat((T + 1) * B, 1),
                            reward_fn=lambda a: (a[:, 0, 0] == 2))
        losses = L.learn(b)
        off.append(abs(float(L.last_is_stats[0]) - 1.0))
    p1 = prob()
    assert losses.shape == (7,) and torch.isfinite(losses).all()
    assert max(off) > 1e-2  # the rollouts were off-policy
    assert p0 < 0.2 and p1 > p0 + 0.3, (p0, p1)


# ------------------------------------------------------------------------------- slow
def _rows(path):
    with open(path) as f:
        return list(csv.reader(f))


@pytest.mark.slow
def test_cli_vtrace_on_the_mono_runtime(tmp_path):
    from microbeast_amd.cli import main
    from microbeast_amd.utils.metrics import LOSS_HEADER
    base = ["--env_size", "4", "--n_actors", "2", "--n_envs", "4", "--unroll_length", "8",
            "--batch_size", "2", "--savedir", str(tmp_path), "--device", "cpu", "--quiet",
            "--checkpoint_every", "2", "--algo", "ppo"]
    assert main(["--exp_name", "v", "--ppo_adv", "vtrace", "--ppo_epochs", "2", "--max_updates",
                 "2", *base]) == 0
    rows = _rows(tmp_path / "vLosses.csv")
    assert rows[0] == LOSS_HEADER + ["approx_kl", "clip_frac", "rho_clip_frac", "c_clip_frac"]
    assert len(rows) == 3
    for r in rows[1:]:
        assert len(r) == len(rows[0])
        assert all(0.0 <= float(x) <= 1.0 for x in r[-2:])
    # with the step column: it stays before the two new ones
    assert main(["--exp_name", "k", "--ppo_adv", "vtrace", "--ppo_minibatches", "2",
                 "--max_updates", "1", *base]) == 0
    rows = _rows(tmp_path / "kLosses.csv")
    assert rows[0] == LOSS_HEADER + ["approx_kl", "clip_frac", "opt_steps", "rho_clip_frac",
                                     "c_clip_frac"]
    assert len(rows[1]) == len(rows[0]) and rows[1][-3] == "2"
    assert all(0.0 <= float(x) <= 1.0 for x in rows[1][-2:])
    # without the flag: no new column
    assert main(["--exp_name", "d", "--max_updates", "1", *base]) == 0
    rows = _rows(tmp_path / "dLosses.csv")
    assert rows[0] == LOSS_HEADER + ["approx_kl", "clip_frac"] and len(rows[1]) == len(rows[0])
