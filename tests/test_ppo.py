"""PPO objective on the CPU (ops/ppo.py, Learner algo="ppo", --algo ppo): the closed-form
gradients against fp64 autograd, GAE against the ported reference helper, a learnable task,
the epoch accounting and the CLI on the mono runtime. (Reference: the learn step is named
PPO_learn, libs/utils.py:277-329, but is V-trace; its GAE helpers are dead code.)"""
import csv

import pytest
import torch

from helpers import synthetic_batch
from microbeast_amd.learner import Learner, LearnerHParams
from microbeast_amd.models.agent import Agent
from microbeast_amd.ops import ppo as P
from ppo_cases import BC, CLIP, EC, GAMMA, LAM, VCLIP, autograd_oracle, recipe

T0, B0 = 37, 300


@pytest.mark.parametrize("value_clip,norm", [(VCLIP, True), (0.0, True), (VCLIP, False)])
def test_closed_form_gradients_match_fp64_autograd(value_clip, norm):
    c = recipe(T0, B0)
    d = torch.float64
    g = P.gae_torch(c["v_old"].to(d), c["rew"].to(d), c["done"], GAMMA, LAM, norm_adv=norm)
    ref = autograd_oracle(c, g.adv, g.ret, g.stats, value_clip=value_clip)
    out = P.ppo_loss_torch(c["lpn"].to(d), c["lpo"].to(d), c["values"].to(d), c["v_old"].to(d),
                           g.adv, g.ret, g.stats, c["ent"].to(d), clip=CLIP,
                           value_clip=value_clip, baseline_cost=BC, entropy_cost=EC)
    # every branch is exercised on this recipe
    active = float((out.g_logp != 0).double().mean())
    assert 0.3 < float(ref["losses"][6]) < 0.9 and 0.3 < active < 0.95
    if value_clip > 0:
        zero_v = float((out.g_value[:T0] == 0).double().mean())
        assert 0.05 < zero_v < 0.95
    torch.testing.assert_close(out.g_logp, ref["g_logp"], rtol=1e-5, atol=0)
    torch.testing.assert_close(out.g_value, ref["g_value"], rtol=1e-5, atol=0)
    torch.testing.assert_close(out.losses, ref["losses"], rtol=1e-9, atol=1e-12)
    assert float(out.g_value[T0].abs().max()) == 0.0
    assert out.g_ent == -EC / (T0 * B0)


def test_fp32_oracle_matches_fp64_autograd():
    """The fp32 run of the same code (what the CPU learner and the GPU tests' oracle use):
    away from the branch boundaries its gradients are the fp64 ones to fp32 rounding (both get
    the same fp32 adv / ret / stats, and an fp32 difference of two fp32 numbers is exact to one
    rounding of the result, so no absolute term is needed)."""
    c = recipe(T0, B0)
    g = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM)
    ref = autograd_oracle(c, g.adv, g.ret, g.stats)
    out = P.ppo_loss_torch(c["lpn"], c["lpo"], c["values"], c["v_old"], g.adv, g.ret, g.stats,
                           c["ent"], clip=CLIP, value_clip=VCLIP, baseline_cost=BC,
                           entropy_cost=EC)
    assert out.g_logp.dtype == torch.float32 and out.losses.shape == (7,)
    keep = (ref["m_ratio"] > 1e-4) & (ref["m_value"] > 1e-4)
    assert float((~keep).double().mean()) <= 0.005
    M = T0 * B0
    atol = 0.0
    torch.testing.assert_close(out.g_logp.double()[keep], ref["g_logp"][keep], rtol=1e-5,
                               atol=atol)
    torch.testing.assert_close(out.g_value.double()[:T0][keep], ref["g_value"][:T0][keep],
                               rtol=1e-5, atol=atol)
    torch.testing.assert_close(out.losses[:6].double(), ref["losses"][:6], rtol=1e-5, atol=1e-6)
    assert abs(float(out.losses[6]) - float(ref["losses"][6])) <= float((~keep).sum()) / M + 1e-7


def test_gae_matches_reference_helper():
    from microbeast_amd.ops.advantages import advantages
    c = recipe(T0, B0)
    g = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM, norm_adv=True)
    pad = torch.zeros(1, B0)
    ref = advantages(torch.cat([c["rew"], pad]).t(), c["v_old"].t(),
                     torch.cat([c["done"].float(), pad]).t(), GAMMA, LAM)  # [B, T+1]
    assert float(ref[:, -1].abs().max()) == 0.0
    torch.testing.assert_close(g.adv, ref[:, :-1].t(), rtol=0, atol=1e-5)
    torch.testing.assert_close(g.ret, ref[:, :-1].t() + c["v_old"][:T0], rtol=0, atol=1e-5)
    a = g.adv.double()
    torch.testing.assert_close(g.stats.double(),
                               torch.stack([a.mean(), 1 / (a.std(unbiased=False) + 1e-8)]),
                               rtol=1e-5, atol=1e-6)
    off = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM, norm_adv=False)
    assert off.stats.tolist() == [0.0, 1.0] and torch.equal(off.adv, g.adv)
    # reward_clip applies to r as in V-trace
    cl = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM, reward_clip=0.5)
    ex = P.gae_torch(c["v_old"], c["rew"].clamp(-0.5, 0.5), c["done"], GAMMA, LAM)
    assert torch.equal(cl.adv, ex.adv)


@pytest.mark.parametrize("epochs", [1, 3])
def test_ppo_learns_to_prefer_rewarded_action(epochs):
    """tests/test_learner.py's toy (reward 1 whenever cell 0's action type is 2) under PPO."""
    torch.manual_seed(0)
    m = Agent((4, 4, 27))
    L = Learner(m, LearnerHParams(lr=3e-3, entropy_cost=0.0, algo="ppo", ppo_epochs=epochs),
                torch.device("cpu"))
    S = 16
    obs = torch.randint(0, 2**26, (1, S), dtype=torch.int32)

    def prob():
        with torch.no_grad():
            logits, _ = m.policy_value(obs)
            return torch.softmax(logits[0, :6], 0)[2].item()

    p0 = prob()
    for it in range(40):
        T, B = 8, 8
        b = synthetic_batch(m, T, B, S, seed=it, obs=obs.repeat((T + 1) * B, 1),
                            reward_fn=lambda a: (a[:, 0, 0] == 2))
        losses = L.learn(b)
    p1 = prob()
    assert losses.shape == (7,) and torch.isfinite(losses).all()
    assert p0 < 0.2 and p1 > p0 + 0.3, (p0, p1)


def test_epoch_accounting(monkeypatch):
    from microbeast_amd import learner as learner_mod
    calls = {"gae": 0, "ppo_loss": 0}

    def counted(name, fn):
        def w(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        return w

    monkeypatch.setattr(learner_mod, "gae", counted("gae", learner_mod.gae))
    monkeypatch.setattr(learner_mod, "ppo_loss", counted("ppo_loss", learner_mod.ppo_loss))
    torch.manual_seed(0)
    m = Agent((4, 4, 27))
    L = Learner(m, LearnerHParams(algo="ppo", ppo_epochs=3), torch.device("cpu"))
    before = L.flat.data.clone()
    losses = L.learn(synthetic_batch(m, 8, 3, 16, seed=0))
    assert calls == {"gae": 1, "ppo_loss": 3}
    assert L.opt.step_count == 3 and L.n_updates == 1
    assert losses.shape == (7,) and torch.isfinite(losses).all()
    assert not torch.equal(L.flat.data, before)
    # on-policy first epoch: ratio 1, nothing clipped; later epochs moved away from it
    torch.manual_seed(0)
    m1 = Agent((4, 4, 27))
    L1 = Learner(m1, LearnerHParams(algo="ppo", ppo_epochs=1), torch.device("cpu"))
    l1 = L1.learn(synthetic_batch(m1, 8, 3, 16, seed=0))
    assert abs(float(l1[4]) - 1.0) < 1e-5 and abs(float(l1[5])) < 1e-6 and float(l1[6]) == 0.0
    assert float(losses[5]) > float(l1[5])


def test_impala_branch_is_unchanged(monkeypatch):
    """algo="impala" ignores every PPO field: bit-equal losses [5] and parameters to a learner
    built with the default hyper-parameters, and neither PPO op runs."""
    from microbeast_amd import learner as learner_mod

    def boom(*a, **k):
        raise AssertionError("a PPO op ran on the IMPALA branch")

    monkeypatch.setattr(learner_mod, "gae", boom)
    monkeypatch.setattr(learner_mod, "ppo_loss", boom)
    outs = []
    for hp in (LearnerHParams(), LearnerHParams(algo="impala", ppo_epochs=3, ppo_clip=0.3,
                                                gae_lambda=0.5, ppo_norm_adv=False)):
        torch.manual_seed(0)
        m = Agent((4, 4, 27))
        L = Learner(m, hp, torch.device("cpu"))
        ls = [L.learn(synthetic_batch(m, 8, 3, 16, seed=s)).clone() for s in (0, 1)]
        outs.append((ls, L.flat.data.clone(), L.opt.step_count))
    (la, pa, sa), (lb, pb, sb) = outs
    assert la[0].shape == (5,) and sa == sb == 2
    assert all(torch.equal(x, y) for x, y in zip(la, lb)) and torch.equal(pa, pb)
    assert LearnerHParams().algo == "impala"


def test_unknown_algo_is_refused(tmp_path):
    from microbeast_amd.config import parse_flags
    from microbeast_amd.train import train
    with pytest.raises(ValueError, match="--algo"):
        LearnerHParams(algo="a2c")
    f = parse_flags(["--algo", "a2c", "--savedir", str(tmp_path), "--exp_name", "x", "--device",
                     "cpu"], interactive=False)
    with pytest.raises(ValueError, match="--algo"):
        train(f)
    d = parse_flags([], interactive=False)
    assert (d.algo, d.gae_lambda, d.ppo_clip, d.ppo_value_clip, d.ppo_epochs, d.ppo_norm_adv) == (
        "impala", 0.95, 0.1, 0.1, 1, True)


def test_phase_timer_sums_marks_of_one_name():
    from microbeast_amd.utils.metrics import PhaseTimer

    class Ev:
        def __init__(self, t):
            self.t = t

        def query(self):
            return True

        def elapsed_time(self, other):
            return other.t - self.t

    pt = PhaseTimer(enabled=False)
    pt.enabled = True
    pt._sets[0] = [("start", Ev(0.0)), ("fwd", Ev(1.0)), ("bwd", Ev(3.0)), ("fwd", Ev(3.5)),
                   ("bwd", Ev(6.0))]
    assert pt.read() == {"fwd": 1.5, "bwd": 4.5}
    pt._sets[0] = [("start", Ev(0.0)), ("fwd", Ev(1.25)), ("bwd", Ev(3.0))]
    assert pt.read() == {"fwd": 1.25, "bwd": 1.75}


def _rows(path):
    with open(path) as f:
        return list(csv.reader(f))


@pytest.mark.slow
def test_cli_ppo_on_the_mono_runtime(tmp_path):
    from microbeast_amd.cli import main
    from microbeast_amd.utils.checkpoint import load_checkpoint
    from microbeast_amd.utils.metrics import LOSS_HEADER
    base = ["--env_size", "4", "--n_actors", "2", "--n_envs", "4", "--unroll_length", "8",
            "--batch_size", "2", "--savedir", str(tmp_path), "--device", "cpu", "--quiet",
            "--checkpoint_every", "2"]
    assert main(["--exp_name", "p", "--algo", "ppo", "--ppo_epochs", "2", "--max_updates", "2",
                 *base]) == 0
    rows = _rows(tmp_path / "pLosses.csv")
    assert rows[0] == LOSS_HEADER + ["approx_kl", "clip_frac"] and len(rows) == 3
    for r in rows[1:]:
        assert len(r) == len(rows[0])
        vals = [float(r[rows[0].index(k)]) for k in ("pg_loss", "value_loss", "total_loss",
                                                     "mean_rho", "approx_kl", "clip_frac")]
        assert all(v == v and abs(v) < 1e9 for v in vals), r
        assert 0.0 <= vals[-1] <= 1.0
    ck = load_checkpoint(str(tmp_path / "p.ckpt"))
    assert ck["n_update"] == 2 and ck["step"] == 2 * 2 * 4 * 8
    assert ck["optimizer_state_dict"]["step"] == 4  # Adam steps once per epoch
    assert main(["--exp_name", "i", "--max_updates", "1", *base]) == 0
    rows = _rows(tmp_path / "iLosses.csv")
    assert rows[0] == LOSS_HEADER and len(rows[1]) == len(LOSS_HEADER)
    assert LOSS_HEADER[-1] == "policy_lag" and LOSS_HEADER[10] == "mean_rho"


def _dp_worker(rank, world, port, outdir):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from microbeast_amd.parallel.dist import destroy, init_distributed
    info = init_distributed(use_cuda=False)
    torch.manual_seed(1234 + rank)  # different init per rank: broadcast must fix it
    m = Agent((4, 4, 27))
    hp = LearnerHParams(bucket_mb=0.5, algo="ppo", ppo_epochs=2, ppo_norm_adv=False)
    L = Learner(m, hp, torch.device("cpu"), info)
    torch.save(L.flat.data.clone(), os.path.join(outdir, f"init{rank}.pt"))
    b = synthetic_batch(m, 6, 3, 16, seed=100 + rank)
    torch.save(b, os.path.join(outdir, f"batch{rank}.pt"))
    L.learn(b)
    assert L.opt.step_count == 2
    torch.save(L.flat.data.clone(), os.path.join(outdir, f"after{rank}.pt"))
    destroy(info)


@pytest.mark.slow
def test_ppo_data_parallel_equals_single_process(tmp_path):
    """Two gloo ranks, two epochs (an all-reduce round per epoch): the update is the
    single-process one on the concatenated batch. Advantage normalisation is off here: with it
    on, each rank uses its own batch's statistics (documented), which is not that update."""
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    init0 = torch.load(tmp_path / "init0.pt")
    a0, a1 = torch.load(tmp_path / "after0.pt"), torch.load(tmp_path / "after1.pt")
    assert torch.equal(init0, torch.load(tmp_path / "init1.pt")) and torch.equal(a0, a1)
    L = Learner(Agent((4, 4, 27)),
                LearnerHParams(algo="ppo", ppo_epochs=2, ppo_norm_adv=False), torch.device("cpu"))
    L.flat.data.copy_(init0)
    b0, b1 = torch.load(tmp_path / "batch0.pt"), torch.load(tmp_path / "batch1.pt")
    L.learn({k: torch.cat([b0[k], b1[k]], dim=1) for k in b0})
    torch.testing.assert_close(L.flat.data, a0, rtol=1e-5, atol=1e-6)
