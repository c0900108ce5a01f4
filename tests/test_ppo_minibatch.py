"""PPO row-block minibatches and target-KL early stopping on the CPU (ops/ppo.py block forms,
Learner._learn_ppo_steps, --ppo_minibatches / --ppo_shuffle / --ppo_target_kl): the block
oracles against the full-batch ones on sliced copies, the unchanged default path, the step
accounting and block orders, the first step against autograd, the stop rule, the refusals, the
toy task and (slow) the CLI on the mono runtime and two gloo ranks."""
import copy
import csv

import pytest
import torch

from helpers import synthetic_batch
from microbeast_amd import learner as learner_mod
from microbeast_amd.learner import Learner, LearnerHParams, ppo_block_order
from microbeast_amd.models.agent import Agent
from microbeast_amd.ops import ppo as P
from ppo_cases import BC, CLIP, EC, GAMMA, LAM, VCLIP, recipe

CPU = torch.device("cpu")


def _learner(seed=0, **kw):
    torch.manual_seed(seed)
    m = Agent((4, 4, 27))
    return m, Learner(m, LearnerHParams(algo="ppo", **kw), CPU)


# ---------------------------------------------------------------------------- oracles
@pytest.mark.parametrize("T,B,K", [(12, 300, 3), (6, 259, 2), (2, 1, 2), (8, 5, 1)])
def test_adv_stats_rows_oracle(T, B, K):
    c = recipe(T, B)
    adv = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM).adv
    st = P.adv_stats_rows_torch(adv, K)
    Tm = T // K
    assert st.shape == (K, 2) and st.dtype == torch.float32
    for k in range(K):
        blk = adv[k * Tm:(k + 1) * Tm]
        torch.testing.assert_close(st[k, 0], blk.mean(), rtol=0, atol=1e-6)
        torch.testing.assert_close(st[k, 1], 1.0 / (blk.std(unbiased=False) + 1e-8), rtol=1e-6,
                                   atol=1e-6)
    off = P.adv_stats_rows_torch(adv, K, norm_adv=False)
    assert off.tolist() == [[0.0, 1.0]] * K
    with pytest.raises(ValueError, match=f"{T + 1} .* {T} "):
        P.adv_stats_rows_torch(adv, T + 1)


@pytest.mark.parametrize("T,B,K,value_clip", [(12, 300, 3, VCLIP), (6, 259, 2, VCLIP),
                                              (2, 1, 2, VCLIP), (12, 300, 3, 0.0)])
def test_block_loss_equals_full_loss_on_sliced_copies(T, B, K, value_clip):
    c = recipe(T, B)
    g = P.gae_torch(c["v_old"], c["rew"], c["done"], GAMMA, LAM)
    stats = P.adv_stats_rows_torch(g.adv, K)
    Tm = T // K
    kw = dict(clip=CLIP, value_clip=value_clip, baseline_cost=BC, entropy_cost=EC)
    mean, per_step = None, []
    for j, k in enumerate(reversed(range(K))):
        t0 = k * Tm
        r = slice(t0, t0 + Tm)
        o = P.ppo_loss_rows_torch(c["lpn"][r], c["lpo"], c["values"][r], c["v_old"], g.adv, g.ret,
                                  stats[k], t0, c["ent"][r], step=j, epoch_mean=mean, **kw)
        mean = o.epoch_mean
        per_step.append(o.losses.clone())
        # the full-batch form on copies of the block; its extra (bootstrap) value row is any row
        values = torch.cat([c["values"][r], torch.full((1, B), 7.0)]).clone()
        blk_stats = torch.stack([g.adv[r].mean(), 1.0 / (g.adv[r].std(unbiased=False) + 1e-8)])
        torch.testing.assert_close(stats[k], blk_stats, rtol=1e-6, atol=1e-6)
        ref = P.ppo_loss_torch(c["lpn"][r].clone(), c["lpo"][r].clone(), values,
                               c["v_old"][t0:t0 + Tm + 1].clone(), g.adv[r].clone(),
                               g.ret[r].clone(), stats[k], c["ent"][r].clone(), **kw)
        assert o.g_logp.shape == (Tm, B) and o.g_value.shape == (Tm, B)
        assert torch.equal(o.g_logp, ref.g_logp)
        assert torch.equal(o.g_value, ref.g_value[:Tm])
        assert torch.equal(o.losses, ref.losses)
        assert o.g_ent == -EC / (Tm * B) == ref.g_ent
    torch.testing.assert_close(mean, torch.stack(per_step).mean(0), rtol=1e-6, atol=1e-6)


# ------------------------------------------------------------------- defaults unchanged
def test_defaults_call_no_minibatch_code(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a K > 1 / target-KL helper ran with the defaults")

    b = None
    outs = []
    for kw in ({}, dict(ppo_minibatches=1, ppo_target_kl=0.0), "patched"):
        if kw == "patched":
            for name in ("ppo_loss_rows", "adv_stats_rows", "ppo_block_order", "host_max"):
                monkeypatch.setattr(learner_mod, name, boom)
            monkeypatch.setattr(Learner, "_learn_ppo_steps", boom)
            monkeypatch.setattr(Agent, "values", boom)
            kw = dict(ppo_minibatches=1, ppo_target_kl=0.0, ppo_epochs=1)
        m, L = _learner(**kw)
        b = b or synthetic_batch(m, 8, 3, 16, seed=0)
        losses = L.learn(b).clone()
        outs.append((losses, L.flat.data.clone()))
        assert L.opt.step_count == 1 and L.last_opt_steps == 1 and L.n_updates == 1
    for losses, flat in outs[1:]:
        assert torch.equal(losses, outs[0][0]) and torch.equal(flat, outs[0][1])
    hp = LearnerHParams()
    assert (hp.ppo_minibatches, hp.ppo_shuffle, hp.ppo_target_kl, hp.ppo_seed) == (1, True, 0.0, 0)


# -------------------------------------------------------------------------- accounting
def _record_blocks(monkeypatch):
    seen = []
    real = learner_mod.ppo_loss_rows

    def rec(logp_new, logp_old, values, v_old, adv, ret, stats, t0, *a, **k):
        seen.append((t0, logp_new.shape[0]))
        return real(logp_new, logp_old, values, v_old, adv, ret, stats, t0, *a, **k)

    monkeypatch.setattr(learner_mod, "ppo_loss_rows", rec)
    return seen


def test_step_accounting_and_block_orders(monkeypatch):
    seen = _record_blocks(monkeypatch)
    calls = {"gae": 0, "stats": 0, "values": 0}
    for name, key in (("gae", "gae"), ("adv_stats_rows", "stats")):
        def counted(*a, _f=getattr(learner_mod, name), _k=key, **k):
            calls[_k] += 1
            return _f(*a, **k)
        monkeypatch.setattr(learner_mod, name, counted)
    real_values = Agent.values

    def values(self, obs):
        calls["values"] += 1
        return real_values(self, obs)

    monkeypatch.setattr(Agent, "values", values)
    K, E, T = 4, 2, 8
    m, L = _learner(ppo_minibatches=K, ppo_epochs=E, ppo_seed=5)
    b = synthetic_batch(m, T, 3, 16, seed=0)
    before = L.flat.data.clone()
    losses = L.learn(b)
    assert L.opt.step_count == 8 and L.n_updates == 1 and L.last_opt_steps == 8
    assert calls == {"gae": 1, "stats": 1, "values": 1}
    assert losses.shape == (7,) and torch.isfinite(losses).all()
    assert not torch.equal(L.flat.data, before)
    assert len(seen) == E * K and all(tm == T // K for _, tm in seen)
    first = [[t0 // (T // K) for t0, _ in seen[e * K:(e + 1) * K]] for e in range(E)]
    for order in first:  # every block once per epoch: a permutation
        assert sorted(order) == list(range(K))
    assert first == [ppo_block_order(5, 0, e, K) for e in range(E)]
    # more rollouts: each (n_updates, epoch) has its own order
    for _ in range(4):
        L.learn(b)
    orders = [[t0 // (T // K) for t0, _ in seen[i:i + K]] for i in range(0, len(seen), K)]
    assert len(orders) == 5 * E and all(sorted(o) == list(range(K)) for o in orders)
    assert len({tuple(o) for o in orders}) > 1
    assert any(orders[n * E] != orders[0] for n in range(1, 5))
    # the same seed repeats them (also from a resumed n_updates), no generator state involved
    del seen[:]
    m2, L2 = _learner(ppo_minibatches=K, ppo_epochs=E, ppo_seed=5)
    L2.n_updates = 3
    L2.learn(b)
    assert [[t0 // (T // K) for t0, _ in seen[i:i + K]] for i in (0, K)] == orders[3 * E:4 * E]
    # no process-wide RNG is consumed by the orders
    torch.manual_seed(11)
    x = torch.rand(3)
    torch.manual_seed(11)
    ppo_block_order(5, 7, 1, K)
    assert torch.equal(torch.rand(3), x)


def test_no_shuffle_visits_blocks_in_order(monkeypatch):
    seen = _record_blocks(monkeypatch)
    m, L = _learner(ppo_minibatches=4, ppo_epochs=2, ppo_shuffle=False)
    L.learn(synthetic_batch(m, 8, 3, 16, seed=0))
    assert seen == [(0, 2), (2, 2), (4, 2), (6, 2)] * 2


# ---------------------------------------------------------------- first step vs autograd
def test_first_block_step_matches_autograd(monkeypatch):
    """K = 2, blocks in order: with every later optimiser step suppressed, the parameter change
    is Adam's on the autograd gradient of the PPO loss written out on rows [0, T/2), normalised
    with that block's own mean and std."""
    T, B, S = 8, 5, 16
    torch.manual_seed(3)
    m = Agent((4, 4, 27), hip_kernels=False)
    with torch.no_grad():
        m.actor.weight.normal_(0, 0.05)
    ref = copy.deepcopy(m)
    hp = LearnerHParams(algo="ppo", ppo_minibatches=2, ppo_epochs=2, ppo_shuffle=False, lr=1e-3)
    L = Learner(m, hp, CPU)
    b = synthetic_batch(m, T, B, S, seed=1)
    b["logp"] = b["logp"] + 0.05 * torch.randn(T + 1, B, generator=torch.Generator().manual_seed(2))
    real_step = L.opt.step
    grads = []

    def first_only(grad_scale=1.0):
        if not grads:
            grads.append(L.flat.grad.clone())
            return real_step(grad_scale=grad_scale)
        L.opt.step_count += 1

    monkeypatch.setattr(L.opt, "step", first_only)
    start = L.flat.data.clone()
    L.learn(b)
    assert L.opt.step_count == 4

    # the same step written out directly on an untouched copy of the model
    Tm = T // 2
    flat = lambda x, t: x[:t].reshape(t * B, *x.shape[2:])  # noqa: E731
    with torch.no_grad():
        v_old = ref.values(flat(b["obs"], T + 1)).view(T + 1, B)
    g = P.gae_torch(v_old, b["reward"][:T], b["done"][:T], hp.gamma, hp.gae_lambda)
    logp, ent, value = ref.evaluate(flat(b["obs"], Tm), flat(b["mask"], Tm), flat(b["action"], Tm))
    adv, ret = g.adv[:Tm].reshape(-1), g.ret[:Tm].reshape(-1)
    a = (adv - adv.mean()) / (adv.std(unbiased=False) + 1e-8)
    ratio = torch.exp(logp - b["logp"][:Tm].reshape(-1))
    pg = -torch.min(ratio * a, ratio.clamp(1 - hp.ppo_clip, 1 + hp.ppo_clip) * a).mean()
    vo = v_old[:Tm].reshape(-1)
    vc = vo + (value - vo).clamp(-hp.ppo_value_clip, hp.ppo_value_clip)
    vl = hp.baseline_cost * torch.max((value - ret) ** 2, (vc - ret) ** 2).mean()
    total = pg + vl - hp.entropy_cost * ent.mean()
    params = list(ref.parameters())
    gr = torch.autograd.grad(total, params)
    # Two fp32 evaluations of one gradient: rtol 1e-4, and an absolute term for entries that
    # are sums with cancellation -- one fp32 rounding (2^-24) of the largest entry of the
    # autograd gradient. Adam's first step is -lr g / (|g| + eps), whose slope in g is at most
    # lr / eps, so the parameter change inherits that term times lr / eps.
    atol_g = 2.0 ** -24 * max(float(gi.abs().max()) for gi in gr)
    for (_, o, n, _), gi in zip(L.flat.slices, gr):
        torch.testing.assert_close(grads[0][o:o + n].view_as(gi), gi, rtol=1e-4, atol=atol_g)
    opt = torch.optim.Adam(params, lr=hp.lr, eps=hp.adam_eps)
    for p, gi in zip(params, gr):
        p.grad = gi
    opt.step()
    for (_, o, n, _), p in zip(L.flat.slices, params):
        torch.testing.assert_close(L.flat.data[o:o + n] - start[o:o + n],
                                   p.detach().reshape(-1) - start[o:o + n], rtol=1e-4,
                                   atol=atol_g * hp.lr / hp.adam_eps)
    assert not torch.equal(L.flat.data, start)


# --------------------------------------------------------------------------- stop rule
@pytest.mark.parametrize("K", [1, 2])
def test_stop_rule_on_real_kl(K):
    E = 3
    m, L = _learner(ppo_minibatches=K, ppo_epochs=E, ppo_target_kl=1e9)
    b = synthetic_batch(m, 8, 3, 16, seed=0)
    b["logp"] = b["logp"] + 0.1 * torch.randn(9, 3, generator=torch.Generator().manual_seed(4))
    L.learn(b)
    assert L.opt.step_count == E * K == L.last_opt_steps and L.n_updates == 1
    m, L = _learner(ppo_minibatches=K, ppo_epochs=E, ppo_target_kl=1e-12)
    start = L.flat.data.clone()
    losses = L.learn(b)
    assert float(losses[5]) > 1e-12  # step 0's KL is non-zero on the perturbed log-probs
    assert L.opt.step_count == 1 == L.last_opt_steps and L.n_updates == 1
    assert not torch.equal(L.flat.data, start)  # the exceeding step itself was applied


@pytest.mark.parametrize("K,form", [(2, "ppo_loss_rows"), (1, "ppo_loss")])
def test_stop_rule_on_an_injected_kl_sequence(monkeypatch, K, form):
    seq = [0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0]
    real = getattr(learner_mod, form)
    n = [0]

    def injected(*a, **k):
        o = real(*a, **k)
        o.losses = o.losses.clone()
        o.losses[5] = seq[n[0]]
        n[0] += 1
        return o

    monkeypatch.setattr(learner_mod, form, injected)
    m, L = _learner(ppo_minibatches=K, ppo_epochs=8 // K, ppo_target_kl=0.1)
    L.learn(synthetic_batch(m, 8, 3, 16, seed=0))
    assert n[0] == 3 and L.opt.step_count == 3 and L.last_opt_steps == 3 and L.n_updates == 1
    # a second rollout starts over
    seq[:] = [0.2] + [0.0] * 7
    n[0] = 0
    L.learn(synthetic_batch(m, 8, 3, 16, seed=1))
    assert n[0] == 1 and L.opt.step_count == 4 and L.last_opt_steps == 1 and L.n_updates == 2


def test_epoch_mean_is_returned(monkeypatch):
    """K > 1: learn returns the mean over the steps of the last epoch entered."""
    real = learner_mod.ppo_loss_rows
    per_step = []

    def rec(*a, **k):
        o = real(*a, **k)
        per_step.append(o.losses.clone())
        return o

    monkeypatch.setattr(learner_mod, "ppo_loss_rows", rec)
    m, L = _learner(ppo_minibatches=4, ppo_epochs=2)
    out = L.learn(synthetic_batch(m, 8, 3, 16, seed=0))
    assert len(per_step) == 8
    torch.testing.assert_close(out, torch.stack(per_step[4:]).mean(0), rtol=1e-6, atol=1e-6)


def test_model_without_a_values_method_falls_back_to_evaluate():
    """GridNet has no value-only forward: the value pass is its ``evaluate`` under no_grad."""
    from microbeast_amd.models.gridnet import GridNetAgent
    torch.manual_seed(0)
    m = GridNetAgent((4, 4, 27), compute_dtype=torch.float32, hip_kernels=False)
    assert not hasattr(m, "values")
    L = Learner(m, LearnerHParams(algo="ppo", ppo_minibatches=2, ppo_epochs=2), CPU)
    start = L.flat.data.clone()
    losses = L.learn(synthetic_batch(m, 4, 3, 16, seed=0))
    assert L.opt.step_count == 4 == L.last_opt_steps and torch.isfinite(losses).all()
    assert not torch.equal(L.flat.data, start)


# --------------------------------------------------------------------------- refusals
def test_refusals(tmp_path, monkeypatch):
    from microbeast_amd import train as train_mod
    from microbeast_amd.config import parse_flags
    with pytest.raises(ValueError, match="--ppo_minibatches 0"):
        LearnerHParams(algo="ppo", ppo_minibatches=0)
    with pytest.raises(ValueError, match="--ppo_target_kl"):
        LearnerHParams(algo="ppo", ppo_target_kl=-1.0)
    m, L = _learner(ppo_minibatches=3)
    with pytest.raises(ValueError, match=r"3\b.*\b8\b"):  # T is known at the first learn only
        L.learn(synthetic_batch(m, 8, 3, 16, seed=0))
    assert L.opt.step_count == 0 and L.n_updates == 0

    def started(*a, **k):
        raise AssertionError("train() got as far as starting a runtime")

    monkeypatch.setattr(train_mod.D, "init_distributed", started)
    base = ["--algo", "ppo", "--savedir", str(tmp_path), "--exp_name", "x", "--device", "cpu",
            "--unroll_length", "8"]
    for extra, match in ((["--ppo_minibatches", "0"], "--ppo_minibatches 0"),
                         (["--ppo_minibatches", "3"], r"3\b.*\b8\b"),
                         (["--ppo_target_kl", "-1"], "--ppo_target_kl")):
        with pytest.raises(ValueError, match=match):
            train_mod.train(parse_flags(base + extra, interactive=False))
    d = parse_flags([], interactive=False)
    assert (d.ppo_minibatches, d.ppo_shuffle, d.ppo_target_kl) == (1, True, 0.0)
    hp = train_mod._hparams(parse_flags(["--seed", "9", "--ppo_shuffle", "false"],
                                        interactive=False), rank=2)
    assert hp.ppo_seed == 11 and hp.ppo_shuffle is False


# --------------------------------------------------------------------------- toy task
def test_minibatch_ppo_learns_to_prefer_rewarded_action():
    """tests/test_ppo.py::test_ppo_learns_to_prefer_rewarded_action (its task, its 40 rollouts
    and its threshold: p0 < 0.2 and p1 > p0 + 0.3) at K = 4, E = 2."""
    torch.manual_seed(0)
    m = Agent((4, 4, 27))
    L = Learner(m, LearnerHParams(lr=3e-3, entropy_cost=0.0, algo="ppo", ppo_epochs=2,
                                  ppo_minibatches=4), CPU)
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
    assert L.opt.step_count == 40 * 8
    assert p0 < 0.2 and p1 > p0 + 0.3, (p0, p1)


# ------------------------------------------------------------------------------- slow
def _rows(path):
    with open(path) as f:
        return list(csv.reader(f))


@pytest.mark.slow
def test_cli_minibatches_on_the_mono_runtime(tmp_path):
    from microbeast_amd.cli import main
    from microbeast_amd.utils.checkpoint import load_checkpoint
    from microbeast_amd.utils.metrics import LOSS_HEADER
    base = ["--env_size", "4", "--n_actors", "2", "--n_envs", "4", "--unroll_length", "8",
            "--batch_size", "2", "--savedir", str(tmp_path), "--device", "cpu", "--quiet",
            "--checkpoint_every", "2", "--algo", "ppo"]
    assert main(["--exp_name", "k", "--ppo_minibatches", "2", "--ppo_epochs", "2",
                 "--max_updates", "2", *base]) == 0
    rows = _rows(tmp_path / "kLosses.csv")
    assert rows[0] == LOSS_HEADER + ["approx_kl", "clip_frac", "opt_steps"] and len(rows) == 3
    for r in rows[1:]:
        assert len(r) == len(rows[0]) and r[-1] == "4"
        assert all(float(x) == float(x) for x in r[-3:])
    ck = load_checkpoint(str(tmp_path / "k.ckpt"))
    assert ck["n_update"] == 2 and ck["optimizer_state_dict"]["step"] == 8
    # the defaults keep the PPO CSV's header as it was
    assert main(["--exp_name", "d", "--max_updates", "1", *base]) == 0
    rows = _rows(tmp_path / "dLosses.csv")
    assert rows[0] == LOSS_HEADER + ["approx_kl", "clip_frac"] and len(rows[1]) == len(rows[0])


def _dp_worker(rank, world, port, outdir):
    import os
    import sys
    sys.path.insert(0, os.path.dirname(__file__))
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    from microbeast_amd import learner as lm
    from microbeast_amd.parallel.dist import destroy, init_distributed
    info = init_distributed(use_cuda=False)
    own = []
    real = lm.host_max

    def spy(x, inf):
        own.append(float(x))
        return real(x, inf)

    lm.host_max = spy
    torch.manual_seed(1234)
    m = Agent((4, 4, 27))
    hp = LearnerHParams(bucket_mb=0.5, algo="ppo", ppo_epochs=2, ppo_minibatches=2,
                        ppo_shuffle=False, ppo_target_kl=1e-3)
    L = Learner(m, hp, torch.device("cpu"), info)
    b = synthetic_batch(m, 6, 3, 16, seed=100 + rank)
    if rank == 1:  # only this rank's behaviour log-probs are off-policy
        b["logp"] = b["logp"] + 0.3 * torch.randn(7, 3, generator=torch.Generator().manual_seed(0))
    L.learn(b)
    torch.save({"flat": L.flat.data.clone(), "steps": L.last_opt_steps, "adam": L.opt.step_count,
                "own_kl": own}, os.path.join(outdir, f"out{rank}.pt"))
    destroy(info)


@pytest.mark.slow
def test_target_kl_stops_every_rank_at_the_same_step(tmp_path):
    """Two gloo ranks, only rank 1's own step-0 KL exceeds the target: both stop after that
    step (the MAX over ranks on the host group) and their parameters stay equal."""
    import socket

    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.start_processes(_dp_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    o0, o1 = torch.load(tmp_path / "out0.pt"), torch.load(tmp_path / "out1.pt")
    assert o0["own_kl"][0] < 1e-3 < o1["own_kl"][0], (o0["own_kl"], o1["own_kl"])
    assert o0["steps"] == o1["steps"] == 1 and o0["adam"] == o1["adam"] == 1
    assert torch.equal(o0["flat"], o1["flat"])
