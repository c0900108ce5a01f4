"""V-trace(lambda) value targets and the UPGO policy term on the CPU (ops/vtrace.py
vtrace_upgo_torch, LearnerHParams.vtrace_lambda / upgo_cost / upgo_rho_bar and their flags): the
fp32 torch form against the fp64 oracle (tests/upgo_cases.py), the exact case with its ties, the
limits (lambda 1 and 0, PPO's V-trace(lambda) returns, every gate open / closed), the gradients
against fp64 autograd, what the oracle's mutants move, the untouched default path, the flags and
refusals, one learner update against autograd and (slow) the CLI on the mono runtime."""
import copy
import csv

import numpy as np
import pytest
import torch

from helpers import synthetic_batch
from microbeast_amd import learner as learner_mod
from microbeast_amd.learner import Learner, LearnerHParams
from microbeast_amd.models.agent import Agent
from microbeast_amd.ops import ppo as P
from microbeast_amd.ops import vtrace as V
from microbeast_amd.ops.vtrace import vtrace_torch, vtrace_upgo, vtrace_upgo_torch
from objective_cases import NONDEFAULT, vtrace_recipe
from upgo_cases import (EXACT, SETTINGS, case, exact_case, gate_margins, kernel_kwargs,
                        oracle_for, upgo_oracle64)

CPU = torch.device("cpu")
D = torch.float64
ARGS = ("lpn", "lpo", "val", "rew", "done", "ent")


def _assert_matches64(out, ref, T):
    """tests/test_vtrace.py's tolerances, with the upgoing returns held like vs and adv."""
    torch.testing.assert_close(out.vs.to(D), ref["vs"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.adv.to(D), ref["adv"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.upgo.to(D), ref["upgo"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.g_logp.to(D), ref["g_logp"], rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(out.g_value[:T].to(D), ref["g_value"], rtol=1e-4, atol=1e-8)
    assert float(out.g_value[T].abs().max()) == 0.0
    assert out.losses.shape == (6,)
    torch.testing.assert_close(out.losses.to(D), ref["losses"], rtol=1e-4, atol=1e-5)


# ------------------------------------------------------------------ torch form vs the oracle
@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("shape", ["37x300", "37x300-done-row", "1x1", "2x1", "9x300-all-done"])
def test_torch_form_matches_oracle(shape, setting):
    c, ref = oracle_for(shape, setting)
    s = SETTINGS[setting]
    T, B = c["lpn"].shape
    out = vtrace_upgo_torch(*(c[k] for k in ARGS), **kernel_kwargs(s))
    assert out.upgo.shape == (T, B) and out.upgo.dtype == torch.float32
    _assert_matches64(out, ref, T)
    assert out.g_ent == -s["entropy_cost"] / float(T * B)
    # the dispatcher takes CPU tensors to the same code
    out2 = vtrace_upgo(*(c[k] for k in ARGS), **kernel_kwargs(s))
    for a, b in ((out.g_logp, out2.g_logp), (out.g_value, out2.g_value), (out.upgo, out2.upgo),
                 (out.losses, out2.losses)):
        assert torch.equal(a, b)
    if shape == "9x300-all-done":  # no recurrence left, in fp64 closed form
        v, r = c["val"].to(D), c["rew"].to(D)
        r = r.clamp(-s["reward_clip"], s["reward_clip"]) if s["reward_clip"] > 0 else r
        rho = torch.exp(c["lpn"].to(D) - c["lpo"].to(D)).clamp(max=s["rho_bar"])
        torch.testing.assert_close(ref["upgo"], r, rtol=0, atol=0)
        torch.testing.assert_close(ref["vs"], v[:T] + rho * (r - v[:T]), rtol=0, atol=1e-14)
        torch.testing.assert_close(out.upgo.to(D), r, rtol=1e-4, atol=1e-4)


def test_torch_form_without_entropy():
    c, ref = oracle_for("37x300", "nondefault", False)
    out = vtrace_upgo_torch(*(c[k] for k in ARGS[:5]), None, **kernel_kwargs(SETTINGS["nondefault"]))
    _assert_matches64(out, ref, 37)
    assert float(out.losses[2]) == 0.0


def test_both_gate_branches_are_taken():
    """About half of the recipe's gates are open, and none is an fp32 near-tie (``case``
    asserts the margin condition; its figures are printed here)."""
    for shape in ("5x63", "64x257", "3x16641", "37x300"):
        for name, s in SETTINGS.items():
            margin, bound, share = gate_margins(case(shape, s), s["gamma"], s["reward_clip"])
            print(f"{shape} {name}: smallest margin {margin:.3g}, largest bound {bound:.3g}, "
                  f"open {share:.3f}")
            assert margin > bound and bound < 5e-6 and 0.45 < share < 0.6


# ----------------------------------------------------------------------------- exact case
def test_exact_case_pins_the_tie():
    c, ties = exact_case()
    T, B = c["lpn"].shape
    assert (T, B) == (8, 64) and len(ties) >= 8
    ref = upgo_oracle64(*(c[k] for k in ARGS), **EXACT)
    for s, b in ties:  # exact ties, behind a step that is not terminal
        assert float(c["rew"][s, b] + 0.5 * c["val"][s + 1, b]) == float(c["val"][s, b])
        assert not bool(c["done"][s - 1, b]) and not bool(c["done"][s, b])
    assert bool(c["done"].any())
    out = vtrace_upgo_torch(*(c[k] for k in ARGS), **kernel_kwargs(EXACT))
    for k, t in (("vs", out.vs), ("upgo", out.upgo), ("adv", out.adv), ("g_logp", out.g_logp),
                 ("g_value", out.g_value[:T])):
        assert torch.equal(ref[k].float().to(D), ref[k]), k  # the fp64 result is an fp32 number
        assert torch.equal(t, ref[k].float()), k
    # a gate that reads a tie as closed (q > V) is another function on this case
    strict = upgo_oracle64(*(c[k] for k in ARGS), **EXACT, mutant="strict")
    for s, b in ties:
        assert float(strict["upgo"][s - 1, b]) != float(ref["upgo"][s - 1, b]), (s, b)
    assert not torch.equal(out.upgo, strict["upgo"].float())


# --------------------------------------------------------------------------------- limits
@pytest.mark.parametrize("kw", [dict(), NONDEFAULT])
def test_lambda_one_without_upgo_is_vtrace(kw):
    c = vtrace_recipe(37, 300)
    a = [c[k] for k in ARGS]
    old = vtrace_torch(*a, **kw)
    new = vtrace_upgo_torch(*a, **kw, lam=1.0, upgo_cost=0.0, upgo_rho_bar=1.7)
    for x, y in ((old.vs, new.vs), (old.adv, new.adv), (old.g_logp, new.g_logp),
                 (old.g_value, new.g_value), (old.losses, new.losses[:5])):
        assert torch.equal(x, y)
    assert old.g_ent == new.g_ent and old.upgo is None and old.losses.shape == (5,)


def test_lambda_zero_is_one_step():
    s = dict(SETTINGS["nondefault"], vtrace_lambda=0.0)
    c = case("37x300", s)
    o = upgo_oracle64(*(c[k] for k in ARGS), **s)
    v, r = c["val"].to(D), c["rew"].to(D).clamp(-s["reward_clip"], s["reward_clip"])
    w = torch.exp(c["lpn"].to(D) - c["lpo"].to(D))
    disc = (~c["done"]).to(D) * s["gamma"]
    one = v[:37] + w.clamp(max=s["rho_bar"]) * (r + disc * v[1:] - v[:37])
    torch.testing.assert_close(o["vs"], one, rtol=0, atol=1e-14)
    out = vtrace_upgo_torch(*(c[k] for k in ARGS), **kernel_kwargs(s))
    torch.testing.assert_close(out.vs.to(D), one, rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("lam", [0.8, 0.3])
def test_value_targets_are_ppo_vtrace_returns(lam):
    """ops/ppo.py's V-trace(lambda) scan (--ppo_adv vtrace) is the same recurrence for ``ret``."""
    s = dict(SETTINGS["nondefault"], vtrace_lambda=lam)
    c = case("37x300", s)
    out = vtrace_upgo_torch(*(c[k] for k in ARGS), **kernel_kwargs(s))
    g, _ = P.vtrace_adv_torch(c["lpn"], c["lpo"], c["val"], c["rew"], c["done"], gamma=s["gamma"],
                              lam=lam, rho_bar=s["rho_bar"], c_bar=s["c_bar"],
                              reward_clip=s["reward_clip"])
    torch.testing.assert_close(out.vs, g.ret, rtol=1e-4, atol=1e-4)
    o = upgo_oracle64(*(c[k] for k in ARGS), **s)
    torch.testing.assert_close(g.ret.to(D), o["vs"], rtol=1e-4, atol=1e-4)


def test_every_gate_open_and_every_gate_closed():
    """(rewards clipped to 0.5 and gamma 0.97: q = r -+ 97 lies on one side of V = -+100)"""
    c = vtrace_recipe(9, 7, seed=3)
    s = SETTINGS["nondefault"]
    T = 9
    r, disc = c["rew"].to(D).clamp(-0.5, 0.5), (~c["done"]).to(D) * s["gamma"]
    for level in (-100.0, 100.0):
        val = torch.full_like(c["val"], level)
        a = (c["lpn"], c["lpo"], val, c["rew"], c["done"], c["ent"])
        o = upgo_oracle64(*a, **s)
        if level < 0:  # every q >= V: the bootstrapped discounted return of the rollout
            want = torch.empty(T, 7, dtype=D)
            nxt = val[T].to(D)
            for t in range(T - 1, -1, -1):
                nxt = r[t] + disc[t] * nxt
                want[t] = nxt
        else:  # every q < V: one step
            want = r + disc * level
        torch.testing.assert_close(o["upgo"], want, rtol=0, atol=1e-12)
        out = vtrace_upgo_torch(*a, **kernel_kwargs(s))
        torch.testing.assert_close(out.upgo.to(D), want, rtol=1e-4, atol=1e-4)


# ------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_gradients_equal_fp64_autograd_of_the_surrogate(setting):
    s = SETTINGS[setting]
    c = case("5x63", s)
    T, B = c["lpn"].shape
    o = upgo_oracle64(*(c[k] for k in ARGS), **s)
    lpn = c["lpn"].to(D).requires_grad_(True)
    val = c["val"].to(D).requires_grad_(True)
    ent = c["ent"].to(D).requires_grad_(True)
    pg = -(lpn * o["adv"]).mean()
    up = -(lpn * o["upgo_adv"]).mean()
    vl = s["baseline_cost"] * ((o["vs"] - val[:T]) ** 2).mean()
    total = pg + s["upgo_cost"] * up + vl - s["entropy_cost"] * ent.mean()
    total.backward()
    torch.testing.assert_close(lpn.grad, o["g_logp"], rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(val.grad[:T], o["g_value"], rtol=1e-12, atol=1e-15)
    assert float(val.grad[T].abs().max()) == 0.0
    out = vtrace_upgo_torch(*(c[k] for k in ARGS), **kernel_kwargs(s))
    torch.testing.assert_close(ent.grad, torch.full_like(ent, out.g_ent), rtol=1e-12, atol=0)
    for got, want in zip(o["losses"][[0, 5, 1, 3]], (pg, up, vl, total)):
        torch.testing.assert_close(got, want.detach(), rtol=1e-12, atol=1e-15)
    torch.testing.assert_close(out.g_logp.to(D), lpn.grad, rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(out.g_value.to(D), val.grad, rtol=1e-4, atol=1e-8)


# -------------------------------------------------------------------------------- mutants
def test_the_recipe_sees_the_mutants():
    """Each wrong reading of the definitions moves the output it touches by more than 100x the
    comparison's atol (1e-4) on the recipe, so the oracle checks above would catch it. The two
    gate mutants move the upgoing return G itself; ``upgo_rho_bar`` swapped with ``pg_rho_bar``
    leaves G alone and moves upgo_adv and adv (G does not depend on a bar); lambda applied to
    delta in place of the trace leaves G alone and moves vs (G does not depend on lambda). The
    factors are printed, never used as a bound."""
    s = SETTINGS["nondefault"]
    c = case("37x300", s)
    a = [c[k] for k in ARGS]
    true = upgo_oracle64(*a, **s)
    moved = {}
    for m in ("gate_vt", "gate_g"):
        moved[m] = float((upgo_oracle64(*a, **s, mutant=m)["upgo"] - true["upgo"]).abs().max())
    sw = upgo_oracle64(*a, **dict(s, upgo_rho_bar=s["pg_rho_bar"], pg_rho_bar=s["upgo_rho_bar"]))
    assert torch.equal(sw["upgo"], true["upgo"]) and torch.equal(sw["vs"], true["vs"])
    moved["bars upgo_adv"] = float((sw["upgo_adv"] - true["upgo_adv"]).abs().max())
    moved["bars adv"] = float((sw["adv"] - true["adv"]).abs().max())
    ld = upgo_oracle64(*a, **s, mutant="lambda_on_delta")
    assert torch.equal(ld["upgo"], true["upgo"])
    moved["lambda_on_delta vs"] = float((ld["vs"] - true["vs"]).abs().max())
    for k, v in moved.items():
        print(f"{k}: moved by {v:.3g} = {v / 1e-4:.0f} x atol")
        assert v > 100 * 1e-4, k
    # and the search form of G is the recurrence
    c5 = case("64x257", s)
    a5 = [c5[k] for k in ARGS]
    val, r = c5["val"].to(D).numpy(), np.clip(c5["rew"].to(D).numpy(), -0.5, 0.5)
    disc = np.where(c5["done"].numpy(), 0.0, s["gamma"])
    G = np.empty_like(r)
    G[63] = r[63] + disc[63] * val[64]
    for t in range(62, -1, -1):
        q1 = r[t + 1] + disc[t + 1] * val[t + 2]
        G[t] = r[t] + disc[t] * np.where(q1 >= val[t + 1], G[t + 1], val[t + 1])
    np.testing.assert_allclose(upgo_oracle64(*a5, **s)["upgo"].numpy(), G, rtol=0, atol=1e-12)


# ---------------------------------------------------------------------- defaults untouched
def _boom(*a, **k):
    raise AssertionError("V-trace(lambda) / UPGO code ran at the default flags")


@pytest.mark.parametrize("algo", ["impala", "ppo"])
def test_default_update_runs_no_new_code(monkeypatch, algo):
    outs = []
    for patched in (False, True):
        if patched:
            monkeypatch.setattr(learner_mod, "vtrace_upgo", _boom)
            monkeypatch.setattr(V, "vtrace_upgo", _boom)
            monkeypatch.setattr(V, "vtrace_upgo_torch", _boom)
        torch.manual_seed(0)
        m = Agent((4, 4, 27))
        L = Learner(m, LearnerHParams(algo=algo), CPU)
        losses = L.learn(synthetic_batch(m, 8, 3, 16, seed=0)).clone()
        outs.append((losses, L.flat.data.clone()))
    assert outs[0][0].shape == ((5,) if algo == "impala" else (7,))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    hp = LearnerHParams()
    assert (hp.vtrace_lambda, hp.upgo_cost, hp.upgo_rho_bar) == (1.0, 0.0, 1.0)


def test_default_update_calls_vtrace_with_the_same_keywords(monkeypatch):
    """The default ``learn`` still calls ``vtrace`` with exactly today's keywords."""
    seen = []
    real = learner_mod.vtrace

    def rec(*a, **k):
        seen.append(sorted(k))
        return real(*a, **k)

    monkeypatch.setattr(learner_mod, "vtrace", rec)
    monkeypatch.setattr(learner_mod, "vtrace_upgo", _boom)
    torch.manual_seed(0)
    m = Agent((4, 4, 27))
    Learner(m, LearnerHParams(), CPU).learn(synthetic_batch(m, 8, 3, 16, seed=0))
    assert seen == [sorted(["gamma", "rho_bar", "c_bar", "pg_rho_bar", "baseline_cost",
                            "entropy_cost", "reward_clip", "ws"])]


# ---------------------------------------------------------------------- flags and refusals
REFUSED = [
    (dict(vtrace_lambda=-0.1), "--vtrace_lambda"),
    (dict(vtrace_lambda=1.5), "--vtrace_lambda"),
    (dict(vtrace_lambda=float("nan")), "--vtrace_lambda"),
    (dict(upgo_cost=-1.0), "--upgo_cost"),
    (dict(upgo_rho_bar=0.0), "--upgo_rho_bar"),
    (dict(upgo_rho_bar=-2.0), "--upgo_rho_bar"),
    (dict(algo="ppo", upgo_cost=0.5), "--algo ppo"),
    (dict(algo="ppo", vtrace_lambda=0.9), "--algo ppo"),
]


@pytest.mark.parametrize("kw,match", REFUSED)
def test_refusals(tmp_path, monkeypatch, kw, match):
    from microbeast_amd import train as train_mod
    from microbeast_amd.config import parse_flags
    with pytest.raises(ValueError, match=match):
        LearnerHParams(**kw)

    def started(*a, **k):
        raise AssertionError("train() got as far as starting a runtime")

    monkeypatch.setattr(train_mod.D, "init_distributed", started)
    argv = ["--savedir", str(tmp_path), "--exp_name", "x", "--device", "cpu", "--unroll_length", "8"]
    for k, v in kw.items():
        argv += ["--" + k, str(v)]
    with pytest.raises(ValueError, match=match):
        train_mod.train(parse_flags(argv, interactive=False))
    assert not list(tmp_path.iterdir())


def test_refusals_of_the_op():
    c = vtrace_recipe(5, 7)
    a = [c[k] for k in ARGS]
    for kw in (dict(lam=-0.1), dict(lam=1.1), dict(upgo_cost=-1.0), dict(upgo_rho_bar=0.0)):
        with pytest.raises(ValueError, match="vtrace_upgo"):
            vtrace_upgo_torch(*a, **kw)
    LearnerHParams(algo="ppo", upgo_rho_bar=2.0)  # (read by nothing while upgo_cost is 0)
    LearnerHParams(vtrace_lambda=0.0, upgo_cost=3.0, upgo_rho_bar=1e9)


@pytest.mark.parametrize("argv,which", [
    (["--vtrace_lambda", "0.9", "--upgo_cost", "0.7", "--upgo_rho_bar", "1.2"], "new"),
    (["--vtrace_lambda", "0.9"], "new"),
    (["--upgo_cost", "0.7"], "new"),
    (["--upgo_rho_bar", "1.2"], "old"),  # the bar of a term that is off
    ([], "old"),
])
def test_flags_reach_the_objective(monkeypatch, argv, which):
    from microbeast_amd import train as train_mod
    from microbeast_amd.config import parse_flags
    flags = parse_flags(argv + ["--gamma", "0.97", "--pg_rho_bar", "1.1"], interactive=False)
    hp = train_mod._hparams(flags)
    assert (hp.vtrace_lambda, hp.upgo_cost, hp.upgo_rho_bar) == (
        flags.vtrace_lambda, flags.upgo_cost, flags.upgo_rho_bar)
    calls = {"old": [], "new": []}
    for name, fn in (("old", learner_mod.vtrace), ("new", learner_mod.vtrace_upgo)):
        def rec(*a, _f=fn, _n=name, **k):
            calls[_n].append(k)
            return _f(*a, **k)
        monkeypatch.setattr(learner_mod, "vtrace" if name == "old" else "vtrace_upgo", rec)
    torch.manual_seed(0)
    m = Agent((4, 4, 27))
    L = Learner(m, hp, CPU)
    start = L.flat.data.clone()
    losses = L.learn(synthetic_batch(m, 8, 3, 16, seed=0))
    assert len(calls[which]) == 1 and not calls["old" if which == "new" else "new"]
    k = calls[which][0]
    assert k["gamma"] == 0.97 and k["pg_rho_bar"] == 1.1
    if which == "new":
        assert (k["lam"], k["upgo_cost"], k["upgo_rho_bar"]) == (
            flags.vtrace_lambda, flags.upgo_cost, flags.upgo_rho_bar)
        assert losses.shape == (6,)
    else:
        assert losses.shape == (5,) and "lam" not in k and "upgo_cost" not in k
    assert torch.isfinite(losses).all() and not torch.equal(L.flat.data, start)


# ---------------------------------------------------------------- one update vs autograd
def test_learner_update_matches_autograd_of_the_surrogate(monkeypatch):
    """One fp32 CPU update with vtrace_lambda 0.9, upgo_cost 1.0: the parameter gradient is
    autograd's of pg + upgo_cost upgo + value - entropy_cost H written out on the same model's
    outputs, with the targets from the fp64 oracle on those outputs (the same fp32 values, whose
    gates are checked to be clear of near-ties). Tolerance:
    tests/test_ppo_minibatch.py::test_first_block_step_matches_autograd's."""
    T, B, S = 8, 5, 16
    torch.manual_seed(3)
    m = Agent((4, 4, 27), hip_kernels=False)
    with torch.no_grad():
        m.actor.weight.normal_(0, 0.05)
    ref = copy.deepcopy(m)
    hp = LearnerHParams(vtrace_lambda=0.9, upgo_cost=1.0, lr=1e-3)
    L = Learner(m, hp, CPU)
    b = synthetic_batch(m, T, B, S, seed=1)
    b["logp"] = b["logp"] + 0.2 * torch.randn(T + 1, B, generator=torch.Generator().manual_seed(2))
    b["done"] = (torch.rand(T + 1, B, generator=torch.Generator().manual_seed(5)) < 0.1).to(torch.uint8)
    real_step = L.opt.step
    grads = []

    def keep(grad_scale=1.0):
        grads.append(L.flat.grad.clone())
        return real_step(grad_scale=grad_scale)

    monkeypatch.setattr(L.opt, "step", keep)
    start = L.flat.data.clone()
    losses = L.learn(b)
    assert losses.shape == (6,) and torch.isfinite(losses).all() and len(grads) == 1

    flat = lambda x, t: x[:t].reshape(t * B, *x.shape[2:])  # noqa: E731
    logp, ent, value = ref.evaluate(flat(b["obs"], T + 1), flat(b["mask"], T), flat(b["action"], T),
                                    n_score=T * B)
    logp, ent, value = logp.view(T, B), ent.view(T, B), value.view(T + 1, B)
    s = dict(gamma=hp.gamma, rho_bar=hp.rho_bar, c_bar=hp.c_bar, pg_rho_bar=hp.pg_rho_bar,
             baseline_cost=hp.baseline_cost, entropy_cost=hp.entropy_cost,
             reward_clip=hp.reward_clip, vtrace_lambda=0.9, upgo_cost=1.0, upgo_rho_bar=1.0)
    gate_margins(dict(val=value.detach(), rew=b["reward"][:T], done=b["done"][:T]), hp.gamma, 0.0)
    o = upgo_oracle64(logp.detach(), b["logp"][:T], value.detach(), b["reward"][:T], b["done"][:T],
                      ent.detach(), **s)
    assert float(o["losses"][4]) < 0.99  # the bar binds: the rollout is off-policy
    pg = -(logp * o["adv"].float()).mean()
    up = -(logp * o["upgo_adv"].float()).mean()
    vl = hp.baseline_cost * ((o["vs"].float() - value[:T]) ** 2).mean()
    total = pg + hp.upgo_cost * up + vl - hp.entropy_cost * ent.mean()
    torch.testing.assert_close(losses.double(), o["losses"], rtol=1e-4, atol=1e-5)
    params = list(ref.parameters())
    gr = torch.autograd.grad(total, params, retain_graph=True)
    atol_g = 2.0 ** -24 * max(float(gi.abs().max()) for gi in gr)
    for (_, off, n, _), gi in zip(L.flat.slices, gr):
        torch.testing.assert_close(grads[0][off:off + n].view_as(gi), gi, rtol=1e-4, atol=atol_g)
    # and without the UPGO term the gradient is another one
    gr0 = torch.autograd.grad(-(logp * o["adv"].float()).mean() + vl
                              - hp.entropy_cost * ent.mean(), params, allow_unused=True)
    assert max(float((x - y).abs().max()) for x, y in zip(gr, gr0) if y is not None) > 100 * atol_g
    assert not torch.equal(L.flat.data, start)


# ------------------------------------------------------------------------------- slow
def _rows(path):
    with open(path) as f:
        return list(csv.reader(f))


@pytest.mark.slow
def test_cli_upgo_on_the_mono_runtime(tmp_path):
    from microbeast_amd.cli import main
    from microbeast_amd.utils.metrics import LOSS_HEADER
    base = ["--env_size", "4", "--n_actors", "2", "--n_envs", "4", "--unroll_length", "8",
            "--batch_size", "2", "--savedir", str(tmp_path), "--device", "cpu", "--quiet",
            "--checkpoint_every", "2"]
    on = ["--exp_name", "u", "--upgo_cost", "1", "--vtrace_lambda", "0.9", *base]
    assert main(on + ["--max_updates", "2"]) == 0
    rows = _rows(tmp_path / "uLosses.csv")
    assert rows[0] == LOSS_HEADER + ["upgo_loss"] and len(rows) == 3
    for r in rows[1:]:
        assert len(r) == len(rows[0])
        for k in ("pg_loss", "value_loss", "entropy_loss", "total_loss", "mean_rho", "upgo_loss"):
            v = float(r[rows[0].index(k)])
            assert v == v and abs(v) < 1e9, (k, r)
    # --resume appends under the same header
    assert main(on + ["--max_updates", "3", "--resume"]) == 0
    rows = _rows(tmp_path / "uLosses.csv")
    assert rows[0] == LOSS_HEADER + ["upgo_loss"]
    assert [r[0] for r in rows[1:]] == ["1", "2", "3"] and len(rows[3]) == len(rows[0])
    # lambda alone: the IMPALA header; and a default run's header and row length are unchanged
    for name, extra in (("l", ["--vtrace_lambda", "0.9"]), ("d", [])):
        assert main(["--exp_name", name, "--max_updates", "1", *extra, *base]) == 0
        rows = _rows(tmp_path / f"{name}Losses.csv")
        assert rows[0] == LOSS_HEADER and len(rows) == 2 and len(rows[1]) == len(LOSS_HEADER)
