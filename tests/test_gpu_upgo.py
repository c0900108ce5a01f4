"""vtrace.hip's mbk_vtrace_upgo on the MI355X (V-trace(lambda) targets + the UPGO term) against
the fp64 oracle (tests/upgo_cases.py) in poisoned buffers, from one lane to 66 partial rows, with
a done row and all dones; the exact case with its ties bit for bit; lambda = 1 without UPGO bit
equal to mbk_vtrace; optional outputs off; bit reproducibility; the launcher's refusals; one HIP
``Learner.learn`` with the term on; and ``--upgo_cost`` / ``--vtrace_lambda`` end to end on the
GPU runtime. Tolerances are those of test_gpu_vtrace.py; no element is left out (the cases'
gates are asserted to be clear of fp32 near-ties, upgo_cases.case)."""
import csv
import os

import pytest
import torch

from microbeast_amd import _native as N
from microbeast_amd.ops.vtrace import VTraceWorkspace, vtrace, vtrace_upgo
from objective_cases import DEFAULTS, NONDEFAULT
from upgo_cases import (EXACT, SETTINGS, SHAPES, UPGO_OFF, case, exact_case, gate_margins,
                        kernel_kwargs, oracle_for, upgo_oracle64)

pytestmark = pytest.mark.gpu

D = torch.float64
ARGS = ("lpn", "lpo", "val", "rew", "done", "ent")
RUNS = {"defaults": ("defaults", True), "nondefault": ("nondefault", True),
        "no-entropy": ("defaults", False)}
GPU_SHAPES = ["1x1", "2x1", "5x63", "64x257", "3x16641", "37x300-done-row", "9x300-all-done"]


def _run(c, dev, ws, s, use_ent=True, want_targets=True):
    """One launch with the partial rows, the losses and the bootstrap gradient row poisoned."""
    T, B = c["lpn"].shape
    nan = float("nan")
    ws.get("upgo_partials", (((B + 255) // 256) * 5,), dev).fill_(nan)
    ws.get("upgo_g_value", (T + 1, B), dev).fill_(nan)
    ws.get("upgo_losses", (6,), dev).fill_(nan)
    d = {k: v.to(dev) for k, v in c.items()}
    return vtrace_upgo(d["lpn"], d["lpo"], d["val"], d["rew"], d["done"],
                       d["ent"] if use_ent else None, want_targets=want_targets, ws=ws,
                       **kernel_kwargs(s))


def _snap(out):
    return [t.clone() for t in (out.g_logp, out.g_value, out.losses)]


@pytest.mark.parametrize("run", list(RUNS))
@pytest.mark.parametrize("shape", GPU_SHAPES)
def test_upgo_kernel_vs_oracle64(cuda, shape, run):
    setting, use_ent = RUNS[run]
    s = SETTINGS[setting]
    c, ref = oracle_for(shape, setting, use_ent)
    T, B = c["lpn"].shape
    ws = VTraceWorkspace()
    out = _run(c, cuda, ws, s, use_ent)
    vs, adv, G = out.vs.cpu().to(D), out.adv.cpu().to(D), out.upgo.cpu().to(D)
    gl, gv, losses = out.g_logp.cpu().to(D), out.g_value.cpu().to(D), out.losses.cpu().to(D)
    print(f"{shape} {run}: max |err| vs {float((vs - ref['vs']).abs().max()):.3g} "
          f"adv {float((adv - ref['adv']).abs().max()):.3g} "
          f"upgo {float((G - ref['upgo']).abs().max()):.3g} "
          f"g_logp {float((gl - ref['g_logp']).abs().max()):.3g} "
          f"losses {(losses - ref['losses']).abs().tolist()}")
    assert gl.shape == (T, B) and gv.shape == (T + 1, B) and losses.shape == (6,)
    torch.testing.assert_close(vs, ref["vs"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(adv, ref["adv"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(G, ref["upgo"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(gl, ref["g_logp"], rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(gv[:T], ref["g_value"], rtol=1e-4, atol=1e-8)
    assert float(gv[T].abs().max()) == 0.0  # (poisoned with NaN before the call)
    torch.testing.assert_close(losses, ref["losses"], rtol=1e-4, atol=1e-5)
    if not use_ent:
        assert float(losses[2]) == 0.0
    assert out.g_ent == -s["entropy_cost"] / float(T * B)
    if SHAPES[shape][3]:  # all dones: G_t = r_t
        r = c["rew"].to(D)
        r = r.clamp(-s["reward_clip"], s["reward_clip"]) if s["reward_clip"] > 0 else r
        assert torch.equal(G, r)
    # the targets are optional outputs: without them the gradients and losses are the same bits
    snap = _snap(out)
    out2 = _run(c, cuda, ws, s, use_ent, want_targets=False)
    assert out2.vs is None and out2.adv is None and out2.upgo is None
    for a, b in zip(snap, _snap(out2)):
        assert torch.equal(a, b)


def test_upgo_kernel_exact_case(cuda):
    """Every fp32 operation of the scan is exact on this case, so the kernel's numbers are the
    fp64 oracle's bit for bit; 24 of its gates are exact ties, which ``>=`` keeps open."""
    c, ties = exact_case()
    T = c["lpn"].shape[0]
    ref = upgo_oracle64(*(c[k] for k in ARGS), **EXACT)
    out = _run(c, cuda, VTraceWorkspace(), EXACT)
    for k, t in (("vs", out.vs), ("upgo", out.upgo), ("adv", out.adv), ("g_logp", out.g_logp),
                 ("g_value", out.g_value[:T])):
        assert torch.equal(t.cpu(), ref[k].float()), k
    assert float(out.g_value[T].abs().max()) == 0.0
    strict = upgo_oracle64(*(c[k] for k in ARGS), **EXACT, mutant="strict")
    for s, b in ties:
        assert float(out.upgo[s - 1, b]) != float(strict["upgo"][s - 1, b])


@pytest.mark.parametrize("kw", [DEFAULTS, NONDEFAULT], ids=["defaults", "nondefault"])
def test_lambda_one_without_upgo_is_mbk_vtrace(cuda, kw):
    s = dict(kw, **UPGO_OFF)
    c = case("37x300", s)
    d = {k: v.to(cuda) for k, v in c.items()}
    ws = VTraceWorkspace()
    old = vtrace(*(d[k] for k in ARGS), want_targets=True, ws=ws, **kw)
    new = _run(c, cuda, ws, s)
    for k, x, y in (("g_logp", old.g_logp, new.g_logp), ("g_value", old.g_value, new.g_value),
                    ("vs", old.vs, new.vs), ("adv", old.adv, new.adv),
                    ("losses", old.losses, new.losses[:5])):
        assert torch.equal(x, y), k
    assert torch.isfinite(new.losses[5])
    # (and the bar of a term that is off changes no gradient bit)
    other = _run(c, cuda, ws, dict(s, upgo_rho_bar=1.7))
    assert torch.equal(other.g_logp, old.g_logp)


@pytest.mark.parametrize("setting", list(SETTINGS))
def test_upgo_kernel_is_bit_reproducible(cuda, setting):
    s = SETTINGS[setting]
    c = case("37x300", s)
    ws = VTraceWorkspace()
    full = lambda o: _snap(o) + [o.vs.clone(), o.adv.clone(), o.upgo.clone()]  # noqa: E731
    a = full(_run(c, cuda, ws, s))
    b = full(_run(c, cuda, ws, s))
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # the same workspace at another B (buffers re-sized), then back
    _run(case("3x16641", s), cuda, ws, s)
    _run(case("5x63", s), cuda, ws, s)
    for x, y in zip(a, full(_run(c, cuda, ws, s))):
        assert torch.equal(x, y)


def test_launcher_refusals(cuda):
    """By return code only: nothing is launched and no pointer is read."""
    x = torch.zeros(8, device=cuda)
    p = x.data_ptr()

    def rc(T=4, B=2, lam=1.0, cost=0.0, bar=1.0):
        return N.kernels().mbk_vtrace_upgo(p, p, p, p, p, p, T, B, 0.99, lam, 1.0, 1.0, 1.0, bar,
                                           0.5, 0.01, cost, 0.0, p, p, p, p, p, p, p,
                                           N.stream_ptr())

    nan = float("nan")
    for kw in (dict(T=0), dict(T=-1), dict(B=0), dict(lam=-0.1), dict(lam=1.5), dict(lam=nan),
               dict(cost=-1.0), dict(cost=nan), dict(bar=0.0), dict(bar=-1.0), dict(bar=nan)):
        assert rc(**kw) == 1, kw  # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0
    c = case("5x63", SETTINGS["defaults"])
    d = {k: v.to(cuda) for k, v in c.items()}
    with pytest.raises(ValueError, match="vtrace_upgo"):  # values without the bootstrap row
        vtrace_upgo(d["lpn"], d["lpo"], d["val"][:5], d["rew"], d["done"], upgo_cost=1.0)
    for kw in (dict(lam=1.5), dict(upgo_cost=-1.0), dict(upgo_rho_bar=0.0)):
        with pytest.raises(RuntimeError, match="vtrace_upgo failed with hipError 1$"):
            vtrace_upgo(*(d[k] for k in ARGS), **kw)


# ----------------------------------------------------------------------------- learner
def test_upgo_learner_update_on_the_device(cuda, monkeypatch):
    """One HIP ``Learner.learn`` with vtrace_lambda 0.9, upgo_cost 1.0 on a real engine rollout
    whose behaviour log-probs are perturbed: the objective is called once with the learner's
    values, and the gradients it seeds the backward with are the fp64 oracle's on the very
    inputs it was given. (Not compared against an fp32 CPU learner end to end: bf16 values flip
    near-tie gates, and no tolerance for that has been measured.)"""
    from helpers import engine_batches
    from microbeast_amd import learner as learner_mod
    from microbeast_amd.learner import Learner, LearnerHParams
    from microbeast_amd.models.agent import Agent
    b = engine_batches(cuda, 8, 2, groups=4, envs=64, T=8, seed=8)[1]
    noise = 0.2 * torch.randn(b["logp"].shape, generator=torch.Generator().manual_seed(11))
    b["logp"] = b["logp"] + noise.to(cuda)
    torch.manual_seed(7)
    L = Learner(Agent((8, 8, 27)), LearnerHParams(vtrace_lambda=0.9, upgo_cost=1.0, gamma=0.97,
                                                  pg_rho_bar=1.1), cuda)
    real = learner_mod.vtrace_upgo
    seen = []

    def rec(*a, **k):
        o = real(*a, **k)
        seen.append(([x.detach().float().cpu().clone() for x in a], dict(k),
                     o.g_logp.cpu().clone(), o.g_value.cpu().clone()))
        return o

    monkeypatch.setattr(learner_mod, "vtrace_upgo", rec)
    start = L.flat.data.clone()
    losses = L.learn(b).cpu()
    assert len(seen) == 1 and L.opt.step_count == 1 and L.n_updates == 1
    a, k, gl, gv = seen[0]
    assert (k["lam"], k["upgo_cost"], k["upgo_rho_bar"], k["gamma"], k["pg_rho_bar"]) == (
        0.9, 1.0, 1.0, 0.97, 1.1) and k["ws"] is L.ws
    lpn, lpo, val, rew, done, ent = a
    T, B = lpn.shape
    assert val.shape == (T + 1, B) and T == 8
    margin, bound, share = gate_margins(dict(val=val, rew=rew, done=done), 0.97, 0.0)
    print(f"gates: smallest margin {margin:.3g}, largest bound {bound:.3g}, open {share:.3f}")
    hp = L.hp
    o = upgo_oracle64(lpn, lpo, val, rew, done, ent, gamma=hp.gamma, rho_bar=hp.rho_bar,
                      c_bar=hp.c_bar, pg_rho_bar=hp.pg_rho_bar, baseline_cost=hp.baseline_cost,
                      entropy_cost=hp.entropy_cost, reward_clip=hp.reward_clip, vtrace_lambda=0.9,
                      upgo_cost=1.0, upgo_rho_bar=1.0)
    print(f"losses {losses.tolist()}\noracle {o['losses'].tolist()}")
    torch.testing.assert_close(gl.to(D), o["g_logp"], rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(gv[:T].to(D), o["g_value"], rtol=1e-4, atol=1e-8)
    assert float(gv[T].abs().max()) == 0.0
    assert losses.shape == (6,) and torch.isfinite(losses).all()
    torch.testing.assert_close(losses.to(D), o["losses"], rtol=1e-4, atol=1e-5)
    assert not torch.equal(L.flat.data, start)


# --------------------------------------------------------------------------------- CLI
def _rows(path):
    with open(path) as f:
        return list(csv.DictReader(f))


def test_gpu_cli_upgo_train_and_eval(cuda, tmp_path):
    from microbeast_amd.cli import main
    from microbeast_amd.utils.checkpoint import load_checkpoint
    from microbeast_amd.utils.metrics import LOSS_HEADER
    args = ["--exp_name", "u", "--runtime", "gpu", "--env_size", "8", "--groups", "2",
            "--envs_per_group", "32", "--unroll_length", "8", "--batch_size", "1",
            "--savedir", str(tmp_path), "--quiet", "--max_episode_steps", "10"]
    assert main(args + ["--upgo_cost", "1", "--vtrace_lambda", "0.9", "--max_updates", "3",
                        "--checkpoint_every", "2"]) == 0
    ck = load_checkpoint(os.path.join(tmp_path, "u.ckpt"))
    assert ck["n_update"] == 3 and ck["optimizer_state_dict"]["step"] == 3
    with open(tmp_path / "uLosses.csv") as f:
        assert f.readline().strip().split(",") == LOSS_HEADER + ["upgo_loss"]
    loss = _rows(tmp_path / "uLosses.csv")
    assert [int(r["update"]) for r in loss] == [1, 2, 3]
    for r in loss:
        for k in ("pg_loss", "value_loss", "entropy_loss", "total_loss", "mean_rho", "upgo_loss"):
            v = float(r[k])
            assert v == v and abs(v) < 1e9, (k, r)
    assert main(args + ["--test", "--eval_envs", "16"]) == 0
    assert len(_rows(tmp_path / "u_eval.csv")) == 16
