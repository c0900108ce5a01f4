"""Learner: parameters actually change (reference D1) and a learnable task is learned
(proves the sign / alignment fixes, reference D3/D4)."""
import copy

import pytest
import torch

from microbeast_amd.learner import Learner, LearnerHParams
from microbeast_amd.models.agent import Agent

from helpers import synthetic_batch


def test_update_changes_weights_and_grads_are_views():
    torch.manual_seed(0)
    m = Agent((4, 4, 27))
    L = Learner(m, LearnerHParams(), torch.device("cpu"))
    before = {k: v.clone() for k, v in m.state_dict().items()}
    losses = L.learn(synthetic_batch(m, 8, 3, 16, seed=0))
    assert torch.isfinite(losses).all()
    changed = [k for k, v in m.state_dict().items() if not torch.equal(v, before[k])]
    assert "actor.weight" in changed and "network.0.conv.weight" in changed
    assert L.flat.check_grad_views()


def test_learns_to_prefer_rewarded_action():
    """Reward 1 whenever cell 0's action type is 2; its probability must rise a lot."""
    torch.manual_seed(0)
    m = Agent((4, 4, 27))
    L = Learner(m, LearnerHParams(lr=3e-3, entropy_cost=0.0), torch.device("cpu"))
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
        L.learn(b)
    p1 = prob()
    assert p0 < 0.2 and p1 > p0 + 0.3, (p0, p1)


# --- the objective's flags reach the kernels' arguments (CPU path; 8x8 map) ---

def _wiring(seed=0, scale_reward=1.0, jitter_logp=0.0):
    torch.manual_seed(seed)
    m = Agent((8, 8, 27))
    with torch.no_grad():  # (the actor starts at zero weights: give the head some signal)
        m.actor.weight.normal_(0, 0.02)
        m.actor.bias.normal_(0, 0.02)
    b = synthetic_batch(m, 8, 3, 64, seed=seed)
    b["reward"] = b["reward"] * scale_reward
    if jitter_logp:
        g = torch.Generator().manual_seed(seed + 1)
        b["logp"] = b["logp"] + torch.randn(b["logp"].shape, generator=g) * jitter_logp
    return m, b


@pytest.mark.parametrize("algo", ["impala", "ppo"])
def test_reward_clip_equals_preclamped_rewards(algo):
    c = 0.5
    m, b = _wiring(scale_reward=50.0)
    assert float((b["reward"].abs() > c).float().mean()) > 0.9
    La = Learner(copy.deepcopy(m), LearnerHParams(algo=algo, reward_clip=c), torch.device("cpu"))
    Lb = Learner(copy.deepcopy(m), LearnerHParams(algo=algo), torch.device("cpu"))
    Lc = Learner(copy.deepcopy(m), LearnerHParams(algo=algo), torch.device("cpu"))
    la = La.learn(b)
    lb = Lb.learn(dict(b, reward=b["reward"].clamp(-c, c)))
    lc = Lc.learn(b)
    assert torch.equal(la, lb) and torch.equal(La.flat.data, Lb.flat.data)
    assert not torch.equal(la, lc)  # and the clip does something on this batch


def test_max_grad_norm_clips_the_learners_own_gradient():
    from objective_cases import adam_oracle64
    m, b = _wiring()
    L0 = Learner(copy.deepcopy(m), LearnerHParams(), torch.device("cpu"))
    L0.learn(b)
    norm = float(L0.flat.grad.double().norm())
    assert L0.opt.last_grad_norm is None
    hp = LearnerHParams(max_grad_norm=0.3 * norm)
    L = Learner(copy.deepcopy(m), hp, torch.device("cpu"))
    p0 = L.flat.data.clone()
    L.learn(b)
    assert torch.equal(L.flat.grad, L0.flat.grad)
    assert float(L.opt.last_grad_norm) == float(L.flat.grad.norm())
    ora = adam_oracle64(p0, lr=hp.lr, eps=hp.adam_eps, max_grad_norm=hp.max_grad_norm)
    ora.step(L.flat.grad)
    assert abs(ora.last_clip - 0.3) < 1e-3
    torch.testing.assert_close(L.flat.data.double(), ora.p, rtol=1e-4, atol=1e-5)
    assert not torch.equal(L.flat.data, L0.flat.data)


def test_vtrace_bars_reach_the_objective():
    from microbeast_amd.ops.vtrace import vtrace_torch
    m, b = _wiring(jitter_logp=0.3)
    bars = dict(rho_bar=1.3, c_bar=0.9, pg_rho_bar=1.1)
    ld = Learner(copy.deepcopy(m), LearnerHParams(), torch.device("cpu")).learn(b)
    lb = Learner(copy.deepcopy(m), LearnerHParams(**bars), torch.device("cpu")).learn(b)
    assert not torch.equal(ld[:2], lb[:2]) and float(lb[4]) > float(ld[4])
    T, B, S = 8, 3, 64
    ref = copy.deepcopy(m)
    with torch.no_grad():
        logp, ent, value = ref.evaluate(b["obs"].reshape((T + 1) * B, S),
                                        b["mask"][:T].reshape(T * B, S, 3),
                                        b["action"][:T].reshape(T * B, S, 7), n_score=T * B)
    for kw, got in ((dict(), ld), (bars, lb)):
        want = vtrace_torch(logp.view(T, B), b["logp"][:T], value.view(T + 1, B), b["reward"][:T],
                            b["done"][:T], ent.view(T, B), **kw).losses
        assert torch.equal(got, want)
    # each bar on its own moves the losses it should: c_bar and rho_bar the value loss,
    # pg_rho_bar only the policy-gradient loss
    one = lambda **kw: Learner(copy.deepcopy(m), LearnerHParams(**kw), torch.device("cpu")).learn(b)  # noqa: E731
    lp = one(pg_rho_bar=1.1)
    assert float(lp[1]) == float(ld[1]) and float(lp[0]) != float(ld[0])
    assert float(one(c_bar=0.9)[1]) != float(ld[1])
    assert float(one(rho_bar=1.3)[4]) > float(ld[4])
