"""V-trace + losses vs a straightforward NumPy double-loop oracle (Espeholt et al. 2018)."""
import numpy as np
import torch

from microbeast_amd.ops.vtrace import vtrace_torch
from objective_cases import DEFAULTS, NONDEFAULT, vtrace_oracle64, vtrace_recipe


def _oracle(lpn, lpo, values, rewards, dones, gamma, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0,
            reward_clip=0.0):
    T, B = lpn.shape
    ratio = np.exp(lpn - lpo)
    rho = np.minimum(rho_bar, ratio)
    c = np.minimum(c_bar, ratio)
    if reward_clip > 0:
        rewards = np.clip(rewards, -reward_clip, reward_clip)
    disc = gamma * (1.0 - dones)
    v = values[:T]
    v_next = values[1:T + 1]
    vs = np.zeros((T, B))
    for b in range(B):
        for s in range(T):
            acc = 0.0
            prod = 1.0
            gpow = 1.0
            for t in range(s, T):
                delta = rho[t, b] * (rewards[t, b] + disc[t, b] * v_next[t, b] - v[t, b])
                acc += gpow * prod * delta
                prod *= c[t, b]
                gpow *= disc[t, b]
            vs[s, b] = v[s, b] + acc
    vs_next = np.concatenate([vs[1:], values[T:T + 1]], 0)
    adv = np.minimum(pg_rho_bar, ratio) * (rewards + disc * vs_next - v)
    return vs, adv


def test_vtrace_matches_oracle():
    rng = np.random.default_rng(0)
    T, B = 9, 5
    lpn = rng.normal(-3, 0.3, (T, B))
    lpo = lpn + rng.normal(0, 0.3, (T, B))
    values = rng.normal(0, 1, (T + 1, B))
    rewards = rng.normal(0, 1, (T, B))
    dones = (rng.random((T, B)) < 0.2).astype(np.float64)
    vs, adv = _oracle(lpn, lpo, values, rewards, dones, 0.99)
    out = vtrace_torch(torch.tensor(lpn, dtype=torch.float32), torch.tensor(lpo, dtype=torch.float32),
                       torch.tensor(values, dtype=torch.float32), torch.tensor(rewards, dtype=torch.float32),
                       torch.tensor(dones.astype(bool)), None, gamma=0.99)
    np.testing.assert_allclose(out.vs.numpy(), vs, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out.adv.numpy(), adv, rtol=1e-4, atol=1e-4)


def test_gradients_equal_autograd_of_losses():
    torch.manual_seed(0)
    T, B = 6, 4
    lpn = (torch.randn(T, B) - 3).requires_grad_(True)
    lpo = lpn.detach() + 0.1 * torch.randn(T, B)
    val = torch.randn(T + 1, B, requires_grad=True)
    rew = torch.randn(T, B)
    done = torch.rand(T, B) < 0.2
    ent = torch.rand(T, B, requires_grad=True)
    out = vtrace_torch(lpn, lpo, val, rew, done, ent, baseline_cost=0.5, entropy_cost=0.01)
    vs, adv = out.vs.detach(), out.adv.detach()
    pg = -(lpn * adv).mean()                      # correct sign (reference D4 had +)
    vl = 0.5 * ((vs - val[:T]) ** 2).mean()        # reference libs/utils.py:323
    el = ent.mean()
    total = pg + vl - 0.01 * el
    total.backward()
    torch.testing.assert_close(lpn.grad, out.g_logp)
    torch.testing.assert_close(val.grad, out.g_value)
    torch.testing.assert_close(ent.grad, torch.full_like(ent, out.g_ent))
    torch.testing.assert_close(out.losses[3], total.detach(), rtol=1e-5, atol=1e-6)


def _small(T=9, B=5, seed=1):
    """Small fp64 inputs with wide importance ratios (most of the bars bind somewhere)."""
    rng = np.random.default_rng(seed)
    lpn = rng.normal(-3, 0.3, (T, B))
    lpo = lpn + rng.normal(0, 0.3, (T, B))
    values = rng.normal(0, 1, (T + 1, B))
    rewards = rng.normal(0, 1, (T, B))
    dones = (rng.random((T, B)) < 0.2).astype(np.float64)
    ent = rng.random((T, B)) * 3
    return lpn, lpo, values, rewards, dones, ent


def _f32(x):
    return torch.tensor(x, dtype=torch.float32)


def _assert_matches64(out, ref, T):
    """The V-trace kernel test's tolerances (tests/test_gpu_kernels.py), against fp64."""
    d = torch.float64
    torch.testing.assert_close(out.vs.to(d), ref["vs"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.adv.to(d), ref["adv"], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(out.g_logp.to(d), ref["g_logp"], rtol=1e-4, atol=1e-8)
    torch.testing.assert_close(out.g_value[:T].to(d), ref["g_value"], rtol=1e-4, atol=1e-8)
    assert float(out.g_value[T].abs().max()) == 0.0
    torch.testing.assert_close(out.losses.to(d), ref["losses"], rtol=1e-4, atol=1e-5)


def test_vtrace_nondefault_settings_match_both_oracles():
    """Three different bars, gamma, both costs and the reward clip off their defaults: the
    double loop pins the recurrence, vtrace_oracle64 (checked here against the double loop in
    fp64) pins vtrace_torch including the losses and gradients."""
    lpn, lpo, values, rewards, dones, ent = _small()
    T = lpn.shape[0]
    nd = NONDEFAULT
    vs, adv = _oracle(lpn, lpo, values, rewards, dones, nd["gamma"], nd["rho_bar"], nd["c_bar"],
                      nd["pg_rho_bar"], nd["reward_clip"])
    ref = vtrace_oracle64(lpn, lpo, values, rewards, dones, ent, **nd)
    np.testing.assert_allclose(ref["vs"].numpy(), vs, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(ref["adv"].numpy(), adv, rtol=1e-12, atol=1e-12)
    # (the inputs rounded to fp32 first, so only vtrace_torch's own arithmetic is compared)
    args32 = [_f32(lpn), _f32(lpo), _f32(values), _f32(rewards)]
    ref32 = vtrace_oracle64(*args32, dones, _f32(ent), **nd)
    out = vtrace_torch(*args32, torch.tensor(dones.astype(bool)), _f32(ent), **nd)
    np.testing.assert_allclose(out.vs.numpy(), vs, rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(out.adv.numpy(), adv, rtol=1e-4, atol=1e-4)
    _assert_matches64(out, ref32, T)
    assert out.g_ent == -nd["entropy_cost"] / (T * lpn.shape[1])


def test_vtrace_recipe_matches_oracle64_and_sees_swapped_bars():
    """vtrace_torch against vtrace_oracle64 on the kernel test's recipe at the defaults and at
    the non-default set; and the recipe can see a mixed-up bar: with the bars permuted the fp64
    targets move by more than 100x the tolerance (1e-4)."""
    c = vtrace_recipe(37, 300)
    a = (c["lpn"], c["lpo"], c["val"], c["rew"], c["done"], c["ent"])
    for kw in (dict(), NONDEFAULT):
        _assert_matches64(vtrace_torch(*a, **kw), vtrace_oracle64(*a, **dict(DEFAULTS, **kw)), 37)
    true = vtrace_oracle64(*a, **NONDEFAULT)
    swapped = vtrace_oracle64(*a, **dict(NONDEFAULT, rho_bar=NONDEFAULT["c_bar"],
                                         c_bar=NONDEFAULT["rho_bar"]))
    assert float((swapped["vs"] - true["vs"]).abs().max()) > 100 * 1e-4
    pg_as_rho = vtrace_oracle64(*a, **dict(NONDEFAULT, pg_rho_bar=NONDEFAULT["rho_bar"]))
    assert float((pg_as_rho["adv"] - true["adv"]).abs().max()) > 100 * 1e-4
    assert torch.equal(pg_as_rho["vs"], true["vs"])
    unclipped = vtrace_oracle64(*a, **dict(NONDEFAULT, reward_clip=0.0))
    assert float((unclipped["vs"] - true["vs"]).abs().max()) > 100 * 1e-4


def test_vtrace_without_entropy():
    c = vtrace_recipe(9, 7, seed=3)
    a = (c["lpn"], c["lpo"], c["val"], c["rew"], c["done"])
    out = vtrace_torch(*a, None, **NONDEFAULT)
    _assert_matches64(out, vtrace_oracle64(*a, None, **NONDEFAULT), 9)
    assert float(out.losses[2]) == 0.0
    assert float(out.losses[3]) == float(out.losses[0] + out.losses[1])
    with_ent = vtrace_torch(*a, c["ent"], **NONDEFAULT)
    assert torch.equal(with_ent.g_logp, out.g_logp) and torch.equal(with_ent.g_value, out.g_value)


def test_gradients_equal_autograd_of_losses_nondefault():
    torch.manual_seed(1)
    T, B = 6, 4
    nd = NONDEFAULT
    lpn = (torch.randn(T, B) - 3).requires_grad_(True)
    lpo = lpn.detach() + 0.3 * torch.randn(T, B)
    val = torch.randn(T + 1, B, requires_grad=True)
    rew = torch.randn(T, B)
    done = torch.rand(T, B) < 0.2
    ent = torch.rand(T, B, requires_grad=True)
    out = vtrace_torch(lpn, lpo, val, rew, done, ent, **nd)
    vs, adv = out.vs.detach(), out.adv.detach()
    pg = -(lpn * adv).mean()
    vl = nd["baseline_cost"] * ((vs - val[:T]) ** 2).mean()
    total = pg + vl - nd["entropy_cost"] * ent.mean()
    total.backward()
    torch.testing.assert_close(lpn.grad, out.g_logp)
    torch.testing.assert_close(val.grad, out.g_value)
    torch.testing.assert_close(ent.grad, torch.full_like(ent, out.g_ent))
    torch.testing.assert_close(out.losses[3], total.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out.losses[0], pg.detach(), rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(out.losses[1], vl.detach(), rtol=1e-5, atol=1e-6)
