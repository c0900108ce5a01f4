"""The fp64 oracle and the shared cases of the V-trace-corrected PPO advantages (``--ppo_adv
vtrace``; tests/test_ppo_vtrace.py, tests/test_gpu_ppo_vtrace.py).

The oracle is written from the definitions as a double loop over (b, t), one scalar at a time:

    w_t   = exp(logp_pi_t - logp_mu_t)
    rho_t = min(rho_bar, w_t)            c_t = lambda * min(c_bar, w_t)
    td_t  = r_t + gamma nd_t v[t+1] - v[t]            (r_t clamped by reward_clip when > 0)
    adv_t = td_t + gamma nd_t lambda d_{t+1}          d_T = 0
    d_t   = rho_t td_t + gamma nd_t c_t d_{t+1}
    ret_t = v[t] + d_t
    stats = (mean adv, 1 / (std adv + 1e-8)), population std; (0, 1) with normalisation off
    is_stats = mean w, share of w > rho_bar, share of w > c_bar
"""
import math

import numpy as np
import torch

from ppo_cases import GAMMA, LAM, recipe

TOL = 1e-4  # rtol = atol of adv / ret: the bound tests/test_gpu_ppo.py uses for them

# (T, B, done_row); "all" = every done set
SHAPES = [(37, 300, None), (5, 259, None), (1, 1, None), (37, 300, 11), (37, 300, "all")]

DEFAULTS = dict(gamma=GAMMA, lam=LAM, rho_bar=1.0, c_bar=1.0, reward_clip=0.0, norm_adv=True)
SETTINGS = {
    "defaults": {},
    # three different numbers: a mixed-up bar misses by far more than the bound
    "mixed": dict(rho_bar=1.3, c_bar=0.9, gamma=0.97, reward_clip=0.5),
    "rho_below_one": dict(rho_bar=0.8),  # clips even w = 1
    "bars_off": dict(rho_bar=1e9, c_bar=1e9),
    "norm_off": dict(norm_adv=False),
}


def settings(name):
    return {**DEFAULTS, **SETTINGS[name]}


def case(T, B, done_row=None):
    """tests/ppo_cases.py:recipe, read as a lagged rollout: the learner's first-pass log-probs
    (``lpn``), the behaviour log-probs (``lpo``), the learner's values (``v_old``)."""
    all_done = done_row == "all"
    c = recipe(T, B, None if all_done else done_row)
    if all_done:
        c["done"][:] = True
    return c


def _np(x):
    return x.detach().cpu().to(torch.float64).numpy() if isinstance(x, torch.Tensor) \
        else np.asarray(x, dtype=np.float64)


def oracle64(logp_pi, logp_mu, v, reward, done, gamma, lam, rho_bar, c_bar, reward_clip=0.0,
             norm_adv=True):
    """fp64, scalar by scalar. Returns a dict of fp64 tensors: adv, ret, td, w, rho [T, B],
    stats [2], is_stats [3], and ``near`` = the share of elements whose |w - bar| / bar < 1e-4
    for either bar (where an fp32 w may fall on the other side)."""
    lp, lm, v, r, dn = _np(logp_pi), _np(logp_mu), _np(v), _np(reward), _np(done)
    T, B = lp.shape
    adv, ret, td_, w_, rho_ = (np.empty((T, B)) for _ in range(5))
    for b in range(B):
        d_next = 0.0
        for t in range(T - 1, -1, -1):
            w = math.exp(lp[t, b] - lm[t, b])
            rho = min(rho_bar, w)
            c = lam * min(c_bar, w)
            rt = r[t, b]
            if reward_clip > 0:
                rt = max(-reward_clip, min(reward_clip, rt))
            nd = 1.0 - dn[t, b]
            td = rt + gamma * nd * v[t + 1, b] - v[t, b]
            adv[t, b] = td + gamma * nd * lam * d_next
            d_next = rho * td + gamma * nd * c * d_next
            ret[t, b] = v[t, b] + d_next
            td_[t, b], w_[t, b], rho_[t, b] = td, w, rho
    M = float(T * B)
    if norm_adv:
        mean = adv.sum() / M
        std = math.sqrt(((adv - mean) ** 2).sum() / M)
        stats = np.array([mean, 1.0 / (std + 1e-8)])
    else:
        stats = np.array([0.0, 1.0])
    is_stats = np.array([w_.sum() / M, (w_ > rho_bar).sum() / M, (w_ > c_bar).sum() / M])
    near = ((np.abs(w_ - rho_bar) / rho_bar < 1e-4) | (np.abs(w_ - c_bar) / c_bar < 1e-4)).sum() / M
    t = torch.from_numpy
    return dict(adv=t(adv), ret=t(ret), td=t(td_), w=t(w_), rho=t(rho_), stats=t(stats),
                is_stats=t(is_stats), near=float(near))


_ORACLES = {}


def oracle_for(shape, name):
    """(case, oracle) of one (shape, setting): computed once and shared; treat both as read-only"""
    key = (shape, name)
    if key not in _ORACLES:
        c = case(*shape)
        s = settings(name)
        _ORACLES[key] = (c, oracle64(c["lpn"], c["lpo"], c["v_old"], c["rew"], c["done"], **s))
    return _ORACLES[key]


def check_against_oracle(g, is_stats, o, norm_adv):
    """adv / ret / normalised adv at TOL; the importance statistics: mean w at TOL, the two
    shares within the share of elements an fp32 w may put on the other side of a bar, which
    must stay <= 0.5 %."""
    f = lambda x: x.detach().cpu().to(torch.float64)  # noqa: E731
    adv, ret, stats, ist = f(g.adv), f(g.ret), f(g.stats), f(is_stats)
    torch.testing.assert_close(adv, o["adv"], rtol=TOL, atol=TOL)
    torch.testing.assert_close(ret, o["ret"], rtol=TOL, atol=TOL)
    torch.testing.assert_close((adv - stats[0]) * stats[1],
                               (o["adv"] - o["stats"][0]) * o["stats"][1], rtol=TOL, atol=TOL)
    if not norm_adv:
        assert stats.tolist() == [0.0, 1.0]
    assert ist.shape == (3,)
    torch.testing.assert_close(ist[0], o["is_stats"][0], rtol=TOL, atol=TOL)
    assert o["near"] <= 0.005
    assert float((ist[1:] - o["is_stats"][1:]).abs().max()) <= o["near"] + 1e-6
