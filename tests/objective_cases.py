"""Shared inputs and fp64 oracles of the V-trace and Adam tests (test_vtrace.py, test_optim.py,
test_learner.py, test_gpu_vtrace.py, test_gpu_adam.py). Written from the definitions (Espeholt
et al. 2018; Kingma & Ba 2015), not from ops/vtrace.py or ops/optim.py, whose internals are fp32."""
import math

import numpy as np
import torch

# the non-default V-trace settings the CPU and GPU tests share: three different bars (a kernel
# that mixes them up is off by far more than any tolerance), and every other knob off its default
NONDEFAULT = dict(gamma=0.97, rho_bar=1.3, c_bar=0.9, pg_rho_bar=1.1, baseline_cost=0.25,
                  entropy_cost=0.02, reward_clip=0.5)
DEFAULTS = dict(gamma=0.99, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, baseline_cost=0.5,
                entropy_cost=0.01, reward_clip=0.0)


def vtrace_recipe(T, B, seed=0, done_row=None):
    """The V-trace kernel test's inputs (tests/test_gpu_kernels.py): seed 0 gives the same
    arrays. ``done_row`` sets that one row of ``done`` to all ones."""
    g = torch.Generator().manual_seed(seed)
    lpn = torch.randn(T, B, generator=g) * 0.3 - 5
    lpo = lpn + torch.randn(T, B, generator=g) * 0.2
    val = torch.randn(T + 1, B, generator=g)
    rew = torch.randn(T, B, generator=g)
    done = torch.rand(T, B, generator=g) < 0.05
    ent = torch.rand(T, B, generator=g) * 3
    if done_row is not None:
        done[done_row] = True
    return dict(lpn=lpn, lpo=lpo, val=val, rew=rew, done=done, ent=ent)


def _np64(x):
    return x.detach().cpu().to(torch.float64).numpy() if isinstance(x, torch.Tensor) \
        else np.asarray(x, dtype=np.float64)


def vtrace_oracle64(lpn, lpo, val, rew, done, ent, gamma, rho_bar, c_bar, pg_rho_bar,
                    baseline_cost, entropy_cost, reward_clip):
    """fp64 V-trace targets, the IMPALA losses and their gradients, by the reverse recurrence
    vs_t - V_t = delta_t + gamma_t c_t (vs_{t+1} - V_{t+1}). Returns a dict of fp64 tensors:
    vs, adv, g_logp [T, B], g_value [T, B] (rows < T; the bootstrap row has no gradient) and
    losses [5] = pg, value, entropy, total, mean rho."""
    lpn, lpo, val, rew = _np64(lpn), _np64(lpo), _np64(val), _np64(rew)
    notdone = 1.0 - _np64(done)
    T, B = lpn.shape
    ratio = np.exp(lpn - lpo)
    rho = np.minimum(rho_bar, ratio)
    c = np.minimum(c_bar, ratio)
    pg_rho = np.minimum(pg_rho_bar, ratio)
    r = np.clip(rew, -reward_clip, reward_clip) if reward_clip > 0 else rew
    disc = gamma * notdone
    vs = np.empty((T + 1, B))
    vs[T] = val[T]
    for t in range(T - 1, -1, -1):
        delta = rho[t] * (r[t] + disc[t] * val[t + 1] - val[t])
        vs[t] = val[t] + delta + disc[t] * c[t] * (vs[t + 1] - val[t + 1])
    adv = pg_rho * (r + disc * vs[1:] - val[:T])
    M = float(T * B)
    pg = -(lpn * adv).sum() / M
    vl = baseline_cost * ((vs[:T] - val[:T]) ** 2).sum() / M
    e = _np64(ent).sum() / M if ent is not None else 0.0
    losses = np.array([pg, vl, e, pg + vl - entropy_cost * e, rho.sum() / M])
    t = torch.from_numpy
    return dict(vs=t(vs[:T].copy()), adv=t(adv), g_logp=t(-adv / M),
                g_value=t(2.0 * baseline_cost * (val[:T] - vs[:T]) / M), losses=t(losses))


class adam_oracle64:
    """fp64 Adam over one flat vector: torch.optim.Adam(weight_decay=wd) semantics after
    clip_grad_norm_. One step: g * grad_scale -> global-norm clip min(1, max / (norm + 1e-6))
    (max_grad_norm > 0) -> + wd * p -> Adam with bias correction. ``last_grad_norm`` is the
    norm of g * grad_scale."""

    def __init__(self, p, lr=2.5e-4, betas=(0.9, 0.999), eps=1e-5, wd=0.0, max_grad_norm=0.0,
                 m=None, v=None, step=0):
        self.p = p.detach().cpu().to(torch.float64).clone()
        self.m = torch.zeros_like(self.p) if m is None else m.detach().cpu().to(torch.float64).clone()
        self.v = torch.zeros_like(self.p) if v is None else v.detach().cpu().to(torch.float64).clone()
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, wd
        self.max_grad_norm = max_grad_norm
        self.step_count = int(step)
        self.last_grad_norm = None
        self.last_clip = 1.0

    def step(self, grad, grad_scale=1.0):
        g = grad.detach().cpu().to(torch.float64) * grad_scale
        norm = float(g.pow(2).sum().sqrt())
        self.last_grad_norm = norm
        self.last_clip = min(1.0, self.max_grad_norm / (norm + 1e-6)) if self.max_grad_norm > 0 else 1.0
        g = g * self.last_clip
        if self.wd:
            g = g + self.wd * self.p
        self.step_count += 1
        b1, b2 = self.betas
        self.m = b1 * self.m + (1.0 - b1) * g
        self.v = b2 * self.v + (1.0 - b2) * g * g
        bc1 = 1.0 - b1 ** self.step_count
        bc2 = 1.0 - b2 ** self.step_count
        self.p = self.p - (self.lr / bc1) * self.m / (self.v.sqrt() / math.sqrt(bc2) + self.eps)
        return self.p
