"""V-trace targets + IMPALA losses + the loss gradients, fused.

Reference: libs/utils.py:277-329 (``PPO_learn``). Differences on purpose:
the policy-gradient sign is the correct ``-mean(logp * adv)``
and inputs are properly time-major (§8 D2).

Device tensors run the HIP kernel (``vtrace.hip``): one lane per trajectory,
reverse scan in registers, gradients written directly. CPU tensors run the
same recurrence with torch ops (also the test oracle).

``vtrace_upgo`` / ``vtrace_upgo_torch`` are the same objective with V-trace(lambda) value targets
(the trace cut by ``lam * min(c_bar, w)``) and the UPGO policy term of AlphaStar (Vinyals et
al. 2019): a second policy gradient on the upgoing return
``G_t = r_t + g_t (q_{t+1} >= V_{t+1} ? G_{t+1} : V_{t+1})``, ``q_t = r_t + g_t V_{t+1}``,
weighted by ``upgo_cost`` and clipped by ``upgo_rho_bar`` (``mbk_vtrace_upgo``, one launch like
``mbk_vtrace``). ``vtrace`` / ``vtrace_torch`` never reach that code.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _native as N


@dataclass
class VTraceOut:
    g_logp: torch.Tensor   # [T, B] dL/dlogp
    g_value: torch.Tensor  # [T+1, B] dL/dV (row T = 0: bootstrap has no gradient)
    g_ent: float           # dL/dentropy per frame (constant)
    losses: torch.Tensor   # [5] pg, value, entropy, total, mean rho (vtrace_upgo: [6], + upgo)
    vs: torch.Tensor | None = None
    adv: torch.Tensor | None = None
    upgo: torch.Tensor | None = None  # vtrace_upgo: [T, B] the upgoing returns G


def vtrace_torch(logp_new, logp_old, values, reward, done, entropy=None, gamma=0.99,
                 rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, baseline_cost=0.5, entropy_cost=0.01,
                 reward_clip=0.0) -> VTraceOut:
    T, B = logp_new.shape
    lpn = logp_new.detach().float()
    ratio = torch.exp(lpn - logp_old.float())
    rho = ratio.clamp(max=rho_bar)
    cs = ratio.clamp(max=c_bar)
    r = reward.float()
    if reward_clip > 0:
        r = r.clamp(-reward_clip, reward_clip)
    disc = (~done.bool()).float() * gamma
    v = values.detach().float()
    v_t, v_tp1 = v[:T], v[1:T + 1]
    deltas = rho * (r + disc * v_tp1 - v_t)
    acc = torch.zeros(B, dtype=torch.float32, device=lpn.device)
    vs_minus_v = torch.empty_like(deltas)
    for t in range(T - 1, -1, -1):
        acc = deltas[t] + disc[t] * cs[t] * acc
        vs_minus_v[t] = acc
    vs = vs_minus_v + v_t
    vs_tp1 = torch.cat([vs[1:], v[T:T + 1]], 0)
    adv = ratio.clamp(max=pg_rho_bar) * (r + disc * vs_tp1 - v_t)
    M = float(T * B)
    g_logp = -adv / M
    g_value = torch.zeros_like(v)
    g_value[:T] = 2.0 * baseline_cost * (v_t - vs) / M
    pg = -(lpn * adv).sum() / M
    vl = baseline_cost * ((vs - v_t) ** 2).sum() / M
    ent = entropy.detach().float().sum() / M if entropy is not None else torch.zeros((), device=lpn.device)
    losses = torch.stack([pg, vl, ent, pg + vl - entropy_cost * ent, rho.mean()])
    return VTraceOut(g_logp, g_value, -entropy_cost / M, losses, vs, adv)


class VTraceWorkspace:
    """Pre-allocated device buffers so the learner step never allocates."""

    def __init__(self):
        self._bufs = {}

    def get(self, name, shape, device):
        t = self._bufs.get(name)
        if t is None or t.shape != torch.Size(shape) or t.device != device:
            t = torch.empty(shape, dtype=torch.float32, device=device)
            self._bufs[name] = t
        return t


def f32c(x):
    """x as a contiguous fp32 tensor: x itself where it already is one (no copy, no launch)"""
    return x.float().contiguous()


def _launch_inputs(logp_new, logp_old, values, reward, done, entropy):
    """``mbk_vtrace`` / ``mbk_vtrace_upgo``'s input arrays: contiguous fp32, done as uint8, the
    learner's own outputs detached; entropy may be None"""
    return (f32c(logp_new.detach()), f32c(logp_old), f32c(values.detach()), f32c(reward),
            done.to(torch.uint8).contiguous(),
            f32c(entropy.detach()) if entropy is not None else None)


def vtrace(logp_new, logp_old, values, reward, done, entropy=None, gamma=0.99, rho_bar=1.0,
           c_bar=1.0, pg_rho_bar=1.0, baseline_cost=0.5, entropy_cost=0.01, reward_clip=0.0,
           want_targets=False, ws: VTraceWorkspace | None = None) -> VTraceOut:
    """logp_new/logp_old/reward/done/entropy: [T, B]; values: [T+1, B]."""
    if not logp_new.is_cuda:
        return vtrace_torch(logp_new, logp_old, values, reward, done, entropy, gamma, rho_bar,
                            c_bar, pg_rho_bar, baseline_cost, entropy_cost, reward_clip)
    T, B = logp_new.shape
    dev = logp_new.device
    ws = ws or VTraceWorkspace()
    g_logp = ws.get("g_logp", (T, B), dev)
    g_value = ws.get("g_value", (T + 1, B), dev)
    partials = ws.get("partials", (((B + 255) // 256) * 4,), dev)
    losses = ws.get("losses", (5,), dev)
    vs = ws.get("vs", (T, B), dev) if want_targets else None
    adv = ws.get("adv", (T, B), dev) if want_targets else None
    lpn, lpo, val, rew, dn, ent = _launch_inputs(logp_new, logp_old, values, reward, done, entropy)
    N.check(N.kernels().mbk_vtrace(
        lpn.data_ptr(), lpo.data_ptr(), val.data_ptr(), rew.data_ptr(), dn.data_ptr(),
        N.ptr(ent), T, B, gamma, rho_bar, c_bar, pg_rho_bar, baseline_cost, entropy_cost,
        reward_clip, N.ptr(vs), N.ptr(adv), g_logp.data_ptr(), g_value.data_ptr(),
        partials.data_ptr(), losses.data_ptr(), N.stream_ptr()), "vtrace")
    return VTraceOut(g_logp, g_value, -entropy_cost / float(T * B), losses, vs, adv)


def _check_upgo(lam, upgo_cost, upgo_rho_bar):
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"vtrace_upgo: lam {lam}: expected 0 <= lam <= 1")
    if not upgo_cost >= 0:
        raise ValueError(f"vtrace_upgo: upgo_cost {upgo_cost}: expected >= 0")
    if not upgo_rho_bar > 0:
        raise ValueError(f"vtrace_upgo: upgo_rho_bar {upgo_rho_bar}: expected > 0")


def vtrace_upgo_torch(logp_new, logp_old, values, reward, done, entropy=None, gamma=0.99,
                      rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, baseline_cost=0.5,
                      entropy_cost=0.01, reward_clip=0.0, lam=1.0, upgo_cost=0.0,
                      upgo_rho_bar=1.0) -> VTraceOut:
    """``vtrace_torch`` with V-trace(lambda) targets and the UPGO term (module doc); losses [6] =
    pg (the V-trace term alone), value, entropy, total, mean rho, upgo (unweighted)."""
    _check_upgo(lam, upgo_cost, upgo_rho_bar)
    T, B = logp_new.shape
    lpn = logp_new.detach().float()
    ratio = torch.exp(lpn - logp_old.float())
    rho = ratio.clamp(max=rho_bar)
    cs = lam * ratio.clamp(max=c_bar)
    r = reward.float()
    if reward_clip > 0:
        r = r.clamp(-reward_clip, reward_clip)
    disc = (~done.bool()).float() * gamma
    v = values.detach().float()
    v_t, v_tp1 = v[:T], v[1:T + 1]
    q = r + disc * v_tp1
    deltas = rho * (q - v_t)
    acc = torch.zeros(B, dtype=torch.float32, device=lpn.device)
    vs_minus_v = torch.empty_like(deltas)
    G = torch.empty_like(deltas)
    # the step after the last is the bootstrap: its tie (q == V) hands row T-1 G = q_{T-1}
    g_next = q_next = v[T]
    for t in range(T - 1, -1, -1):
        acc = deltas[t] + disc[t] * cs[t] * acc
        vs_minus_v[t] = acc
        g_next = r[t] + disc[t] * torch.where(q_next >= v_tp1[t], g_next, v_tp1[t])
        G[t] = g_next
        q_next = q[t]
    vs = vs_minus_v + v_t
    vs_tp1 = torch.cat([vs[1:], v[T:T + 1]], 0)
    adv = ratio.clamp(max=pg_rho_bar) * (r + disc * vs_tp1 - v_t)
    uadv = ratio.clamp(max=upgo_rho_bar) * (G - v_t)
    M = float(T * B)
    g_logp = -(adv + upgo_cost * uadv) / M
    g_value = torch.zeros_like(v)
    g_value[:T] = 2.0 * baseline_cost * (v_t - vs) / M
    pg = -(lpn * adv).sum() / M
    up = -(lpn * uadv).sum() / M
    vl = baseline_cost * ((vs - v_t) ** 2).sum() / M
    ent = entropy.detach().float().sum() / M if entropy is not None else torch.zeros((), device=lpn.device)
    losses = torch.stack([pg, vl, ent, pg + upgo_cost * up + vl - entropy_cost * ent, rho.mean(),
                          up])
    return VTraceOut(g_logp, g_value, -entropy_cost / M, losses, vs, adv, G)


def vtrace_upgo(logp_new, logp_old, values, reward, done, entropy=None, gamma=0.99, rho_bar=1.0,
                c_bar=1.0, pg_rho_bar=1.0, baseline_cost=0.5, entropy_cost=0.01, reward_clip=0.0,
                lam=1.0, upgo_cost=0.0, upgo_rho_bar=1.0, want_targets=False,
                ws: VTraceWorkspace | None = None) -> VTraceOut:
    """``vtrace`` with V-trace(lambda) targets and the UPGO term. Its workspace buffers have keys
    of their own (``upgo_*``), so ``vtrace``'s outputs in the same workspace stay untouched."""
    if not logp_new.is_cuda:
        return vtrace_upgo_torch(logp_new, logp_old, values, reward, done, entropy, gamma,
                                 rho_bar, c_bar, pg_rho_bar, baseline_cost, entropy_cost,
                                 reward_clip, lam, upgo_cost, upgo_rho_bar)
    T, B = logp_new.shape
    if values.shape != (T + 1, B) or logp_old.shape != (T, B) or reward.shape != (T, B) \
            or done.shape != (T, B) or (entropy is not None and entropy.shape != (T, B)):
        raise ValueError("vtrace_upgo: logp_new / logp_old / reward / done / entropy [T, B] and "
                         "values [T+1, B] expected")
    dev = logp_new.device
    ws = ws or VTraceWorkspace()
    g_logp = ws.get("upgo_g_logp", (T, B), dev)
    g_value = ws.get("upgo_g_value", (T + 1, B), dev)
    partials = ws.get("upgo_partials", (((B + 255) // 256) * 5,), dev)
    losses = ws.get("upgo_losses", (6,), dev)
    vs = ws.get("upgo_vs", (T, B), dev) if want_targets else None
    adv = ws.get("upgo_adv", (T, B), dev) if want_targets else None
    G = ws.get("upgo_ret", (T, B), dev) if want_targets else None
    lpn, lpo, val, rew, dn, ent = _launch_inputs(logp_new, logp_old, values, reward, done, entropy)
    N.check(N.kernels().mbk_vtrace_upgo(
        lpn.data_ptr(), lpo.data_ptr(), val.data_ptr(), rew.data_ptr(), dn.data_ptr(),
        N.ptr(ent), T, B, gamma, lam, rho_bar, c_bar, pg_rho_bar, upgo_rho_bar, baseline_cost,
        entropy_cost, upgo_cost, reward_clip, N.ptr(vs), N.ptr(adv), N.ptr(G),
        g_logp.data_ptr(), g_value.data_ptr(), partials.data_ptr(), losses.data_ptr(),
        N.stream_ptr()), "vtrace_upgo")
    return VTraceOut(g_logp, g_value, -entropy_cost / float(T * B), losses, vs, adv, G)
