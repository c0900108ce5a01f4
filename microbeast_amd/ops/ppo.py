"""PPO objective: GAE(lambda) advantages + clipped surrogate / clipped value losses and
their gradients, beside V-trace (``ops/vtrace.py``).

Reference: the learn step is called ``PPO_learn`` (libs/utils.py:277-329) but is IMPALA
V-trace, and its advantage helpers (``get_deltas`` / ``get_advantages``,
libs/utils.py:104-163; here ``ops/advantages.py``) are never called (C13). This is the
working PPO path (Schulman et al. 2017).

Inputs are time-major like V-trace's: ``logp_new / logp_old / reward / done / entropy``
``[T, B]``, values ``[T+1, B]``; ``M = T * B``, ``nd_t = 1 - done_t``.

``gae`` runs once per rollout on ``v_old``, a detached snapshot of the values the LEARNER
computes in the rollout's first epoch -- not the behaviour values the actors stored: the
engine never writes the behaviour value of a slot's bootstrap row T (it closes only obs, mask
and the active-cell bitmap into the previous slot; the mono runtime stores its values under
another key, ``baseline``). The learner's own epoch-0 values need no engine work and behave the
same on both runtimes.

    delta_t = r_t + gamma nd_t v_old[t+1] - v_old[t]
    A_t     = delta_t + gamma lambda nd_t A_{t+1},  A_T = 0
    R_t     = A_t + v_old[t]
    stats   = (mean A, 1 / (std A + 1e-8))   population std over the M elements; (0, 1) with
              ``norm_adv`` off. Under data parallelism each rank normalises with its own
              batch's statistics (no collective).

``vtrace_adv`` (``--ppo_adv vtrace``) takes ``gae``'s place when the rollout was acted by an
older policy mu, as the asynchronous actors' rollouts are: ``gae`` is unbiased only for
pi = mu. It is a V-trace(lambda) reverse scan (Espeholt et al. 2018, with lambda folded into
the trace) on the same value snapshot ``v`` = ``v_old`` and the log-probs ``logp_pi`` of the
pass that gave it, against the batch's behaviour log-probs ``logp_mu``:

    w_t   = exp(logp_pi_t - logp_mu_t)
    rho_t = min(rho_bar, w_t)            c_t = lambda min(c_bar, w_t)
    td_t  = r_t + gamma nd_t v[t+1] - v[t]
    A_t   = td_t + gamma nd_t lambda d_{t+1},  d_T = 0
    d_t   = rho_t td_t + gamma nd_t c_t d_{t+1}          (d = vs - v)
    R_t   = v[t] + d_t
    stats as above; is_stats = [mean w, share of w > rho_bar, share of w > c_bar]

A_t is r_t + gamma nd_t ((1-lambda) v[t+1] + lambda vs_{t+1}) - v[t]. With w = 1 and both bars
>= 1 it is GAE's A_t and R_t is GAE's; at lambda = 1 R_t is V-trace's vs_t. The policy
gradient's own importance weight is the surrogate's ratio, so ``pg_rho_bar`` plays no part.

``ppo_loss`` runs once per epoch, with ``A^ = (A - stats[0]) * stats[1]`` and
``ratio = exp(logp_new - logp_old)``:

    pg       = -mean(min(ratio A^, clamp(ratio, 1-eps, 1+eps) A^))
    value    = baseline_cost mean(max((v-R)^2, (v_c-R)^2)),
               v_c = v_old + clamp(v - v_old, -eps_v, eps_v)   (eps_v = 0: plain (v-R)^2)
    dL/dlogp = -A^ ratio / M, or 0 where (A^ > 0 and ratio > 1+eps) or (A^ < 0 and ratio < 1-eps)
    dL/dv    = 2 bc (v-R)/M where (v-R)^2 >= (v_c-R)^2; else 2 bc (v_c-R)/M where
               |v - v_old| <= eps_v; else 0.  Row T of g_value is 0. (Inside the clip range
               v_c = v, so the middle case is the first one: the code tests |v - v_old| > eps_v
               and does not compare two roundings of the same error.)
    dL/dH    = -entropy_cost / M
    losses   = [pg, value, entropy, total = pg + value - entropy_cost entropy, mean ratio,
                approx_kl = mean((ratio-1) - log ratio), clip_frac = mean(|ratio-1| > eps)]

Row-block minibatches (``--ppo_minibatches K``): block k is rows [k T/K, (k+1) T/K) of the
rollout, all B columns -- contiguous in a time-major slot. ``adv_stats_rows`` gives every block
its own ``stats`` pair in one launch, and ``ppo_loss_rows`` is ``ppo_loss`` on one block: the
step's own [T/K, B] logp_new / values / entropy (no bootstrap row, so g_value is [T/K, B]) with
rows t0.. of the rollout-wide logp_old / v_old / adv / ret and ``M = T/K * B``. It also keeps
``epoch_mean``, the ordered running mean of the epoch's per-step losses.

Device tensors run the HIP kernels (``ppo.hip``: a one-lane-per-column reverse scan with
per-block (n, mean, M2) partials, and one vectorised elementwise pass); a missing kernel is an
error. CPU tensors run the same maths in fp32 torch ops (``gae_torch`` / ``vtrace_adv_torch`` /
``ppo_loss_torch`` /
``adv_stats_rows_torch`` / ``ppo_loss_rows_torch``: the test oracle, and what the mono
runtime's CPU learner runs).
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from .. import _native as N
from .vtrace import VTraceWorkspace, f32c


@dataclass
class GaeOut:
    adv: torch.Tensor    # [T, B] unnormalised advantages
    ret: torch.Tensor    # [T, B] value targets adv + v_old[:T]
    stats: torch.Tensor  # [2] mean, 1 / (std + 1e-8) of adv ((0, 1): normalisation off)


@dataclass
class PPOOut:
    g_logp: torch.Tensor   # [T, B] dL/dlogp
    g_value: torch.Tensor  # [T+1, B] dL/dV (row T = 0: bootstrap has no gradient)
    g_ent: float           # dL/dentropy per frame (constant)
    losses: torch.Tensor   # [7] pg, value, entropy, total, mean ratio, approx_kl, clip_frac
    adv: torch.Tensor | None = None
    ret: torch.Tensor | None = None
    epoch_mean: torch.Tensor | None = None  # [7] block form: mean of the epoch's steps so far


def _f(x):
    """fp32 compute; float64 inputs stay float64 (the tests' high-precision runs)"""
    return x.detach() if x.dtype == torch.float64 else x.detach().float()


def gae_torch(v_old, reward, done, gamma=0.99, lam=0.95, reward_clip=0.0,
              norm_adv=True) -> GaeOut:
    T, B = reward.shape
    v = _f(v_old)
    r = reward.to(v.dtype)
    if reward_clip > 0:
        r = r.clamp(-reward_clip, reward_clip)
    disc = (~done.bool()).to(v.dtype) * gamma
    delta = r + disc * v[1:T + 1] - v[:T]
    acc = torch.zeros(B, dtype=v.dtype, device=v.device)
    adv = torch.empty_like(delta)
    for t in range(T - 1, -1, -1):
        acc = delta[t] + disc[t] * lam * acc
        adv[t] = acc
    if norm_adv:
        stats = torch.stack([adv.mean(), 1.0 / (adv.std(unbiased=False) + 1e-8)])
    else:
        stats = torch.tensor([0.0, 1.0], dtype=v.dtype, device=v.device)
    return GaeOut(adv, adv + v[:T], stats)


def vtrace_adv_torch(logp_pi, logp_mu, v, reward, done, gamma=0.99, lam=0.95, rho_bar=1.0,
                     c_bar=1.0, reward_clip=0.0, norm_adv=True):
    """``gae_torch`` with V-trace(lambda) importance weights (module docstring). Returns
    (GaeOut, is_stats [3])."""
    if not (rho_bar > 0 and c_bar > 0):
        raise ValueError(f"rho_bar {rho_bar} / c_bar {c_bar}: expected > 0")
    T, B = reward.shape
    v = _f(v)
    dt = v.dtype
    w = torch.exp(_f(logp_pi).to(dt) - logp_mu.to(dt))
    rho = w.clamp(max=rho_bar)
    c = lam * w.clamp(max=c_bar)
    r = reward.to(dt)
    if reward_clip > 0:
        r = r.clamp(-reward_clip, reward_clip)
    disc = (~done.bool()).to(dt) * gamma
    td = r + disc * v[1:T + 1] - v[:T]
    acc = torch.zeros(B, dtype=dt, device=v.device)
    adv = torch.empty_like(td)
    d = torch.empty_like(td)
    for t in range(T - 1, -1, -1):
        adv[t] = td[t] + disc[t] * lam * acc
        acc = rho[t] * td[t] + disc[t] * c[t] * acc
        d[t] = acc
    if norm_adv:
        stats = torch.stack([adv.mean(), 1.0 / (adv.std(unbiased=False) + 1e-8)])
    else:
        stats = torch.tensor([0.0, 1.0], dtype=dt, device=v.device)
    is_stats = torch.stack([w.mean(), (w > rho_bar).to(dt).mean(), (w > c_bar).to(dt).mean()])
    return GaeOut(adv, v[:T] + d, stats), is_stats


def ppo_loss_torch(logp_new, logp_old, values, v_old, adv, ret, stats, entropy=None, clip=0.1,
                   value_clip=0.1, baseline_cost=0.5, entropy_cost=0.01) -> PPOOut:
    T, B = logp_new.shape
    M = float(T * B)
    lpn = _f(logp_new)
    dt = lpn.dtype
    lr = lpn - logp_old.to(dt)
    ratio = torch.exp(lr)
    a = (adv.to(dt) - stats[0].to(dt)) * stats[1].to(dt)
    lo, hi = 1.0 - clip, 1.0 + clip
    s1, s2 = ratio * a, ratio.clamp(lo, hi) * a
    out = ((a > 0) & (ratio > hi)) | ((a < 0) & (ratio < lo))
    g_logp = torch.where(out, torch.zeros_like(s1), -s1 / M)
    v_all = values.detach().to(dt)
    v, vo, R = v_all[:T], v_old.to(dt)[:T], ret.to(dt)
    e = v - R
    e1 = e * e
    vterm, gv = e1, e
    if value_clip > 0:
        # inside the clip range v_c = v (the first case); outside it v_c = v_old +- eps_v is
        # constant in v, so where its error is the larger one the gradient is 0
        d = v - vo
        ec = vo + d.clamp(-value_clip, value_clip) - R
        e2 = ec * ec
        alt = (d.abs() > value_clip) & (e1 < e2)
        vterm = torch.where(alt, e2, e1)
        gv = torch.where(alt, torch.zeros_like(e), e)
    g_value = torch.zeros_like(v_all)
    g_value[:T] = 2.0 * baseline_cost * gv / M
    pg = -torch.minimum(s1, s2).sum() / M
    vl = baseline_cost * vterm.sum() / M
    ent = (entropy.detach().to(dt).sum() / M if entropy is not None
           else torch.zeros((), dtype=dt, device=ratio.device))
    losses = torch.stack([pg, vl, ent, pg + vl - entropy_cost * ent, ratio.mean(),
                          ((ratio - 1.0) - lr).mean(),
                          ((ratio - 1.0).abs() > clip).to(dt).mean()])
    return PPOOut(g_logp, g_value, -entropy_cost / M, losses, adv, ret)


def adv_stats_rows_torch(adv, K: int, norm_adv=True) -> torch.Tensor:
    """[K, 2]: (mean, 1 / (std + 1e-8)) of each block of T / K rows of adv [T, B] (population
    std); every pair (0, 1) with ``norm_adv`` off."""
    T = adv.shape[0]
    if K < 1 or T % K != 0:
        raise ValueError(f"ppo_minibatches {K} does not divide the {T} rows of the rollout")
    a = _f(adv).reshape(K, -1)
    if not norm_adv:
        return torch.tensor([[0.0, 1.0]] * K, dtype=a.dtype, device=a.device)
    return torch.stack([a.mean(1), 1.0 / (a.std(1, unbiased=False) + 1e-8)], 1)


def ppo_loss_rows_torch(logp_new, logp_old, values, v_old, adv, ret, stats, t0: int,
                        entropy=None, clip=0.1, value_clip=0.1, baseline_cost=0.5,
                        entropy_cost=0.01, step: int = 0, epoch_mean=None) -> PPOOut:
    """``ppo_loss_torch`` on rows [t0, t0 + Tm): logp_new / values / entropy are the step's own
    [Tm, B] arrays (g_value is [Tm, B]: no bootstrap row), logp_old / v_old / adv / ret the
    rollout-wide ones, stats the block's pair. epoch_mean: the running mean of the epoch's
    steps before this one (ignored at step 0); the returned one includes this step."""
    Tm = logp_new.shape[0]
    r = slice(t0, t0 + Tm)
    o = ppo_loss_torch(logp_new, logp_old[r], values, v_old[r], adv[r], ret[r], stats, entropy,
                       clip, value_clip, baseline_cost, entropy_cost)
    mean = o.losses if step == 0 else epoch_mean + (o.losses - epoch_mean) / float(step + 1)
    return PPOOut(o.g_logp, o.g_value, o.g_ent, o.losses, adv, ret, mean)


def _loss_inputs(logp_new, logp_old, values, v_old, adv, ret, stats, entropy):
    """``mbk_ppo_loss`` / ``mbk_ppo_loss_rows``'s input arrays, detached contiguous fp32: the seven
    in the launchers' order, then the entropy or None"""
    arrays = [f32c(x.detach()) for x in (logp_new, logp_old, values, v_old, adv, ret, stats)]
    return (*arrays, f32c(entropy.detach()) if entropy is not None else None)


def gae(v_old, reward, done, gamma=0.99, lam=0.95, reward_clip=0.0, norm_adv=True,
        ws: VTraceWorkspace | None = None) -> GaeOut:
    """v_old: [T+1, B]; reward / done: [T, B]. The outputs live in ``ws`` (reused by the next
    call with the same shape)."""
    if not v_old.is_cuda:
        return gae_torch(v_old, reward, done, gamma, lam, reward_clip, norm_adv)
    T, B = reward.shape
    dev = v_old.device
    ws = ws or VTraceWorkspace()
    adv = ws.get("ppo_adv", (T, B), dev)
    ret = ws.get("ppo_ret", (T, B), dev)
    partials = ws.get("ppo_gae_partials", (((B + 255) // 256) * 3,), dev)
    stats = ws.get("ppo_stats", (2,), dev)
    vo, rew = f32c(v_old.detach()), f32c(reward)
    dn = done.to(torch.uint8).contiguous()
    N.check(N.kernels().mbk_gae(vo.data_ptr(), rew.data_ptr(), dn.data_ptr(), T, B, gamma, lam,
                                reward_clip, int(bool(norm_adv)), adv.data_ptr(), ret.data_ptr(),
                                partials.data_ptr(), stats.data_ptr(), N.stream_ptr()), "gae")
    return GaeOut(adv, ret, stats)


def vtrace_adv(logp_pi, logp_mu, v, reward, done, gamma=0.99, lam=0.95, rho_bar=1.0, c_bar=1.0,
               reward_clip=0.0, norm_adv=True, ws: VTraceWorkspace | None = None):
    """logp_pi / logp_mu / reward / done: [T, B]; v: [T+1, B], the values of the pass that gave
    logp_pi. Returns (GaeOut, is_stats [3] = mean w, share of w > rho_bar, share of w > c_bar);
    the outputs live in ``ws`` under keys of their own (not ``gae``'s)."""
    if not v.is_cuda:
        return vtrace_adv_torch(logp_pi, logp_mu, v, reward, done, gamma, lam, rho_bar, c_bar,
                                reward_clip, norm_adv)
    T, B = reward.shape
    dev = v.device
    ws = ws or VTraceWorkspace()
    adv = ws.get("ppo_vt_adv", (T, B), dev)
    ret = ws.get("ppo_vt_ret", (T, B), dev)
    partials = ws.get("ppo_vt_partials", (((B + 255) // 256) * 6,), dev)
    stats = ws.get("ppo_vt_stats", (2,), dev)
    is_stats = ws.get("ppo_vt_is_stats", (3,), dev)
    lpi, lmu, vo, rew = (f32c(x.detach()) for x in (logp_pi, logp_mu, v, reward))
    dn = done.to(torch.uint8).contiguous()
    if not (lpi.shape == lmu.shape == dn.shape == (T, B)) or vo.numel() != (T + 1) * B:
        raise ValueError("vtrace_adv: logp_pi / logp_mu / done [T, B] and v [T+1, B] expected")
    N.check(N.kernels().mbk_vtrace_adv(
        lpi.data_ptr(), lmu.data_ptr(), vo.data_ptr(), rew.data_ptr(), dn.data_ptr(), T, B, gamma,
        lam, rho_bar, c_bar, reward_clip, int(bool(norm_adv)), adv.data_ptr(), ret.data_ptr(),
        partials.data_ptr(), stats.data_ptr(), is_stats.data_ptr(), N.stream_ptr()),
        "vtrace_adv")
    return GaeOut(adv, ret, stats), is_stats


def ppo_loss(logp_new, logp_old, values, v_old, adv, ret, stats, entropy=None, clip=0.1,
             value_clip=0.1, baseline_cost=0.5, entropy_cost=0.01,
             ws: VTraceWorkspace | None = None) -> PPOOut:
    """logp_new / logp_old / adv / ret / entropy: [T, B]; values / v_old: [T+1, B]; stats: [2]
    (``gae``'s)."""
    if not logp_new.is_cuda:
        return ppo_loss_torch(logp_new, logp_old, values, v_old, adv, ret, stats, entropy, clip,
                              value_clip, baseline_cost, entropy_cost)
    T, B = logp_new.shape
    dev = logp_new.device
    ws = ws or VTraceWorkspace()
    g_logp = ws.get("ppo_g_logp", (T, B), dev)
    g_value = ws.get("ppo_g_value", (T + 1, B), dev)
    partials = ws.get("ppo_partials", ((((T + 1) * B + 255) // 256) * 6,), dev)
    losses = ws.get("ppo_losses", (7,), dev)
    lpn, lpo, val, vo, ad, rt, st, ent = _loss_inputs(logp_new, logp_old, values, v_old, adv,
                                                      ret, stats, entropy)
    N.check(N.kernels().mbk_ppo_loss(
        lpn.data_ptr(), lpo.data_ptr(), val.data_ptr(), vo.data_ptr(), ad.data_ptr(),
        rt.data_ptr(), N.ptr(ent), st.data_ptr(), T, B, 1.0 - clip, 1.0 + clip, clip, value_clip,
        baseline_cost, entropy_cost, g_logp.data_ptr(), g_value.data_ptr(), partials.data_ptr(),
        losses.data_ptr(), N.stream_ptr()), "ppo_loss")
    return PPOOut(g_logp, g_value, -entropy_cost / float(T * B), losses, adv, ret)


def adv_stats_rows(adv, K: int, norm_adv=True, ws: VTraceWorkspace | None = None) -> torch.Tensor:
    """adv: [T, B] (``gae``'s) -> [K, 2], the (mean, 1 / (std + 1e-8)) of each block of T / K
    rows. One launch for all K blocks; the result lives in ``ws``."""
    if not adv.is_cuda:
        return adv_stats_rows_torch(adv, K, norm_adv)
    T, B = adv.shape
    if K < 1 or T % K != 0:
        raise ValueError(f"ppo_minibatches {K} does not divide the {T} rows of the rollout")
    dev = adv.device
    ws = ws or VTraceWorkspace()
    nb = min(256, ((T // K) * B + 255) // 256)
    partials = ws.get("ppo_rows_stats_partials", (K * nb * 3,), dev)
    stats = ws.get("ppo_rows_stats", (K, 2), dev)
    ad = f32c(adv.detach())
    N.check(N.kernels().mbk_adv_stats_rows(ad.data_ptr(), T, B, K, int(bool(norm_adv)),
                                           partials.data_ptr(), stats.data_ptr(),
                                           N.stream_ptr()), "adv_stats_rows")
    return stats


def ppo_loss_rows(logp_new, logp_old, values, v_old, adv, ret, stats, t0: int, entropy=None,
                  clip=0.1, value_clip=0.1, baseline_cost=0.5, entropy_cost=0.01, step: int = 0,
                  epoch_mean=None, ws: VTraceWorkspace | None = None) -> PPOOut:
    """The block form of ``ppo_loss``: logp_new / values / entropy [Tm, B] are one step's own
    arrays over rows [t0, t0 + Tm) of the rollout; logp_old / adv / ret [>= t0 + Tm, B] and
    v_old are the rollout-wide arrays; stats [2] is the block's pair (a row of
    ``adv_stats_rows``). ``step`` is the step's index in its epoch: ``epoch_mean`` [7] of the
    result is the ordered running mean of the epoch's per-step losses, kept on the device."""
    if not logp_new.is_cuda:
        return ppo_loss_rows_torch(logp_new, logp_old, values, v_old, adv, ret, stats, t0,
                                   entropy, clip, value_clip, baseline_cost, entropy_cost, step,
                                   epoch_mean)
    Tm, B = logp_new.shape
    if t0 < 0 or min(logp_old.shape[0], v_old.shape[0], adv.shape[0], ret.shape[0]) < t0 + Tm:
        raise ValueError(f"rows [{t0}, {t0 + Tm}) are outside the rollout")
    if values.numel() != Tm * B or stats.numel() != 2:
        raise ValueError("ppo_loss_rows: values [Tm, B] and stats [2] expected")
    dev = logp_new.device
    ws = ws or VTraceWorkspace()
    g_logp = ws.get("ppo_rows_g_logp", (Tm, B), dev)
    g_value = ws.get("ppo_rows_g_value", (Tm, B), dev)
    partials = ws.get("ppo_rows_partials", (((Tm * B + 255) // 256) * 6,), dev)
    losses = ws.get("ppo_rows_losses", (7,), dev)
    mean = ws.get("ppo_epoch_mean", (7,), dev)
    lpn, lpo, val, vo, ad, rt, st, ent = _loss_inputs(logp_new, logp_old, values, v_old, adv,
                                                      ret, stats, entropy)
    N.check(N.kernels().mbk_ppo_loss_rows(
        lpn.data_ptr(), lpo.data_ptr(), val.data_ptr(), vo.data_ptr(), ad.data_ptr(),
        rt.data_ptr(), N.ptr(ent), st.data_ptr(), t0, Tm, B, 1.0 - clip, 1.0 + clip, clip,
        value_clip, baseline_cost, entropy_cost, step, g_logp.data_ptr(), g_value.data_ptr(),
        partials.data_ptr(), losses.data_ptr(), mean.data_ptr(), N.stream_ptr()),
        "ppo_loss_rows")
    return PPOOut(g_logp, g_value, -entropy_cost / float(Tm * B), losses, adv, ret, mean)
