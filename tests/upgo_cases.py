"""Shared inputs and the fp64 oracle of the V-trace(lambda) + UPGO tests (test_upgo.py,
test_gpu_upgo.py). Written from the definitions (Espeholt et al. 2018; Vinyals et al. 2019), not
from ops/vtrace.py, whose internals are fp32:

  w_t = exp(logp_new_t - logp_old_t),  g_t = done_t ? 0 : gamma,  r_t clipped when reward_clip > 0
  vs_t - V_t = rho_t d_t + g_t lambda min(c_bar, w_t) (vs_{t+1} - V_{t+1}),  vs_T = V_T
  adv_t = min(pg_rho_bar, w_t) (r_t + g_t vs_{t+1} - V_t)
  q_t = r_t + g_t V_{t+1},  G_{T-1} = q_{T-1},
  G_t = r_t + g_t (q_{t+1} >= V_{t+1} ? G_{t+1} : V_{t+1}),  upgo_adv_t = min(upgo_rho_bar, w_t)(G_t - V_t)

``upgo_oracle64`` does not evaluate G by that recurrence: for every (t, b) it walks forward to
the first step m at which the return stops following the rollout and sums the rewards up to it.
The recurrence (``_scan_G``) is kept beside it for the mutants only.

The gate is discontinuous: an fp32 evaluation of q_{t+1} that is correct to rounding may still
land on the other side of V_{t+1} at a near-tie. ``case`` therefore asserts that every fp64
margin |q_{t+1} - V_{t+1}| exceeds 4 * 2^-23 * (|r_{t+1}| + |V_{t+2}| + |V_{t+1}|) (a few fp32
roundings of the three terms), and the tests then compare every element."""
import functools

import numpy as np
import torch

from objective_cases import DEFAULTS, NONDEFAULT, _np64, vtrace_recipe

# the new knobs off their defaults on top of DEFAULTS, and NONDEFAULT extended: four different bars
UPGO_ON = dict(vtrace_lambda=0.8, upgo_cost=0.7, upgo_rho_bar=1.2)
UPGO_OFF = dict(vtrace_lambda=1.0, upgo_cost=0.0, upgo_rho_bar=1.0)
SETTINGS = {
    "defaults": dict(DEFAULTS, **UPGO_ON),
    "nondefault": dict(NONDEFAULT, **UPGO_ON),
}
SHAPES = {
    "1x1": (1, 1, None, False),
    "2x1": (2, 1, None, False),            # the smallest T at which a gate exists
    "5x63": (5, 63, None, False),          # less than one wave
    "64x257": (64, 257, None, False),      # one lane in the second block
    "3x16641": (3, 16641, None, False),    # 66 partial rows: the finalize kernel loops
    "37x300": (37, 300, None, False),
    "37x300-done-row": (37, 300, 11, False),
    "9x300-all-done": (9, 300, None, True),  # G_t = r_t, vs_t = V_t + rho_t (r_t - V_t)
}


def kernel_kwargs(s):
    """A settings dict in ops.vtrace.vtrace_upgo's keywords (``vtrace_lambda`` is ``lam``)."""
    s = dict(s)
    s["lam"] = s.pop("vtrace_lambda")
    return s


def _rewards(rew, reward_clip):
    return np.clip(rew, -reward_clip, reward_clip) if reward_clip > 0 else rew


def _walk_G(r, disc, val, stop):
    """G_t = sum_{k=t..m} (prod_{j=t..k-1} g_j) r_k + (prod_{j=t..m} g_j) V_{m+1}, m the first
    step >= t at which ``stop[m]`` holds (``stop[T-1]`` is all true). Vectorised over columns."""
    T, B = r.shape
    G = np.zeros((T, B))
    for t in range(T):
        live = np.ones(B, dtype=bool)
        prod = np.ones(B)
        for k in range(t, T):
            G[t] += np.where(live, prod * r[k], 0.0)
            prod = prod * disc[k]
            ends = live & stop[k]
            G[t] += np.where(ends, prod * val[k + 1], 0.0)
            live &= ~stop[k]
            if not live.any():
                break
    return G


def _scan_G(r, disc, val, q, gate):
    """The recurrence, for the mutants: ``gate(t, G_next)`` -> follow the rollout at step t."""
    T, B = r.shape
    G = np.empty((T, B))
    G[T - 1] = q[T - 1]
    for t in range(T - 2, -1, -1):
        G[t] = r[t] + disc[t] * np.where(gate(t, G[t + 1]), G[t + 1], val[t + 1])
    return G


def upgo_oracle64(lpn, lpo, val, rew, done, ent, gamma, rho_bar, c_bar, pg_rho_bar, baseline_cost,
                  entropy_cost, reward_clip, vtrace_lambda, upgo_cost, upgo_rho_bar, mutant=None):
    """fp64 tensors: vs, adv, upgo (G), upgo_adv, g_logp [T, B], g_value [T, B] (rows < T) and
    losses [6] = pg, value, entropy, total, mean rho, upgo. ``mutant`` (never the oracle):
    ``strict`` (the gate is q > V), ``gate_vt`` (the gate compares q_{t+1} with V_t),
    ``gate_g`` (the gate tests G_{t+1} in q_{t+1}'s place), ``lambda_on_delta`` (lambda scales
    delta_t, not the trace)."""
    assert mutant in (None, "strict", "gate_vt", "gate_g", "lambda_on_delta")
    lpn, lpo, val, rew = _np64(lpn), _np64(lpo), _np64(val), _np64(rew)
    dn = _np64(done) != 0
    T, B = lpn.shape
    ratio = np.exp(lpn - lpo)
    rho = np.minimum(rho_bar, ratio)
    c = np.minimum(c_bar, ratio)
    r = _rewards(rew, reward_clip)
    disc = np.where(dn, 0.0, gamma)
    vs = np.empty((T + 1, B))
    vs[T] = val[T]
    for t in range(T - 1, -1, -1):
        delta = rho[t] * (r[t] + disc[t] * val[t + 1] - val[t])
        if mutant == "lambda_on_delta":
            vs[t] = val[t] + vtrace_lambda * delta + disc[t] * c[t] * (vs[t + 1] - val[t + 1])
        else:
            vs[t] = val[t] + delta + disc[t] * vtrace_lambda * c[t] * (vs[t + 1] - val[t + 1])
    adv = np.minimum(pg_rho_bar, ratio) * (r + disc * vs[1:] - val[:T])
    q = r + disc * val[1:]
    if mutant == "gate_g":
        G = _scan_G(r, disc, val, q, lambda t, g_next: g_next >= val[t + 1])
    else:
        # the return leaves the rollout after step m: the episode ends there, the rollout ends
        # there, or the next step does worse than the value estimate
        stop = np.ones((T, B), dtype=bool)
        if mutant == "strict":
            stop[:T - 1] = dn[:T - 1] | (q[1:] <= val[1:T])
        elif mutant == "gate_vt":
            stop[:T - 1] = dn[:T - 1] | (q[1:] < val[:T - 1])
        else:
            stop[:T - 1] = dn[:T - 1] | (q[1:] < val[1:T])
        G = _walk_G(r, disc, val, stop)
    uadv = np.minimum(upgo_rho_bar, ratio) * (G - val[:T])
    M = float(T * B)
    pg = -(lpn * adv).sum() / M
    up = -(lpn * uadv).sum() / M
    vl = baseline_cost * ((vs[:T] - val[:T]) ** 2).sum() / M
    e = _np64(ent).sum() / M if ent is not None else 0.0
    losses = np.array([pg, vl, e, pg + upgo_cost * up + vl - entropy_cost * e, rho.sum() / M, up])
    t = torch.from_numpy
    return dict(vs=t(vs[:T].copy()), adv=t(adv), upgo=t(G), upgo_adv=t(uadv),
                g_logp=t(-(adv + upgo_cost * uadv) / M),
                g_value=t(2.0 * baseline_cost * (val[:T] - vs[:T]) / M), losses=t(losses))


def gate_margins(c, gamma, reward_clip):
    """(smallest |q_s - V_s|, largest bound 4 * 2^-23 (|r_s| + |V_{s+1}| + |V_s|), share of open
    gates) over the gates s = 1..T-1 of a case, in fp64; (inf, 0, nan) when T = 1."""
    val, dn = _np64(c["val"]), _np64(c["done"]) != 0
    r = _rewards(_np64(c["rew"]), reward_clip)
    T = r.shape[0]
    if T < 2:
        return float("inf"), 0.0, float("nan")
    q = r + np.where(dn, 0.0, gamma) * val[1:]
    margin = np.abs(q[1:] - val[1:T])
    bound = 4 * 2.0 ** -23 * (np.abs(r[1:]) + np.abs(val[2:]) + np.abs(val[1:T]))
    assert (margin > bound).all(), "a gate of this case is an fp32 near-tie"
    return float(margin.min()), float(bound.max()), float((q[1:] >= val[1:T]).mean())


@functools.lru_cache(maxsize=None)
def _recipe(shape):
    T, B, done_row, all_done = SHAPES[shape]
    c = vtrace_recipe(T, B, 0, done_row)
    if all_done:
        c["done"] = torch.ones_like(c["done"])
    return c


def case(shape, s):
    """objective_cases.vtrace_recipe at seed 0 for a SHAPES key, with its gates checked to be
    clear of fp32 near-ties under the settings ``s``. The tensors are shared: do not write."""
    c = _recipe(shape)
    gate_margins(c, s["gamma"], s["reward_clip"])
    return c


@functools.lru_cache(maxsize=None)
def oracle_for(shape, setting, use_ent=True):
    """(case, oracle) of a SHAPES key under a SETTINGS key, computed once per session."""
    s = SETTINGS[setting]
    c = case(shape, s)
    return c, upgo_oracle64(c["lpn"], c["lpo"], c["val"], c["rew"], c["done"],
                            c["ent"] if use_ent else None, **s)


EXACT = dict(gamma=0.5, rho_bar=1.0, c_bar=1.0, pg_rho_bar=1.0, baseline_cost=0.5,
             entropy_cost=0.0, reward_clip=0.0, vtrace_lambda=0.5, upgo_cost=0.5, upgo_rho_bar=1.0)
EXACT_TIE_COLUMNS = 24


def exact_case():
    """T = 8, B = 64 (M = 512), gamma = lambda = 0.5, bars 1, logp_new == logp_old in multiples
    of 0.5 about -5, values and rewards multiples of 0.5 in [-2, 2], dones in a few of the
    columns >= 24. Column b < 24 holds an exact tie q_s == V_s at s = 1 + b % 6: V_s in [-1, 1],
    V_{s+1} = -2 and r_s = V_s - 0.5 V_{s+1}; r_{s+1} = 2 keeps the return at s away from V_s, so
    a gate that reads the tie as closed changes G_{s-1}. Every fp32 operation of the scan is exact
    here (dyadic numbers of at most 19 significant bits), so fp32 results equal the fp64 ones
    bit for bit, ties included. Returns (case, [(s, b), ...])."""
    T, B = 8, 64
    g = torch.Generator().manual_seed(0)
    half = lambda lo, hi, *shape: torch.randint(lo, hi + 1, shape, generator=g).float() * 0.5  # noqa: E731
    lpn = -5.0 + half(-2, 2, T, B)
    val, rew = half(-4, 4, T + 1, B), half(-4, 4, T, B)
    done = torch.zeros(T, B, dtype=torch.bool)
    done[:, EXACT_TIE_COLUMNS:] = torch.rand(T, B - EXACT_TIE_COLUMNS, generator=g) < 0.1
    ties = []
    for b in range(EXACT_TIE_COLUMNS):
        s = 1 + b % 6
        val[s, b] = half(-2, 2, 1)[0]
        val[s + 1, b] = -2.0
        rew[s, b] = val[s, b] - 0.5 * val[s + 1, b]
        rew[s + 1, b] = 2.0  # q_{s+1} >= 1 and G_{s+1} >= 0 > V_{s+1}: G_s != V_s, the tie counts
        ties.append((s, b))
    ent = half(0, 6, T, B)
    return dict(lpn=lpn, lpo=lpn.clone(), val=val, rew=rew, done=done, ent=ent), ties
