"""``--test`` mode: evaluate a checkpoint (the reference's ``test()`` is a stub
that prints "Testing...", microbeast.py:267-268).

Two modes:

* ``--eval_envs 0`` (default): ``--n_envs`` envs stepped from Python until the first
  ``--eval_episodes`` episodes have finished.
* ``--eval_envs N``: N envs, each contributing exactly the FIRST episode it finishes
  (``first_episodes``); the run ends when every env has one. Selecting the first episodes to
  finish over all envs instead keeps the short games, which are mostly losses. With a GPU the
  envs run on the native engine (``GpuActorRuntime`` without a learner: ``get_batch`` /
  ``release``, never a publish), else one vec-env is stepped from Python under the same rule.
  Writes ``{exp}_eval.csv`` (one row per env) and ``{exp}_eval_summary.csv`` (per opponent).

``--eval_greedy`` acts with the arg-max action of every component in either mode.
"""
from __future__ import annotations

import csv
import math
import os
import time

import torch

from .config import Flags
from .envs.synthetic import create_env
from .models.factory import make_model
from .utils.checkpoint import load_checkpoint
from .utils.metrics import EPISODE_HEADER

SUMMARY_HEADER = ["opponent", "episodes", "wins", "draws", "losses", "win_rate", "win_rate_lo",
                  "win_rate_hi", "mean_return", "mean_steps"]


def first_episodes(selected: dict, records, n_envs: int | None = None, base: int = 0) -> dict:
    """The selection rule of ``--eval_envs``: every env contributes the first episode it
    finishes. ``records`` are (return, steps, env_index, winner[, opponent]) tuples in finishing
    order; those of an env that already has one (a fast env's later episodes) are dropped.
    ``selected`` {env_index: record} is updated and returned; with ``n_envs`` a record of an env
    outside [base, base + n_envs) is an error. The run is complete at len(selected) == n_envs."""
    for r in records:
        i = int(r[2])
        if n_envs is not None and not base <= i < base + n_envs:
            raise ValueError(f"episode of env {i}: outside [{base}, {base + n_envs})")
        if i not in selected:
            selected[i] = tuple(r)
    return selected


def wilson_interval(wins: int, n: int, z: float = 1.96) -> tuple[float, float]:
    """Wilson score interval of a binomial proportion (95 % at z = 1.96); (0, 1) for n = 0."""
    if n <= 0:
        return 0.0, 1.0
    p = wins / n
    den = 1.0 + z * z / n
    mid = (p + z * z / (2 * n)) / den
    half = z * math.sqrt(p * (1.0 - p) / n + z * z / (4.0 * n * n)) / den
    return max(0.0, mid - half), min(1.0, mid + half)


def _opponent_name(opp: int) -> str:
    from .runtime.gpu_actors import BOT_IDS

    names = {v: k for k, v in BOT_IDS.items()}
    return names.get(-1 - int(opp), f"snapshot_{int(opp)}" if opp >= 0 else f"bot_{-1 - int(opp)}")


def summarize(episodes) -> list[dict]:
    """One row per opponent (in bot-id order) plus a final ``all`` row. A win is winner == 0,
    a draw winner < 0, anything else a loss (as runtime/league.py counts them)."""
    def row(name, eps):
        n = len(eps)
        wins = sum(1 for r in eps if int(r[3]) == 0)
        draws = sum(1 for r in eps if int(r[3]) < 0)
        lo, hi = wilson_interval(wins, n)
        return {"opponent": name, "episodes": n, "wins": wins, "draws": draws,
                "losses": n - wins - draws, "win_rate": wins / max(n, 1), "win_rate_lo": lo,
                "win_rate_hi": hi, "mean_return": sum(float(r[0]) for r in eps) / max(n, 1),
                "mean_steps": sum(int(r[1]) for r in eps) / max(n, 1)}

    by = {}
    for r in episodes:
        by.setdefault(int(r[4]) if len(r) > 4 else -1, []).append(r)
    rows = [row(_opponent_name(o), by[o]) for o in sorted(by, reverse=True)]  # -1 - id: id order
    return rows + [row("all", list(episodes))]


def _load(flags: Flags, dev, checkpoint: str | None):
    path = checkpoint or flags.checkpoint or os.path.join(flags.savedir, f"{flags.exp_name}.ckpt")
    model = make_model(flags, dev)
    if os.path.exists(path):
        ck = load_checkpoint(path)
        model.load_state_dict(ck["model_state_dict"])
        src = path
    elif flags.allow_random_init:
        src = "random-init (no checkpoint found, --allow_random_init)"
    else:  # an evaluation of untrained weights must not pass for a checkpoint's result
        raise FileNotFoundError(
            f"--test: no checkpoint at {path!r}; train first, pass --checkpoint PATH, or "
            f"--allow_random_init to evaluate random-init weights")
    model.eval()
    return model, src


def evaluate(flags: Flags, checkpoint: str | None = None, greedy: bool = False) -> dict:
    greedy = bool(greedy or flags.eval_greedy)
    if flags.eval_envs < 0:
        raise ValueError(f"--eval_envs {flags.eval_envs}: expected >= 0")
    if flags.eval_envs > 0:
        return _evaluate_envs(flags, checkpoint, greedy)
    dev = torch.device("cuda" if (flags.device != "cpu" and torch.cuda.is_available()) else "cpu")
    model, src = _load(flags, dev, checkpoint)
    n = flags.n_envs
    env = create_env(flags.env_size, n, flags.max_episode_steps, seed=flags.seed + 777,
                     opponents=flags.opponent_list(), reward_weight=flags.reward_weights(),
                     env=flags.env)
    S = flags.env_size ** 2
    obs = torch.zeros(n, S, dtype=torch.int32)
    mask = torch.zeros(n, S, 3, dtype=torch.int32)
    env.reset_compact(obs, mask)
    rng = torch.tensor([flags.seed * 31 + 5, 0], dtype=torch.int64, device=dev)
    gen = torch.Generator().manual_seed(flags.seed)
    episodes = []
    steps = 0
    while len(episodes) < flags.eval_episodes and steps < 100 * flags.max_episode_steps:
        with torch.no_grad():
            o, m = obs.to(dev), mask.to(dev)
            if greedy:
                from .ops import cell_head
                logits, _ = model.policy_value(o)
                a = cell_head.greedy(logits, m)
            else:
                a, _, _ = model.act(o, m, rng_state=rng if dev.type == "cuda" else None,
                                    generator=gen)
        env.step_compact(a.cpu())
        episodes.extend(env.drain_episodes())
        steps += 1
    episodes = episodes[:flags.eval_episodes]
    out_path = os.path.join(flags.savedir, f"{flags.exp_name}_eval.csv")
    os.makedirs(flags.savedir or ".", exist_ok=True)
    with open(out_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Return", "steps", "env_index", "winner"])
        for r in episodes:
            w.writerow([float(r[0]), int(r[1]), int(r[2]), int(r[3])])
    rets = [float(r[0]) for r in episodes]
    res = {"checkpoint": src, "episodes": len(episodes),
           "mean_return": sum(rets) / max(len(rets), 1),
           "win_rate": sum(1 for r in episodes if r[3] == 0) / max(len(episodes), 1),
           "csv": out_path}
    print(f"Testing... {res}", flush=True)
    return res


# ------------------------------------------------------------------ --eval_envs N
def _engine_wanted(flags: Flags) -> bool:
    """The engine path: a GPU is present and the GPU actor runtime would be chosen for these
    flags (train.resolve_runtime) and would accept them (it refuses --dtype fp32)."""
    from .train import resolve_runtime

    want_cuda = flags.device == "cuda" or (flags.device == "auto" and torch.cuda.is_available())
    if flags.device == "cuda" and not torch.cuda.is_available():
        raise RuntimeError("--device cuda needs a GPU")
    return want_cuda and resolve_runtime(flags, want_cuda) == "gpu" and flags.dtype != "fp32"


def _run_engine(flags: Flags, model, dev, greedy: bool):
    """N envs on the GPU engine without a learner. Returns ({env: record}, frames, acting)."""
    from .ops.optim import FlatParams
    from .runtime.gpu_actors import GpuActorRuntime

    N_, E, T = flags.eval_envs, flags.envs_per_group, flags.unroll_length
    if N_ <= E:
        G, E = 1, N_
    elif N_ % E:
        raise ValueError(f"--eval_envs {N_}: above --envs_per_group {E} it must be a multiple of it")
    else:
        G = N_ // E
    # an env finishes its first episode within max_episode_steps + 1 steps (the simulator
    # truncates there), i.e. ceil((max + 1) / T) rollouts of its group, + 2 for the slots in
    # flight around the one that holds the episode's end
    max_slots = G * (-(-(flags.max_episode_steps + 1) // T) + 2)
    flat = FlatParams(model, dev)
    rt = GpuActorRuntime(lambda: make_model(flags, "cpu"), flags.env_size, G, E, T, 1, dev,
                         n_threads=flags.actor_threads or None,
                         max_steps=flags.max_episode_steps, seed=flags.seed + 777,
                         bots=flags.opponent_list(), reward_weight=flags.reward_weights(),
                         fp8_policy=flags.fp8_policy or flags.dtype == "fp8",
                         n_lanes=max(1, min(flags.policy_lanes, G)), greedy=greedy)
    try:
        acting = "fused" if rt.fused_act else "graph"
        rt.start(flat)
        selected, slots_used = {}, 0
        while len(selected) < N_:
            if slots_used >= max_slots:
                raise RuntimeError(
                    f"--eval_envs: {len(selected)} of {N_} envs finished an episode within "
                    f"{max_slots} rollout slots (max_episode_steps {flags.max_episode_steps}, "
                    f"unroll {T}): the simulator must end every episode by then")
            _, slots = rt.get_batch(1, timeout=flags.batch_timeout)
            rt.release(slots)
            slots_used += 1
            first_episodes(selected, rt.drain_episodes(), N_)
        return selected, slots_used * E * T, acting
    finally:
        rt.close()


def _run_host(flags: Flags, model, dev, greedy: bool):
    """The same rule over one vec-env stepped from Python with ``model.act``."""
    N_ = flags.eval_envs
    env = create_env(flags.env_size, N_, flags.max_episode_steps, seed=flags.seed + 777,
                     opponents=flags.opponent_list(), reward_weight=flags.reward_weights(),
                     env=flags.env)
    S = flags.env_size ** 2
    obs = torch.zeros(N_, S, dtype=torch.int32)
    mask = torch.zeros(N_, S, 3, dtype=torch.int32)
    env.reset_compact(obs, mask)
    rng = torch.tensor([flags.seed * 31 + 5, 0], dtype=torch.int64, device=dev)
    gen = torch.Generator().manual_seed(flags.seed)
    selected, steps = {}, 0
    while len(selected) < N_:
        if steps > flags.max_episode_steps + 1:
            raise RuntimeError(
                f"--eval_envs: {len(selected)} of {N_} envs finished an episode within "
                f"{steps} steps (max_episode_steps {flags.max_episode_steps})")
        with torch.no_grad():
            a, _, _ = model.act(obs.to(dev), mask.to(dev),
                                rng_state=rng if dev.type == "cuda" else None, generator=gen,
                                greedy=greedy)
        env.step_compact(a.cpu(), obs, mask)
        steps += 1
        first_episodes(selected, env.drain_episodes(), N_)
    return selected, steps * N_, "host"


def _evaluate_envs(flags: Flags, checkpoint: str | None, greedy: bool) -> dict:
    if flags.self_play:
        raise ValueError("--eval_envs evaluates against the scripted --opponents; it cannot be "
                         "combined with --self_play (league snapshots are not evaluated)")
    engine = _engine_wanted(flags)
    cuda = engine or (flags.device != "cpu" and torch.cuda.is_available())
    # (an indexed device: the models' per-device kernel state is keyed by it)
    dev = torch.device("cuda", torch.cuda.current_device()) if cuda else torch.device("cpu")
    model, src = _load(flags, dev, checkpoint)
    if dev.type == "cuda":
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    selected, frames, acting = (_run_engine if engine else _run_host)(flags, model, dev, greedy)
    seconds = time.perf_counter() - t0
    episodes = [selected[i] for i in sorted(selected)]
    os.makedirs(flags.savedir or ".", exist_ok=True)
    out_path = os.path.join(flags.savedir, f"{flags.exp_name}_eval.csv")
    with open(out_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(EPISODE_HEADER)
        for r in episodes:
            w.writerow([float(r[0]), int(r[1]), int(r[2]), int(r[3]),
                        int(r[4]) if len(r) > 4 else -1])
    rows = summarize(episodes)
    sum_path = os.path.join(flags.savedir, f"{flags.exp_name}_eval_summary.csv")
    with open(sum_path, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(SUMMARY_HEADER)
        for r in rows:
            w.writerow([r[k] if isinstance(r[k], (str, int)) else round(r[k], 6)
                        for k in SUMMARY_HEADER])
    tot = rows[-1]
    res = {"checkpoint": src, "episodes": len(episodes), "mean_return": tot["mean_return"],
           "win_rate": tot["win_rate"], "csv": out_path, "summary_csv": sum_path,
           "per_opponent": {r["opponent"]: {k: r[k] for k in SUMMARY_HEADER[1:]}
                            for r in rows[:-1]},
           "mode": "engine" if engine else "host", "acting": acting, "greedy": greedy,
           "frames": int(frames), "seconds": seconds, "fps": frames / max(seconds, 1e-9)}
    print(f"Testing... {res}", flush=True)
    return res
