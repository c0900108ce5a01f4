"""``--test --eval_envs N`` on the GPU engine: every env's first episode, per-opponent summary
with Wilson intervals, greedy acting through the fused two-launch step (16x16) and the
captured-graph step (other shapes), and a trained checkpoint through the CLI entry point."""
import csv

import pytest

from microbeast_amd.cli import main
from microbeast_amd.config import parse_flags

pytestmark = pytest.mark.gpu

SUMMARY = ["opponent", "episodes", "wins", "draws", "losses", "win_rate", "win_rate_lo",
           "win_rate_hi", "mean_return", "mean_steps"]


def _evaluate(tmp, name, *extra):
    from microbeast_amd.evaluate import evaluate
    flags = parse_flags(["--test", "--allow_random_init", "--exp_name", name, "--savedir",
                         str(tmp), "--actor_threads", "4", *extra], interactive=False)
    return evaluate(flags)


def _check(tmp, name, n, max_steps):
    with open(tmp / f"{name}_eval.csv") as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Return", "steps", "env_index", "winner", "opponent"]
    body = rows[1:]
    assert len(body) == n
    idx = [int(r[2]) for r in body]
    assert idx == sorted(idx) and len(set(idx)) == n
    assert all(0 < int(r[1]) <= max_steps for r in body)
    # envs take the default opponent list round-robin: env i plays bot list[i % 6]
    bots = [0, 0, 0, 1, 2, 3]
    assert all(int(r[4]) == -1 - bots[int(r[2]) % 6] for r in body)
    with open(tmp / f"{name}_eval_summary.csv") as f:
        srows = list(csv.DictReader(f))
    assert list(srows[0]) == SUMMARY and srows[-1]["opponent"] == "all"
    assert int(srows[-1]["episodes"]) == n
    assert sum(int(r["episodes"]) for r in srows[:-1]) == n
    assert {r["opponent"] for r in srows[:-1]} == {"coac", "random_biased", "light_rush",
                                                   "worker_rush"}
    for r in srows:
        assert int(r["wins"]) + int(r["draws"]) + int(r["losses"]) == int(r["episodes"])
        assert float(r["win_rate_lo"]) <= float(r["win_rate"]) <= float(r["win_rate_hi"])
    for k in ("wins", "draws", "losses"):
        assert sum(int(r[k]) for r in srows[:-1]) == int(srows[-1][k])
    return body, srows


E_FLAGS = ["--env_size", "16", "--eval_envs", "64", "--unroll_length", "16",
           "--max_episode_steps", "96"]


def test_engine_eval_fused_greedy(cuda, tmp_path):
    r1 = _evaluate(tmp_path, "a", *E_FLAGS, "--eval_greedy")
    assert r1["mode"] == "engine" and r1["acting"] == "fused" and r1["greedy"] is True
    assert r1["episodes"] == 64 and r1["frames"] > 0 and r1["fps"] > 0 and r1["seconds"] > 0
    assert set(r1["per_opponent"]) == {"coac", "random_biased", "light_rush", "worker_rush"}
    _check(tmp_path, "a", 64, 96)
    r2 = _evaluate(tmp_path, "b", *E_FLAGS, "--eval_greedy")
    assert r2["acting"] == "fused"
    for suffix in ("_eval.csv", "_eval_summary.csv"):
        assert (tmp_path / f"a{suffix}").read_bytes() == (tmp_path / f"b{suffix}").read_bytes()


def test_engine_eval_fused_sampled(cuda, tmp_path):
    r = _evaluate(tmp_path, "s", *E_FLAGS)
    assert r["mode"] == "engine" and r["acting"] == "fused" and r["greedy"] is False
    _check(tmp_path, "s", 64, 96)


def test_engine_eval_graph_path(cuda, tmp_path):
    r = _evaluate(tmp_path, "g", "--env_size", "8", "--eval_envs", "37", "--unroll_length", "16",
                  "--max_episode_steps", "120", "--eval_greedy")
    assert r["mode"] == "engine" and r["acting"] == "graph" and r["greedy"] is True
    _check(tmp_path, "g", 37, 120)


def test_engine_eval_refuses_ragged_groups(cuda, tmp_path):
    with pytest.raises(ValueError, match="multiple"):
        _evaluate(tmp_path, "r", "--env_size", "8", "--eval_envs", "48", "--envs_per_group", "32")


def test_trained_checkpoint_evaluates_through_cli(cuda, tmp_path):
    train = ["--exp_name", "t", "--runtime", "gpu", "--env_size", "8", "--groups", "2",
             "--envs_per_group", "32", "--unroll_length", "8", "--batch_size", "1", "--savedir",
             str(tmp_path), "--quiet", "--max_episode_steps", "40"]
    assert main(train + ["--max_updates", "2"]) == 0
    assert (tmp_path / "t.ckpt").exists()
    assert main(train + ["--test", "--eval_envs", "32", "--eval_greedy"]) == 0
    _check(tmp_path, "t", 32, 40)


def test_set_greedy_only_before_start(cuda):
    from microbeast_amd.models.agent import Agent
    from microbeast_amd.ops.optim import FlatParams
    from microbeast_amd.runtime.gpu_actors import GpuActorRuntime
    rt = GpuActorRuntime(lambda: Agent((8, 8, 27)), 8, 1, 16, 4, 1, cuda, n_threads=1,
                         max_steps=20, greedy=True)
    try:
        assert rt.engine.greedy() is True
        rt.engine.set_greedy(False)
        rt.engine.set_greedy(True)
        rt.start(FlatParams(Agent((8, 8, 27)).to(cuda), cuda))
        with pytest.raises(RuntimeError, match="set_greedy"):
            rt.engine.set_greedy(False)
        _, slots = rt.get_batch(1, timeout=60)
        rt.release(slots)
        rt.stop()
        with pytest.raises(RuntimeError, match="set_greedy"):  # also after a stop
            rt.engine.set_greedy(False)
    finally:
        rt.close()
