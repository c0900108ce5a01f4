"""Checkpoint evaluation with ``--eval_envs`` (every env's first episode) and greedy acting,
on the CPU: flags, the torch greedy sampler, the selection rule, the Wilson interval and the
host-stepped evaluation path (evaluate.py)."""
import csv
import math

import pytest
import torch

from microbeast_amd.config import Flags, parse_flags
from microbeast_amd.ops import cell_head
from microbeast_amd.ops.cell_head import OFFS, pack_mask

HOST = ["--test", "--allow_random_init", "--device", "cpu", "--env_size", "4", "--eval_envs", "12",
        "--max_episode_steps", "40"]


def test_flag_defaults_and_parsing():
    assert Flags().eval_envs == 0 and Flags().eval_greedy is False
    f = parse_flags(["--test"], interactive=False)
    assert f.eval_envs == 0 and f.eval_greedy is False
    f = parse_flags(["--test", "--eval_envs", "64", "--eval_greedy"], interactive=False)
    assert f.eval_envs == 64 and f.eval_greedy is True
    assert parse_flags(["--eval_greedy", "false"], interactive=False).eval_greedy is False


def _tied_problem(seed=0, n=5, S=9):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, S * 78, generator=g)
    mask = torch.rand(n, S, 78, generator=g) < 0.5
    z = logits.view(n, S, 78)
    # exact ties at the legal maximum: the lowest legal index must win
    mask[0, 0, :6] = torch.tensor([False, True, False, True, True, False])
    z[0, 0, :6] = torch.tensor([9.0, 3.0, 8.0, 3.0, 3.0, 7.0])      # -> 1
    mask[1, 2, 29:78] = False
    mask[1, 2, 40], mask[1, 2, 41], mask[1, 2, 70] = True, True, True
    z[1, 2, 40], z[1, 2, 41], z[1, 2, 70] = 2.5, 2.5, 2.5            # -> 40 - 29 = 11
    z[1, 2, 30] = 50.0                                               # masked: never chosen
    mask[2, 3] = False                                               # a fully masked cell
    mask[3, 1, 22:29] = False                                        # a fully masked segment
    mask[4, 4, 6:10] = torch.tensor([False, False, True, False])     # a single legal bit
    return logits, mask


def test_cpu_greedy_sample_matches_greedy_and_scoring():
    logits, mask = _tied_problem()
    bits = pack_mask(mask)
    a, lp = cell_head.sample(logits, bits, greedy=True)
    assert a.dtype == torch.uint8 and torch.equal(a, cell_head.greedy(logits, bits))
    lp_ref, _ = cell_head.score(logits, bits, a)
    assert torch.equal(lp, lp_ref)
    assert int(a[0, 0, 0]) == 1 and int(a[1, 2, 6]) == 11 and int(a[4, 4, 1]) == 2
    assert int(a[2, 3].sum()) == 0 and int(a[3, 1, 5]) == 0
    # every chosen action is legal wherever its segment has a legal action
    al = a.long()
    for k in range(7):
        seg = mask[..., OFFS[k]:OFFS[k + 1]]
        assert bool((seg.gather(-1, al[..., k:k + 1]).squeeze(-1) | ~seg.any(-1)).all())
    # a fully masked cell: action 0, log-prob 0
    one = torch.randn(1, 78)
    a1, lp1 = cell_head.sample(one, torch.zeros(1, 1, 3, dtype=torch.int32), greedy=True)
    assert int(a1.sum()) == 0 and float(lp1) == 0.0
    # no random numbers: generators do not matter
    a2, lp2 = cell_head.sample(logits, bits, generator=torch.Generator().manual_seed(9),
                               greedy=True)
    assert torch.equal(a, a2) and torch.equal(lp, lp2)


def test_agent_act_greedy_cpu():
    from microbeast_amd.models.agent import Agent
    torch.manual_seed(0)
    m = Agent((8, 8, 27), compute_dtype=torch.float32, hip_kernels=False).eval()
    torch.nn.init.normal_(m.actor.weight, std=0.05)
    g = torch.Generator().manual_seed(1)
    obs = torch.randint(0, 2 ** 26, (5, 64), dtype=torch.int32, generator=g)
    bits = pack_mask(torch.rand(5, 64, 78, generator=g) < 0.3)
    a1, lp1, v1 = m.act(obs, bits, generator=torch.Generator().manual_seed(1), greedy=True)
    a2, lp2, _ = m.act(obs, bits, generator=torch.Generator().manual_seed(2), greedy=True)
    with torch.no_grad():
        logits, v = m.policy_value(obs)
    assert torch.equal(a1, cell_head.greedy(logits, bits))
    assert torch.equal(a1, a2) and torch.equal(lp1, lp2) and torch.equal(v1, v)
    a3, _, _ = m.act(obs, bits, generator=torch.Generator().manual_seed(1))
    assert not torch.equal(a1, a3)  # the default still samples


def test_gridnet_act_greedy_cpu():
    from microbeast_amd.models.gridnet import GridNetAgent
    torch.manual_seed(0)
    m = GridNetAgent((8, 8, 27), compute_dtype=torch.float32, hip_kernels=False).eval()
    g = torch.Generator().manual_seed(1)
    obs = torch.randint(0, 2 ** 26, (3, 64), dtype=torch.int32, generator=g)
    bits = pack_mask(torch.rand(3, 64, 78, generator=g) < 0.3)
    a, lp, _ = m.act(obs, bits, greedy=True)
    with torch.no_grad():
        logits, _ = m.policy_value(obs)
    assert torch.equal(a, cell_head.greedy(logits, bits))
    assert torch.equal(lp, cell_head.score(logits, bits, a)[0])


def test_first_episode_selection():
    from microbeast_amd.evaluate import first_episodes, summarize
    # env 0 finishes three short losses before env 1 finishes one long win
    stream = [(-9.0, 50, 0, 1, -1), (-8.0, 40, 0, 1, -1), (-7.0, 45, 0, 1, -1),
              (12.0, 390, 1, 0, -2), (-6.0, 30, 0, 1, -1), (3.0, 100, 1, 0, -2)]
    sel = {}
    first_episodes(sel, stream[:2], 2)
    assert len(sel) == 1
    first_episodes(sel, stream[2:], 2)
    assert sorted(sel) == [0, 1]
    assert sel[0] == stream[0] and sel[1] == stream[3]
    rows = summarize([sel[0], sel[1]])
    assert [r["opponent"] for r in rows] == ["coac", "random_biased", "all"]
    assert rows[-1]["episodes"] == 2 and rows[-1]["wins"] == 1 and rows[-1]["losses"] == 1
    assert rows[-1]["mean_steps"] == 220.0  # not the 4 losses + 2 wins of the raw stream
    with pytest.raises(ValueError):
        first_episodes({}, [(0.0, 1, 2, 0, -1)], 2)
    with pytest.raises(ValueError):
        first_episodes({}, [(0.0, 1, 4, 0, -1)], 2, base=5)


def test_wilson_interval_closed_form():
    from microbeast_amd.evaluate import wilson_interval
    z = 1.96
    for w, n in [(0, 10), (5, 10), (10, 10)]:
        p = w / n
        c = (p + z * z / (2 * n)) / (1 + z * z / n)
        h = z * math.sqrt(p * (1 - p) / n + z * z / (4 * n * n)) / (1 + z * z / n)
        lo, hi = wilson_interval(w, n)
        assert lo == pytest.approx(max(0.0, c - h), abs=1e-12)
        assert hi == pytest.approx(min(1.0, c + h), abs=1e-12)
        assert 0.0 <= lo <= p <= hi <= 1.0
    # known values (z = 1.96): 0/10 -> [0, 0.2775], 5/10 -> [0.2366, 0.7634], 10/10 -> [0.7225, 1]
    assert wilson_interval(0, 10)[0] == pytest.approx(0.0, abs=1e-12)
    assert wilson_interval(0, 10)[1] == pytest.approx(0.2775, abs=1e-4)
    assert wilson_interval(5, 10) == pytest.approx((0.2366, 0.7634), abs=1e-4)
    assert wilson_interval(10, 10)[0] == pytest.approx(0.7225, abs=1e-4)
    assert wilson_interval(10, 10)[1] == pytest.approx(1.0, abs=1e-12)


def _run(tmp_path, name, extra=()):
    from microbeast_amd.evaluate import evaluate
    flags = parse_flags(HOST + ["--exp_name", name, "--savedir", str(tmp_path)] + list(extra),
                        interactive=False)
    res = evaluate(flags)
    return res, (tmp_path / f"{name}_eval.csv"), (tmp_path / f"{name}_eval_summary.csv")


def _check_outputs(res, ep_path, sum_path, n, max_steps, counts):
    with open(ep_path) as f:
        rows = list(csv.reader(f))
    assert rows[0] == ["Return", "steps", "env_index", "winner", "opponent"]
    body = rows[1:]
    assert len(body) == n
    idx = [int(r[2]) for r in body]
    assert idx == sorted(idx) and len(set(idx)) == n
    assert all(int(r[1]) <= max_steps for r in body)
    with open(sum_path) as f:
        srows = list(csv.DictReader(f))
    assert list(srows[0]) == ["opponent", "episodes", "wins", "draws", "losses", "win_rate",
                              "win_rate_lo", "win_rate_hi", "mean_return", "mean_steps"]
    assert srows[-1]["opponent"] == "all"
    assert {r["opponent"]: int(r["episodes"]) for r in srows} == counts
    for r in srows:
        assert int(r["wins"]) + int(r["draws"]) + int(r["losses"]) == int(r["episodes"])
        assert float(r["win_rate_lo"]) <= float(r["win_rate"]) <= float(r["win_rate_hi"])
    assert res["episodes"] == n and set(res["per_opponent"]) == set(counts) - {"all"}
    assert res["frames"] > 0 and res["seconds"] > 0 and res["fps"] > 0


def test_host_path_evaluation(tmp_path):
    res, ep, sm = _run(tmp_path, "h")
    assert res["mode"] == "host" and res["acting"] == "host" and res["greedy"] is False
    counts = {"coac": 6, "random_biased": 2, "light_rush": 2, "worker_rush": 2, "all": 12}
    _check_outputs(res, ep, sm, 12, 40, counts)


def test_host_path_greedy_is_deterministic(tmp_path):
    r1, ep1, sm1 = _run(tmp_path, "g1", ["--eval_greedy"])
    r2, ep2, sm2 = _run(tmp_path, "g2", ["--eval_greedy"])
    assert r1["greedy"] is True and r1["mode"] == "host"
    assert ep1.read_bytes() == ep2.read_bytes() and sm1.read_bytes() == sm2.read_bytes()
    counts = {"coac": 6, "random_biased": 2, "light_rush": 2, "worker_rush": 2, "all": 12}
    _check_outputs(r1, ep1, sm1, 12, 40, counts)


def test_eval_envs_zero_keeps_the_old_loop(tmp_path):
    from microbeast_amd.evaluate import evaluate
    flags = parse_flags(["--test", "--allow_random_init", "--device", "cpu", "--env_size", "4",
                         "--max_episode_steps", "30", "--eval_episodes", "3", "--eval_greedy",
                         "--exp_name", "old", "--savedir", str(tmp_path)], interactive=False)
    res = evaluate(flags)
    assert "mode" not in res and res["episodes"] == 3
    with open(tmp_path / "old_eval.csv") as f:
        assert f.readline().strip() == "Return,steps,env_index,winner"
    assert not (tmp_path / "old_eval_summary.csv").exists()


def test_self_play_with_eval_envs_is_refused(tmp_path):
    from microbeast_amd.evaluate import evaluate
    flags = parse_flags(["--test", "--allow_random_init", "--device", "cpu", "--self_play",
                         "--eval_envs", "8", "--savedir", str(tmp_path)], interactive=False)
    with pytest.raises(ValueError, match="--self_play"):
        evaluate(flags)
