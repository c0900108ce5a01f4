"""bench.py's own options: ``--dump-outputs`` (what the last timed update computed, as .npy
files under a byte budget) and ``--full`` (the measurements beyond the headline figure)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_budget_and_seeded_sample(tmp_path, monkeypatch):
    """An array over its share of the budget is cut to the same sorted sample for the same
    seed; a smaller one is written whole; everything is float32 and within the budget."""
    import torch

    import bench

    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 200)  # 200 floats in all
    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    small = torch.tensor([[1, 2], [3, 4]], dtype=torch.int32)
    for d in ("a", "b"):
        bench._dump_outputs(str(tmp_path / d), {"big": big, "small": small}, seed=7)
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (196,)  # what the small array left
    assert np.array_equal(a, b) and np.all(np.diff(a) > 0)  # values are their own indices
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, [[1, 2], [3, 4]])
    assert a.nbytes + s.nbytes <= 4 * 200
    bench._dump_outputs(str(tmp_path / "c"), {"big": big, "small": small}, seed=8)
    assert not np.array_equal(a, np.load(tmp_path / "c" / "big.npy"))


def _run_bench(out_dir, *extra):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--settle", "2", "--groups", "2", "--envs_per_group", "128", "--unroll", "16",
           "--threads", "2", "--dump-outputs", str(out_dir), *extra]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(out_dir / f) for f in sorted(os.listdir(out_dir))}


@pytest.mark.gpu
def test_bench_full_and_dump_outputs(cuda, tmp_path):
    """Two small runs with the same arguments: the result line keeps its fields, ``--steps``
    sets the timed steps, ``--full`` adds the sync-timed phase split, and the dumped arrays
    (one rollout's rows, the losses and the parameters of the update on it) are the same bit
    for bit in both runs."""
    out, arrs = _run_bench(tmp_path / "a", "--full")
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out
    assert out["steps"] == 3 and out["ms_per_step"] > 0 and out["value"] > 0
    assert out["learner_phase_s"]  # --full
    assert set(arrs) == {"losses", "params", "batch_logp", "batch_value", "batch_reward"}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 << 20
    assert arrs["losses"].shape == (5,) and arrs["losses"][2] > 0  # entropy of a fresh policy
    assert arrs["params"].ndim == 1 and arrs["params"].size > 5e6 and arrs["params"].std() > 0
    for k in ("batch_logp", "batch_value", "batch_reward"):
        assert arrs[k].shape == (17, 128)
    assert (arrs["batch_logp"] <= 0).all() and (arrs["batch_logp"] < 0).any()
    out2, arrs2 = _run_bench(tmp_path / "b")
    assert "learner_phase_s" not in out2
    for k, a in arrs.items():
        np.testing.assert_array_equal(a, arrs2[k], err_msg=k)
