"""bench.py on the device: a plain run does the timed steps only and prints the headline line, and --dump-outputs
writes the last timed step's rollout reproducibly (float32 / float64 .npy files within the byte budget)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
NAMES = ("envs", "nodes", "edges", "states", "receivers", "senders", "rewards", "costs")

pytestmark = pytest.mark.gpu


def _load(d):
    return {os.path.basename(f)[:-4]: np.load(f) for f in sorted(glob.glob(os.path.join(str(d), "*.npy")))}


def test_dump_outputs_is_the_sampled_rollout(cuda, tmp_path, monkeypatch):
    """dump_outputs on a small engine: with a budget below the whole rollout it writes a seeded sample of envs whose
    rows are the engine's Rollout bit for bit, the same sample every time, within the budget."""
    import bench
    from dgppo_fov_amd.env import make_env
    from dgppo_fov_amd.trainer.rollout import RolloutEngine

    B, T = 48, 5
    env = make_env("LidarSpread", 8, num_obs=3, device=cuda)
    eng = RolloutEngine(env, B, T, cuda)
    gen = torch.Generator(device=cuda)
    gen.manual_seed(5)
    eng.actions.uniform_(-1.0, 1.0, generator=gen)
    r = eng.run(key=11)
    torch.cuda.synchronize(cuda)

    bench.dump_outputs(eng, str(tmp_path / "all"))
    full = _load(tmp_path / "all")
    assert set(full) == set(NAMES)
    assert np.array_equal(full["envs"], np.arange(B))  # everything fits the default budget
    per_env = sum(v.nbytes for v in full.values()) // B
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4096 + 17 * per_env + per_env // 2)
    bench.dump_outputs(eng, str(tmp_path / "a"))
    bench.dump_outputs(eng, str(tmp_path / "b"))
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    files = glob.glob(os.path.join(str(tmp_path / "a"), "*.npy"))
    assert sum(os.path.getsize(f) for f in files) <= bench.DUMP_BUDGET_BYTES
    idx = a["envs"].astype(np.int64)
    assert len(idx) == 17 and len(set(idx)) == 17 and np.array_equal(idx, np.sort(idx)) and idx.max() < B
    for k in NAMES:
        assert a[k].dtype in (np.float32, np.float64), k
        assert np.array_equal(a[k], b[k]), k
        assert np.array_equal(a[k], full[k][idx]), k
    g, ng, sel = r.graph, r.next_graph, torch.as_tensor(idx, device=cuda)
    for k in ("nodes", "edges", "states", "receivers", "senders"):
        assert a[k].shape[:2] == (17, T + 1)
        assert np.array_equal(a[k][:, :T], getattr(g, k)[sel].cpu().numpy()), k
        assert np.array_equal(a[k][:, 1:], getattr(ng, k)[sel].cpu().numpy()), k
    assert np.array_equal(a["rewards"], r.rewards[sel].cpu().numpy())
    assert np.array_equal(a["costs"], r.costs[sel].cpu().numpy())


def test_plain_run_prints_the_headline_line_and_dumps(cuda, tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR`: one JSON line with the headline fields,
    none of the --full measurements, and the rollout files within 64 MB."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR",
                                                             "MASTER_PORT", "LOCAL_WORLD_SIZE")}
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs",
                          str(tmp_path)], env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    (line,) = [x for x in out.stdout.splitlines() if x.startswith("{")]
    d = json.loads(line)
    assert d["steps"] == 3 and d["warmup"] == 1 and d["unit"] == "env-steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["full"] is False and d["ms_per_step"] > 0
    envs, T = d["config"]["n_env_per_gpu"], d["config"]["T"]
    assert abs(d["value"] - envs * T / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    for k in ("ppo", "roofline", "cpu_baseline", "cpu_baseline_update", "cpu_baseline_rollout", "env_step_kernel_us"):
        assert k not in d, k
    arrs = _load(tmp_path)
    assert set(arrs) == set(NAMES)
    assert sum(os.path.getsize(f) for f in glob.glob(os.path.join(str(tmp_path), "*.npy"))) <= 64 * 10 ** 6
    n = len(arrs["envs"])
    assert 1 <= n <= envs and arrs["nodes"].shape[:2] == (n, T + 1) and arrs["rewards"].shape == (n, T)
    assert all(v.dtype in (np.float32, np.float64) and np.isfinite(v).all() for v in arrs.values())
