"""Times of the fused sensor kernel against the chained launches: env.observe and
get_graph(lidar_data=lidar_hits(LidarNoise(lidar_scan))) at 4096 LidarSpread envs (n = 8, 3 obstacles), sigma = 0.05 and
dropout = 0.2, measured as scripts/sensor_time.py does (device events around `--calls` back-to-back calls through the
Python API, `--windows` windows alternating); and a captured `collect` (128 envs, a whole episode) with and without the
sensor model.  Prints one JSON line (median, min, max; microseconds per call, milliseconds per collect)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dgppo_fov_amd.algo import make_algo  # noqa: E402
from dgppo_fov_amd.env import make_env  # noqa: E402
from dgppo_fov_amd.utils.sensor import LidarNoise  # noqa: E402


def windows(fns, calls, n_windows, scale):
    for f in fns.values():  # warm-up
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(n_windows):
        for name, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                f()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * scale / calls)
    return {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
            for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--collect-envs", type=int, default=128)
    ap.add_argument("--collect-windows", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sigma, dropout = 0.05, 0.2
    env = make_env("LidarSpread", 8, num_obs=3, device=dev)
    s = env.reset(key=1, n_env=args.envs).env_states
    agent, ob = s.agent, s.obstacle
    out = env.empty_graph((args.envs,), dev)
    sensor = LidarNoise(sigma, dropout, 3, sense_range=float(env.params["comm_radius"]))
    kernels = windows({
        "observe": lambda: env.observe(s, 1, sigma=sigma, dropout=dropout, seed=3, out=out),
        "observe_perfect": lambda: env.observe(s, 1, sigma=0.0, dropout=0.0, seed=3, out=out),
        "scan_noise_hits_graph": lambda: env.get_graph(s, out=out, lidar_data=env.lidar_hits(
            agent, sensor(env.lidar_scan(agent, ob), 1))),
        "get_graph": lambda: env.get_graph(s, out=out),
    }, args.calls, args.windows, 1e3)

    def algo_of(**flags):
        return make_algo("dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                         action_dim=env.action_dim, n_agents=env.num_agents, batch_size=16384, seed=0, device=dev,
                         **flags)

    plain, sensed = algo_of(), algo_of(lidar_noise=sigma, lidar_dropout=dropout)
    collects = windows({
        "collect": lambda: plain.collect(plain.params, 5, n_env=args.collect_envs),
        "collect_sensed": lambda: sensed.collect(sensed.params, 5, n_env=args.collect_envs),
    }, 3, args.collect_windows, 1.0)
    print(json.dumps({"envs": args.envs, "calls": args.calls, "windows": args.windows, "us_per_call": kernels,
                      "collect_envs": args.collect_envs, "steps": env.max_episode_steps, "ms_per_collect": collects}))


if __name__ == "__main__":
    main()
