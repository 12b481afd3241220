"""Times of LiDAR body returns: env.observe and env.lidar_scan with and without `bodies`, with the
sensor model (sigma = 0.05, dropout = 0.2), at 4096 LidarSpread envs of n = 8 agents and 3 obstacles and of n = 32 agents
and 8 obstacles, measured as scripts/observe_time.py does (device events around `--calls` back-to-back calls through the
Python API, `--windows` windows alternating); and a captured `collect` (128 envs, a whole episode) under the sensor
model with and without the flag.  Prints one JSON line (median, min, max; microseconds per call, milliseconds per
collect)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dgppo_fov_amd.algo import make_algo  # noqa: E402
from dgppo_fov_amd.env import make_env  # noqa: E402
from observe_time import windows  # noqa: E402


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
    kernels = {}
    for n, obs in ((8, 3), (32, 8)):
        env = make_env("LidarSpread", n, num_obs=obs, device=dev)
        s = env.reset(key=1, n_env=args.envs).env_states
        agent, ob = s.agent, s.obstacle
        out = env.empty_graph((args.envs,), dev)
        noisy = dict(sigma=sigma, dropout=dropout, seed=3, out=out)
        kernels[f"n{n}_o{obs}"] = windows({
            "observe": lambda: env.observe(s, 1, **noisy),
            "observe_bodies": lambda: env.observe(s, 1, bodies=True, **noisy),
            "lidar_scan": lambda: env.lidar_scan(agent, ob),
            "lidar_scan_bodies": lambda: env.lidar_scan(agent, ob, bodies=True),
        }, args.calls, args.windows, 1e3)

    env = make_env("LidarSpread", 8, num_obs=3, device=dev)

    def algo_of(**flags):
        return make_algo("dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                         action_dim=env.action_dim, n_agents=env.num_agents, batch_size=16384, seed=0, device=dev,
                         lidar_noise=sigma, lidar_dropout=dropout, **flags)

    sensed, bodies = algo_of(), algo_of(lidar_bodies=True)
    collects = windows({
        "collect_sensed": lambda: sensed.collect(sensed.params, 5, n_env=args.collect_envs),
        "collect_sensed_bodies": lambda: bodies.collect(bodies.params, 5, n_env=args.collect_envs),
    }, 3, args.collect_windows, 1.0)
    print(json.dumps({"envs": args.envs, "calls": args.calls, "windows": args.windows, "us_per_call": kernels,
                      "collect_envs": args.collect_envs, "steps": env.max_episode_steps, "ms_per_collect": collects}))


if __name__ == "__main__":
    main()
