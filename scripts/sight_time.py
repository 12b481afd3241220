"""Times of line-of-sight neighbour sensing: env.observe with and without `occlusion`, with the
sensor model (sigma = 0.05, dropout = 0.2) and without it, and env.line_of_sight alone, at 4096 LidarSpread envs (n = 8,
3 obstacles), measured as scripts/observe_time.py does (device events around `--calls` back-to-back calls through the
Python API, `--windows` windows alternating); and a captured `collect` (128 envs, a whole episode) with and without
occlusion.  Prints one JSON line (median, min, max; microseconds per call, milliseconds per collect)."""
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
    env = make_env("LidarSpread", 8, num_obs=3, device=dev)
    s = env.reset(key=1, n_env=args.envs).env_states
    agent, ob = s.agent, s.obstacle
    out = env.empty_graph((args.envs,), dev)
    kernels = windows({
        "observe": lambda: env.observe(s, 1, sigma=sigma, dropout=dropout, seed=3, out=out),
        "observe_occlusion": lambda: env.observe(s, 1, sigma=sigma, dropout=dropout, seed=3, out=out, occlusion=True),
        "observe_perfect": lambda: env.observe(s, 1, sigma=0.0, dropout=0.0, seed=3, out=out),
        "observe_perfect_occlusion": lambda: env.observe(s, 1, sigma=0.0, dropout=0.0, seed=3, out=out, occlusion=True),
        "line_of_sight": lambda: env.line_of_sight(agent, ob),
    }, args.calls, args.windows, 1e3)

    def algo_of(**flags):
        return make_algo("dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                         action_dim=env.action_dim, n_agents=env.num_agents, batch_size=16384, seed=0, device=dev,
                         **flags)

    plain, perfect, hidden = algo_of(), algo_of(lidar_noise=0.0, lidar_dropout=0.0), algo_of(lidar_occlusion=True)
    collects = windows({
        "collect": lambda: plain.collect(plain.params, 5, n_env=args.collect_envs),
        "collect_observed": lambda: perfect.collect(perfect.params, 5, n_env=args.collect_envs),
        "collect_occlusion": lambda: hidden.collect(hidden.params, 5, n_env=args.collect_envs),
    }, 3, args.collect_windows, 1.0)
    print(json.dumps({"envs": args.envs, "calls": args.calls, "windows": args.windows, "us_per_call": kernels,
                      "collect_envs": args.collect_envs, "steps": env.max_episode_steps, "ms_per_collect": collects}))


if __name__ == "__main__":
    main()
