"""Times of the sensor-in-the-loop kernels against plain get_graph: env.lidar_scan, env.lidar_hits,
get_graph(lidar_data=), the three chained, and get_graph of the same build, at 4096 LidarSpread envs (n = 8, 3
obstacles).  Device events around `--calls` back-to-back calls through the Python API (host launch included),
`--windows` windows alternating between the five; prints one JSON line (median, min, max in microseconds per call)."""
import argparse
import json
import statistics
import sys
import os

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dgppo_fov_amd.env import make_env  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    env = make_env("LidarSpread", 8, num_obs=3, device=dev)
    g = env.reset(key=1, n_env=args.envs)
    s = g.env_states
    agent, ob = s.agent, s.obstacle
    alpha = env.lidar_scan(agent, ob)
    hits = env.lidar_hits(agent, alpha)
    out = env.empty_graph((args.envs,), dev)
    fns = {
        "lidar_scan": lambda: env.lidar_scan(agent, ob),
        "lidar_hits": lambda: env.lidar_hits(agent, alpha),
        "get_graph_hits": lambda: env.get_graph(s, out=out, lidar_data=hits),
        "scan_hits_graph": lambda: env.get_graph(s, out=out, lidar_data=env.lidar_hits(agent, env.lidar_scan(agent, ob))),
        "get_graph": lambda: env.get_graph(s, out=out),
    }
    for f in fns.values():  # warm-up
        for _ in range(5):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(args.windows):
        for name, f in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                f()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) * 1e3 / args.calls)
    print(json.dumps({"envs": args.envs, "calls": args.calls, "windows": args.windows, "us_per_call": {
        k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        for k, v in times.items()}}))


if __name__ == "__main__":
    main()
