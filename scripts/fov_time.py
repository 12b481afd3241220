"""Times of field-of-view neighbour sensing: env.observe with and without `fov`, with the sensor
model (sigma = 0.05, dropout = 0.2) and without it, with `fov` and `occlusion` together, and env.field_of_view alone, at
4096 LidarOmniTarget envs (n = 8, 3 obstacles), measured as scripts/observe_time.py does (device events around `--calls`
back-to-back calls through the Python API, `--windows` windows alternating).  Prints one JSON line (median, min, max;
microseconds per call)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dgppo_fov_amd.env import make_env  # noqa: E402
from observe_time import windows  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--windows", type=int, default=40)
    ap.add_argument("--fov", type=float, default=60.0)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    sigma, dropout, fov = 0.05, 0.2, args.fov
    env = make_env("LidarOmniTarget", 8, num_obs=3, device=dev)
    s = env.reset(key=1, n_env=args.envs).env_states
    out = env.empty_graph((args.envs,), dev)
    noisy, perfect = dict(sigma=sigma, dropout=dropout, seed=3, out=out), dict(sigma=0.0, dropout=0.0, seed=3, out=out)
    kernels = windows({
        "observe": lambda: env.observe(s, 1, **noisy),
        "observe_fov": lambda: env.observe(s, 1, fov=fov, **noisy),
        "observe_occlusion": lambda: env.observe(s, 1, occlusion=True, **noisy),
        "observe_fov_occlusion": lambda: env.observe(s, 1, fov=fov, occlusion=True, **noisy),
        "observe_perfect": lambda: env.observe(s, 1, **perfect),
        "observe_perfect_fov": lambda: env.observe(s, 1, fov=fov, **perfect),
        "field_of_view": lambda: env.field_of_view(s.agent, fov),
    }, args.calls, args.windows, 1e3)
    print(json.dumps({"envs": args.envs, "calls": args.calls, "windows": args.windows, "fov": fov,
                      "us_per_call": kernels}))


if __name__ == "__main__":
    main()
