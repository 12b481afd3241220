"""Time VMASEnv.render_frames against the store-only floor, by the method of scripts/render_time.py.

5 episodes x 128 frames at S = 1000 (the reference's dpi 100) of VMASWheel (7 primitives per frame) and
VMASReverseTransport (10), from a random-action rollout: HIP events around render_frames into a preallocated buffer,
interleaved in one process with a fill_ of the same output bytes (what it costs only to store the images).  Writes one
JSON file (profiles/vmas_render_time.json).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dgppo_fov_amd.env import make_env  # noqa: E402
from dgppo_fov_amd.trainer.rollout import RolloutEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/vmas_render_time.json")
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    S, B, T = args.size, args.episodes, args.frames
    rows = []
    for eid, prims in (("VMASWheel", 7), ("VMASReverseTransport", 10)):
        env = make_env(eid, 3, max_step=T, device=dev)
        eng = RolloutEngine(env, B, T, dev)
        eng.actions.uniform_(-1, 1)
        roll = eng.run(1)
        out = torch.empty((B, T, S, S, 4), dtype=torch.uint8, device=dev)
        flat = out.view(-1)
        ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
        t_render, t_fill = [], []
        for r in range(args.rounds + 2):  # two warm-up rounds, then alternate
            a, b, c = ev(), ev(), ev()
            a.record()
            env.render_frames(roll.graph, size=S, out=out)
            b.record()
            flat.fill_(255)
            c.record()
            torch.cuda.synchronize()
            if r >= 2:
                t_render.append(a.elapsed_time(b))
                t_fill.append(b.elapsed_time(c))
        row = dict(env=eid, frames=B * T, size=S, out_bytes=out.numel(), primitives_per_frame=prims,
                   render_ms_median=statistics.median(t_render), render_ms_min=min(t_render),
                   fill_ms_median=statistics.median(t_fill), fill_ms_min=min(t_fill))
        row["render_over_fill"] = row["render_ms_median"] / row["fill_ms_median"]
        del out, flat
        rows.append(row)
        print(json.dumps(row))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), method="HIP events, interleaved in one process, "
                       f"{args.rounds} rounds after 2 warm-up rounds; fill = torch fill_ of the same output bytes",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
