"""Time env.render_frames against the store-only floor, and the host side of env.render_video next to it.

5 episodes x 128 frames at S = 1000 (the reference's dpi 100) of LidarSpread n = 8 / 3 obstacles and n = 32 / 8
obstacles, from a random-action rollout: HIP events around render_frames into a preallocated buffer, interleaved in one
process with a torch.full of the same output bytes (what it costs only to store the images).  Then one
render_video call per config (128 frames: device frames + copy + Pillow text, quantisation and GIF encoding), with the
device + copy part timed on its own so the Pillow share is visible.  Writes one JSON file (profiles/render_time.json).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dgppo_fov_amd.env import make_env  # noqa: E402
from dgppo_fov_amd.trainer.rollout import RolloutEngine  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/render_time.json")
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--episodes", type=int, default=5)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--no-video", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    S, B, T = args.size, args.episodes, args.frames
    rows = []
    for n, obs in ((8, 3), (32, 8)):
        env = make_env("LidarSpread", n, num_obs=obs, max_step=T, device=dev)
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
        row = dict(env="LidarSpread", n=n, obs=obs, frames=B * T, size=S, out_bytes=out.numel(),
                   primitives_per_frame=env.n_edges + 2 * n + obs,
                   render_ms_median=statistics.median(t_render), render_ms_min=min(t_render),
                   fill_ms_median=statistics.median(t_fill), fill_ms_min=min(t_fill))
        row["render_over_fill"] = row["render_ms_median"] / row["fill_ms_median"]
        if not args.no_video:
            unsafe = (roll.costs >= 0.0).any(dim=-1)[0]
            with tempfile.TemporaryDirectory() as d:
                t0 = time.perf_counter()
                env.render_video(roll, f"{d}/e.gif", unsafe, dpi=S // 10, episode=0)
                row["render_video_s_per_episode"] = time.perf_counter() - t0
            g = roll.graph
            sub = env._assemble(g.nodes[0], g.edges[0], g.states[0], g.receivers[0], g.senders[0],
                                None if eng.obstacles is None else eng.obstacles[0].expand(T, -1, -1))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            env.render_frames(sub, size=S)[..., :3].cpu()
            row["device_frames_and_copy_s_per_episode"] = time.perf_counter() - t0
            row["pillow_s_per_episode"] = row["render_video_s_per_episode"] - row["device_frames_and_copy_s_per_episode"]
        del out, flat
        rows.append(row)
        print(json.dumps(row))
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), method="HIP events, interleaved in one process, "
                       f"{args.rounds} rounds after 2 warm-up rounds; fill = torch fill_ of the same output bytes",
                       rows=rows), f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
