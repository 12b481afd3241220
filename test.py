"""Evaluation of a trained checkpoint with the reference's CLI (test.py:22-193 of Tw6249/dgppo_fov):
episode return, max cost and safe rate (1 - mean over agents of max over t of any(cost >= 0),
test.py:100-139), optionally on a different agent / obstacle count or env than training
(-n, --obs, --env), appending `test_log.csv` with --log in the reference's column order
(test.py:142-146).

Episodes are environments: episode i is env i of ONE batched rollout (Philox keyed (--seed, i)),
so `--epi 1000` is a single hipGraph replay over 1000 envs; `--offset k` skips the first k
episodes, as the reference's `test_keys[offset:]` does.  --cpu / --debug are accepted and ignored (there is no CPU
path).

Videos are opt-in: `--video` renders the first `--max-videos` (default 5) evaluated episodes with env.render_video
(frames rasterised on the GPU, header text and GIF encoding by Pillow on the host, --dpi honoured: the scene is
10 * dpi pixels square) to `<path>/videos/<step>/<stamp>_n{n}_epi{ii:02}_reward..._cost..._sr....gif`, the reference's
names with .gif for .mp4 (no ffmpeg).  The reference renders every episode unless --no-video is given; here the
default is no video, so a 1000-episode evaluation does not encode 1000 GIFs, and --no-video stays accepted (it wins
over --video).  The metric lines are the same with and without --video.

`--cbf AGENT` (with --video) draws the learned safety value under each rendered episode: h = -max over the cost
components of Vh, had agent AGENT stood at each node of a `--cbf-grid` G x G grid (default 32) with everything else
and the carry fixed (utils/field.py value_field).  Red is predicted unsafe, blue safe, the black line the boundary of
the learned safe set.  It needs an algorithm with get_Vh (dgppo, hcbfcrpo).  The VMAS envs render through the same
--video path (their own pictures: env/vmas render_frames); --cbf is refused for them, since they have no get_graph of
given states to sweep.

Beyond the reference: `--scene PATH` evaluates on the initial states stored in a scene file
(dgppo_fov_amd/utils/scene.py) instead of seeds -- episodes are rows [offset:epi] of the file, all of its rows when
--epi is not given -- and `--dump-scene PATH` writes the initial states of the episodes that ran, so
`--dump-scene s.npz` then `--scene s.npz` replays the same episodes (deterministic policy: the same numbers).

`--lidar-noise SIGMA` / `--lidar-dropout P` (Lidar envs with obstacles) put a sensor model between the world and the
policy (trainer/rollout.py SensorRolloutEngine, utils/sensor.py LidarNoise seeded from --seed): the policy sees LiDAR
ranges with Gaussian noise of std SIGMA world units and beams dropped with probability P, while the env steps, the
rewards and the costs stay the true ones.  Either flag routes the evaluation through that loop; the summary line then
names both values.  `--lidar-occlusion` (same envs, with or without the noise flags, no config.yaml entry needed) also
drops every agent-agent edge whose receiver has no line of sight to its sender past the obstacles from the graphs the
policy sees (env.line_of_sight, utils/sensor.py mask_unseen).  `--lidar-fov DEG` (LidarBicycleTarget and
LidarOmniTarget, no config.yaml entry needed, combines with the other three) drops every agent-agent edge whose sender is
outside the receiver's forward cone of half angle DEG (env.field_of_view).  `--lidar-bodies` (Lidar envs with
obstacles, no config.yaml entry needed, combines with the other four) lets the beams return off the other agents'
bodies as well (env.lidar_scan(bodies=True)): a robot whose edge is hidden still shows up as an anonymous hit row."""
import argparse
import os

import numpy as np
import yaml


def _config(path):
    with open(os.path.join(path, "config.yaml")) as f:
        cfg = {}
        for d in yaml.safe_load_all(f):  # train.py dumps vars(args) then algo.config
            cfg.update(d or {})
    return cfg


def test(args):
    print(f"> Running test.py {args}")
    import torch

    from dgppo_fov_amd.algo import make_algo
    from dgppo_fov_amd.env import make_env
    from dgppo_fov_amd.trainer.rollout import RolloutEngine

    np.random.seed(args.seed)
    cfg = _config(args.path)
    env_id = cfg["env"] if args.env is None else args.env
    if args.cbf is not None and args.video and not args.no_video and str(env_id).startswith("VMAS"):
        # refused before anything is loaded or run
        raise SystemExit(f"--cbf is not built for {env_id}: the VMAS envs have no get_graph of given states, so the "
                         "value sweep that draws the field cannot be run")
    dev = torch.device("cuda", 0)
    num_agents = cfg["num_agents"] if args.num_agents is None else args.num_agents
    env = make_env(env_id=env_id, num_agents=num_agents,
                   num_obs=cfg["obs"] if args.obs is None else args.obs, n_rays=cfg.get("n_rays", 32),
                   max_step=args.max_step, full_observation=args.full_observation, device=dev)
    algo = make_algo(cfg["algo"], env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=env.num_agents, cost_weight=cfg.get("cost_weight", 0.0),
                     actor_gnn_layers=cfg["actor_gnn_layers"], Vl_gnn_layers=cfg["Vl_gnn_layers"],
                     Vh_gnn_layers=cfg.get("Vh_gnn_layers", 1), lr_actor=cfg["lr_actor"], lr_Vl=cfg["lr_Vl"],
                     max_grad_norm=2.0, seed=cfg["seed"], use_rnn=cfg.get("use_rnn", True),
                     rnn_layers=cfg.get("rnn_layers", 1), use_lstm=cfg.get("use_lstm", False),
                     batch_size=cfg.get("batch_size", 16384), rnn_step=cfg.get("rnn_step", 16), device=dev)
    sensed = (args.lidar_noise is not None or args.lidar_dropout is not None or args.lidar_occlusion
              or args.lidar_fov is not None)
    if sensed:  # refused before anything is loaded or run
        from dgppo_fov_amd.utils.sensor import Sensing

        sigma, drop = args.lidar_noise or 0.0, args.lidar_dropout or 0.0
        try:
            sensing = Sensing.of(env, "--lidar-noise / --lidar-dropout / --lidar-occlusion / --lidar-fov", sigma, drop,
                                 args.lidar_occlusion, args.lidar_fov)
        except (ValueError, NotImplementedError) as e:
            raise SystemExit(str(e))
    else:
        sensing = None
    if args.lidar_bodies:  # likewise
        from dgppo_fov_amd.utils.sensor import bodies_option

        try:
            bodies_option(env, "--lidar-bodies", True)
        except (ValueError, NotImplementedError) as e:
            raise SystemExit(str(e))
    if args.cbf is not None and args.video and not args.no_video:  # refused before anything is loaded or run
        if not callable(getattr(algo, "get_Vh", None)):
            raise SystemExit(f"--cbf needs an algorithm with get_Vh; {cfg['algo']} has none")
        if not 0 <= args.cbf < env.num_agents:
            raise SystemExit(f"--cbf {args.cbf} is not an agent index in [0, {env.num_agents})")
        if args.cbf_grid < 2:
            raise SystemExit(f"--cbf-grid {args.cbf_grid} < 2")
    model_path = os.path.join(args.path, "models")
    step = args.step if args.step is not None else max(int(d) for d in os.listdir(model_path) if d.isdigit())
    print("step: ", step)
    algo.load(model_path, step)  # the networks are agent-count agnostic: -n may differ from training

    scene = None
    if args.scene is not None:
        from dgppo_fov_amd.utils.scene import load_scene

        scene = load_scene(args.scene, env, dev)
        rows = int(scene[0].shape[0])
        if args.epi is None:
            args.epi = rows
        if rows < args.epi:
            raise SystemExit(f"--scene {args.scene} holds {rows} episodes, fewer than --epi {args.epi}")
    elif args.epi is None:
        args.epi = 5
    episodes = list(range(args.offset, args.epi))
    if not episodes:
        raise SystemExit(f"--offset {args.offset} leaves no episodes of --epi {args.epi}")
    mode = RolloutEngine.MODE_SAMPLE if args.stochastic else RolloutEngine.MODE_DET
    init_state = None
    if scene is not None:  # episodes are rows [offset:epi] of the file
        cut = lambda t: None if t is None else t[args.offset:args.epi]  # noqa: E731
        init_state = type(scene)(*(cut(part) for part in scene))
    if sensed or args.lidar_bodies:
        from dgppo_fov_amd.trainer.rollout import SensorRolloutEngine

        sensor = sensing.model(float(env.params["comm_radius"]), seed=args.seed) if sensing is not None else None
        eng = SensorRolloutEngine(env, len(episodes), env.max_episode_steps, dev, env_offset=args.offset,
                                  actor=algo.actor, mode=mode, sensor=sensor, init_state=init_state, sensing=sensing,
                                  bodies=args.lidar_bodies)
    else:
        eng = RolloutEngine(env, len(episodes), env.max_episode_steps, dev, env_offset=args.offset, actor=algo.actor,
                            mode=mode, init_state=init_state)
    roll = eng.run(args.seed)
    if args.dump_scene is not None:
        from dgppo_fov_amd.utils.scene import save_scene

        save_scene(args.dump_scene, env, eng.graph_at(0).env_states)
    rewards = roll.rewards.sum(1).double().cpu().numpy()  # (epi,)
    costs = roll.costs.amax(dim=(1, 2, 3)).double().cpu().numpy()
    # unsafe_mask on the pre-step graphs: the stored costs ARE env.get_cost(rollout.graph)
    is_unsafe = (roll.costs >= 0.0).any(dim=-1).amax(dim=1).cpu().numpy()  # (epi, n)
    for k, i in enumerate(episodes):
        rate = 1 - is_unsafe[k].mean()
        print(f"epi: {i}, reward: {rewards[k]:.3f}, cost: {costs[k]:.3f}, safe rate: {rate * 100:.3f}%")
    safe_mean, safe_std = (1 - is_unsafe).mean(), (1 - is_unsafe).std()
    print(f"reward: {np.mean(rewards):.3f}, min/max reward: {np.min(rewards):.3f}/{np.max(rewards):.3f}, "
          f"cost: {np.mean(costs):.3f}, min/max cost: {np.min(costs):.3f}/{np.max(costs):.3f}, "
          f"safe_rate: {safe_mean * 100:.3f}%" + (f", lidar noise: {sigma:g}, lidar dropout: {drop:g}" if sensed else "") +
          (", lidar occlusion: on" if args.lidar_occlusion else "") +
          (f", lidar fov: {args.lidar_fov:g}" if args.lidar_fov is not None else "") +
          (", lidar bodies: on" if args.lidar_bodies else ""))
    if args.log:
        with open(os.path.join(args.path, "test_log.csv"), "a") as f:
            f.write(f"{env.num_agents},{args.epi},{env.max_episode_steps},{env.area_size},{env.params['n_obs']},"
                    f"{safe_mean * 100:.3f},{safe_std * 100:.3f}\n")
    if args.video and not args.no_video:  # test.py:148-159 of the reference, opt-in and capped here
        import datetime

        stamp = datetime.datetime.now().strftime("%m%d-%H%M")
        videos_dir = os.path.join(args.path, "videos", f"{step}")
        os.makedirs(videos_dir, exist_ok=True)
        Ta_is_unsafe = (roll.costs >= 0.0).any(dim=-1)  # (epi, T, n)
        for k, i in list(enumerate(episodes))[:max(args.max_videos, 0)]:
            rate = (1 - is_unsafe[k].mean()) * 100
            name = f"n{num_agents}_epi{i:02}_reward{rewards[k]:.3f}_cost{costs[k]:.3f}_sr{rate:.0f}"
            viz_opts = {}
            if args.cbf is not None:
                from dgppo_fov_amd.utils.field import FieldLayer, grid_axes, value_field

                xs, ys = grid_axes(env, args.cbf_grid)
                h = -value_field(algo, roll, k, args.cbf, xs, ys).amax(dim=-1)  # (T, G, G)
                viz_opts["field"] = FieldLayer.centred(h.contiguous(), xs, ys, f"h = -max Vh, agent {args.cbf}")
            env.render_video(roll, os.path.join(videos_dir, f"{stamp}_{name}.gif"), Ta_is_unsafe[k], viz_opts,
                             dpi=args.dpi, episode=k)
    return dict(reward=float(np.mean(rewards)), cost=float(np.mean(costs)), safe_rate=float(safe_mean))


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument("--path", type=str, required=True)
    parser.add_argument("--no-video", action="store_true", default=False)
    parser.add_argument("--video", action="store_true", default=False)  # opt-in (the reference: on unless --no-video)
    parser.add_argument("--max-videos", type=int, default=5)
    parser.add_argument("--epi", type=int, default=None)  # 5 without --scene, every row of the file with it
    parser.add_argument("--scene", type=str, default=None)
    parser.add_argument("--dump-scene", type=str, default=None)
    parser.add_argument("--step", type=int, default=None)
    parser.add_argument("--obs", type=int, default=None)
    parser.add_argument("--stochastic", action="store_true", default=False)
    parser.add_argument("--full-observation", action="store_true", default=False)
    parser.add_argument("--debug", action="store_true", default=False)
    parser.add_argument("--cpu", action="store_true", default=False)
    parser.add_argument("--max-step", type=int, default=None)
    parser.add_argument("--log", action="store_true", default=False)
    parser.add_argument("-n", "--num-agents", type=int, default=None)
    parser.add_argument("--seed", type=int, default=1234)
    parser.add_argument("--env", type=str, default=None)
    parser.add_argument("--offset", type=int, default=0)
    parser.add_argument("--dpi", type=int, default=100)
    parser.add_argument("--cbf", type=int, default=None, metavar="AGENT")  # with --video: the Vh field of this agent
    parser.add_argument("--cbf-grid", type=int, default=32, metavar="G")
    # sensor in the loop (Lidar envs): range noise std in world units, per-beam dropout probability
    parser.add_argument("--lidar-noise", type=float, default=None, metavar="SIGMA")
    parser.add_argument("--lidar-dropout", type=float, default=None, metavar="P")
    parser.add_argument("--lidar-occlusion", action="store_true", default=False)  # obstacles hide agents from each other
    parser.add_argument("--lidar-fov", type=float, default=None, metavar="DEG")  # half angle of the camera cone
    parser.add_argument("--lidar-bodies", action="store_true", default=False)  # beams return off the other agents too
    return parser


def main():
    return test(build_parser().parse_args())


if __name__ == "__main__":
    main()
