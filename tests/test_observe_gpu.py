"""Training under the LiDAR sensor model on the GPU: the fused dgppo_lidar_observe kernel against the chained launches
(lidar_scan | LidarNoise | lidar_hits | get_graph(lidar_data=), which tests/test_sensor_gpu.py pins to the oracle),
NoisyLidarRolloutEngine against SensorRolloutEngine, the algorithms' collect / update on observed graphs, train.py's
flags.

Bar: BIT-EXACT (torch.equal; NaN equal to NaN for graphs of NaN states).  Shapes: B <= 7, T = 6."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib, ops
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.trainer.rollout import NoisyLidarRolloutEngine, RolloutEngine, SensorRolloutEngine
from dgppo_fov_amd.utils.sensor import LidarNoise

from test_sensor_gpu import (FIELDS, LOOP_CASES, LOOP_IDS, T, adversarial, assert_outputs_equal, assert_same_graph,
                             dev_of, lidar_env, loop_setup, misaligned_out, outputs)

pytestmark = pytest.mark.gpu

ENVS = ["LidarSpread", "LidarTarget", "LidarBicycleTarget", "LidarOmniTarget"]
SHAPES = [(1, 1, 1), (3, 2, 8), (8, 3, 32), (3, 16, 33), (2, 3, 128)]  # (n, obs, R); top_k = min(8, R)
# the last floors most returns to 0: ties that only the stable rank resolves
MODELS = [(0.0, 0.0), (0.05, 0.0), (0.0, 0.3), (0.05, 0.3), (0.0, 1.0), (1e3, 0.0)]
B = 5


def sensor_of(env, sigma, dropout, seed):
    return LidarNoise(sigma, dropout, seed, sense_range=float(env.params["comm_radius"]))


def chain(env, state, t, sigma, dropout, seed):
    """The definition: (observed graph, the clean alpha, the sensed alpha) by the chained launches."""
    agent, goal, ob = state
    alpha = env.lidar_scan(agent, ob)
    seen = sensor_of(env, sigma, dropout, seed)(alpha, t)
    return env.get_graph(state, lidar_data=env.lidar_hits(agent, seen)), alpha, seen


def scene_of(env, key, n_env=B):
    """A reset's (agent, goal, obstacle records) with agent 0 of every env moved to 0.3 beside the centre of obstacle 0
    on the +x side: its beam along -x (ray 0 of every ray table) runs through that centre, so it has a return
    (or the agent is inside, alpha = 0) whatever the ray count."""
    s = env.reset(key=key, n_env=n_env).env_states
    agent, goal, ob = s.agent.clone(), s.goal.clone(), s.obstacle.packed.clone()
    agent[:, 0, 0] = ob[:, 0, 0] + 0.3
    agent[:, 0, 1] = ob[:, 0, 1]
    return agent, goal, ob


def hit_rows(env):
    n, k = env.num_agents, env.params["top_k_rays"]
    return slice(n + env.num_goals, n + env.num_goals + n * k)


def bites(env, state, t, sigma, dropout, seed, clean):
    """Does the chain alone, at this seed, exercise the model: noise moved a hit row, dropout dropped some returns and
    kept others."""
    g, alpha, seen = chain(env, state, t, sigma, dropout, seed)
    ok = True
    if sigma > 0:
        ok &= not torch.equal(g.states[:, hit_rows(env)], clean.states[:, hit_rows(env)])
    if 0 < dropout < 1:
        ret = alpha <= 1.0
        dropped = ret & (seen == 1e6)
        ok &= bool(dropped.any()) and bool((ret & ~dropped).any())
    return ok, g


def biting_seed(env, state, t, sigma, dropout, clean, first):
    for seed in range(first, first + 64):
        ok, g = bites(env, state, t, sigma, dropout, seed, clean)
        if ok:
            return seed, g
    raise AssertionError(f"no seed in [{first}, {first + 64}) makes the chain non-trivial at {(sigma, dropout, t)}")


# ---- 1. the kernel against the chain ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,obs,R", SHAPES, ids=[f"n{n}-o{o}-R{r}" for n, o, r in SHAPES])
@pytest.mark.parametrize("eid", ENVS)
def test_observe_equals_the_chain(cuda, eid, n, obs, R):
    env, _ = lidar_env(eid, n, obs, R, cuda)
    state = scene_of(env, 40 + R)
    clean = env.get_graph(state)
    assert bool((env.lidar_scan(state[0], state[2]) <= 1.0).any())  # the scene has returns
    for sigma, dropout in MODELS:
        for t in (0, 5):
            seed, ref = biting_seed(env, state, t, sigma, dropout, clean, first=11 + t)
            if sigma == 0 and dropout == 0:
                assert_same_graph(ref, clean, "the chain without a model is get_graph")
            for sd in (seed, torch.tensor([seed], dtype=torch.int64, device=cuda)):
                got = env.observe(state, t, sigma=sigma, dropout=dropout, seed=sd)
                assert_same_graph(got, ref, (eid, sigma, dropout, t, type(sd).__name__))
                assert torch.equal(got.node_type, ref.node_type)
    # the returned graph carries the obstacles: it steps like the true one's states would
    a = torch.rand(B, n, env.action_dim, device=cuda) * 2 - 1
    r1, r2 = env.step(clean, a), env.step(env.observe(state, 0, sigma=0.0, dropout=0.0, seed=0), a)
    assert_same_graph(r2.graph, r1.graph, "step")


def test_observe_of_lidar_line_runs_the_chain(cuda):
    """The variant env is not fused: env.observe chains the launches itself (tensor seed and env_offset included)."""
    env = make_env("LidarLine", 3, num_obs=2, device=cuda)
    state = scene_of(env, 43)
    clean = env.get_graph(state)
    for sigma, dropout in MODELS:
        seed, ref = biting_seed(env, state, 5, sigma, dropout, clean, first=3)
        for sd in (seed, torch.tensor([seed], dtype=torch.int64, device=cuda)):
            assert_same_graph(env.observe(state, 5, sigma=sigma, dropout=dropout, seed=sd), ref, (sigma, dropout))
    wide = tuple(torch.cat([x[:2], x]) for x in state)  # rows 2:7 hold the scene
    ref, _, _ = chain(env, wide, 1, 0.05, 0.3, 9)
    got = env.observe(state, 1, sigma=0.05, dropout=0.3, seed=9, env_offset=2)
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(ref, f)[2:]), f


def test_observe_on_the_adversarial_scene(cuda):
    """Agents inside obstacles, a NaN position, an agent far outside the arena, with noise and dropout on."""
    env, spec, agent, ob, (_, ref_alpha) = adversarial(cuda)
    assert np.isnan(ref_alpha).any() and (ref_alpha == 0).all(-1).any()
    dev = dev_of(cuda)
    goal = np.zeros_like(agent)
    goal[..., :2] = np.random.default_rng(3).uniform(0, spec.area, goal[..., :2].shape)
    state = (dev(agent), dev(goal), dev(ob))
    for sigma, dropout in MODELS:
        ref, alpha, seen = chain(env, state, 2, sigma, dropout, 17)
        if sigma > 0 or dropout > 0:
            assert not torch.equal(seen.nan_to_num(nan=-1.0), alpha.nan_to_num(nan=-1.0))
        assert bool(seen.isnan().any())  # NaN passes the model
        assert_same_graph(env.observe(state, 2, sigma=sigma, dropout=dropout, seed=17), ref, (sigma, dropout))


@pytest.mark.parametrize("eid", ["LidarSpread", "LidarOmniTarget"])
def test_env_offset_selects_the_noise_rows(cuda, eid):
    env, _ = lidar_env(eid, 3, 2, 32, cuda)
    state = scene_of(env, 51, n_env=3)
    wide = tuple(torch.cat([x, x[:1], x]) for x in state)  # 7 envs, rows 4:7 hold the scene
    ref, _, _ = chain(env, wide, 3, 0.05, 0.3, 23)
    got = env.observe(state, 3, sigma=0.05, dropout=0.3, seed=23, env_offset=4)
    for f in FIELDS:
        assert torch.equal(getattr(got, f), getattr(ref, f)[4:7]), f
    zero = env.observe(state, 3, sigma=0.05, dropout=0.3, seed=23)  # and the offset matters
    assert not torch.equal(zero.states, got.states)
    assert torch.equal(zero.states, ref.states[:3])


@pytest.mark.parametrize("eid,n,obs,R", [("LidarSpread", 8, 3, 32), ("LidarOmniTarget", 3, 2, 8),
                                         ("LidarBicycleTarget", 3, 16, 33)])
def test_out_may_be_misaligned_or_alias_the_state(cuda, eid, n, obs, R):
    env, _ = lidar_env(eid, n, obs, R, cuda)
    state = scene_of(env, 61)
    ref, _, _ = chain(env, state, 4, 0.05, 0.3, 5)
    kw = dict(sigma=0.05, dropout=0.3, seed=5)
    assert_same_graph(env.observe(state, 4, out=misaligned_out(env, B, cuda), **kw), ref, "4-byte aligned edges")
    # out= a graph whose own state rows are the argument
    live = env.get_graph(state)
    for f in ("nodes", "edges", "receivers", "senders"):
        getattr(live, f).fill_(-7)
    got = env.observe(live.env_states, 4, out=live, **kw)
    assert got.states.data_ptr() == live.states.data_ptr()
    assert_same_graph(got, ref, "in place")
    # a time-major buffer's strided block
    buf = env.empty_graph((2, B), cuda)
    at = env._assemble(buf.nodes[1], buf.edges[1], buf.states[1], buf.receivers[1], buf.senders[1], state[2])
    assert_same_graph(env.observe(state, 4, out=at, **kw), ref, "buffer block")


# ---- 2. the op against the raw C-ABI ------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 8, 3), ("LidarOmniTarget", 3, 2)])
def test_op_matches_c_abi_and_opcheck(cuda, eid, n, obs):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    agent, goal, ob = scene_of(env, 71)
    rays, h = env._ray_table(cuda), env._cfg_handle
    model = sensor_of(env, 0.05, 0.3, 0)
    scale, below, flags = model.sigma / model.sense_range, model._drop_below, _lib.OBSERVE_NOISE | _lib.OBSERVE_DROPOUT
    key = torch.tensor([29], dtype=torch.int64, device=cuda)
    outs = [env.empty_graph((B,), cuda) for _ in range(3)]
    o = outs[0]
    torch.ops.dgppo.lidar_observe(h, agent, goal, ob, rays, None, 29, 0, 2, scale, below, flags, o.nodes, o.edges,
                                  o.states, o.receivers, o.senders)
    o = outs[1]
    torch.ops.dgppo.lidar_observe(h, agent, goal, ob, rays, key, 0, 0, 2, scale, below, flags, o.nodes, o.edges,
                                  o.states, o.receivers, o.senders)
    o = outs[2]
    io = _lib.LidarObserveIO()
    io.agent, io.agent_stride = agent.data_ptr(), ops._stride(agent, 2)
    io.goal, io.goal_stride = goal.data_ptr(), ops._stride(goal, 2)
    io.obstacles, io.obstacles_stride = ob.data_ptr(), ops._stride(ob, 2)
    io.ray_dirs = rays.data_ptr()
    io.nodes, io.nodes_stride = o.nodes.data_ptr(), ops._stride(o.nodes, 2)
    io.edges, io.edges_stride = o.edges.data_ptr(), ops._stride(o.edges, 2)
    io.out_states, io.out_states_stride = o.states.data_ptr(), ops._stride(o.states, 2)
    io.receivers, io.senders, io.edge_index_stride = o.receivers.data_ptr(), o.senders.data_ptr(), ops._stride(o.receivers, 1)
    io.n_env, io.flags, io.env_offset, io.t = B, flags, 0, 2
    io.seed, io.seed_ptr, io.noise_scale, io.drop_below = 29, None, scale, below
    name = "dgppo_lidar_observe"
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(env.cfg), ctypes.byref(io), _lib.stream_handle(cuda)), name)
    ref, _, _ = chain(env, (agent, goal, ob), 2, 0.05, 0.3, 29)
    for got, what in zip(outs, ("op, int seed", "op, tensor seed", "raw")):
        assert_same_graph(got, ref, what)
    o = env.empty_graph((B,), cuda)
    torch.library.opcheck(torch.ops.dgppo.lidar_observe.default,
                          (h, agent, goal, ob, rays, key, 0, 0, 2, scale, below, flags, o.nodes, o.edges, o.states,
                           o.receivers, o.senders), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError, match="contiguous"):
        torch.ops.dgppo.lidar_observe(h, agent[..., ::2], goal, ob, rays, None, 29, 0, 2, scale, below, flags, o.nodes,
                                      o.edges, o.states, o.receivers, o.senders)
    # envs without a LiDAR: refused by the entry point itself, device pointers and all
    for other in (make_env("MPESpread", n, num_obs=obs, device=cuda), make_env(eid, n, num_obs=0, device=cuda)):
        assert getattr(_lib.load(), name)(ctypes.byref(other.cfg), ctypes.byref(io), _lib.stream_handle(cuda)) == \
            _lib.DGPPO_EINVAL


# ---- 3. the engine -------------------------------------------------------------------------------------------------------
def noisy_engine(cuda, case, sigma, dropout):
    env, actor, scene, _ = loop_setup(cuda, case)
    return NoisyLidarRolloutEngine(env, case[3], T, cuda, actor=actor, mode=case[4], sigma=sigma, dropout=dropout,
                                   init_state=scene)


def seen_of(eng):
    """The engine's observed graphs of steps 0..T-1, (B, T, ...) clones."""
    o = eng.observed
    return {"seen_" + f: getattr(o, f)[:, :T].clone() for f in FIELDS}


@pytest.mark.parametrize("sigma,dropout", [(0.05, 0.2), (0.0, 0.5), (1e3, 0.0)])
@pytest.mark.parametrize("case", LOOP_CASES, ids=LOOP_IDS)
def test_engine_equals_the_sensor_engine(cuda, case, sigma, dropout):
    env, actor, scene, plain = loop_setup(cuda, case)
    n = case[1]

    def definition(key):
        eng = SensorRolloutEngine(env, case[3], T, cuda, actor=actor, mode=case[4],
                                  sensor=sensor_of(env, sigma, dropout, key), init_state=scene)
        eng.run(key)
        out = outputs(eng)
        out.update({"seen_" + f: getattr(eng.observed, f).clone() for f in FIELDS})
        return out

    ref7, ref8 = definition(7), definition(8)
    assert not torch.equal(ref7["seen_states"], ref8["seen_states"])  # the key seeds the noise
    rows = hit_rows(env)  # and the model bites: the hit rows seen differ from the same run's true ones
    assert not torch.equal(ref7["seen_states"][:, :, rows], ref7["states"][:T].transpose(0, 1)[:, :, rows])
    eager = noisy_engine(cuda, case, sigma, dropout)
    roll = eager.run(7)
    got = dict(outputs(eager), **seen_of(eager))
    assert_outputs_equal(got, ref7, "eager")
    for f in FIELDS:  # run returns the TRUE rollout
        assert torch.equal(getattr(roll.graph, f), ref7[f][:T].transpose(0, 1)), f
    # obs[T]: the chain on the final true state
    s = eager.buf.states[T]
    last, _, _ = chain(env, (s[:, :n], s[:, n:n + env.num_goals], scene[2]), T, sigma, dropout, 7)
    for f in FIELDS:
        assert torch.equal(getattr(eager.observed, f)[:, T], getattr(last, f)), f
    # observed_rollout: the observed graphs around the true run
    obs = eager.observed_rollout()
    for f in FIELDS:
        assert torch.equal(getattr(obs.graph, f), ref7["seen_" + f]), f
        assert torch.equal(getattr(obs.next_graph, f)[:, :-1], ref7["seen_" + f][:, 1:]), f
        assert torch.equal(getattr(obs.next_graph, f)[:, -1], getattr(last, f)), f
        assert getattr(obs.graph, f).transpose(0, 1).is_contiguous()  # the update reads them in place
    assert torch.equal(obs.rewards, roll.rewards) and torch.equal(obs.costs, roll.costs)
    assert torch.equal(obs.actions, roll.actions) and torch.equal(obs.rnn_states, roll.rnn_states)
    assert type(obs)._fields == type(roll)._fields
    # captured: one hipGraph, a replay with a new key draws new noise
    cap = noisy_engine(cuda, case, sigma, dropout).capture()
    for key, ref in ((7, ref7), (8, ref8)):
        cap.run(key)
        assert_outputs_equal(dict(outputs(cap), **seen_of(cap)), ref, f"captured, key {key}")
    # the truth depends on the observation through the actions only
    replay = RolloutEngine(env, case[3], T, cuda, init_state=scene)
    replay.actions.copy_(cap.actions)
    replay.run(0)
    assert_outputs_equal(outputs(replay), ref8, "replayed actions", FIELDS + ("rewards", "costs"))


@pytest.mark.parametrize("case", LOOP_CASES, ids=LOOP_IDS)
def test_perfect_sensor_is_the_plain_engine(cuda, case):
    env, actor, scene, plain = loop_setup(cuda, case)
    for eng in (noisy_engine(cuda, case, 0.0, 0.0), noisy_engine(cuda, case, 0.0, 0.0).capture()):
        eng.run(7)
        assert_outputs_equal(outputs(eng), plain, "perfect sensor")
        for f in FIELDS:
            assert torch.equal(getattr(eng.obs, f), plain[f]), f  # all T + 1 observed graphs are the true ones


# ---- 4. training ------------------------------------------------------------------------------------------------------
TB = 4


def train_setup(cuda, algo="dgppo", eid="LidarSpread", **flags):
    env = make_env(eid, 3, num_obs=2, max_step=T, device=cuda)
    return env, make_algo(algo, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                          action_dim=env.action_dim, n_agents=3, batch_size=TB * T, rnn_step=3, seed=2, device=cuda,
                          **flags)


def params_of(algo):
    return {k: v.clone() for k, v in algo.params.items()}


def test_perfect_sensor_trains_like_the_plain_algorithm(cuda):
    _, plain = train_setup(cuda)
    _, sensed = train_setup(cuda, lidar_noise=0.0, lidar_dropout=0.0)
    assert plain.sensor is None and sensed.sensor == (0.0, 0.0)
    for step, key in enumerate((5, 6)):
        for algo in (plain, sensed):
            algo.update(algo.collect(algo.params, key, n_env=TB), step)
    assert isinstance(sensed._engine(TB, RolloutEngine.MODE_SAMPLE), NoisyLidarRolloutEngine)
    assert not isinstance(plain._engine(TB, RolloutEngine.MODE_SAMPLE), NoisyLidarRolloutEngine)
    for k, v in plain.params.items():
        assert torch.equal(v, sensed.params[k]), k


@pytest.mark.parametrize("algo_name,eid", [("dgppo", "LidarSpread"), ("dgppo", "LidarOmniTarget"),
                                           ("informarl", "LidarSpread")])
def test_training_on_observed_graphs(cuda, algo_name, eid):
    env, algo = train_setup(cuda, algo_name, eid, lidar_noise=0.05, lidar_dropout=0.2)
    before = params_of(algo)
    roll = algo.collect(algo.params, 5, n_env=TB)
    eng = algo._engine(TB, RolloutEngine.MODE_SAMPLE)
    true = eng.rollout()
    rows = hit_rows(env)
    assert not torch.equal(roll.graph.states[:, :, rows], true.graph.states[:, :, rows])
    assert not torch.equal(roll.next_graph.states[:, -1, rows], true.next_graph.states[:, -1, rows])
    n = env.num_agents  # the agents' and goals' rows are the true ones
    assert torch.equal(roll.graph.states[:, :, :n + env.num_goals], true.graph.states[:, :, :n + env.num_goals])
    # rewards and costs: the true ones of the definition's run on the same key
    ref = SensorRolloutEngine(env, TB, T, cuda, actor=algo.actor, mode=RolloutEngine.MODE_SAMPLE,
                              sensor=sensor_of(env, 0.05, 0.2, 5)).run(5)
    assert torch.equal(roll.rewards, ref.rewards) and torch.equal(roll.costs, ref.costs)
    assert torch.equal(roll.actions, ref.actions) and roll.costs.shape[-1] == env.n_cost
    info = algo.update(roll, 0)
    assert info and all(bool(torch.as_tensor(v).double().isfinite().all()) for v in info.values()), info
    for k in algo.NETS:  # every net the algorithm trains moved
        assert bool(torch.isfinite(algo.params[k]).all()) and not torch.equal(algo.params[k], before[k]), k
    if algo_name == "dgppo":  # the det rollout inside update ran under the sensor too
        det = algo._engine(TB, RolloutEngine.MODE_DET)
        assert isinstance(det, NoisyLidarRolloutEngine)
        assert not torch.equal(det.obs.states[:, :, rows], det.buf.states[:, :, rows])


def test_hcbfcrpo_refuses_the_sensor(cuda):
    with pytest.raises(ValueError, match="get_cost"):
        train_setup(cuda, "hcbfcrpo", lidar_noise=0.05)
    _, algo = train_setup(cuda, "hcbfcrpo")  # and is untouched without the flags
    assert algo.sensor is None


# ---- 5. train.py --------------------------------------------------------------------------------------------------------
def test_cli_trains_under_the_sensor_flags(cuda, tmp_path, monkeypatch, capsys):
    import yaml
    from test_train_gpu import _entry

    test_py, train_py = _entry("test"), _entry("train")
    eid = "LidarSpread"
    argv = ["train.py", "--env", eid, "-n", "3", "--algo", "dgppo", "--obs", "2", "--steps", "2", "--n-env-train", "8",
            "--batch-size", "256", "--n-env-test", "4", "--eval-interval", "1", "--save-interval", "2", "--log-dir",
            str(tmp_path), "--lidar-noise", "0.05", "--lidar-dropout", "0.2"]
    monkeypatch.setattr(sys, "argv", argv)
    train_py.main()
    (run,) = glob.glob(os.path.join(str(tmp_path), eid, "dgppo", "seed0_*"))
    with open(os.path.join(run, "config.yaml")) as f:
        cfg = {}
        for d in yaml.safe_load_all(f):
            cfg.update(d or {})
    assert cfg["lidar_noise"] == 0.05 and cfg["lidar_dropout"] == 0.2
    capsys.readouterr()
    # test.py keeps its meaning: a perfect sensor unless its own flags say otherwise
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", run, "--epi", "4", "--max-step", "6"])
    res = test_py.main()
    out = capsys.readouterr().out
    assert set(res) == {"reward", "cost", "safe_rate"} and all(np.isfinite(v) for v in res.values())
    assert "lidar noise" not in out and out.count("epi: ") == 4
