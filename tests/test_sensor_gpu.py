"""Sensor in the loop on the GPU: dgppo_lidar_scan, dgppo_lidar_hits and dgppo_env_get_graph_hits against the NumPy
oracle, the ops against the raw C-ABI, SensorRolloutEngine against the plain engine, LidarNoise, and test.py's flags.

Bar: BIT-EXACT (NaN equal to NaN), as everywhere in the env tests.  Shapes: B <= 24, T <= 6."""
import ctypes
import glob
import os
import sys

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib, ops
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import ENV, make_env
from dgppo_fov_amd.trainer.rollout import RolloutEngine, SensorRolloutEngine
from dgppo_fov_amd.utils.sensor import LidarNoise
from oracle import env as O

from env_cases import _np, adversarial_lidar_scene, assert_graph_equal
from sensor_ref import hits_ref, hand_made_alpha

pytestmark = pytest.mark.gpu

F = np.float32
FIELDS = ("nodes", "edges", "states", "receivers", "senders")
LIDAR_CONFIGS = [("LidarSpread", 8, 3), ("LidarTarget", 5, 1), ("LidarBicycleTarget", 8, 3), ("LidarOmniTarget", 8, 3),
                 ("LidarOmniTarget", 3, 2), ("LidarLine", 3, 2), ("LidarSpread", 1, 3)]
LIDAR_IDS = [f"{e}-n{n}-o{o}" for e, n, o in LIDAR_CONFIGS]


def lidar_env(eid, n, obs, R, dev):
    """(env, oracle spec) at R rays, top_k = min(8, R)."""
    k = min(8, R)
    params = dict(ENV[eid].PARAMS, n_obs=obs, n_rays=R, top_k_rays=k)
    return ENV[eid](num_agents=n, params=params, device=dev), O.Spec(eid, n, obs, n_rays=R, top_k=k)


def oracle_lidar(spec, agent, ob):
    with np.errstate(all="ignore"):
        return O.lidar(np.ascontiguousarray(agent[..., :2]), ob, O.ray_table(spec.n_rays, spec.comm_r), spec.top_k)


def assert_same_graph(a, b, what=""):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        assert x.shape == y.shape, (what, f)
        same = (x == y) | ((x != x) & (y != y))
        assert bool(same.all()), (what, f, int((~same).sum()))


def dev_of(cuda):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- 1. scan and hits against the oracle -------------------------------------------------------------------------
_SCENES = {}


def reset_scene(cuda, n, obs, R):
    """A reset's agents and obstacles on the device with the oracle's (hits, alpha), computed once per shape."""
    key = (n, obs, R)
    if key not in _SCENES:
        env, spec = lidar_env("LidarSpread", n, obs, R, cuda)
        ag, _, ob = O.env_reset(spec, 100 + R, 5)  # the oracle's reset: the scene does not depend on a GPU kernel
        dev = dev_of(cuda)
        _SCENES[key] = (env, spec, dev(ag), dev(ob), oracle_lidar(spec, ag, ob))
    return _SCENES[key]


@pytest.mark.parametrize("R", [1, 8, 32, 33, 128])
@pytest.mark.parametrize("n,obs", [(n, o) for n in (1, 3, 8) for o in (1, 3, 16)])
def test_scan_and_hits_match_oracle_on_reset_scenes(cuda, n, obs, R):
    env, spec, agent, ob, (ref_hits, ref_alpha) = reset_scene(cuda, n, obs, R)
    alpha = env.lidar_scan(agent, ob)
    assert alpha.shape == (5, n, R) and alpha.dtype == torch.float32
    np.testing.assert_array_equal(_np(alpha), ref_alpha)
    # fed the oracle's own alpha
    hits = env.lidar_hits(agent, torch.from_numpy(ref_alpha).to(cuda))
    assert hits.shape == (5, n, spec.top_k, 2)
    np.testing.assert_array_equal(_np(hits), ref_hits)


def adversarial(cuda):
    """adversarial_lidar_scene at n = 8, O = 3, B = 24 plus a NaN agent position (env 6) and an agent outside
    [-2, 2]^2 (env 7); with the oracle's (hits, alpha)."""
    if "adv" not in _SCENES:
        env, spec = lidar_env("LidarSpread", 8, 3, 32, cuda)
        ag, gl, ob = O.env_reset(spec, 12, 24)
        states, ob, _ = adversarial_lidar_scene(spec, np.concatenate([ag, gl], 1), ob, seed=5)
        agent = states[:, :8].copy()
        agent[6, 0, 0] = np.nan
        agent[7, 1, :2] = (2.5, -3.0)
        _SCENES["adv"] = (env, spec, agent, ob, oracle_lidar(spec, agent, ob))
    return _SCENES["adv"]


def test_scan_and_hits_match_oracle_on_adversarial_scene(cuda):
    env, spec, agent, ob, (ref_hits, ref_alpha) = adversarial(cuda)
    dev = dev_of(cuda)
    assert np.isnan(ref_alpha).any() and (ref_alpha == 0).all(-1).any() and (ref_alpha == F(1e6)).any()  # the scene bites
    alpha = env.lidar_scan(dev(agent), dev(ob))
    np.testing.assert_array_equal(_np(alpha), ref_alpha)
    np.testing.assert_array_equal(_np(env.lidar_hits(dev(agent), dev(ref_alpha))), ref_hits)
    # and the two kernels chained are the culling kernels of get_graph (the wave kernel at this shape)
    hits = env.lidar_hits(dev(agent), alpha)
    np.testing.assert_array_equal(_np(hits), ref_hits)


@pytest.mark.parametrize("R", [32, 8, 33, 128])
def test_hits_of_hand_made_alphas(cuda, R):
    """Rows the ray cast never produces, against the NumPy restatement (tests/sensor_ref.py); R = 8 is k == R."""
    env, spec = lidar_env("LidarTarget", 3, 2, R, cuda)
    alpha = hand_made_alpha(R, 3, seed=R)
    B = alpha.shape[0]
    agent = np.random.default_rng(1).uniform(-0.5, 2.0, (B, 3, 4)).astype(F)
    ref = hits_ref(agent, alpha, O.ray_table(R, spec.comm_r), spec.top_k)
    dev = dev_of(cuda)
    got = env.lidar_hits(dev(agent), dev(alpha))
    np.testing.assert_array_equal(_np(got), ref)
    # a (B, n, R) view with a free per-env stride is read in place
    wide = torch.zeros(B, 5, R, device=cuda)
    wide[:, :3] = dev(alpha)
    np.testing.assert_array_equal(_np(env.lidar_hits(dev(agent), wide[:, :3])), ref)


@pytest.mark.parametrize("eid,n,obs", LIDAR_CONFIGS, ids=LIDAR_IDS)
def test_hits_of_scan_equal_get_lidar_data(cuda, eid, n, obs):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    g = env.reset(key=21, n_env=5)
    for t in range(2):
        s = g.env_states
        ref = env.get_lidar_data(s.agent, s.obstacle)
        got = env.lidar_hits(s.agent, env.lidar_scan(s.agent, s.obstacle))
        assert got.shape == ref.shape and torch.equal(got, ref), (eid, t)
        g = env.step(g, torch.rand(5, n, env.action_dim, device=cuda) * 2 - 1).graph


# ---- 2. graph from hits ------------------------------------------------------------------------------------------
def hand_made_hits(spec, agent, seed):
    """(B, n, k, 2): random points, one env at 1e6 scale, a NaN, and for each agent of env 2 points exactly at
    comm_radius and comm_radius - 0.1 from it along +x and +y (the two mask edges)."""
    rng = np.random.default_rng(seed)
    B, n, k = agent.shape[0], spec.n, spec.top_k
    H = rng.uniform(-0.5, 2.0, (B, n, k, 2)).astype(F)
    H[:, :, 0] = agent[:, :, :2] + rng.uniform(-0.3, 0.3, (B, n, 2)).astype(F)  # some inside the mask
    H[1] = (rng.uniform(-1, 1, (n, k, 2)) * 1e6).astype(F)
    H[3, 0, 1, 0] = np.nan
    r = F(spec.comm_r)
    for i in range(n):
        p = agent[2, i, :2]
        H[2, i, 0] = p + np.array([r, 0], F)
        H[2, i, 1] = p + np.array([0, r - F(0.1)], F)
        H[2, i, 2] = p - np.array([F(spec.comm_r - 0.1), 0], F)
        H[2, i, 3] = p - np.array([0, r], F)
    return H


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("eid", ["LidarSpread", "LidarTarget", "LidarBicycleTarget", "LidarOmniTarget"])
def test_graph_from_hits_matches_oracle(cuda, eid, n):
    env = make_env(eid, n, num_obs=2, device=cuda)
    spec = O.Spec(eid, n, 2)
    B = 5
    rng = np.random.default_rng(n)
    agent = rng.uniform(-1.5, 1.5, (B, n, spec.sd)).astype(F)
    agent[..., :2] = rng.uniform(-0.3, spec.area + 0.3, (B, n, 2)).astype(F)
    goal = np.zeros((B, spec.ng, spec.sd), F)
    goal[..., :2] = rng.uniform(0.0, spec.area, (B, spec.ng, 2)).astype(F)
    H = hand_made_hits(spec, agent, seed=7)
    dev = dev_of(cuda)
    g = env.get_graph((dev(agent), dev(goal), None), lidar_data=dev(H))
    with np.errstate(all="ignore"):
        ref = O.build_graph(spec, agent, goal, H)
    assert_graph_equal(g, ref, f"{eid} n={n}")
    np.testing.assert_array_equal(_np(g.node_type[0]), O.node_type(spec))
    assert g.env_states.obstacle is None
    # both sides of the mask occur among the agent-hit edges
    hit_recv = ref["receivers"][:, spec.n * spec.n + spec.n_ag:]
    assert (hit_recv == spec.n_nodes - 1).any() and (hit_recv != spec.n_nodes - 1).any()


def misaligned_out(env, B, dev):
    g = env.empty_graph((B,), dev)
    raw = torch.empty(g.edges.numel() + 1, device=dev)
    edges = raw[1:].view(g.edges.shape)
    assert edges.data_ptr() % 8 == 4
    return env._assemble(g.nodes, edges, g.states, g.receivers, g.senders, None)


@pytest.mark.parametrize("eid,n,obs", LIDAR_CONFIGS, ids=LIDAR_IDS)
def test_round_trip_through_lidar_data(cuda, eid, n, obs):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    B = 5
    g = env.reset(key=31, n_env=B)
    s = g.env_states
    H = env.get_lidar_data(s.agent, s.obstacle).contiguous()
    g2 = env.get_graph(s, lidar_data=H)
    assert_same_graph(g2, g, "lidar_data round trip")
    assert torch.equal(g2.node_type, g.node_type)
    assert_same_graph(env.get_graph(s, out=misaligned_out(env, B, cuda), lidar_data=H), g, "4-byte aligned edges")
    # out= the graph whose own env_states are the argument
    live = env.reset(key=31, n_env=B)
    for f in ("nodes", "edges", "receivers", "senders"):
        getattr(live, f).fill_(-7)
    g3 = env.get_graph(live.env_states, out=live, lidar_data=H)
    assert g3.states.data_ptr() == live.states.data_ptr()
    assert_same_graph(g3, g, "in place")
    # with the obstacles in the state the graph steps like the plain one; without them step refuses
    a = torch.rand(B, n, env.action_dim, device=cuda) * 2 - 1
    r1, r2 = env.step(g, a), env.step(g2, a)
    assert_same_graph(r2.graph, r1.graph, "step")
    assert torch.equal(r1.reward, r2.reward) and torch.equal(r1.cost, r2.cost)
    blind = env.get_graph((s.agent, s.goal, None), lidar_data=H)
    assert_same_graph(blind, g, "sensor only")
    with pytest.raises(ValueError, match="carries no obstacles"):
        env.step(blind, a)
    with pytest.raises(ValueError, match="lidar_data is on"):
        env.get_graph(s, lidar_data=H.cpu())


# ---- 3. the ops against the raw C-ABI ---------------------------------------------------------------------------
def _raw(env, name, io):
    _lib.check(getattr(_lib.load(), name)(ctypes.byref(env.cfg), ctypes.byref(io), _lib.stream_handle(env.device)), name)


@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 8, 3), ("LidarOmniTarget", 3, 2), ("LidarLine", 3, 2)])
def test_ops_match_c_abi_and_opcheck(cuda, eid, n, obs):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    B, R, k = 5, env.params["n_rays"], env.params["top_k_rays"]
    g = env.reset(key=61, n_env=B)
    s = g.env_states
    agent, goal, ob, rays = s.agent, s.goal, s.obstacle.packed, env._ray_table(cuda)
    h = env._cfg_handle
    checks = ("test_schema", "test_faketensor")
    # lidar_scan
    a_op, a_raw = torch.empty(B, n, R, device=cuda), torch.empty(B, n, R, device=cuda)
    torch.ops.dgppo.lidar_scan(h, agent, ob, rays, a_op)
    io = _lib.LidarScanIO()
    io.agent, io.agent_stride = agent.data_ptr(), ops._stride(agent, 2)
    io.obstacles, io.obstacles_stride = ob.data_ptr(), ops._stride(ob, 2)
    io.ray_dirs, io.alpha, io.alpha_stride, io.n_env = rays.data_ptr(), a_raw.data_ptr(), n * R, B
    _raw(env, "dgppo_lidar_scan", io)
    assert torch.equal(a_op, a_raw) and torch.equal(a_op, env.lidar_scan(agent, ob))
    torch.library.opcheck(torch.ops.dgppo.lidar_scan.default, (h, agent, ob, rays, torch.empty_like(a_op)),
                          test_utils=checks)
    # lidar_hits
    h_op, h_raw = torch.empty(B, n, k, 2, device=cuda), torch.empty(B, n, k, 2, device=cuda)
    torch.ops.dgppo.lidar_hits(h, agent, a_op, rays, h_op)
    io = _lib.LidarHitsIO()
    io.agent, io.agent_stride = agent.data_ptr(), ops._stride(agent, 2)
    io.alpha, io.alpha_stride = a_op.data_ptr(), n * R
    io.ray_dirs, io.hits, io.hits_stride, io.n_env = rays.data_ptr(), h_raw.data_ptr(), n * k * 2, B
    _raw(env, "dgppo_lidar_hits", io)
    assert torch.equal(h_op, h_raw) and torch.equal(h_op, env.get_lidar_data(agent, s.obstacle))
    torch.library.opcheck(torch.ops.dgppo.lidar_hits.default, (h, agent, a_op, rays, torch.empty_like(h_op)),
                          test_utils=checks)
    # env_get_graph_hits
    outs = [env.empty_graph((B,), cuda) for _ in range(2)]
    o = outs[0]
    torch.ops.dgppo.env_get_graph_hits(h, agent, goal, h_op, o.nodes, o.edges, o.states, o.receivers, o.senders)
    o = outs[1]
    io = _lib.EnvGraphHitsIO()
    io.agent, io.agent_stride = agent.data_ptr(), ops._stride(agent, 2)
    io.goal, io.goal_stride = goal.data_ptr(), ops._stride(goal, 2)
    io.hits, io.hits_stride = h_op.data_ptr(), n * k * 2
    io.nodes, io.nodes_stride = o.nodes.data_ptr(), ops._stride(o.nodes, 2)
    io.edges, io.edges_stride = o.edges.data_ptr(), ops._stride(o.edges, 2)
    io.out_states, io.out_states_stride = o.states.data_ptr(), ops._stride(o.states, 2)
    io.receivers, io.senders, io.edge_index_stride = o.receivers.data_ptr(), o.senders.data_ptr(), ops._stride(o.receivers, 1)
    io.n_env = B
    _raw(env, "dgppo_env_get_graph_hits", io)
    assert_same_graph(outs[0], outs[1], "op vs raw")
    assert_same_graph(outs[0], g, "op vs reset")
    o = env.empty_graph((B,), cuda)
    torch.library.opcheck(torch.ops.dgppo.env_get_graph_hits.default,
                          (h, agent, goal, h_op, o.nodes, o.edges, o.states, o.receivers, o.senders), test_utils=checks)
    with pytest.raises(ValueError, match="contiguous"):
        torch.ops.dgppo.lidar_hits(h, agent, a_op[..., ::2], rays, h_op)


# ---- 4. the loop ----------------------------------------------------------------------------------------------------
LOOP_CASES = [("LidarSpread", 3, 2, 4, RolloutEngine.MODE_DET), ("LidarOmniTarget", 3, 2, 4, RolloutEngine.MODE_DET),
              ("LidarSpread", 8, 3, 5, RolloutEngine.MODE_SAMPLE)]
LOOP_IDS = ["spread-det", "omni-det", "spread-n8-sample"]
T = 6
_LOOP = {}


def blind_sensor(alpha, t):
    return torch.full_like(alpha, 1e6)


def loop_setup(cuda, case):
    """(env, actor, the scene of a reset, the plain engine's outputs from that scene and key 7), once per case."""
    if case not in _LOOP:
        eid, n, obs, B, mode = case
        env = make_env(eid, n, num_obs=obs, max_step=T, device=cuda)
        algo = make_algo("dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                         action_dim=env.action_dim, n_agents=n, batch_size=B * T, rnn_step=3, seed=2, device=cuda)
        s = env.reset(key=3, n_env=B).env_states
        scene = (s.agent.clone(), s.goal.clone(), s.obstacle.packed.clone())
        plain = RolloutEngine(env, B, T, cuda, actor=algo.actor, mode=mode, init_state=scene)
        plain.run(7)
        _LOOP[case] = (env, algo.actor, scene, outputs(plain))
    return _LOOP[case]


def outputs(eng):
    b = eng.buf
    out = dict(nodes=b.nodes, edges=b.edges, states=b.states, receivers=b.receivers, senders=b.senders,
               rewards=eng.rewards, costs=eng.costs, actions=eng.actions)
    if eng.actor is not None and eng.mode != RolloutEngine.MODE_RANDOM:
        out["rnn"] = eng.rnn
        if eng.mode == RolloutEngine.MODE_SAMPLE:
            out["log_pis"] = eng.log_pis
    return {k: v.clone() for k, v in out.items()}


def assert_outputs_equal(x, y, what, keys=None):
    for k in keys or x:
        assert torch.equal(x[k], y[k]), (what, k)


def sensed(cuda, case, sensor):
    env, actor, scene, _ = loop_setup(cuda, case)
    eng = SensorRolloutEngine(env, case[3], T, cuda, actor=actor, mode=case[4], sensor=sensor, init_state=scene)
    roll = eng.run(7)
    return eng, roll


@pytest.mark.parametrize("sensor", [lambda a, t: a, LidarNoise(0.0, 0.0, seed=9)], ids=["identity", "noise-0-0"])
@pytest.mark.parametrize("case", LOOP_CASES, ids=LOOP_IDS)
def test_identity_sensor_is_the_plain_engine(cuda, case, sensor):
    env, actor, scene, ref = loop_setup(cuda, case)
    eng, roll = sensed(cuda, case, sensor)
    assert ref["actions"].abs().max() > 0
    assert_outputs_equal(outputs(eng), ref, "identity sensor")
    # the observed graphs are the true ones, (B, T, ...)
    obs = eng.observed
    for f in FIELDS:
        assert getattr(obs, f).shape[:2] == (case[3], T)
        assert torch.equal(getattr(obs, f), getattr(roll.graph, f)), f
    with pytest.raises(NotImplementedError):
        eng.capture()


@pytest.mark.parametrize("case", LOOP_CASES, ids=LOOP_IDS)
def test_blind_sensor(cuda, case):
    env, actor, scene, ref = loop_setup(cuda, case)
    eid, n, obs, B, mode = case
    eng, roll = sensed(cuda, case, blind_sensor)
    out = outputs(eng)
    # every agent-hit edge of the observed graphs is masked to the pad node
    k = env.params["top_k_rays"]
    first = env.n_edges - n * k
    pad = env.n_nodes - 1
    seen = eng.observed
    assert bool((seen.receivers[..., first:] == pad).all()) and bool((seen.senders[..., first:] == pad).all())
    assert not bool((roll.graph.receivers[..., first:] == pad).all())  # the true graphs do see obstacles
    # the truth depends on the observation through the actions only
    replay = RolloutEngine(env, B, T, cuda, init_state=scene)
    replay.actions.copy_(eng.actions)
    replay.run(0)
    assert_outputs_equal(outputs(replay), out, "replayed actions", FIELDS + ("rewards", "costs"))
    # observed[t] recomputed outside the engine
    for t in range(T):
        agent, goal = eng.buf.states[t][:, :n], eng.buf.states[t][:, n:n + env.num_goals]
        hits = env.lidar_hits(agent, blind_sensor(env.lidar_scan(agent, scene[2]), t))
        g = env.get_graph((agent, goal, scene[2]), lidar_data=hits)
        for f in FIELDS:
            assert torch.equal(getattr(g, f), getattr(seen, f)[:, t]), (t, f)


def test_lidar_noise_in_the_loop(cuda):
    case = LOOP_CASES[0]
    env, actor, scene, ref = loop_setup(cuda, case)
    n, k = case[1], env.params["top_k_rays"]
    hit_rows = slice(n + env.num_goals, n + env.num_goals + n * k)

    def run(sensor):
        eng, _ = sensed(cuda, case, sensor)
        out = outputs(eng)
        out.update({"seen_" + f: getattr(eng.observed, f).clone() for f in FIELDS})
        return out

    a, b = run(LidarNoise(0.05, 0.2, seed=11)), run(LidarNoise(0.05, 0.2, seed=11))
    assert_outputs_equal(a, b, "same seed")
    c = run(LidarNoise(0.05, 0.2, seed=12))
    assert not torch.equal(a["seen_states"][:, :, hit_rows], c["seen_states"][:, :, hit_rows])
    clean, noisy = run(LidarNoise(0.0, 0.0, seed=11)), run(LidarNoise(0.05, 0.0, seed=11))
    assert not torch.equal(clean["seen_states"][:, :, hit_rows], noisy["seen_states"][:, :, hit_rows])
    assert_outputs_equal(run(LidarNoise(0.0, 1.0, seed=11)), run(blind_sensor), "dropout 1 is blind")
    # the sensor itself: returns get noise floored at 0, non-returns and NaN pass, draws differ across t
    alpha = env.lidar_scan(scene[0], scene[2])
    alpha[0, 0, 0] = float("nan")
    s = LidarNoise(0.05, 0.0, seed=4)
    y0, y1 = s(alpha, 0), s(alpha, 1)
    ret = alpha <= 1.0
    assert bool(ret.any()) and bool((alpha == 1e6).any())
    assert torch.equal(y0[~ret & ~alpha.isnan()], alpha[~ret & ~alpha.isnan()]) and bool(y0[0, 0, 0].isnan())
    assert bool((y0[ret] >= 0).all()) and not torch.equal(y0[ret], alpha[ret]) and not torch.equal(y0[ret], y1[ret])
    assert torch.equal(s(alpha, 0).nan_to_num(nan=-1.0), y0.nan_to_num(nan=-1.0))  # reproducible for (seed, t)
    d = LidarNoise(0.0, 0.5, seed=4)(alpha, 0)
    dropped = (d == 1e6) & ret
    assert 0 < int(dropped.sum()) < int(ret.sum()) and torch.equal(d[~dropped & ~alpha.isnan()], alpha[~dropped & ~alpha.isnan()])


# ---- 5. test.py -----------------------------------------------------------------------------------------------------
def test_cli_sensor_flags(cuda, tmp_path, monkeypatch, capsys):
    from test_train_gpu import _entry

    test_py, train_py = _entry("test"), _entry("train")
    eid, n, obs = "LidarSpread", 3, 2
    argv = ["train.py", "--env", eid, "-n", str(n), "--algo", "dgppo", "--obs", str(obs), "--steps", "2",
            "--n-env-train", "8", "--batch-size", "256", "--n-env-test", "4", "--eval-interval", "1",
            "--save-interval", "2", "--log-dir", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", argv)
    train_py.main()
    (run,) = glob.glob(os.path.join(str(tmp_path), eid, "dgppo", "seed0_*"))
    base = ["test.py", "--path", run, "--epi", "4", "--max-step", "6"]
    monkeypatch.setattr(sys, "argv", base)
    plain = test_py.main()
    capsys.readouterr()
    monkeypatch.setattr(sys, "argv", base + ["--lidar-noise", "0", "--lidar-dropout", "0"])
    clean = test_py.main()
    out = capsys.readouterr().out
    assert clean == plain and set(plain) == {"reward", "cost", "safe_rate"}
    assert "lidar noise: 0, lidar dropout: 0" in out and out.count("epi: ") == 4
    monkeypatch.setattr(sys, "argv", base + ["--lidar-dropout", "1"])
    blind = test_py.main()
    out = capsys.readouterr().out
    assert "lidar noise: 0, lidar dropout: 1" in out and out.count("epi: ") == 4
    assert set(blind) == set(plain) and all(np.isfinite(v) for v in blind.values())
    monkeypatch.setattr(sys, "argv", base + ["--env", "MPESpread", "--lidar-noise", "0.1"])
    with pytest.raises(SystemExit, match="no LiDAR"):
        test_py.main()
