"""env.get_graph on the GPU (dgppo_env_get_graph: the block, variant and wave kernels of caller-given states).

Bar: BIT-EXACT, as for reset and step (tests/test_env_gpu.py): against the graphs reset / step produced from the same
states, and against the NumPy oracle on hand-made states the reset never draws -- agents outside the arena, state
columns beyond every state_lim, a 1.2 x 0.9 obstacle, an obstacle outside [-2, 2]^2 (the culling's ineligible
branches), theta = 0 obstacles, an agent at an obstacle centre, coincident agents."""
import ctypes

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib, ops
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.env.obstacle import Rectangle
from dgppo_fov_amd.trainer.rollout import RolloutEngine
from oracle import env as O

from test_env_gpu import CONFIGS as BASE_CONFIGS, _np, assert_graph_equal

pytestmark = pytest.mark.gpu

FIELDS = ("nodes", "edges", "states", "receivers", "senders")
# (env, n, obstacles, B): the base configs at B <= 16 (B <= 6 at n = 32; 5 on the wave shape, whose workgroups
# hold 4 envs) plus the five variants
CONFIGS = [(eid, n, obs, 5 if (n, obs) == (8, 3) else min(B, 6 if n == 32 else 8)) for eid, n, obs, B in BASE_CONFIGS]
CONFIGS += [("LidarLine", 3, 2, 6), ("MPELine", 3, 2, 6), ("MPEFormation", 4, 1, 6), ("MPECorridor", 3, 2, 6),
            ("MPEConnectSpread", 3, 1, 6)]
IDS = [f"{c[0]}-n{c[1]}-o{c[2]}" for c in CONFIGS]


def assert_same_graph(a, b, what=""):
    for f in FIELDS + ("node_type",):
        assert torch.equal(getattr(a, f), getattr(b, f)), (what, f)


def clone_state(s):
    return type(s)(*(None if p is None else (Rectangle(p.packed.clone()) if isinstance(p, Rectangle) else p.clone())
                     for p in s))


def misaligned_out(env, B, dev):
    """An output graph whose edge buffer is only 4-byte aligned: the wave kernels' float4 stores cannot take it."""
    g = env.empty_graph((B,), dev)
    raw = torch.empty(g.edges.numel() + 1, device=dev)
    edges = raw[1:].view(g.edges.shape)
    assert edges.data_ptr() % 8 == 4
    return env._assemble(g.nodes, edges, g.states, g.receivers, g.senders, None)


# ---- 1. reset round trip -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_reset_round_trip(cuda, cfg):
    eid, n, obs, B = cfg
    env = make_env(eid, n, num_obs=obs, device=cuda)
    g = env.reset(key=31, n_env=B)
    g2 = env.get_graph(g.env_states)
    torch.cuda.synchronize()
    assert_same_graph(g2, g, "round trip")
    if env._obstacle_fields() > 0 and env.n_obs > 0:  # the returned graph carries the obstacles: it can be stepped
        assert torch.equal(g2.env_states.obstacle.packed, g.env_states.obstacle.packed)
    a = torch.rand(B, n, env.action_dim, device=cuda) * 2 - 1
    r1, r2 = env.step(g, a), env.step(g2, a)
    assert_same_graph(r2.graph, r1.graph, "step after get_graph")
    assert torch.equal(r1.reward, r2.reward) and torch.equal(r1.cost, r2.cost)


def test_reset_round_trip_block_kernel_and_misaligned_out(cuda):
    """LidarSpread n8 o3 takes the wave kernel; with the block kernels forced, or an out= graph whose edges view is
    offset by one float, the workgroup-per-env kernel runs instead -- same bits."""
    env = make_env("LidarSpread", 8, num_obs=3, device=cuda)
    B = 5
    g = env.reset(key=32, n_env=B)
    lib = _lib.load()
    prev = lib.dgppo_env_set_step_kernel(1)
    try:
        g_block = env.get_graph(g.env_states)
        torch.cuda.synchronize()
    finally:
        lib.dgppo_env_set_step_kernel(prev)
    assert_same_graph(g_block, g, "block kernel")
    g_mis = env.get_graph(g.env_states, out=misaligned_out(env, B, cuda))
    torch.cuda.synchronize()
    assert_same_graph(g_mis, g, "misaligned out")
    assert_same_graph(env.get_graph(g.env_states), g, "wave kernel")


@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 8, 3), ("LidarTarget", 5, 1), ("MPESpread", 3, 3),
                                       ("LidarLine", 3, 2)])
def test_get_graph_in_place(cuda, eid, n, obs):
    """out= the graph whose own env_states are the argument: every env's rows are staged before its first store."""
    env = make_env(eid, n, num_obs=obs, device=cuda)
    B = 5
    ref = env.reset(key=33, n_env=B)
    g = env.reset(key=33, n_env=B)
    for f in ("nodes", "edges", "receivers", "senders"):
        getattr(g, f).fill_(-7)
    g2 = env.get_graph(g.env_states, out=g)
    torch.cuda.synchronize()
    assert g2.states.data_ptr() == g.states.data_ptr()
    assert_same_graph(g2, ref, "in place")


# ---- 2. oracle parity on hand-made states ------------------------------------------------------------------
def hand_made_scene(spec, B, seed):
    """agent (B, n, sd), goal (B, ng, sd), third ((B, O, 16) records / (B, O, 4) MPE states) as numpy float32."""
    rng = np.random.default_rng(seed)
    F = np.float32
    n, sd, ng, Oo, area = spec.n, spec.sd, spec.ng, spec.n_obs, spec.area
    agent = rng.uniform(-1.5, 1.5, (B, n, sd)).astype(F)  # beyond every state_lim; omni headings not unit
    agent[..., :2] = rng.uniform(-0.3, area + 0.3, (B, n, 2)).astype(F)
    goal = np.zeros((B, ng, sd), F)
    goal[..., :2] = rng.uniform(0.0, area, (B, ng, 2)).astype(F)
    mpe = spec.engine == O.ENGINE_MPE
    center = rng.uniform(0.0, area, (B, Oo, 2)).astype(F)
    width = rng.uniform(0.1, 0.3, (B, Oo)).astype(F)
    height = rng.uniform(0.1, 0.3, (B, Oo)).astype(F)
    theta = rng.uniform(-np.pi, 2 * np.pi, (B, Oo)).astype(F)
    if Oo > 0:
        theta[0] = 0.0  # env 0: theta = 0 obstacles, agent 0 at an obstacle centre
        agent[0, 0, :2] = center[0, 0]
        width[1, 0], height[1, 0] = 1.2, 0.9  # env 1: a 1.2 x 0.9 obstacle (circumradius > 0.5)
        center[2, 0] = (2.3, -2.1)  # env 2: an obstacle outside [-2, 2]^2
    if n > 1:
        agent[1, 1, :2] = agent[1, 0, :2]  # env 1: two coincident agents
    agent[3, 0, :2] = (2.5, -3.0)  # env 3: an agent outside [-2, 2]^2
    if mpe:
        third = np.zeros((B, Oo, sd), F)
        third[..., :2] = center
    else:
        t = torch.from_numpy
        third = Rectangle.create(t(center), t(width), t(height), t(theta)).packed.numpy()
        np.testing.assert_array_equal(third, O.make_rectangles(center, width, height, theta))
    return agent, goal, third


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_hand_made_states_match_oracle(cuda, cfg):
    eid, n, obs, B = cfg
    env = make_env(eid, n, num_obs=obs, device=cuda)
    spec = O.Spec(eid, n, obs)
    agent, goal, third = hand_made_scene(spec, B, seed=5)
    dev = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    mpe = spec.engine == O.ENGINE_MPE
    ob = dev(third) if spec.n_obs > 0 else None
    g = env.get_graph((dev(agent), dev(goal), ob if mpe or ob is None else Rectangle(ob)))
    torch.cuda.synchronize()
    ref = O.initial_graph(spec, agent, goal, third)
    assert_graph_equal(g, ref, "get_graph")
    np.testing.assert_array_equal(_np(g.node_type[0]), O.node_type(spec))
    # one step from that graph
    rng = np.random.default_rng(6)
    a = rng.uniform(-1.5, 1.5, (B, n, spec.ad)).astype(np.float32)
    if spec.ad == 3:
        a[..., 2] *= 1000.0
    res = env.step(g, dev(a))
    sref = O.env_step(spec, ref["states"], None if mpe else third, a)
    torch.cuda.synchronize()
    assert_graph_equal(res.graph, sref, "step")
    np.testing.assert_array_equal(_np(res.cost), sref["cost"], err_msg="cost")
    np.testing.assert_array_equal(_np(res.reward), sref["reward"], err_msg="reward")


# ---- 3. mid-episode ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid,n,obs,B", [("LidarSpread", 8, 3, 5), ("LidarBicycleTarget", 8, 3, 5),
                                         ("LidarOmniTarget", 3, 2, 6), ("MPESpread", 3, 3, 6), ("LidarSpread", 32, 8, 3)])
def test_mid_episode_states_rebuild_their_graph(cuda, eid, n, obs, B):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    g = env.reset(key=41, n_env=B)
    gen = torch.Generator(device=cuda)
    gen.manual_seed(9)
    for t in range(6):
        assert_same_graph(env.get_graph(g.env_states), g, f"t={t}")
        a = torch.empty(B, n, env.action_dim, device=cuda).uniform_(-1.0, 1.0, generator=gen)
        g = env.step(g, a).graph


# ---- 4. get_lidar_data / get_reward ------------------------------------------------------------------------
@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 8, 3), ("LidarBicycleTarget", 3, 2), ("LidarOmniTarget", 3, 2),
                                       ("MPESpread", 3, 3)])
def test_get_lidar_data_and_get_reward(cuda, eid, n, obs):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    B = 5
    g = env.reset(key=51, n_env=B)
    a = torch.rand(B, n, env.action_dim, device=cuda) * 2 - 1
    assert torch.equal(env.get_reward(g, a), env.step(g, a).reward)
    if eid.startswith("MPE"):
        with pytest.raises(ValueError):
            env.get_lidar_data(g.env_states.agent, None)
        return
    k = env.params["top_k_rays"]
    hits = env.get_lidar_data(g.env_states.agent, g.env_states.obstacle)
    assert hits.shape == (B, n, k, 2)
    assert torch.equal(hits, g.states[:, 2 * n:2 * n + n * k, :2].reshape(B, n, k, 2))


# ---- 5 / 6. rollouts from scenes ---------------------------------------------------------------------------
def _engine_outputs(eng):
    b = eng.buf
    out = [b.nodes, b.edges, b.states, b.receivers, b.senders, eng.rewards, eng.costs]
    if eng.actor is not None:
        out += [eng.actions, eng.rnn]
    return [x.clone() for x in out]


def _assert_outputs_equal(x, y, what):
    for i, (a, b) in enumerate(zip(x, y)):
        assert torch.equal(a, b), (what, i)


@pytest.mark.parametrize("eid,n,obs,B,lanes", [("LidarSpread", 8, 3, 5, 1), ("MPESpread", 3, 3, 5, 1),
                                               ("LidarTarget", 5, 1, 4, 1), ("LidarSpread", 8, 3, 8, 2)])
def test_engine_from_init_state_random_actions(cuda, eid, n, obs, B, lanes):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    T = 8
    gen = torch.Generator(device=cuda)
    gen.manual_seed(3)
    actions = torch.empty(T, B, n, env.action_dim, device=cuda).uniform_(-1.0, 1.0, generator=gen)

    def from_key(key):
        e = RolloutEngine(env, B, T, cuda, lanes=lanes)
        e.actions.copy_(actions)
        e.run(key)
        return _engine_outputs(e), clone_state(e.graph_at(0).env_states)

    def from_scene(scene, fused=True):
        e = RolloutEngine(env, B, T, cuda, lanes=lanes, fused=fused, init_state=scene)
        e.actions.copy_(actions)
        return e

    ref7, scene7 = from_key(7)
    ref8, scene8 = from_key(8)
    assert not torch.equal(ref7[2], ref8[2])
    for fused in (True, False):
        eng = from_scene(clone_state(scene7), fused)
        eng.run(0)
        _assert_outputs_equal(_engine_outputs(eng), ref7, f"eager fused={fused}")
    if eng.obstacles is not None:  # the steps read the scene's own records
        assert eng.obstacles.data_ptr() == eng.init_state[2].packed.data_ptr()
    # captured: the hipGraph reads the caller's tensors, so a scene edited in place is what the next replay runs
    live = clone_state(scene7)
    cap = from_scene(live).capture()
    cap.run(0)
    _assert_outputs_equal(_engine_outputs(cap), ref7, "captured")
    for dst, src in zip(live, scene8):
        if dst is not None:
            getattr(dst, "packed", dst).copy_(getattr(src, "packed", src))
    cap.run(0)
    eager8 = from_scene(clone_state(scene8))
    eager8.run(0)
    _assert_outputs_equal(_engine_outputs(cap), _engine_outputs(eager8), "captured, second scene")
    _assert_outputs_equal(_engine_outputs(cap), ref8, "second scene vs its reset")
    # a scene that does not fit is refused where the engine is built, and the message names the field
    third = "obs" if eid.startswith("MPE") else "obstacle"
    with pytest.raises(ValueError, match="init_state.agent"):
        RolloutEngine(env, B, T, cuda, init_state=(scene7[0][:, :-1], scene7[1], scene7[2]))
    with pytest.raises(ValueError, match=f"init_state.{third} "):
        RolloutEngine(env, B, T, cuda, init_state=(scene7[0], scene7[1], getattr(scene7[2], "packed", scene7[2])[:, :-1]))
    with pytest.raises(ValueError, match=f"init_state.agent must hold {B} envs"):
        RolloutEngine(env, B, T, cuda, init_state=tuple(None if p is None else p[:-1] for p in scene7))
    with pytest.raises(ValueError, match="init_state.goal must be a float32 tensor"):
        RolloutEngine(env, B, T, cuda, init_state=(scene7[0], scene7[1].double(), scene7[2]))


@pytest.mark.parametrize("mode", [RolloutEngine.MODE_DET, RolloutEngine.MODE_SAMPLE], ids=["det", "sample"])
def test_engine_from_init_state_with_actor(cuda, mode):
    eid, n, obs, B, T = "LidarSpread", 3, 3, 4, 8
    env = make_env(eid, n, num_obs=obs, max_step=T, device=cuda)
    algo = make_algo("dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=n, batch_size=B * T, rnn_step=4, seed=2, device=cuda)

    def from_key(key):
        e = RolloutEngine(env, B, T, cuda, actor=algo.actor, mode=mode)
        e.run(key)
        return _engine_outputs(e), clone_state(e.graph_at(0).env_states)

    def from_scene(scene):
        return RolloutEngine(env, B, T, cuda, actor=algo.actor, mode=mode, init_state=scene)

    ref7, scene7 = from_key(7)
    ref8, scene8 = from_key(8)
    assert ref7[7].abs().max() > 0 and not torch.equal(ref7[7], ref8[7])  # actions
    b = from_scene(clone_state(scene7))
    b.run(7)  # (the key still seeds the sampling noise)
    _assert_outputs_equal(_engine_outputs(b), ref7, "eager")
    # captured get_graph -> (actor, step) x T: a second scene copied into the live tensors is what the next replay
    # runs, policy workspace and RNN carries included
    live = clone_state(scene7)
    c = from_scene(live).capture()
    c.run(7)
    _assert_outputs_equal(_engine_outputs(c), ref7, "captured")
    for dst, src in zip(live, scene8):
        if dst is not None:
            getattr(dst, "packed", dst).copy_(getattr(src, "packed", src))
    c.run(8)
    eager8 = from_scene(clone_state(scene8))
    eager8.run(8)
    _assert_outputs_equal(_engine_outputs(c), _engine_outputs(eager8), "captured, second scene")
    _assert_outputs_equal(_engine_outputs(c), ref8, "second scene vs its reset")


# ---- 7. the op ------------------------------------------------------------------------------------------------
def _raw_get_graph(env, state, out):
    io = _lib.EnvGraphIO()
    agent, goal, third = state[0], state[1], getattr(state[2], "packed", state[2])
    io.agent, io.agent_stride = agent.data_ptr(), ops._stride(agent, 2)
    io.goal, io.goal_stride = goal.data_ptr(), ops._stride(goal, 2)
    io.third, io.third_stride = third.data_ptr(), ops._stride(third, 2)
    io.ray_dirs = env._ray_table(agent.device).data_ptr()
    io.nodes, io.nodes_stride = out.nodes.data_ptr(), ops._stride(out.nodes, 2)
    io.edges, io.edges_stride = out.edges.data_ptr(), ops._stride(out.edges, 2)
    io.out_states, io.out_states_stride = out.states.data_ptr(), ops._stride(out.states, 2)
    io.receivers, io.senders = out.receivers.data_ptr(), out.senders.data_ptr()
    io.edge_index_stride = ops._stride(out.receivers, 1)
    io.n_env = agent.shape[0]
    _lib.check(_lib.load().dgppo_env_get_graph(ctypes.byref(env.cfg), ctypes.byref(io),
                                               _lib.stream_handle(agent.device)), "dgppo_env_get_graph")


@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 8, 3), ("LidarTarget", 5, 1), ("MPESpread", 3, 3)])
def test_op_matches_c_abi_and_opcheck(cuda, eid, n, obs):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    B = 5
    g = env.reset(key=61, n_env=B)
    s = g.env_states
    third = getattr(s[2], "packed", s[2])
    outs = []
    for path in ("op", "raw"):
        out = env.empty_graph((B,), cuda)
        if path == "op":
            torch.ops.dgppo.env_get_graph(env._cfg_handle, s[0], s[1], third, env._ray_table(cuda), out.nodes,
                                          out.edges, out.states, out.receivers, out.senders)
        else:
            _raw_get_graph(env, s, out)
        torch.cuda.synchronize()
        outs.append(out)
    assert_same_graph(outs[0], outs[1], "op vs raw")
    assert_same_graph(outs[0], g, "op vs reset")
    out = env.empty_graph((B,), cuda)
    torch.library.opcheck(torch.ops.dgppo.env_get_graph.default,
                          (env._cfg_handle, s[0], s[1], third, env._ray_table(cuda), out.nodes, out.edges, out.states,
                           out.receivers, out.senders), test_utils=("test_schema", "test_faketensor"))
    with pytest.raises(ValueError, match="contiguous"):
        torch.ops.dgppo.env_get_graph(env._cfg_handle, s[0][..., ::2], s[1], third, env._ray_table(cuda), out.nodes,
                                      out.edges, out.states, out.receivers, out.senders)
