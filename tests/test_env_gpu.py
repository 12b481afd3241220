"""GPU parity: the fused HIP env kernels (dgppo_env_reset / dgppo_env_step, through the C-ABI)
against the NumPy oracle on the same inputs.  Bar: BIT-EXACT for every graph field, cost and
reward (integer/index work and the fp32 arithmetic are done in the same op order with no FMA
contraction on either side); the only tolerance below is for the bicycle's continuous fields,
which go through the same deterministic sin/cos/atan2 and are also expected to be exact."""
import numpy as np
import pytest
import torch

from dgppo_fov_amd.env import make_env
from env_cases import _np, adversarial_lidar_scene, assert_graph_equal, oracle_third  # noqa: F401
from oracle import env as O

pytestmark = pytest.mark.gpu

CONFIGS = [
    ("MPETarget", 3, 0, 32),
    ("MPESpread", 3, 3, 64),
    ("LidarSpread", 8, 3, 64),
    ("LidarTarget", 8, 3, 32),
    ("LidarBicycleTarget", 8, 3, 64),
    ("LidarSpread", 32, 8, 6),
    ("LidarSpread", 1, 3, 16),
    ("LidarSpread", 8, 0, 16),
    ("LidarTarget", 5, 1, 16),
    ("LidarOmniTarget", 8, 3, 64),
    ("LidarOmniTarget", 3, 2, 32),
    ("LidarOmniTarget", 1, 3, 8),
    ("LidarOmniTarget", 4, 0, 8),
]
IDS = [f"{c[0]}-n{c[1]}-o{c[2]}" for c in CONFIGS]


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_reset_matches_oracle(cuda, cfg):
    eid, n, obs, B = cfg
    env = make_env(eid, n, num_obs=obs, device=cuda)
    spec = O.Spec(eid, n, obs)
    g = env.reset(key=1234, n_env=B)
    torch.cuda.synchronize()
    ag, gl, third = O.env_reset(spec, 1234, B)
    ref = O.initial_graph(spec, ag, gl, third)
    assert_graph_equal(g, ref, "reset")
    if spec.engine != O.ENGINE_MPE and obs > 0:
        np.testing.assert_array_equal(_np(g.env_states.obstacle.packed), third)
    assert g.node_type.shape == (B, spec.n_nodes)
    np.testing.assert_array_equal(_np(g.node_type[0]), O.node_type(spec))


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_step_chain_matches_oracle(cuda, cfg):
    eid, n, obs, B = cfg
    env = make_env(eid, n, num_obs=obs, device=cuda)
    spec = O.Spec(eid, n, obs)
    g = env.reset(key=99, n_env=B)
    rng = np.random.default_rng(1)
    states = _np(g.states)
    third = oracle_third(spec, g)
    for t in range(6):
        a = rng.uniform(-1.5, 1.5, (B, n, spec.ad)).astype(np.float32)  # includes out-of-range actions (clipped)
        if spec.ad == 3:
            a[..., 2] *= 1000.0  # Omni angular acceleration, clipped at +-1000
        res = env.step(g, torch.from_numpy(a).to(cuda))
        ref = O.env_step(spec, states, third, a)
        torch.cuda.synchronize()
        assert_graph_equal(res.graph, ref, f"step{t}")
        np.testing.assert_array_equal(_np(res.cost), ref["cost"], err_msg=f"cost step{t}")
        np.testing.assert_array_equal(_np(res.reward), ref["reward"], err_msg=f"reward step{t}")
        assert not res.done.any()
        g, states = res.graph, ref["states"]


def test_step_edge_cases(cuda):
    """Agent inside an obstacle (alpha=0 -> hits = start), NaN / inf actions, agents on top of
    each other (zero distance), agents clipped at the walls."""
    eid, n, obs, B = "LidarSpread", 4, 2, 8
    env = make_env(eid, n, num_obs=obs, device=cuda)
    spec = O.Spec(eid, n, obs)
    g = env.reset(key=5, n_env=B)
    states = _np(g.states).copy()
    ob = _np(g.env_states.obstacle.packed).copy()
    states[0, 0, :2] = ob[0, 0, :2]  # agent 0 of env 0 at an obstacle centre
    states[1, 1, :2] = states[1, 0, :2]  # coincident agents
    states[2, :n, 0] = 1.5  # on the wall
    states[2, :n, 2] = 0.5
    a = np.random.default_rng(2).uniform(-1, 1, (B, n, 2)).astype(np.float32)
    a[3, 0, 0] = np.nan
    a[4, 1, 1] = np.inf
    a[5, 2, 0] = -1e30
    gin = env._assemble(g.nodes, g.edges, torch.from_numpy(states).to(cuda), g.receivers, g.senders,
                        torch.from_numpy(ob).to(cuda))
    res = env.step(gin, torch.from_numpy(a).to(cuda))
    ref = O.env_step(spec, states, ob, a)
    torch.cuda.synchronize()
    assert_graph_equal(res.graph, ref, "edge-cases")
    c, rc = _np(res.cost), ref["cost"]
    assert np.array_equal(c, rc) or np.array_equal(np.isnan(c), np.isnan(rc))
    r, rr = _np(res.reward), ref["reward"]
    assert np.array_equal(np.isnan(r), np.isnan(rr)) and np.array_equal(r[~np.isnan(r)], rr[~np.isnan(rr)])
    # agent inside the obstacle at the NEXT state? its hits are its own position (alpha = 0)
    inside = O.inside_rect(ref["next_agent"][0, 0, 0], ref["next_agent"][0, 0, 1], ob[0], 0.0).any()
    if inside:
        hits = ref["states"][0, 2 * n:2 * n + 8, :2]
        np.testing.assert_array_equal(hits, np.broadcast_to(ref["next_agent"][0, 0, :2], hits.shape))


def test_full_size_lidar_spread_bit_exact(cuda):
    """BASELINE config: LidarSpread n=8, obs=3, 4096 envs — the whole batch, bit-exact."""
    eid, n, obs, B = "LidarSpread", 8, 3, 4096
    env = make_env(eid, n, num_obs=obs, device=cuda)
    spec = O.Spec(eid, n, obs)
    g = env.reset(key=2024, n_env=B)
    a = np.random.default_rng(3).uniform(-1, 1, (B, n, 2)).astype(np.float32)
    res = env.step(g, torch.from_numpy(a).to(cuda))
    ref = O.env_step(spec, _np(g.states), _np(g.env_states.obstacle.packed), a)
    torch.cuda.synchronize()
    assert_graph_equal(res.graph, ref, "full")
    np.testing.assert_array_equal(_np(res.cost), ref["cost"])
    np.testing.assert_array_equal(_np(res.reward), ref["reward"])


def test_step_writes_into_strided_rollout_buffer(cuda):
    """step_into with (B, T+1, ...) views: the kernel honours per-env strides."""
    eid, n, obs, B, T = "LidarSpread", 3, 2, 8, 4
    env = make_env(eid, n, num_obs=obs, device=cuda)
    buf = env.empty_graph((B, T + 1), cuda)
    g0 = env.reset(key=3, n_env=B)
    for f in ("nodes", "edges", "states", "receivers", "senders"):
        getattr(buf, f)[:, 0].copy_(getattr(g0, f))
    ob = g0.env_states.obstacle.packed
    rew = torch.empty(B, T, device=cuda)
    cost = torch.empty(B, T, n, 2, device=cuda)
    acts = torch.rand(B, T, n, 2, device=cuda) * 2 - 1
    cur = env._assemble(buf.nodes[:, 0], buf.edges[:, 0], buf.states[:, 0], buf.receivers[:, 0], buf.senders[:, 0], ob)
    ref_g = g0
    for t in range(T):
        out = env._assemble(buf.nodes[:, t + 1], buf.edges[:, t + 1], buf.states[:, t + 1], buf.receivers[:, t + 1],
                            buf.senders[:, t + 1], ob)
        cur = env.step_into(cur, acts[:, t], out, rew[:, t], cost[:, t])
        ref = env.step(ref_g, acts[:, t].contiguous())
        torch.cuda.synchronize()
        for f in ("nodes", "edges", "states", "receivers", "senders"):
            assert torch.equal(getattr(cur, f), getattr(ref.graph, f)), f
        assert torch.equal(rew[:, t], ref.reward) and torch.equal(cost[:, t], ref.cost)
        ref_g = ref.graph


@pytest.mark.parametrize("eid", ["LidarSpread", "LidarOmniTarget"])
def test_misaligned_edge_buffers_take_the_generic_kernels(cuda, eid):
    """The wave-per-env kernels store edge rows as float4 / float2; an edge buffer that is only 4-byte
    aligned must be routed to the workgroup-per-env kernels, with the same results (reset and step)."""
    n, obs, B = 8, 3, 12
    env = make_env(eid, n, num_obs=obs, device=cuda)
    spec = O.Spec(eid, n, obs)

    g_ref = env.reset(key=77, n_env=B)
    ob = torch.empty_like(g_ref.env_states.obstacle.packed)

    def misaligned_graph():
        g = env.empty_graph((B,), cuda)
        raw = torch.empty(g.edges.numel() + 1, device=cuda)
        edges = raw[1:].view(g.edges.shape)
        assert edges.data_ptr() % 8 == 4
        return env._assemble(g.nodes, edges, g.states, g.receivers, g.senders, ob)

    out0 = misaligned_graph()
    g_mis = env.reset(key=77, n_env=B, out=out0, obstacles_out=ob)
    torch.cuda.synchronize()
    for f in ("nodes", "edges", "states", "receivers", "senders"):
        assert torch.equal(getattr(g_mis, f), getattr(g_ref, f)), ("reset", f)
    a = torch.rand(B, n, spec.ad, device=cuda) * 2 - 1
    res_ref = env.step(g_ref, a)
    out1 = misaligned_graph()
    rew = torch.empty(B, device=cuda)
    cost = torch.empty(B, n, env.n_cost, device=cuda)
    g1 = env.step_into(g_mis, a, out1, rew, cost)
    ref = O.env_step(spec, _np(g_ref.states), _np(g_ref.env_states.obstacle.packed), _np(a))
    torch.cuda.synchronize()
    assert_graph_equal(g1, ref, "misaligned step")
    for f in ("nodes", "edges", "states", "receivers", "senders"):
        assert torch.equal(getattr(g1, f), getattr(res_ref.graph, f)), ("step", f)
    assert torch.equal(rew, res_ref.reward) and torch.equal(cost, res_ref.cost)


def test_golden_fixtures_on_gpu(cuda):
    import glob
    import os

    files = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "env_*.npz")))
    assert files, "tests/golden/env_*.npz missing (run tests/golden/make_golden.py)"
    for fn in files:
        z = np.load(fn, allow_pickle=False)
        eid = str(z["env_id"])
        n, obs, seed = int(z["n"]), int(z["n_obs"]), int(z["seed"])
        B = z["states0"].shape[0]
        env = make_env(eid, n, num_obs=obs, device=cuda)
        g = env.reset(key=seed, n_env=B)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(_np(g.states), z["states0"], err_msg=fn)
        res = env.step(g, torch.from_numpy(z["action"]).to(cuda))
        torch.cuda.synchronize()
        for f in ("nodes", "edges", "states", "receivers", "senders"):
            np.testing.assert_array_equal(_np(getattr(res.graph, f)), z[f], err_msg=f"{fn}:{f}")
        np.testing.assert_array_equal(_np(res.reward), z["reward"], err_msg=fn)
        np.testing.assert_array_equal(_np(res.cost), z["cost"], err_msg=fn)


@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 8, 3), ("MPESpread", 3, 3)])
def test_env_shards_equal_global_slices(cuda, eid, n, obs):
    """Multi-GPU env sharding: rank r's reset with env_offset = r*B reproduces envs
    [r*B, (r+1)*B) of a single-process reset, bit for bit, and so does every step."""
    env = make_env(eid, n, num_obs=obs, device=cuda)
    full = env.reset(key=9, n_env=8)
    part = env.reset(key=9, n_env=4, env_offset=4)
    for k in ("nodes", "edges", "states", "receivers", "senders"):
        assert torch.equal(getattr(full, k)[4:], getattr(part, k)), k
    a = torch.rand(8, n, 2, device=cuda) * 2 - 1
    nf = env.step(full, a)
    npart = env.step(part, a[4:].contiguous())
    assert torch.equal(nf.graph.nodes[4:], npart.graph.nodes) and torch.equal(nf.reward[4:], npart.reward)


def _adversarial_lidar_inputs(env, spec, B, seed, cuda):
    """env_cases.adversarial_lidar_scene on the GPU env's own reset arrays, as a graph the step kernels take."""
    g = env.reset(key=seed, n_env=B)
    states, ob, a = adversarial_lidar_scene(spec, _np(g.states), _np(g.env_states.obstacle.packed), seed)
    gin = env._assemble(g.nodes, g.edges, torch.from_numpy(states).to(cuda), g.receivers, g.senders,
                        torch.from_numpy(ob).to(cuda))
    return gin, states, ob, a


@pytest.mark.parametrize("eid", ["LidarSpread", "LidarTarget", "LidarBicycleTarget", "LidarOmniTarget"])
def test_wave_step_kernel_adversarial(cuda, eid):
    """The wave-per-env step kernel (exact ray culling + compacted ray cast) against the oracle and
    against the workgroup-per-env kernel, bit for bit, on adversarial inputs."""
    from dgppo_fov_amd import _lib

    n, obs, B = 8, 3, 256
    env = make_env(eid, n, num_obs=obs, device=cuda)
    spec = O.Spec(eid, n, obs)
    gin, states, ob, a = _adversarial_lidar_inputs(env, spec, B, 77, cuda)
    at = torch.from_numpy(a).to(cuda)
    lib = _lib.load()
    prev = lib.dgppo_env_set_step_kernel(0)
    try:
        res = env.step(gin, at)
        lib.dgppo_env_set_step_kernel(1)
        res_blk = env.step(gin, at)
    finally:
        lib.dgppo_env_set_step_kernel(max(prev, 0))
    torch.cuda.synchronize()
    ref = O.env_step(spec, states, ob, a)
    for f in ("nodes", "edges", "states", "receivers", "senders"):
        x, y = getattr(res.graph, f), getattr(res_blk.graph, f)
        same = (x == y) | (torch.isnan(x) & torch.isnan(y)) if x.is_floating_point() else (x == y)
        assert bool(same.all()), f"wave vs block kernel: {f}"
    assert_graph_equal(res.graph, ref, f"{eid} adversarial")
    c, rc = _np(res.cost), ref["cost"]
    assert np.array_equal(np.isnan(c), np.isnan(rc)) and np.array_equal(c[~np.isnan(c)], rc[~np.isnan(rc)])
    r, rr = _np(res.reward), ref["reward"]
    assert np.array_equal(np.isnan(r), np.isnan(rr)) and np.array_equal(r[~np.isnan(r)], rr[~np.isnan(rr)])


def test_omni_step_edge_cases(cuda):
    """LidarOmniTarget: agent inside an obstacle, coincident agents (FoV norm 0), headings that are not
    unit vectors, NaN / huge actions, angular rates at the limit."""
    eid, n, obs, B = "LidarOmniTarget", 4, 2, 8
    env = make_env(eid, n, num_obs=obs, device=cuda)
    spec = O.Spec(eid, n, obs)
    g = env.reset(key=11, n_env=B)
    states = _np(g.states).copy()
    ob = _np(g.env_states.obstacle.packed).copy()
    states[0, 0, :2] = ob[0, 0, :2]
    states[1, 1, :2] = states[1, 0, :2]
    states[2, :n, 2:4] = [0.3, 0.4]
    states[3, :n, 6] = 99.0
    states[4, :n, 4:6] = -1.9
    a = np.random.default_rng(2).uniform(-1, 1, (B, n, 3)).astype(np.float32)
    a[5, 0, 0] = np.nan
    a[6, 1, 2] = 1e30
    a[7, 2, 2] = -np.inf
    gin = env._assemble(g.nodes, g.edges, torch.from_numpy(states).to(cuda), g.receivers, g.senders,
                        torch.from_numpy(ob).to(cuda))
    res = env.step(gin, torch.from_numpy(a).to(cuda))
    ref = O.env_step(spec, states, ob, a)
    torch.cuda.synchronize()
    assert_graph_equal(res.graph, ref, "omni edge cases")
    c, rc = _np(res.cost), ref["cost"]
    assert np.array_equal(np.isnan(c), np.isnan(rc)) and np.array_equal(c[~np.isnan(c)], rc[~np.isnan(rc)])
    r, rr = _np(res.reward), ref["reward"]
    assert np.array_equal(np.isnan(r), np.isnan(rr)) and np.array_equal(r[~np.isnan(r)], rr[~np.isnan(rr)])


def test_omni_reset_chain_headings(cuda):
    """Reset points agent i at agent i+1 (unit heading) and keeps agents >= D = 0.2 apart."""
    env = make_env("LidarOmniTarget", 6, num_obs=3, device=cuda)
    g = env.reset(key=5, n_env=64)
    st = _np(g.states)
    ag = st[:, :6]
    d = ag[:, 1:, :2] - ag[:, :-1, :2]
    u = d / (np.linalg.norm(d, axis=-1, keepdims=True) + 1e-8)
    np.testing.assert_allclose(ag[:, :-1, 2:4], u, atol=1e-6)
    np.testing.assert_allclose(np.linalg.norm(ag[:, -1, 2:4], axis=-1), 1.0, atol=1e-6)
    pd = np.linalg.norm(ag[:, :, None, :2] - ag[:, None, :, :2], axis=-1) + np.eye(6) * 9
    assert (pd > 0.2).all()
    assert (ag[..., 4:] == 0).all()
