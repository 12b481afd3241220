"""LiDAR sees agents on the GPU: dgppo_lidar_scan_bodies against the NumPy reference (tests/bodies_ref.py), the fused
dgppo_lidar_observe_bodies against the chain get_graph(lidar_hits(LidarNoise(lidar_scan(bodies=True)))) [+ mask_unseen],
a body return as a hit row of the observed graph, the two sensor engines against each other, training and test.py.

Bar: BIT-EXACT (torch.equal / array equality on float bits; NaN equal to NaN): the paths share one arithmetic, and the
reference restates it one rounded float32 operation per statement.  Scenes are hand-made (agents dense enough that
bodies return, cones and walls hide neighbours); every property a scene is there for is asserted on the reference."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import ENV, make_env
from dgppo_fov_amd.trainer.rollout import NoisyLidarRolloutEngine, RolloutEngine, SensorRolloutEngine
from dgppo_fov_amd.utils.sensor import LidarNoise, mask_unseen
from oracle import env as O

import bodies_ref as R
from env_cases import _np
from test_sensor_gpu import FIELDS, assert_outputs_equal, assert_same_graph, dev_of, outputs

pytestmark = pytest.mark.gpu

F = np.float32
B = 8
NONE = F(1e6)
LIDAR = ("LidarSpread", "LidarTarget", "LidarBicycleTarget", "LidarOmniTarget", "LidarLine")
HEADING = ("LidarBicycleTarget", "LidarOmniTarget")


def cases(ns):
    """(env, n) over the five LiDAR envs; LidarLine has two landmarks for at least two agents, so it has no n = 1."""
    return [(e, n) for e in LIDAR for n in ns if not (e == "LidarLine" and n < 2)]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_bits_equal(got, ref, what=""):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype == F, what
    bad = bits(got) != bits(ref)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} differ, first at {np.argwhere(bad)[0]}: " \
                          f"{got[bad][:4]} vs {ref[bad][:4]}"


def lidar_env(eid, n, obs, rays, dev, **kw):
    """The env at `rays` beams, top_k = min(8, rays); LidarLine at n >= 8 gets an arena its landmarks fit in."""
    params = dict(ENV[eid].PARAMS, n_obs=obs, n_rays=rays, top_k_rays=min(8, rays))
    if eid == "LidarLine" and n >= 8:
        kw["area_size"] = 0.5 * n
    return ENV[eid](num_agents=n, params=params, device=dev, **kw)


def random_scene(env, n, obs, seed, nb=B, box=1.0):
    """(agent (nb, n, sd), goal, obstacles (nb, obs, 16)) as NumPy: positions uniform in [0, box]^2 (dense: bodies are in
    range of each other), unit headings in columns 2, 3 where the env has them, rectangles of mixed sizes."""
    rng = np.random.default_rng(seed)
    sd = env.state_dim
    agent = rng.uniform(-0.5, 0.5, (nb, n, sd)).astype(F)
    agent[..., :2] = rng.uniform(0, box, (nb, n, 2))
    if sd > 4:
        th = rng.uniform(-np.pi, np.pi, (nb, n))
        agent[..., 2], agent[..., 3] = np.cos(th), np.sin(th)
    goal = np.zeros((nb, env.num_goals, sd), F)
    goal[..., :2] = rng.uniform(0, box, (nb, env.num_goals, 2))
    ob = np.stack([O.make_rectangles(rng.uniform(0, box, (obs, 2)), rng.uniform(0.05, 0.4, obs),
                                     rng.uniform(0.05, 0.4, obs), rng.uniform(0, 2 * np.pi, obs)) for _ in range(nb)])
    return agent, goal, ob.astype(F)


def rho_of(env):
    return float(env.params["car_radius"])


# ---- 1. the scan ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid,n", cases([1, 2, 3, 8, 64]))
def test_scan_matches_reference_on_random_scenes(cuda, eid, n):
    dev = dev_of(cuda)
    box = {1: 1.0, 2: 0.5, 3: 0.6, 8: 1.0, 64: 3.0}[n]  # dense enough that bodies are in range of each other
    in_the_open = behind_a_wall = False
    for rays in (1, 32, 33, 128):
        for obs in (1, 3, 16):
            env = lidar_env(eid, n, obs, rays, cuda)
            agent, _, ob = random_scene(env, n, obs, seed=1000 * n + 10 * rays + obs, box=box)
            a, o = dev(agent), dev(ob)
            tab = _np(env._ray_table(cuda))
            today = env.lidar_scan(a, o)
            a_obs = _np(today)
            ref = R.scan_bodies_ref(a_obs, agent, tab, rho_of(env))
            got = env.lidar_scan(a, o, bodies=True)
            what = (eid, n, rays, obs)
            assert got.shape == (B, n, rays) and got.dtype == torch.float32
            assert_bits_equal(_np(got), ref, what)
            assert torch.equal(env.lidar_scan(a, o, bodies=False), today), what  # and False is today's scan
            assert torch.equal(env.lidar_scan(a, o), today) and bits(_np(today)).tolist() == bits(a_obs).tolist()
            if n == 1:
                assert_bits_equal(ref, a_obs, what)  # no body to see
            elif rays >= 32:  # the scene bites: beams that return off a body, beams that do not
                body = R.body_alpha_ref(agent, tab, rho_of(env))
                in_the_open |= bool(((ref < a_obs) & (a_obs == NONE)).any())
                behind_a_wall |= bool(((body <= 1) & (a_obs < body)).any())
    assert n == 1 or (in_the_open and behind_a_wall)  # bodies in front of nothing, and walls in front of bodies


def adversarial_scene(env, n=8, obs=3):
    """One batch of 8 envs on a random scene whose obstacles are moved away from the cast (and turned: a beam parallel to
    an edge is the scan's documented NaN), each env with one hand-made property (asserted on the reference by the test)."""
    agent, goal, ob = random_scene(env, n, obs, seed=77, box=3.0)
    far = O.make_rectangles(np.full((obs, 2), 30.0), np.full(obs, 0.2), np.full(obs, 0.2), np.full(obs, 0.3)).astype(F)
    for b in (0, 1, 3, 4, 5, 6):
        ob[b] = far
    agent[0, 1, :2] = agent[0, 0, :2]  # 0: coincident agents
    agent[1, 1, :2] = agent[1, 0, :2] + F(0.03)  # 1: overlapping discs: the centre within rho
    ob[2, 0] = O.make_rectangles(np.array([[1.0, 1.0]]), np.array([0.4]), np.array([0.4]), np.array([0.3]))[0]
    agent[2, 0, :2] = (1.0, 1.0)  # 2: an agent inside a rectangle (its a_obs is 0) ...
    agent[2, 1, :2] = (1.35, 1.0)  # ... and one just outside, which sees the rectangle's face first
    agent[3, 2, 0] = np.nan  # 3: a NaN row
    agent[3, 0, :2], agent[3, 1, :2] = (0.5, 0.5), (0.7, 0.5)
    agent[4, 2, 1] = np.inf  # 4: an infinite row
    agent[4, 0, :2], agent[4, 1, :2] = (0.5, 0.5), (0.7, 0.5)
    agent[5, 0, :2], agent[5, 1, :2] = (0.5, 0.5), (0.85, 0.5)  # 5: a body exactly behind a wall
    ob[5, 0] = O.make_rectangles(np.array([[0.7, 0.5]]), np.array([0.02]), np.array([0.4]), np.array([0.1]))[0]
    agent[6, 0, :2], agent[6, 1, :2] = (0.25, 0.5), (0.35, 0.5)  # 6: discs that touch: cc is 0 or a rounding away
    return agent, goal, ob.astype(F)


def test_scan_matches_reference_on_the_adversarial_batch(cuda):
    n, rays = 8, 32
    env = lidar_env("LidarSpread", n, 3, rays, cuda)
    agent, _, ob = adversarial_scene(env)
    dev = dev_of(cuda)
    tab = _np(env._ray_table(cuda))
    a_obs = _np(env.lidar_scan(dev(agent), dev(ob)))
    body = R.body_alpha_ref(agent, tab, rho_of(env))
    ref = R.nearer_alpha_ref(a_obs, body)
    ahead = rays // 2
    assert tab[ahead, 0] == F(0.5) and abs(tab[ahead, 1]) < 1e-6  # the beam along +x
    assert (ref[0, :2] == 0).all() and (ref[1, :2] == 0).all()  # coincident and overlapping: every beam returns at 0
    assert (a_obs[2, 0] == 0).all() and (ref[2, 0] == 0).all()  # inside a rectangle: is_in zeroes the scan, bodies or not
    assert a_obs[2, 1, 0] < body[2, 1, 0] <= 1 and ref[2, 1, 0] == a_obs[2, 1, 0]  # and its face hides the agent inside
    for b in (3, 4):  # the broken row returns nothing, sees nothing, and the pair beside it is intact
        assert (body[b, 2] == NONE).all() and not np.isnan(body[b]).any()
        assert abs(float(ref[b, 0, ahead]) - 0.3) <= 1e-6 and abs(float(ref[b, 1, 0]) - 0.3) <= 1e-6
    assert body[5, 0, ahead] < 1 and a_obs[5, 0, ahead] < body[5, 0, ahead] and ref[5, 0, ahead] == a_obs[5, 0, ahead]
    assert (ref[6, :2] <= 1).any()
    assert_bits_equal(_np(env.lidar_scan(dev(agent), dev(ob), bodies=True)), ref, "adversarial")
    # a NaN a_obs stays NaN: an obstacle with a NaN corner
    ob2 = ob.copy()
    ob2[3, 0, 8] = np.nan
    a_obs2 = _np(env.lidar_scan(dev(agent), dev(ob2)))
    assert np.isnan(a_obs2[3]).any() and (body[3][np.isnan(a_obs2[3])] <= 1).any()
    assert_bits_equal(_np(env.lidar_scan(dev(agent), dev(ob2), bodies=True)), R.nearer_alpha_ref(a_obs2, body), "NaN wall")
    # a view of a rollout buffer: the per-env stride is the graph's, the rows are read in place
    buf = env.empty_graph((B,), cuda)
    buf.states[:, :n] = dev(agent)
    view = buf.states[:, :n]
    assert not view.is_contiguous()
    assert_bits_equal(_np(env.lidar_scan(view, dev(ob), bodies=True)), ref, "strided")


def test_opcheck_of_both_ops(cuda):
    env = lidar_env("LidarOmniTarget", 3, 3, 32, cuda)
    agent, goal, ob = (dev_of(cuda)(x) for x in random_scene(env, 3, 3, seed=5))
    h, rays = env._cfg_handle, env._ray_table(cuda)
    checks = ("test_schema", "test_faketensor")
    alpha = torch.empty(B, 3, 32, device=cuda)
    torch.ops.dgppo.lidar_scan_bodies(h, agent, ob, rays, alpha)
    assert torch.equal(alpha, env.lidar_scan(agent, ob, bodies=True))
    torch.library.opcheck(torch.ops.dgppo.lidar_scan_bodies.default, (h, agent, ob, rays, torch.empty_like(alpha)),
                          test_utils=checks)
    o = env.empty_graph((B,), cuda)
    key = torch.tensor([29], dtype=torch.int64, device=cuda)
    flags = 31
    torch.library.opcheck(torch.ops.dgppo.lidar_observe_bodies.default,
                          (h, agent, goal, ob, rays, key, 0, 0, 2, 0.1, -0.8, flags, 60.0, o.nodes, o.edges, o.states,
                           o.receivers, o.senders), test_utils=checks)
    for op in (torch.ops.dgppo.lidar_observe_fov,):  # the older ops keep refusing the new flag
        with pytest.raises(ValueError, match="DGPPO_EINVAL"):
            op(h, agent, goal, ob, rays, key, 0, 0, 2, 0.1, -0.8, flags, 60.0, o.nodes, o.edges, o.states, o.receivers,
               o.senders)
    for op in (torch.ops.dgppo.lidar_observe, torch.ops.dgppo.lidar_observe_los):
        with pytest.raises(ValueError, match="DGPPO_EINVAL"):
            op(h, agent, goal, ob, rays, key, 0, 0, 2, 0.1, -0.8, 16, o.nodes, o.edges, o.states, o.receivers, o.senders)


# ---- 2. the fused observe ---------------------------------------------------------------------------------------------
OFF, T_OBS, SEED = 3, 2, 11
_OBSERVE = {}


def observe_scene(cuda, eid, n):
    if (eid, n) not in _OBSERVE:
        env = lidar_env(eid, n, 3, 32, cuda)
        host = random_scene(env, n, 3, seed=31 * n + len(eid))
        _OBSERVE[eid, n] = (env, tuple(dev_of(cuda)(x) for x in host), host)
    return _OBSERVE[eid, n]


def chain(env, state, sigma, dropout, occ, fov):
    """The definition on the whole batch: row b draws at row b of the noise streams."""
    agent, goal, ob = state
    model = LidarNoise(sigma, dropout, SEED, sense_range=float(env.params["comm_radius"]))
    alpha = model(env.lidar_scan(agent, ob, bodies=True), T_OBS)
    g = env.get_graph(state, lidar_data=env.lidar_hits(agent, alpha))
    if occ or fov is not None:
        vis = env.line_of_sight(agent, ob) if occ else None
        if fov is not None:
            cone = env.field_of_view(agent, fov)
            vis = cone if vis is None else vis & cone
        mask_unseen(g, vis)
    return g


@pytest.mark.parametrize("eid,n", cases([1, 3, 8]))
def test_observe_with_bodies_is_the_chain(cuda, eid, n):
    env, state, host = observe_scene(cuda, eid, n)
    tail = tuple(x[OFF:] for x in state)
    key = torch.tensor([SEED], dtype=torch.int64, device=cuda)
    for sigma in (0.0, 0.05):
        for dropout in (0.0, 0.2):
            for occ in (False, True):
                for fov in ((None, 60.0) if eid in HEADING else (None,)):
                    what = (eid, n, sigma, dropout, occ, fov)
                    want = chain(env, state, sigma, dropout, occ, fov)
                    kw = dict(sigma=sigma, dropout=dropout, occlusion=occ, fov=fov, bodies=True)
                    assert_same_graph(env.observe(state, T_OBS, seed=SEED, **kw), want, what)
                    # a non-zero env_offset and a tensor seed: rows OFF.. of the same streams
                    got = env.observe(tail, T_OBS, seed=key, env_offset=OFF, **kw)
                    for f in FIELDS:
                        x, y = getattr(got, f), getattr(want, f)[OFF:]
                        assert bool(((x == y) | ((x != x) & (y != y))).all()), (what, f, "offset")
                    plain = env.observe(state, T_OBS, seed=SEED, **dict(kw, bodies=False))
                    if n > 1:  # and the keyword matters: hit rows moved onto bodies
                        assert not torch.equal(plain.states, want.states), what
                    else:
                        assert_same_graph(plain, want, what)
    # out= the graph whose own state rows are the argument: every input is staged before the first store
    kw = dict(sigma=0.05, dropout=0.2, seed=SEED, occlusion=True, bodies=True)
    ref = env.observe(state, T_OBS, **kw)
    live = env.get_graph(state)
    for f in ("nodes", "edges", "receivers", "senders"):
        getattr(live, f).fill_(-7)
    got = env.observe(live.env_states, T_OBS, out=live, **kw)
    assert got.states.data_ptr() == live.states.data_ptr()
    assert_same_graph(got, ref, (eid, n, "in place"))


def test_observe_scenes_hide_neighbours_that_bodies_still_show(cuda):
    """Non-vacuity of the scenes above, on the reference: in-range pairs are hidden by the cone, and the draws depend
    on env_offset."""
    env, state, host = observe_scene(cuda, "LidarOmniTarget", 8)
    a = env.observe(state, T_OBS, sigma=0.05, dropout=0.2, seed=SEED, fov=60.0, occlusion=True, bodies=True)
    b = env.observe(state, T_OBS, sigma=0.05, dropout=0.2, seed=SEED, bodies=True)
    assert not torch.equal(a.receivers, b.receivers)
    c = env.observe(state, T_OBS, sigma=0.05, dropout=0.2, seed=SEED, bodies=True, env_offset=4)
    assert not torch.equal(b.states, c.states)
    body = R.body_alpha_ref(host[0], _np(env._ray_table(cuda)), rho_of(env))
    assert (body <= 1).any(-1).all(-1).any()  # an env every agent of which has a body in range


# ---- 3. a body hit becomes a hit row ------------------------------------------------------------------------------------
def test_a_body_return_becomes_a_hit_row_with_an_edge(cuda):
    n, rays = 2, 32
    env = make_env("LidarSpread", n, num_obs=1, device=cuda)
    k, ng, pad = int(env.params["top_k_rays"]), env.num_goals, env.n_nodes - 1
    agent = np.zeros((1, n, 4), F)
    agent[0, 0, :2], agent[0, 1, :2] = (0.5, 0.5), (0.7, 0.5)  # 0.2 apart in the open
    goal = np.zeros((1, ng, 4), F)
    goal[..., :2] = 1.0
    ob = O.make_rectangles(np.array([[30.0, 30.0]]), np.array([0.2]), np.array([0.2]), np.array([0.3]))[None].astype(F)
    dev = dev_of(cuda)
    state = (dev(agent), dev(goal), dev(ob))
    tab = _np(env._ray_table(cuda))
    ref = R.scan_bodies_ref(np.full((1, n, rays), NONE, F), agent, tab, rho_of(env))
    assert int((ref[0, 0] <= 1).sum()) == 3 and abs(float(ref[0, 0, rays // 2]) - 0.3) <= 1e-6
    seen = env.observe(state, 0, sigma=0.0, dropout=0.0, seed=1, bodies=True)
    blind = env.observe(state, 0, sigma=0.0, dropout=0.0, seed=1)
    hit0, edge0 = n + ng, env.n_edges - n * k  # agent 0's first hit row and its edge
    # the nearest return is the beam dead ahead: start + (end - start) * alpha
    a = ref[0, 0, rays // 2]
    end = F(0.5) + tab[rays // 2]
    want = (F(0.5) + (end - F(0.5)) * a).astype(F)
    assert_bits_equal(_np(seen.states[0, hit0, :2]), want, "hit point")
    assert abs(float(want[0]) - 0.65) <= 1e-6 and abs(float(want[1]) - 0.5) <= 1e-6
    assert int(seen.receivers[0, edge0]) == 0 and int(seen.senders[0, edge0]) == hit0
    assert int((seen.receivers[0, edge0:edge0 + k] != pad).sum()) == 3  # the three beams that meet the body
    assert int(seen.receivers[0, edge0 + k]) == 1 and int(seen.senders[0, edge0 + k]) == hit0 + k  # and agent 1 sees 0
    # the obstacle-hit node type, a position only: no identity, no velocity
    assert torch.equal(seen.nodes[0, hit0, :2], seen.states[0, hit0, :2])
    assert torch.equal(seen.nodes[0, hit0, 2:], blind.nodes[0, hit0, 2:]) and bool((seen.states[0, hit0, 2:] == 0).all())
    assert bool((blind.receivers[0, edge0:] == pad).all()) and bool((blind.senders[0, edge0:] == pad).all())
    # the true graph is untouched by the option
    assert_same_graph(env.get_graph(state), blind, "get_graph")


# ---- 4. the engines -------------------------------------------------------------------------------------------------------
T, EB, EN = 4, 4, 3
_ENGINE = {}


def engine_setup(cuda):
    if not _ENGINE:
        env = make_env("LidarSpread", EN, num_obs=2, max_step=T, device=cuda)
        algo = make_algo("dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                         action_dim=env.action_dim, n_agents=EN, batch_size=EB * T, rnn_step=2, seed=2, device=cuda)
        host = random_scene(env, EN, 2, seed=9, nb=EB, box=0.8)
        host[0][..., 2:] = 0  # at rest
        _ENGINE["x"] = (env, algo.actor, tuple(dev_of(cuda)(x) for x in host))
    return _ENGINE["x"]


def run_definition(cuda, sigma, dropout, key, bodies=True, noise=True):
    env, actor, sc = engine_setup(cuda)
    sensor = LidarNoise(sigma, dropout, key, sense_range=float(env.params["comm_radius"])) if noise else None
    eng = SensorRolloutEngine(env, EB, T, cuda, actor=actor, mode=RolloutEngine.MODE_DET, sensor=sensor,
                              init_state=tuple(x.clone() for x in sc), **({"bodies": True} if bodies else {}))
    eng.run(key)
    out = outputs(eng)
    out.update({"seen_" + f: getattr(eng.observed, f).clone() for f in FIELDS})
    return out


def run_noisy(cuda, sigma, dropout, key, capture):
    env, actor, sc = engine_setup(cuda)
    eng = NoisyLidarRolloutEngine(env, EB, T, cuda, actor=actor, mode=RolloutEngine.MODE_DET, sigma=sigma,
                                  dropout=dropout, init_state=tuple(x.clone() for x in sc), bodies=True)
    if capture:
        eng.capture()
    eng.run(key)
    out = outputs(eng)
    out.update({"seen_" + f: getattr(eng.observed, f)[:, :T].clone() for f in FIELDS})
    return out, eng


@pytest.mark.parametrize("sigma,dropout", [(0.0, 0.0), (0.05, 0.2)])
def test_engines_agree_and_the_truth_follows_the_actions_only(cuda, sigma, dropout):
    env, actor, sc = engine_setup(cuda)
    ref = run_definition(cuda, sigma, dropout, 7)
    for capture in (False, True):
        got, eng = run_noisy(cuda, sigma, dropout, 7, capture)
        assert eng.bodies is True
        assert_outputs_equal(got, ref, f"bodies on, captured {capture}")
        s = eng.buf.states[T]  # obs[T]: the observation of the final true state
        last = env.observe((s[:, :EN], s[:, EN:EN + env.num_goals], sc[2]), T, sigma=sigma, dropout=dropout, seed=7,
                           bodies=True)
        for f in FIELDS:
            assert torch.equal(getattr(eng.observed, f)[:, T], getattr(last, f)), f
    if sigma == 0 and dropout == 0:  # sensor=None means identity once the flag is on
        assert_outputs_equal(run_definition(cuda, sigma, dropout, 7, noise=False), ref, "sensor None")
    # the flag matters: the observed hit rows differ from the run without it
    off = run_definition(cuda, sigma, dropout, 7, bodies=False)
    assert not torch.equal(off["seen_states"], ref["seen_states"])
    # the true rollout replayed from the recorded actions: the truth depends on the observation through them only
    replay = RolloutEngine(env, EB, T, cuda, mode=RolloutEngine.MODE_RANDOM, init_state=tuple(x.clone() for x in sc))
    replay.actions.copy_(ref["actions"])
    replay.run(0)
    assert_outputs_equal(outputs(replay), ref, "replayed actions", FIELDS + ("rewards", "costs"))


# ---- 5. training ----------------------------------------------------------------------------------------------------------
TT, TB, KEY = 4, 8, 5


def train_setup(cuda, n, **flags):
    env = make_env("LidarSpread", n, num_obs=2, max_step=TT, device=cuda)
    return env, make_algo("dgppo", env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                          action_dim=env.action_dim, n_agents=n, batch_size=TB * TT, rnn_step=2, seed=2, device=cuda,
                          **flags)


def test_training_with_bodies(cuda):
    env, algo = train_setup(cuda, 3, lidar_bodies=True)
    assert algo.bodies is True and algo.sensed and algo.sensing is None
    before = {k: v.clone() for k, v in algo.params.items()}
    roll = algo.collect(algo.params, KEY, n_env=TB)
    eng = algo._engine(TB, RolloutEngine.MODE_SAMPLE)
    assert isinstance(eng, NoisyLidarRolloutEngine) and eng.bodies is True and (eng.sigma, eng.dropout) == (0.0, 0.0)
    true = eng.rollout()
    assert torch.equal(roll.rewards, true.rewards) and torch.equal(roll.costs, true.costs)
    for f in ("receivers", "senders"):  # agent-agent and agent-goal edges are the true ones: only hits can differ
        first = env.n_edges - 3 * int(env.params["top_k_rays"])
        assert torch.equal(getattr(roll.graph, f)[..., :first], getattr(true.graph, f)[..., :first]), f
    info = algo.update(roll, 0)
    assert info and all(bool(torch.as_tensor(v).double().isfinite().all()) for v in info.values()), info
    for k in algo.NETS:
        assert bool(torch.isfinite(algo.params[k]).all()) and not torch.equal(algo.params[k], before[k]), k


def test_training_alone_in_the_arena_is_training_without_the_flag(cuda):
    """n = 1: no body exists to see, so two collect + update rounds give the parameter bits of lidar_noise=0.0."""
    _, on = train_setup(cuda, 1, lidar_bodies=True)
    _, off = train_setup(cuda, 1, lidar_noise=0.0)
    assert on.bodies and not off.bodies and on.sensed and off.sensed
    for algo in (on, off):
        for step in range(2):
            algo.update(algo.collect(algo.params, KEY + step, n_env=TB), step)
    for k in on.NETS:
        assert bool(torch.isfinite(on.params[k]).all()) and torch.equal(on.params[k], off.params[k]), k


# ---- 6. the CLI -----------------------------------------------------------------------------------------------------------
def test_cli_tests_with_bodies(cuda, tmp_path, monkeypatch, capsys):
    from test_train_gpu import _entry

    test_py, train_py = _entry("test"), _entry("train")
    eid = "LidarSpread"
    argv = ["train.py", "--env", eid, "-n", "3", "--algo", "dgppo", "--obs", "2", "--steps", "2", "--n-env-train", "8",
            "--batch-size", "256", "--n-env-test", "4", "--eval-interval", "1", "--save-interval", "2", "--log-dir",
            str(tmp_path), "--lidar-bodies"]
    monkeypatch.setattr(sys, "argv", argv)
    train_py.main()
    (run,) = glob.glob(os.path.join(str(tmp_path), eid, "dgppo", "seed0_*"))
    import json

    import yaml

    with open(os.path.join(run, "config.yaml")) as f:
        cfg = {}
        for d in yaml.safe_load_all(f):
            cfg.update(d or {})
    assert cfg["lidar_bodies"] is True and cfg["lidar_noise"] is None
    with open(os.path.join(run, "train_args.json")) as f:
        assert json.load(f)["lidar_bodies"] is True
    with pytest.raises(SystemExit, match="lidar_bodies"):  # --resume without it is refused
        train_py.check_resume_args(train_py.build_parser().parse_args(argv[1:-1]), run, world=1)
    capsys.readouterr()
    for extra in ([], ["--lidar-bodies"], ["--lidar-bodies", "--lidar-occlusion", "--lidar-noise", "0.05"]):
        monkeypatch.setattr(sys, "argv", ["test.py", "--path", run, "--epi", "4", "--max-step", "6"] + extra)
        res = test_py.main()
        out = capsys.readouterr().out
        assert set(res) == {"reward", "cost", "safe_rate"} and all(np.isfinite(v) for v in res.values())
        assert (", lidar bodies: on" in out) == ("--lidar-bodies" in extra) and out.count("epi: ") == 4
        assert ("lidar noise: 0.05" in out) == ("--lidar-noise" in extra)
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", run, "--epi", "4", "--env", "MPESpread", "--lidar-bodies"])
    with pytest.raises(SystemExit, match="no LiDAR"):
        test_py.main()
