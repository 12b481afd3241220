"""The persistent env rollout kernels (dgppo_env_rollout: the Lidar wave kernel at 1 / 4 / 8 envs per workgroup, the
MPE wave kernel, the workgroup-per-env kernel at every SizeTag, the REBUILD-then-block route) against the NumPy oracle
chain, every field of every step bit for bit.  The cases are env_cases.CASES; each asserts through
ops.env_rollout_plan that it takes the route written next to it before it launches, runs in buffers with guard envs
and guard steps around the used slice (prefilled with a sentinel that must come back bit-identical: the waves past
the last env store nothing), and restores the WPG / step-kernel selectors.  The captured replay (f) is the one
exception to the guards: a RolloutEngine owns its buffers, which have no room around them."""
import functools

import numpy as np
import pytest
import torch

from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.trainer.rollout import RolloutEngine
from env_cases import (ADV_B, ADV_SEED, AUTO_WPG, FULL_LISTS_KEY, CASES, GRAPH_FIELDS, LIDAR_IDS, _np,
                       adversarial_chain_inputs, assert_case_plan, assert_chain_equal, case_tensors, chain_actions,
                       forced, full_lists_inputs, host_buffers, oracle_chain, plan_of)
from oracle import env as O

pytestmark = pytest.mark.gpu
KEY = 31


def _third(spec, third):
    return None if spec.engine == O.ENGINE_MPE else third


@functools.lru_cache(maxsize=None)
def _reset_chain(eid, n, obs, B, T, kind, key=KEY, env_offset=0):
    """Oracle reset + chain of a "reset" scene (shared by the cases that differ only in WPG / the way into graph 0;
    read-only)."""
    spec = O.Spec(eid, n, obs)
    ag, gl, third = O.env_reset(spec, key, B, env_offset)
    g0 = O.initial_graph(spec, ag, gl, third)
    acts = _actions(spec, T, B, kind)
    return g0, third, acts, oracle_chain(spec, g0["states"], _third(spec, third), acts)


def _actions(spec, T, B, kind):
    a = chain_actions(spec, T, B, seed=5)
    if kind == "uniform+nan+inf":
        a[2, 1, 0, 0] = np.nan
        a[5, 2, spec.n - 1, 1] = np.inf
    return a


def _assert_graph0(got, g0, what):
    for f in GRAPH_FIELDS:
        a, b = got[f][0], g0[f]
        same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
        assert same.all(), f"{what}: graph 0 {f} differs from O.initial_graph at {np.argwhere(~same)[0]}"


def _launch(name, case, env, rb, ob, acts, rebuild):
    """Assert the route through the plan, then the one dgppo_env_rollout call."""
    pl = plan_of(env, rb.buf, ob, acts, rb.rewards, rb.costs, rebuild)
    assert_case_plan(name, case, pl)
    env.rollout_into(rb.buf, ob, acts, rb.rewards, rb.costs, rebuild_first=rebuild)
    torch.cuda.synchronize()


def _run_reset_case(name, cuda):
    case = CASES[name]
    env = make_env(case.eid, case.n, num_obs=case.obs, device=cuda)
    g0, third, a, chain = _reset_chain(case.eid, case.n, case.obs, case.B, case.T, case.actions)
    with forced(case.wpg, case.mode):
        rb, ob, _ = case_tensors(env, case, cuda)
        acts = torch.from_numpy(a).to(cuda)
        if case.rebuild:  # states-only reset where the wave kernels take graph 0 (else the full reset)
            env.reset_states(KEY, n_env=case.B, out=rb.graph0(), obstacles_out=ob)
        else:
            env.reset(KEY, n_env=case.B, out=rb.graph0(), obstacles_out=ob)
        _launch(name, case, env, rb, ob, acts, case.rebuild)
    got = rb.host()
    _assert_graph0(got, g0, name)
    assert_chain_equal(got, chain, name)
    rb.assert_guards_untouched(name)


A_CASES = [k for k in CASES if k.startswith("a-")]
B_CASES = [k for k in CASES if k.startswith("b-")]
D_RESET_CASES = [k for k in CASES if k.startswith("d-") and CASES[k].scene == "reset"]


@pytest.mark.parametrize("name", A_CASES)
def test_every_lidar_wave_instantiation(cuda, name):
    """(a) 4 Lidar env types x WPG 1 / 4 / 8, B = 19 (two full workgroups of 8 plus 3 live waves; a partial workgroup
    at WPG 4 too), T = 33 (two action chunks plus one step), states-only reset + rebuild_first and full reset."""
    _run_reset_case(name, cuda)


@pytest.mark.parametrize("name", B_CASES)
def test_episode_lengths(cuda, name):
    """(b) the default 128-step episode (8 action chunks) and the chunk edges T = 1 / 15 / 16 / 17 / 32."""
    _run_reset_case(name, cuda)


@pytest.mark.parametrize("name", D_RESET_CASES)
def test_other_persistent_kernels(cuda, name):
    """(d) env_rollout_block_kernel at every SizeTag (staged and prefetched actions), mpe_rollout_wave_kernel for both
    goals, and the REBUILD launch before the block kernel (per-step edge stride 4 k + 2 floats); actions with one
    NaN and one inf."""
    _run_reset_case(name, cuda)


# ---- (c) adversarial scenes ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _adversarial_chain(eid):
    """Scene and oracle chain of the adversarial rollout, from the GPU env's own reset arrays (read-only)."""
    cuda = torch.device("cuda:0")
    env = make_env(eid, 8, num_obs=3, device=cuda)
    spec = O.Spec(eid, 8, 3)
    g = env.reset(key=ADV_SEED, n_env=ADV_B)
    st = _np(g.states)
    agent, goal, ob, acts = adversarial_chain_inputs(spec, st[:, :8], st[:, 8:16], _np(g.env_states.obstacle.packed))
    with np.errstate(all="ignore"):
        g0 = O.initial_graph(spec, agent, goal, ob)
    return agent, goal, ob, acts, g0, oracle_chain(spec, g0["states"], ob, acts)


def _run_scene_case(name, cuda, agent, goal, ob_np, a, g0, chain):
    case = CASES[name]
    env = make_env(case.eid, case.n, num_obs=case.obs, device=cuda)
    n = case.n
    with forced(case.wpg, case.mode):
        rb, _, _ = case_tensors(env, case, cuda)
        ob = torch.from_numpy(ob_np).to(cuda)
        acts = torch.from_numpy(a).to(cuda)
        if case.rebuild:  # the agent / goal rows as a states-only reset leaves them
            rb.buf.states[0][:, :n].copy_(torch.from_numpy(agent))
            rb.buf.states[0][:, n:2 * n].copy_(torch.from_numpy(goal))
        else:
            env.get_graph((torch.from_numpy(agent).to(cuda), torch.from_numpy(goal).to(cuda), ob), out=rb.graph0())
        _launch(name, case, env, rb, ob, acts, case.rebuild)
    got = rb.host()
    _assert_graph0(got, g0, name)
    assert_chain_equal(got, chain, name)
    rb.assert_guards_untouched(name)


C_CASES = [k for k in CASES if CASES[k].scene == "adversarial"]


@pytest.mark.parametrize("name", C_CASES)
def test_adversarial_scenes_through_the_persistent_kernels(cuda, name):
    """(c), and (d)'s block kernel: 256 envs of kinds b % 8 (a workgroup of 8 holds one of each: the NaN-corner /
    far-obstacle env, whose every triple is cast, next to the tiny-obstacle env), T = 6 with NaN actions at t = 0 and
    t = 3, inf and -1e30 at t = 4; graph 0 through get_graph (loaded) and from rows written into states[0]
    (rebuild_first)."""
    agent, goal, ob, acts, g0, chain = _adversarial_chain(CASES[name].eid)
    _run_scene_case(name, cuda, agent, goal, ob, acts, g0, chain)


def test_item_list_at_capacity_beside_empty_lists(cuda):
    """(c) WPG 8: workgroup 0's eight envs keep every (agent, obstacle, ray) triple (8 x 768 pooled items: the list
    at capacity), workgroup 1's envs have small eligible obstacles no ray reaches (no items)."""
    name = "c-LidarSpread-w8-full-lists"
    case = CASES[name]
    spec = O.Spec(case.eid, 8, 3)
    ag, gl, ob, a = full_lists_inputs(spec, *O.env_reset(spec, FULL_LISTS_KEY, case.B))
    assert a.shape[:2] == (case.T, case.B)
    with np.errstate(all="ignore"):
        g0 = O.initial_graph(spec, ag, gl, ob)
    _run_scene_case(name, cuda, ag, gl, ob, a, g0, oracle_chain(spec, g0["states"], ob, a))


# ---- (e) the automatic threshold ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(AUTO_WPG))
def test_automatic_wpg_threshold(cuda, name):
    """(e) nothing forced: 2049 envs run 8 envs per workgroup (grid 257, one live wave in the last), 2047 run 4.
    Against the step kernel (RolloutEngine(fused=False)) for every env, and the oracle chain for the first and last
    32 envs."""
    case = CASES[name]
    B, T = case.B, case.T
    env = make_env(case.eid, 8, num_obs=3, device=cuda)
    spec = O.Spec(case.eid, 8, 3)
    a = chain_actions(spec, T, B, seed=5)
    acts = torch.from_numpy(a).to(cuda)
    ref = RolloutEngine(env, B, T, cuda, fused=False)
    ref.actions.copy_(acts)
    ref.run(key=KEY)
    with forced(0, 0):
        rb, ob, _ = case_tensors(env, case, cuda)
        env.reset_states(KEY, n_env=B, out=rb.graph0(), obstacles_out=ob)
        pl = plan_of(env, rb.buf, ob, acts, rb.rewards, rb.costs, True)
        assert_case_plan(name, case, pl)
        assert (pl.wpg, pl.grid) == ((8, 257) if B == 2049 else (4, 512))
        env.rollout_into(rb.buf, ob, acts, rb.rewards, rb.costs, rebuild_first=True)
        torch.cuda.synchronize()
    for f in GRAPH_FIELDS:
        assert torch.equal(getattr(rb.buf, f), getattr(ref.buf, f)), f
    assert torch.equal(rb.rewards, ref.rewards) and torch.equal(rb.costs, ref.costs)
    got = rb.host()
    for lo in (0, B - 32):
        ag, gl, third = O.env_reset(spec, KEY, 32, env_offset=lo)
        g0 = O.initial_graph(spec, ag, gl, third)
        part = {f: v[:, lo:lo + 32] for f, v in got.items()}
        _assert_graph0(part, g0, f"{name} envs {lo}..")
        assert_chain_equal(part, oracle_chain(spec, g0["states"], third, a[:, lo:lo + 32]), f"{name} envs {lo}..")
    rb.assert_guards_untouched(name)


# ---- (f) capture ----------------------------------------------------------------------------------------------------
def test_captured_rollout_replays_match_their_own_reset(cuda):
    """(f) case a-LidarSpread-w8 captured into a hipGraph (RolloutEngine.capture) and replayed with two keys: each
    replay equals the oracle chain of its own reset.  (The engine's own buffers: no guard regions here; the same
    launch runs guarded as case a-LidarSpread-w8-rebuild.)"""
    case = CASES["a-LidarSpread-w8-rebuild"]
    env = make_env(case.eid, 8, num_obs=3, device=cuda)
    with forced(8, 0):
        eng = RolloutEngine(env, case.B, case.T, cuda, fused=True)
        a = _actions(O.Spec(case.eid, 8, 3), case.T, case.B, case.actions)
        eng.actions.copy_(torch.from_numpy(a))
        pl = plan_of(env, eng.buf, eng.obstacles, eng.actions, eng.rewards, eng.costs, True)
        assert_case_plan("a-LidarSpread-w8-rebuild", case, pl)
        eng.capture()
        for key in (KEY, 1234):
            eng.run(key=key)
            torch.cuda.synchronize()
            g0, _, _, chain = _reset_chain(case.eid, 8, 3, case.B, case.T, case.actions, key=key)
            got = host_buffers(eng.buf, eng.rewards, eng.costs)
            _assert_graph0(got, g0, f"replay key {key}")
            assert_chain_equal(got, chain, f"replay key {key}")


def test_case_table_is_complete():
    """Every case of env_cases.CASES is run by exactly one test above."""
    ran = (set(A_CASES) | set(B_CASES) | set(D_RESET_CASES) | set(C_CASES) | set(AUTO_WPG) |
           {"c-LidarSpread-w8-full-lists"})
    assert ran == set(CASES) and set(LIDAR_IDS) == {CASES[k].eid for k in A_CASES}
