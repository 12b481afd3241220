"""dgppo_env_rollout_plan, the host dispatch of dgppo_env_rollout, checked without a GPU: the route rule restated in
Python over a sweep of configs, sizes, alignments and selectors; the two read-once environment knobs in child
processes; the coverage of the GPU case table (env_cases.CASES, run by test_rollout_oracle_gpu.py) against what the
sweep reaches; negative controls for env_cases.assert_chain_equal; and the adversarial chain on the oracle alone."""
import ctypes
import functools
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dgppo_fov_amd import _lib
from dgppo_fov_amd.env import ENV, make_env
from env_cases import (ADV_B, ADV_SEED, ADV_T, CASES, FULL_LISTS_KEY, LIDAR_IDS, adversarial_chain_inputs,
                       assert_case_plan, assert_chain_equal, case_tensors, chain_actions, first_chain_mismatch, forced,
                       full_lists_inputs, oracle_chain, plan_key, plan_of)
from oracle import env as O

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = _lib.DGPPO_EINVAL
LIDAR, BICYCLE, MPE, OMNI = (_lib.DGPPO_ENGINE_LIDAR, _lib.DGPPO_ENGINE_BICYCLE, _lib.DGPPO_ENGINE_MPE,
                             _lib.DGPPO_ENGINE_OMNI)
LDS_MAX, K_ACT_STAGE = 160 * 1024, 4096
BASE = 0x7F0000100000  # a 16-byte aligned fake address: the plan never dereferences


# ---- the kernels' LDS carves, restated (csrc/env_step.hip) ------------------------------------------------------
def _r4(x):
    return (x + 3) & ~3


@functools.lru_cache(maxsize=None)
def block_carve(n, sd, O_, R, k, lidar):
    """Carve::total (floats) of the workgroup-per-env kernels."""
    dist_n = max(2 * n * n + n * max(k, O_), 256)
    parts = [2 * n * sd + (0 if lidar else O_ * sd), n * k * 2 if lidar else 0, O_ * 16 if lidar else 0,
             O_ * 8 if lidar else 0, n * 2, n * sd, n * R * 2 if lidar else 0, n * R * 2 if lidar else 0,
             n * k * 2 if lidar else 0, n, 5 * n, 4 * n, dist_n,
             _r4(2 * O_ + 4 + n * R) + 4 * R if lidar else 0]
    return sum(_r4(p) for p in parts)


def wave_carve(sd):
    """wv::Carve<SD, 3>::total (floats): per-wave carve of the Lidar wave kernels (n = 8, 32 rays, top-8)."""
    nxt = 16 * sd
    obst = nxt + _r4(8 * sd)
    uni = obst + 3 * 16 + 3 * 8 + 2 * 32 + 8 * 32 + 8 * 8 * 2 + 8 * 32
    return _r4(uni + max(8 * 3 * 32 + 64, 8 * (2 * 32 + 4)))


ROLLOUT_ACT_FLOATS = 16 * 8 * 3  # wv::kRolloutActFloats: a 16-step action chunk per wave
MPE_WAVE_FLOATS = 48 + 32 * 2 * 3  # wv::mpew::TOTAL: carve + a 32-step action chunk


def size_tag(c):
    """visit_sizes: compile-time sizes for the BASELINE configs, else run-time sizes at 256 or 128 threads."""
    n, o = c.n_agents, c.n_obs
    if c.engine == MPE:
        return (64, 3, 3, 0, 0) if (n, o) == (3, 3) else ((64, 3, 0, 0, 0) if (n, o) == (3, 0) else (64, 0, -1, 0, 0))
    if (c.n_rays, c.top_k) == (32, 8) and (n, o) in ((8, 3), (32, 8)):
        return (256, n, o, 32, 8)
    return (256, 0, -1, 0, 0) if n * c.n_rays >= 256 else (128, 0, -1, 0, 0)


def step_launch(c, wave0, n_env):
    """One dgppo_env_step launch: (threads, grid, LDS bytes) or EINVAL."""
    lidar = c.engine != MPE
    if c.variant != 0:
        lds = 4 * (block_carve(c.n_agents, 4, c.n_obs, c.n_rays, c.top_k, lidar) + 10 * c.n_agents + 8)
        return EINVAL if lds > 64 * 1024 else (64, n_env, lds)
    if wave0:
        return 256, (n_env + 3) // 4, 16 * wave_carve(c.state_dim)
    cv = block_carve(c.n_agents, c.state_dim, c.n_obs, c.n_rays, c.top_k, lidar)
    if c.engine == OMNI:
        n, nh = c.n_agents, (c.n_agents * c.top_k if c.n_obs > 0 else 0)
        lds = 4 * (cv + _r4(3 * n) + _r4(n * n) + _r4(n * (nh + 1)) + 8 * n)
        return EINVAL if lds > 64 * 1024 else (256, n_env, lds)
    return size_tag(c)[0], n_env, 4 * cv


def expected_plan(c, r, wpg_forced, step_mode, block_rollout=True, mpe_wave=True):
    """The rule documented at dgppo_env_rollout / dgppo_env_rollout_plan (include/dgppo_hip.h), in the order the
    routes are tried.  c: a finalized EnvCfg, r: an EnvRolloutIO with every pointer set.  Returns EINVAL or a dict of
    the plan's fields."""
    io = r.step
    if r.T < 0 or io.n_env < 0:
        return EINVAL
    none = dict(route="NONE", wpg=0, size=None, stage=0, rebuild=0, threads=0, grid=0, lds=0, steps=0)
    if (r.T == 0 and not r.rebuild_first) or io.n_env == 0:
        return none

    def wave(t_edges, t_states, step=0):
        """The wave kernels' config and alignment for graph `step`'s buffers with these per-step strides."""
        q = 2 if c.engine == OMNI else 4
        edges, states = io.edges + 4 * step * r.t_edges, io.out_states + 4 * step * r.t_states
        e_ok = edges % (4 * q) == 0 and io.edges_stride % q == 0 and t_edges % q == 0
        s_ok = c.state_dim != 4 or (states % 16 == 0 and io.out_states_stride % 4 == 0 and t_states % 4 == 0)
        return (c.engine != MPE and c.variant == 0 and (c.n_agents, c.n_rays, c.top_k, c.n_obs) == (8, 32, 8, 3)
                and step_mode == 0 and e_ok and s_ok)

    n_env = io.n_env
    if wave(r.t_edges, r.t_states):
        w = wpg_forced or (8 if n_env >= 2048 else 4)
        return dict(none, route="LIDAR_WAVE", wpg=w, threads=64 * w, grid=-(-n_env // w),
                    lds=w * 4 * (wave_carve(c.state_dim) + ROLLOUT_ACT_FLOATS))
    rebuild = int(bool(r.rebuild_first) and wave(0, 0))
    if (block_rollout and mpe_wave and r.T > 0 and c.engine == MPE and c.variant == 0 and
            (c.n_agents, c.n_obs) == (3, 3) and step_mode == 0 and io.edges % 16 == 0 and io.edges_stride % 4 == 0
            and r.t_edges % 4 == 0):
        return dict(none, route="MPE_WAVE", wpg=4, threads=256, grid=(n_env + 3) // 4, lds=16 * MPE_WAVE_FLOATS,
                    rebuild=rebuild)
    if block_rollout and r.T > 0 and c.variant == 0 and c.engine != OMNI and c.n_agents <= 32:
        cv = block_carve(c.n_agents, c.state_dim, c.n_obs, c.n_rays, c.top_k, c.engine != MPE)
        act = r.T * 2 * c.n_agents
        stage = int(act <= K_ACT_STAGE and 4 * (cv + _r4(act)) <= 64 * 1024)
        tag = size_tag(c)
        return dict(none, route="BLOCK", size=tag, stage=stage, rebuild=rebuild, threads=tag[0], grid=n_env,
                    lds=4 * (cv + (_r4(act) if stage else 0)))
    out = dict(none, route="STEP_LOOP", rebuild=rebuild, steps=r.T)
    if r.T > 0:
        st = step_launch(c, wave(0, 0, step=1), n_env)  # the first step's launch: it writes graph 1
        if st == EINVAL:
            return EINVAL
        out.update(threads=st[0], grid=st[1], lds=st[2])
    return out


# ---- the sweep ------------------------------------------------------------------------------------------------------
ALIGNMENTS = {  # float offsets of (edges base, states base, edges stride, states stride, t_edges, t_states)
    "aligned": (0, 0, 0, 0, 0, 0), "edges+1": (1, 0, 0, 0, 0, 0), "edges+2": (2, 0, 0, 0, 0, 0),
    "states+1": (0, 1, 0, 0, 0, 0), "states+2": (0, 2, 0, 0, 0, 0), "estride+1": (0, 0, 1, 0, 0, 0),
    "estride+2": (0, 0, 2, 0, 0, 0), "sstride+1": (0, 0, 0, 1, 0, 0), "sstride+2": (0, 0, 0, 2, 0, 0),
    "t_edges+1": (0, 0, 0, 0, 1, 0), "t_edges+2": (0, 0, 0, 0, 2, 0), "t_states+1": (0, 0, 0, 0, 0, 1),
    "t_states+2": (0, 0, 0, 0, 0, 2),
}
NS, OBS = (1, 3, 4, 8, 32, 33), (0, 1, 2, 3, 8)
N_ENVS, TS = (0, 1, 7, 8, 9, 2047, 2048, 2049, 4096), (0, 1, 15, 16, 17, 128, 700)
SELECTORS = tuple(itertools.product((0, 1, 4, 8), (0, 1)))  # (forced WPG, step-kernel mode)


def _envs():
    """Every non-VMAS env id x n x n_obs the env classes accept (some force n_obs or refuse sizes), once each."""
    seen, out = set(), []
    for eid in (e for e in ENV if not e.startswith("VMAS")):
        for n, obs in itertools.product(NS, OBS):
            try:
                env = make_env(eid, n, num_obs=obs, device="cpu")
            except (ValueError, AssertionError):
                continue
            key = (eid, n, env.cfg.n_obs)
            if key not in seen:
                seen.add(key)
                out.append(env)
    return out


def fake_io(c, n_env, T, rebuild, align="aligned"):
    """A dgppo_env_rollout_io of time-major buffers at fake addresses with the wanted misalignment."""
    de, ds, dse, dss, dte, dts = ALIGNMENTS[align]
    r = _lib.EnvRolloutIO()
    io = r.step
    B = max(n_env, 1)
    rows = {"states": c.n_nodes * c.state_dim, "nodes": c.n_nodes * c.node_dim, "edges": c.n_edges * c.edge_dim,
            "index": c.n_edges, "action": c.n_agents * c.action_dim, "cost": c.n_agents * c.n_cost}
    for k, f in enumerate(("states", "obstacles", "action", "ray_dirs", "nodes", "edges", "out_states", "receivers",
                           "senders", "reward", "cost")):
        setattr(io, f, BASE + (k << 32))
    io.edges += 4 * de
    io.out_states += 4 * ds
    io.states = io.out_states
    io.states_stride = io.out_states_stride = rows["states"] + dss
    io.obstacles_stride, io.action_stride, io.nodes_stride = 16 * max(c.n_obs, 1), rows["action"], rows["nodes"]
    io.edges_stride, io.edge_index_stride = rows["edges"] + dse, rows["index"]
    io.reward_stride, io.cost_stride = 1, rows["cost"]
    return resize_io(r, n_env, T, rebuild, align)


def resize_io(r, n_env, T, rebuild, align):
    """Set fake_io's env count, T and rebuild_first (and the per-step strides that follow from them) in place."""
    dte, dts = ALIGNMENTS[align][4:]
    io, B = r.step, max(n_env, 1)
    io.n_env = n_env
    r.T, r.rebuild_first = T, rebuild
    r.t_states, r.t_nodes, r.t_edges = B * io.states_stride + dts, B * io.nodes_stride, B * io.edges_stride + dte
    r.t_index, r.t_action, r.t_reward, r.t_cost = B * io.edge_index_stride, B * io.action_stride, B, B * io.cost_stride
    return r


def _plan(c, r):
    pl = _lib.EnvRolloutPlan()
    rc = _lib.load().dgppo_env_rollout_plan(ctypes.byref(c), ctypes.byref(r), ctypes.byref(pl))
    return rc, pl


def _knob(name):
    """The read-once knobs as the library reads them: off only for a value that atoi() turns into 0."""
    v = os.environ.get(name)
    if v is None:
        return True
    digits = v.strip()
    sign = digits[:1] in "+-" and len(digits) > 1
    lead = "".join(itertools.takewhile(str.isdigit, digits[1:] if sign else digits))
    return bool(int(lead or "0"))


def _wave_shaped(env):
    c = env.cfg
    return (c.n_agents, c.n_obs) == ((3, 3) if c.engine == MPE else (8, 3))


THIN = ((2048,), (0, 17))  # n_env and T of the thin grid


def sweep(selectors=SELECTORS):
    """(env, r, align, (wpg, mode)) of the sweep.  The configs the wave kernels can take (Lidar n = 8 / 3 obstacles,
    MPE n = 3 / 3 obstacles, and the line variant of that size) get the full cross product.  Every other config
    crosses every alignment with every selector on a thin grid (n_env 2048, T 0 / 17, rebuild_first 0 / 1) --
    neither may change its plan, which is what this part shows -- and the full n_env x T x rebuild_first grid with
    three (alignment, selector) pairs."""
    rest = (("aligned", (0, 0)), ("t_edges+1", (1, 1)), ("states+2", (8, 0)))
    full = tuple(itertools.product(N_ENVS, TS, (0, 1)))
    thin = tuple(itertools.product(THIN[0], THIN[1], (0, 1)))
    for env in _envs():
        for align, sel in itertools.product(ALIGNMENTS, selectors):
            grid = full if _wave_shaped(env) or (align, sel) in rest else thin
            r = fake_io(env.cfg, 1, 1, 0, align)  # one struct per (config, alignment), resized in place
            for n_env, T, rebuild in grid:
                yield env, resize_io(r, n_env, T, rebuild, align), align, sel


def _check(env, r, pl, rc, want, what):
    if want == EINVAL:
        assert rc == EINVAL and pl.route_name == "NONE" and pl.grid == 0, what
        return
    got = dict(route=pl.route_name, wpg=pl.wpg, size=pl.size_tag, stage=pl.stage, rebuild=pl.rebuild,
               threads=pl.threads, grid=pl.grid, lds=pl.lds_bytes, steps=pl.step_launches)
    assert rc == 0 and got == want, (what, got, want)
    assert 0 <= pl.lds_bytes <= LDS_MAX, what
    n_env = r.step.n_env
    if pl.route_name in ("LIDAR_WAVE", "MPE_WAVE"):
        assert (pl.grid - 1) * pl.wpg < n_env <= pl.grid * pl.wpg and pl.threads == 64 * pl.wpg, what
    elif pl.route_name == "BLOCK":
        act = r.T * 2 * env.cfg.n_agents
        assert pl.grid == n_env and pl.threads == pl.size_block, what
        total = pl.lds_bytes + (0 if pl.stage else 4 * _r4(act))  # carve + the whole episode's actions
        assert pl.stage == int(act <= K_ACT_STAGE and total <= 64 * 1024), what


def run_sweep(selectors=SELECTORS, block_rollout=None, mpe_wave=None):
    """Check every sweep case against expected_plan; returns (coverage keys reached, routes counted, EINVALs)."""
    lib = _lib.load()
    block_rollout = _knob("DGPPO_ENV_BLOCK_ROLLOUT") if block_rollout is None else block_rollout
    mpe_wave = _knob("DGPPO_MPE_WAVE") if mpe_wave is None else mpe_wave
    keys, routes, refused = set(), {}, 0
    with forced(0, 0):
        last = None
        for env, r, align, sel in sweep(selectors):
            if sel != last:
                assert lib.dgppo_env_set_rollout_wpg(sel[0]) >= 0 and lib.dgppo_env_set_step_kernel(sel[1]) >= 0
                last = sel
            rc, pl = _plan(env.cfg, r)
            want = expected_plan(env.cfg, r, sel[0], sel[1], block_rollout, mpe_wave)
            _check(env, r, pl, rc, want, (type(env).__name__, env.cfg.n_agents, env.cfg.n_obs, r.step.n_env, r.T,
                                          r.rebuild_first, align, sel))
            if want == EINVAL:
                refused += 1
                continue
            keys.add(plan_key(env, pl))
            routes[pl.route_name] = routes.get(pl.route_name, 0) + 1
    return keys, routes, refused


KNOB_VARS = ("DGPPO_ENV_BLOCK_ROLLOUT", "DGPPO_MPE_WAVE", "DGPPO_ROLLOUT_WPG", "DGPPO_ENV_STEP_KERNEL")


def _child(expr, **knobs):
    """json of `expr` evaluated in this module (as m) in a fresh process whose environment has the four knob
    variables removed, then `knobs` set: the library reads them once per process."""
    code = (f"import sys, json; sys.path.insert(0, {os.path.dirname(HERE)!r}); sys.path.insert(0, {HERE!r}); "
            f"import test_env_rollout_plan_cpu as m; print(json.dumps({expr}))")
    env = {k: v for k, v in os.environ.items() if k not in KNOB_VARS}
    out = subprocess.run([sys.executable, "-c", code], env=dict(env, **knobs), capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()[-3000:]
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


def report():
    """The whole sweep, checked, and the coverage of the GPU case table (run in a child at the default knobs)."""
    keys, routes, refused = run_sweep()
    return dict(keys=sorted(_key_str(k) for k in keys), routes=routes, refused=refused, reached=case_table_keys())


@functools.lru_cache(maxsize=None)
def default_report():
    """report() at the default knobs, whatever this process was started with; shared by the two tests below."""
    return _child("m.report()")


def test_plan_sweep_follows_the_documented_rule():
    rep = default_report()  # every plan was held to expected_plan in the child; a mismatch fails it
    keys, routes, refused = [tuple(k.split(":")) for k in rep["keys"]], rep["routes"], rep["refused"]
    print(f"[env rollout plan] {sum(routes.values())} plans: {routes}, {refused} refused, {len(keys)} coverage keys")
    assert set(routes) == {"NONE", "LIDAR_WAVE", "MPE_WAVE", "BLOCK", "STEP_LOOP"}
    assert refused > 0  # LidarOmniTarget n = 33 with obstacles: the step kernel's LDS passes 64 KB
    assert {k[1] for k in keys if k[0] == "LIDAR_WAVE"} == {"wpg1", "wpg4", "wpg8"}
    assert any(k[0] == "BLOCK" and k[-1] == "rebuild1" for k in keys)
    assert any(k[0] == "STEP_LOOP" and k[-1] == "rebuild1" for k in keys)


def test_plan_refuses_what_the_rollout_refuses():
    lib = _lib.load()
    env = make_env("LidarSpread", 8, num_obs=3, device="cpu")
    c = env.cfg
    pl = _lib.EnvRolloutPlan()
    good = fake_io(c, 9, 17, 1)
    assert lib.dgppo_env_rollout_plan(ctypes.byref(c), ctypes.byref(good), None) == EINVAL
    assert lib.dgppo_env_rollout_plan(None, ctypes.byref(good), ctypes.byref(pl)) == EINVAL
    assert lib.dgppo_env_rollout_plan(ctypes.byref(c), None, ctypes.byref(pl)) == EINVAL
    for f, v in (("T", -1), ("n_env", -1)):
        r = fake_io(c, 9, 17, 1)
        setattr(r if f == "T" else r.step, f, v)
        assert _plan(c, r)[0] == EINVAL, f
    for f in ("states", "action", "nodes", "edges", "out_states", "receivers", "senders", "reward", "cost", "obstacles",
              "ray_dirs"):
        r = fake_io(c, 9, 17, 1)
        setattr(r.step, f, None)
        rc, pl = _plan(c, r)
        assert rc == EINVAL and pl.route_name == "NONE", f
        r.T, r.rebuild_first = 0, 0  # nothing to do comes before the pointer checks
        assert _plan(c, r)[0] == 0, f
    mpe = make_env("MPESpread", 3, num_obs=3, device="cpu").cfg
    r = fake_io(mpe, 9, 17, 0)
    r.step.obstacles = r.step.ray_dirs = None  # MPE reads neither
    assert _plan(mpe, r)[0] == 0
    bad = _lib.EnvCfg.from_buffer_copy(c)
    bad.n_agents = 65
    assert _plan(bad, good)[0] == EINVAL
    vm = make_env("VMASWheel", 3, device="cpu").cfg
    rc, pl = _plan(vm, fake_io(c, 9, 17, 0))
    assert rc == 0 and pl.route_name == "VMAS" and pl.grid == 0


def test_wpg_selector():
    lib = _lib.load()
    c = make_env("LidarSpread", 8, num_obs=3, device="cpu").cfg
    with forced(0, 0):
        for bad in (-1, 2, 3, 5, 16):
            assert lib.dgppo_env_set_rollout_wpg(bad) == EINVAL
        assert lib.dgppo_env_set_rollout_wpg(8) == 0
        assert _plan(c, fake_io(c, 9, 17, 1))[1].wpg == 8
        assert lib.dgppo_env_set_rollout_wpg(1) == 8
        assert _plan(c, fake_io(c, 4096, 17, 1))[1].wpg == 1
        assert lib.dgppo_env_set_rollout_wpg(0) == 1
        assert [_plan(c, fake_io(c, b, 17, 1))[1].wpg for b in (2047, 2048)] == [4, 8]


# ---- the read-once knobs, one child each --------------------------------------------------------------------------
def knob_probe():
    """Routes of three configs (run in a child process with a knob set)."""
    out = {}
    for eid, n, obs in (("LidarSpread", 8, 3), ("LidarSpread", 4, 2), ("MPESpread", 3, 3)):
        c = make_env(eid, n, num_obs=obs, device="cpu").cfg
        rc, pl = _plan(c, fake_io(c, 9, 17, 1))
        out[f"{eid}-{n}"] = [rc, pl.route_name, pl.size_tag, pl.step_launches]
    keys, routes, _ = run_sweep(selectors=((0, 0),))  # the rule holds under the knob too
    out["routes"] = sorted(routes)
    return out


_WAVE8 = [0, "LIDAR_WAVE", None, 0]


@pytest.mark.parametrize("knob,want", [
    ("DGPPO_ENV_BLOCK_ROLLOUT", {"LidarSpread-8": _WAVE8, "LidarSpread-4": [0, "STEP_LOOP", None, 17],
                                 "MPESpread-3": [0, "STEP_LOOP", None, 17],
                                 "routes": ["LIDAR_WAVE", "NONE", "STEP_LOOP"]}),
    ("DGPPO_MPE_WAVE", {"LidarSpread-8": _WAVE8, "LidarSpread-4": [0, "BLOCK", [128, 0, -1, 0, 0], 0],
                        "MPESpread-3": [0, "BLOCK", [64, 3, 3, 0, 0], 0],
                        "routes": ["BLOCK", "LIDAR_WAVE", "NONE", "STEP_LOOP"]})])
def test_read_once_knobs(knob, want):
    assert _child("m.knob_probe()", **{knob: "0"}) == want


# ---- coverage of the GPU case table -------------------------------------------------------------------------------
def _key_str(k):
    route, wpg, engine, goal, size, stage, rebuild = k
    eng = {LIDAR: "LIDAR", BICYCLE: "BICYCLE", MPE: "MPE", OMNI: "OMNI"}[engine]
    tag = "" if size is None else ":size" + ",".join(map(str, size))
    return f"{route}:wpg{wpg}:{eng}:{'TARGET' if goal else 'SPREAD'}{tag}:stage{stage}:rebuild{rebuild}"


def case_table_keys():
    """The coverage keys the GPU case table reaches, every case's plan checked on the way."""
    reached = set()
    for name, case in CASES.items():
        env = make_env(case.eid, case.n, num_obs=case.obs, device="cpu")
        with forced(case.wpg, case.mode):
            rb, ob, acts = case_tensors(env, case, "cpu")
            pl = plan_of(env, rb.buf, ob, acts, rb.rewards, rb.costs, case.rebuild)
        assert_case_plan(name, case, pl)
        assert pl.lds_bytes <= LDS_MAX
        reached.add(_key_str(plan_key(env, pl)))
    return sorted(reached)


def test_gpu_case_table_reaches_what_the_sweep_reaches():
    """Coverage is defined at the default knobs: default_report's child runs without the knob variables."""
    rep = default_report()
    reached, sweep_keys = set(rep["reached"]), set(rep["keys"])
    uncovered = set(json.load(open(os.path.join(HERE, "golden", "env_rollout_uncovered.json"))))
    assert reached <= sweep_keys, sorted(reached - sweep_keys)
    assert sweep_keys - reached == uncovered, (sorted(sweep_keys - reached - uncovered),
                                               sorted(uncovered - (sweep_keys - reached)))
    # never a persistent kernel the bench configurations run, and no wave instantiation at all
    assert not any(k.startswith(("LIDAR_WAVE", "MPE_WAVE")) for k in uncovered)


# ---- negative controls for assert_chain_equal ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def omni_chain():
    """5 oracle steps of LidarOmniTarget n = 8 / 3 obstacles (16 envs, one NaN action), with the buffers a rollout
    that matches it would hold."""
    spec = O.Spec("LidarOmniTarget", 8, 3)
    ag, gl, third = O.env_reset(spec, 3, 16)
    g0 = O.initial_graph(spec, ag, gl, third)
    a = chain_actions(spec, 5, 16, seed=4)
    a[1, 5, 2, 0] = np.nan
    chain = oracle_chain(spec, g0["states"], third, a)
    got = {f: np.concatenate([g0[f][None], chain[f]]) for f in ("nodes", "edges", "states", "receivers", "senders")}
    got["reward"], got["cost"] = chain["reward"].copy(), chain["cost"].copy()
    for v in got.values():
        v.setflags(write=False)
    return spec, third, a, chain, got


def _mutable(got):
    return {f: v.copy() for f, v in got.items()}


def test_chain_comparison_accepts_the_chain_itself(omni_chain):
    _, _, _, chain, got = omni_chain
    assert first_chain_mismatch(got, chain) is None
    assert_chain_equal(got, chain)
    assert np.isnan(chain["states"]).any()  # NaN equal to NaN is exercised


def test_control_stale_current_hits(omni_chain):
    """Step 3 run on step 1's "current hits" (what a kernel would see if LDS kept the hits of an earlier step): the
    next graph is unchanged (its hits are cast afresh), the Omni obstacle cost of step 3 is not."""
    spec, third, a, chain, got = omni_chain
    n = spec.n
    hits = slice(2 * n, 2 * n + spec.n_hits)
    stale = got["states"][3].copy()
    stale[:, hits] = got["states"][1][:, hits]
    assert not np.array_equal(stale, got["states"][3], equal_nan=True)
    with np.errstate(all="ignore"):
        ref = O.env_step(spec, stale, third, a[3])
    bad = _mutable(got)
    for f in ("nodes", "edges", "states", "receivers", "senders"):
        bad[f][4] = ref[f]
    bad["reward"][3], bad["cost"][3] = ref["reward"], ref["cost"]
    t, f, env, idx = first_chain_mismatch(bad, chain)
    assert (t, f) == (3, "cost") and idx[1] >= 1, (t, f, env, idx)  # a cost component past agent collisions
    with pytest.raises(AssertionError, match="step 3, field cost"):
        assert_chain_equal(bad, chain)


def test_control_swapped_edge_rows(omni_chain):
    _, _, _, chain, got = omni_chain
    bad = _mutable(got)
    e = bad["edges"][3, 7]  # graph 3 = the chain's step 2
    row = next(i for i in range(len(e) - 1) if not np.array_equal(e[i], e[i + 1], equal_nan=True))
    e[[row, row + 1]] = e[[row + 1, row]]
    t, f, env, idx = first_chain_mismatch(bad, chain)
    assert (t, f, env, idx[0]) == (2, "edges", 7, row)


def test_control_reward_one_ulp(omni_chain):
    _, _, _, chain, got = omni_chain
    bad = _mutable(got)
    assert np.isfinite(bad["reward"][4, 11])
    bad["reward"][4, 11] = np.nextafter(bad["reward"][4, 11], np.float32(np.inf))
    assert first_chain_mismatch(bad, chain) == (4, "reward", 11, ())


def test_control_nan_turned_into_a_number(omni_chain):
    _, _, _, chain, got = omni_chain
    bad = _mutable(got)
    t, env, row, col = (int(i) for i in np.argwhere(np.isnan(chain["states"]))[0])
    bad["states"][t + 1, env, row, col] = 0.0
    bad["nodes"][t + 1, env, row, col] = 0.0  # the node row carries the same state
    assert first_chain_mismatch(bad, chain) == (t, "nodes", env, (row, col))
    bad["nodes"][t + 1] = got["nodes"][t + 1]
    assert first_chain_mismatch(bad, chain) == (t, "states", env, (row, col))


# ---- the adversarial fixture on the reference alone -------------------------------------------------------------
@pytest.mark.parametrize("eid", LIDAR_IDS)
def test_adversarial_chain_runs_through_the_oracle_and_stays_mostly_finite(eid):
    """The chain of test_rollout_oracle_gpu.py (c) itself -- ADV_B envs, reset key ADV_SEED, ADV_T steps -- built from
    O.env_reset arrays: the oracle runs it without
    raising, NaN rows persist, and at least 7 of every 8 envs of each of the eight scene kinds keep finite agent
    rows to the last step -- a NaN blanket cannot make the GPU comparison vacuous."""
    spec = O.Spec(eid, 8, 3)
    # the arrays the GPU env's reset gives (test_env_gpu holds the two equal)
    ag, gl, ob = O.env_reset(spec, ADV_SEED, ADV_B)
    agent, goal, ob, acts = adversarial_chain_inputs(spec, ag, gl, ob)
    assert acts.shape == (ADV_T, ADV_B, 8, spec.ad) and ADV_B % 8 == 0 and ADV_B >= 24
    with np.errstate(all="ignore"):
        g0 = O.initial_graph(spec, agent, goal, ob)
    chain = oracle_chain(spec, g0["states"], ob, acts)
    finite = np.isfinite(chain["states"][-1][:, :8]).all(axis=(1, 2))
    for kind in range(8):
        of_kind = finite[kind::8]
        assert of_kind.sum() * 8 >= 7 * of_kind.size, (kind, int(of_kind.sum()), of_kind.size)
    # the NaN actions: env 6 from step 0, env 9 from step 3 on, for the rest of the episode
    assert not np.isfinite(chain["states"][:, 6, :8]).all(axis=(1, 2)).any()
    assert np.isfinite(chain["states"][:3, 9, :8]).all()
    assert not np.isfinite(chain["states"][3:, 9, :8]).all(axis=(1, 2)).any()
    assert np.isfinite(chain["reward"]).sum() >= 0.8 * chain["reward"].size


def test_full_lists_scene_runs_through_the_oracle():
    spec = O.Spec("LidarSpread", 8, 3)
    ag, gl, ob, a = full_lists_inputs(spec, *O.env_reset(spec, FULL_LISTS_KEY, 16))
    # envs 0..7: no obstacle is eligible for culling (wave_const in csrc/env_step.hip: every centre and corner
    # coordinate within +-2 and the circumradius, with its margin, at most 0.5), so every triple is cast
    with np.errstate(invalid="ignore"):
        pts = ob[:8, :, 8:].reshape(8, 3, 4, 2)
        rho = np.sqrt(((pts - ob[:8, :, None, :2]) ** 2).sum(-1).max(-1)) * np.float32(1.0001) + np.float32(1e-6)
        elig = (np.abs(pts) <= 2).all(axis=(2, 3)) & (np.abs(ob[:8, :, :2]) <= 2).all(-1) & (rho <= 0.5)
    assert not elig.any(), np.argwhere(elig)
    assert (rho[:, 2] > 0.55).all()  # the scaled obstacle is out by its radius, not by a coordinate
    # envs 8..15: eligible obstacles out of every ray's reach in every step
    pts = ob[8:, :, 8:].reshape(8, 3, 4, 2)
    rho = np.sqrt(((pts - ob[8:, :, None, :2]) ** 2).sum(-1).max(-1))
    assert (np.abs(pts) <= 2).all() and (rho < 0.1).all()
    with np.errstate(all="ignore"):
        g0 = O.initial_graph(spec, ag, gl, ob)
    chain = oracle_chain(spec, g0["states"], ob, a)
    pos = np.concatenate([g0["states"][None, 8:, :8, :2], chain["states"][:, 8:, :8, :2]])
    corners = ob[8, :, 8:].reshape(12, 2)
    d = np.linalg.norm(pos[..., None, :] - corners, axis=-1).min()
    assert d > 0.5 + 0.05 and np.isfinite(pos).all()
    # ... so their lidar edges are all masked (receiver = sender = the pad node)
    E0 = 8 * 8 + 8 * 8
    assert (chain["receivers"][:, 8:, E0:] == spec.n_nodes - 1).all()
