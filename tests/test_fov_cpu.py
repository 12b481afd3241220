"""Field-of-view neighbour sensing without a GPU: the NumPy reference (tests/fov_ref.py) on hand-made known answers and
against the oracle's own FoV cost, the mistakes the reference must be able to catch, dgppo_agent_fov's and
dgppo_lidar_observe_fov's declarations, struct layout and argument checks (none of which launches), the torch ops'
registration and fake kernels, and the refusals and flags of env.field_of_view / env.observe / the engines / make_algo /
train.py / test.py on device="cpu" envs."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib, ops  # noqa: F401  (registers torch.ops.dgppo.*)
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import ENV, make_env
from dgppo_fov_amd.trainer.rollout import NoisyLidarRolloutEngine, SensorRolloutEngine
from oracle import env as O

import fov_ref as R
from test_capi import ROOT, _c_layout, declared_functions

F = np.float32
OBSERVE_POINTERS = ("agent", "goal", "obstacles", "ray_dirs", "nodes", "edges", "out_states", "receivers", "senders")
FOV_POINTERS = ("agent", "in_fov")
# the reset scene sets of tests/test_fov_gpu.py: (env, n, obstacles, full_observation) -> unseen / in-range ordered
# pairs at 60 degrees over the 32 envs of key 7
RESET_CASES = {("LidarOmniTarget", 3, 3, False): (22, 56), ("LidarOmniTarget", 8, 3, False): (205, 394),
               ("LidarOmniTarget", 3, 3, True): (70, 192), ("LidarBicycleTarget", 3, 3, False): (28, 42),
               ("LidarBicycleTarget", 2, 1, True): (34, 64)}
HEADING = (("LidarOmniTarget", 7), ("LidarBicycleTarget", 5))
NO_HEADING = ("LidarSpread", "LidarTarget", "LidarLine")


def reset_scene(case):
    eid, n, obs, full = case
    spec = O.Spec(eid, n, obs, full_observation=full)
    return spec, O.env_reset(spec, 7, 32)


# ---- 1. the reference ---------------------------------------------------------------------------------------------------
def test_cone_cosines_of_the_known_answers():
    assert R.cone_cos(0.001) == F(1.0)  # exactly
    assert R.cone_cos(90.0) == F(-4.371139e-08) and R.cone_cos(90.0) != 0
    assert R.cone_cos(60.0) > 0 and R.cone_cos(180.0) == F(-1.0)
    # the library's own host routine (dgppo_env_cfg_finalize's c_cos_fov) gives the same bits
    for deg in (0.001, 30.0, 60.0, 90.0, 120.0, 180.0):
        cls = ENV["LidarOmniTarget"]
        env = cls(num_agents=2, area_size=None, max_step=4, dt=0.03, params=dict(cls.PARAMS, fov_angle_deg=deg),
                  device="cpu")
        assert F(env.cfg.c_cos_fov) == R.cone_cos(deg), deg


@pytest.mark.parametrize("name", list(R.kat_scenes()))
def test_reference_known_answers(name):
    agent, deg, expect = R.kat_scenes()[name]
    got = R.field_of_view_ref(agent[None], deg)[0]
    np.testing.assert_array_equal(got, expect)
    assert got.diagonal().all()


def test_reference_margins_of_the_pinned_answers():
    kats = R.kat_scenes()
    h = {name: R.fov_margin(agent[None], deg)[0, 0, 1] for name, (agent, deg, _) in kats.items()}
    (at_quarter,) = [v for k, v in h.items() if "0.25" in k]
    (at_tiny,) = [v for k, v in h.items() if "1e-6" in k]
    assert at_quarter == F(0.0) and at_tiny == F(1.0000008e-08)
    (coincident,) = [v for k, v in h.items() if "coincident at 60" in k]
    assert coincident == R.cone_cos(60.0) * F(1e-8) > 0  # nrm = lx = 0: the sign of cb decides


def test_reference_is_the_oracles_fov_cost_on_the_chain():
    """field_of_view_ref(agent, fov_angle_deg)[b, i, i + 1] == (oracle cost[b, i, 2] < 0): on random headings, both
    sides well populated (at reset every chain pair is inside the cone)."""
    spec = O.Spec("LidarOmniTarget", 8, 3)
    rng = np.random.default_rng(5)
    agent = np.zeros((32, 8, 7), F)
    agent[..., :2] = rng.uniform(0, spec.area, (32, 8, 2))
    th = rng.uniform(-np.pi, np.pi, (32, 8))
    agent[..., 2], agent[..., 3] = np.cos(th).astype(F), np.sin(th).astype(F)
    cost = O.get_cost_omni(spec, agent, np.zeros((32, 8 * spec.top_k, 2), F))
    inside = cost[:, :-1, 2] < 0
    assert min(int(inside.sum()), int((~inside).sum())) * 10 >= inside.size
    seen = R.field_of_view_ref(agent, spec.params["fov_angle_deg"])
    idx = np.arange(7)
    np.testing.assert_array_equal(seen[:, idx, idx + 1], inside)
    _, (ag, _, _) = reset_scene(("LidarOmniTarget", 8, 3, False))
    assert R.field_of_view_ref(ag, 60.0)[:, idx, idx + 1].all()  # why reset scenes cannot serve that test


@pytest.mark.parametrize("case", list(RESET_CASES), ids=lambda c: f"{c[0]}-n{c[1]}-o{c[2]}" + ("-full" if c[3] else ""))
def test_reference_counts_and_mistakes_on_the_reset_scenes(case):
    spec, (ag, _, _) = reset_scene(case)
    inr = R.in_range_ref(spec, ag)
    right = R.field_of_view_ref(ag, 60.0)
    assert (int((~right & inr).sum()), int(inr.sum())) == RESET_CASES[case]
    for deg in (30.0, 60.0, 120.0):
        right = R.field_of_view_ref(ag, deg)
        assert (~right & inr).any() and (right & inr).any(), deg  # in-range pairs on both sides of the cone
        for mistake in ("sender_heading", "swapped"):  # the gross mistakes change the in-range mask of every scene set
            wrong = R.field_of_view_ref(ag, deg, mistake)
            assert ((wrong != right) & inr).any(), (mistake, deg)


def test_reference_catches_the_fine_mistakes_on_the_known_answers():
    """The dropped 1e-8 and `<` for `<=` change no pair of the reset scenes (no pair sits on a cone's edge there); they
    change the known answers, which the GPU tests run through the kernel as well."""
    kats = R.kat_scenes()
    agent = np.stack([k[0] for k in kats.values()])
    changed = {m: [] for m in R.MISTAKES}
    for b, (name, (ag, deg, expect)) in enumerate(kats.items()):
        for m in R.MISTAKES:
            if not np.array_equal(R.field_of_view_ref(agent[b:b + 1], deg, m)[0], expect):
                changed[m].append(name)
    assert all(changed[m] for m in R.MISTAKES), changed
    assert any("0.25" in k for k in changed["strict"]) and any("1e-6" in k for k in changed["no_eps"])
    for case in RESET_CASES:
        _, (ag, _, _) = reset_scene(case)
        for m in ("no_eps", "strict"):
            np.testing.assert_array_equal(R.field_of_view_ref(ag, 60.0, m), R.field_of_view_ref(ag, 60.0))


def test_mask_unseen_ref_changes_receivers_and_senders_only():
    case = ("LidarOmniTarget", 3, 3, True)
    spec, (ag, gl, ob) = reset_scene(case)
    hits, _ = O.lidar(np.ascontiguousarray(ag[..., :2]), ob, O.ray_table(spec.n_rays, spec.comm_r), spec.top_k)
    true = O.build_graph(spec, ag, gl, hits)
    seen = R.field_of_view_ref(ag, 60.0)
    got = R.mask_unseen_ref(spec, true, seen)
    for f in ("nodes", "edges", "states"):
        np.testing.assert_array_equal(got[f], true[f])
    n, pad = spec.n, spec.n_nodes - 1
    flat = seen.reshape(32, n * n)
    for f in ("receivers", "senders"):
        np.testing.assert_array_equal(got[f][:, n * n:], true[f][:, n * n:])
        np.testing.assert_array_equal(got[f][:, :n * n][flat], true[f][:, :n * n][flat])
        assert (got[f][:, :n * n][~flat] == pad).all()
    assert (got["receivers"] != true["receivers"]).sum() == RESET_CASES[case][0]  # the in-range unseen pairs


# ---- 2. the C entries ---------------------------------------------------------------------------------------------------
def test_header_signatures_and_exports_agree():
    lib = _lib.load()
    assert "dgppo_agent_fov" in declared_functions() and hasattr(lib, "dgppo_agent_fov")
    assert "dgppo_lidar_observe_fov" in declared_functions() and hasattr(lib, "dgppo_lidar_observe_fov")
    assert _lib.SIGNATURES["dgppo_agent_fov"] == (ctypes.c_int, [ctypes.POINTER(_lib.EnvCfg),
                                                                 ctypes.POINTER(_lib.AgentFovIO), ctypes.c_void_p])
    assert _lib.SIGNATURES["dgppo_lidar_observe_fov"] == (
        ctypes.c_int, [ctypes.POINTER(_lib.EnvCfg), ctypes.POINTER(_lib.LidarObserveIO), ctypes.c_float,
                       ctypes.c_void_p])
    assert lib.dgppo_abi_version() == 14 == _lib.ABI_VERSION  # new symbols, no new ABI number
    with open(os.path.join(ROOT, "include", "dgppo_hip.h")) as f:
        src = f.read()
    assert re.search(r"#define\s+DGPPO_OBSERVE_FOV\s+8\b", src)
    assert re.search(r"int\s+dgppo_lidar_observe_fov\(const dgppo_env_cfg\*\s*cfg,\s*const dgppo_lidar_observe_io\*\s*io,"
                     r"\s*float\s+half_angle_deg,\s*void\*\s*stream\);", src)
    assert _lib.OBSERVE_FOV == 8 and _lib.OBSERVE_SIGHT == 4


def test_ctypes_mirror_matches_c_layout():
    names = [f[0] for f in _lib.AgentFovIO._fields_]
    assert names == ["agent", "agent_stride", "in_fov", "in_fov_stride", "half_angle_deg", "n_env"]
    got = _c_layout("dgppo_agent_fov_io", names)
    assert got[0] == ctypes.sizeof(_lib.AgentFovIO)
    for field, off in zip(names, got[1:]):
        assert getattr(_lib.AgentFovIO, field).offset == off, field
    # the observe io is the one dgppo_lidar_observe takes: its layout did not change
    names = [f[0] for f in _lib.LidarObserveIO._fields_]
    got = _c_layout("dgppo_lidar_observe_io", names)
    assert got[0] == ctypes.sizeof(_lib.LidarObserveIO) == 176
    for field, off in zip(names, got[1:]):
        assert getattr(_lib.LidarObserveIO, field).offset == off, field


def _host_io(cls, pointers, n_env=1, **fields):
    """An io whose pointers are non-NULL host addresses: only for calls that return before any launch."""
    buf = (ctypes.c_float * 4)()
    io = cls()
    for f in pointers:
        setattr(io, f, ctypes.addressof(buf))
    io.n_env = n_env
    for k, v in fields.items():
        setattr(io, k, v)
    return io, buf


BAD_ANGLES = (0.0, -1.0, 180.00002, 360.0, float("nan"), float("inf"), float("-inf"))
NO_HEADING_CFGS = (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=2)), ("LidarTarget", dict(num_obs=2)),
                   ("LidarLine", dict(num_obs=2)), ("LidarSpread", dict(num_obs=0)), ("VMASWheel", {}))


def test_agent_fov_argument_checks_do_not_launch():
    fn = _lib.load().dgppo_agent_fov
    for eid, _ in HEADING:
        env = make_env(eid, 3, num_obs=2, device="cpu")
        cfg = ctypes.byref(env.cfg)
        io, keep = _host_io(_lib.AgentFovIO, FOV_POINTERS, half_angle_deg=60.0)
        assert fn(cfg, None, None) == _lib.DGPPO_EINVAL
        assert fn(None, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
        for field in FOV_POINTERS:
            io, keep = _host_io(_lib.AgentFovIO, FOV_POINTERS, half_angle_deg=60.0)
            setattr(io, field, None)
            assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, field
        io, keep = _host_io(_lib.AgentFovIO, FOV_POINTERS, n_env=-1, half_angle_deg=60.0)
        assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
        for deg in BAD_ANGLES:
            for n_env in (0, 1):
                io, keep = _host_io(_lib.AgentFovIO, FOV_POINTERS, n_env=n_env, half_angle_deg=deg)
                assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (deg, n_env)
        for deg in (1e-3, 60.0, 180.0):  # n_env == 0: answered before any pointer is read
            io = _lib.AgentFovIO()
            io.half_angle_deg = deg
            assert fn(cfg, ctypes.byref(io), None) == 0, deg
        # it reads no obstacles: an env without any is served
        bare = make_env(eid, 3, num_obs=0, device="cpu")
        io = _lib.AgentFovIO()
        io.half_angle_deg = 60.0
        assert fn(ctypes.byref(bare.cfg), ctypes.byref(io), None) == 0
    for eid, kw in NO_HEADING_CFGS:
        other = make_env(eid, 3, device="cpu", **kw)
        for n_env in (0, 1):
            io, keep = _host_io(_lib.AgentFovIO, FOV_POINTERS, n_env=n_env, half_angle_deg=60.0)
            assert fn(ctypes.byref(other.cfg), ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (eid, n_env)


def test_observe_fov_argument_checks_do_not_launch():
    lib = _lib.load()
    fn = lib.dgppo_lidar_observe_fov
    deg = ctypes.c_float(60.0)
    for eid, _ in HEADING:
        env = make_env(eid, 3, num_obs=2, device="cpu")
        cfg = ctypes.byref(env.cfg)
        io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS)
        assert fn(cfg, None, deg, None) == _lib.DGPPO_EINVAL
        assert fn(None, ctypes.byref(io), deg, None) == _lib.DGPPO_EINVAL
        for flags in (0, 4, 8, 15):
            for field in OBSERVE_POINTERS:
                io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS, flags=flags)
                setattr(io, field, None)
                assert fn(cfg, ctypes.byref(io), deg, None) == _lib.DGPPO_EINVAL, (field, flags)
        for field, bad in (("n_env", -1), ("t", -1), ("env_offset", -1), ("flags", 16), ("flags", 24), ("flags", -1)):
            io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS, flags=8)
            setattr(io, field, bad)
            assert fn(cfg, ctypes.byref(io), deg, None) == _lib.DGPPO_EINVAL, (field, bad)
        for flags in range(16):  # every accepted flag set; n_env == 0 is answered before any pointer is read
            io = _lib.LidarObserveIO()
            io.flags = flags
            assert fn(cfg, ctypes.byref(io), deg, None) == 0, flags
            assert fn(cfg, ctypes.byref(io), ctypes.c_float(180.0), None) == 0, flags
        for bad in BAD_ANGLES:
            for n_env in (0, 1):
                io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS, n_env=n_env, flags=8 | 4)
                assert fn(cfg, ctypes.byref(io), ctypes.c_float(bad), None) == _lib.DGPPO_EINVAL, (bad, n_env)
            io = _lib.LidarObserveIO()  # without the bit the angle is not read: dgppo_lidar_observe_los
            io.flags = 4
            assert fn(cfg, ctypes.byref(io), ctypes.c_float(bad), None) == 0, bad
        # the other two entries keep refusing the new bit
        for flags in (8, 12, 9):
            io = _lib.LidarObserveIO()
            io.flags = flags
            assert lib.dgppo_lidar_observe(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
            assert lib.dgppo_lidar_observe_los(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    for eid, kw in NO_HEADING_CFGS + (("LidarOmniTarget", dict(num_obs=0)),):
        other = make_env(eid, 3, device="cpu", **kw)
        for n_env in (0, 1):
            io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS, n_env=n_env, flags=8)
            assert fn(ctypes.byref(other.cfg), ctypes.byref(io), deg, None) == _lib.DGPPO_EINVAL, (eid, n_env)
    # a Lidar env without a heading is still served without the bit, as by dgppo_lidar_observe_los
    spread = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    io = _lib.LidarObserveIO()
    io.flags = 7
    assert fn(ctypes.byref(spread.cfg), ctypes.byref(io), deg, None) == 0


# ---- 3. the ops -----------------------------------------------------------------------------------------------------------
def test_ops_registered_and_trace_under_fake_tensors():
    s = str(torch.ops.dgppo.lidar_observe_fov.default._schema)
    old = str(torch.ops.dgppo.lidar_observe_los.default._schema)
    assert ", float half_angle_deg, " in s
    alias = lambda x: re.sub(r"\(a\d+!\)", "(a!)", x)  # noqa: E731  (the alias sets are numbered by position)
    assert alias(s.replace("dgppo::lidar_observe_fov(", "dgppo::lidar_observe_los(").replace(
        ", float half_angle_deg, ", ", ")) == alias(old), s  # lidar_observe_los's schema plus the angle behind the flags
    s = str(torch.ops.dgppo.agent_fov.default._schema)
    assert re.fullmatch(r"dgppo::agent_fov\((Sym)?[Ii]nt cfg, Tensor agent, float half_angle_deg, "
                        r"Tensor\(a\d+!\) in_fov\) -> \(\)", s), s
    env = make_env("LidarOmniTarget", 3, num_obs=2, device="cpu")
    B, n, R_, sd = 2, 3, 32, 7
    from torch._subclasses.fake_tensor import FakeTensorMode

    def observe(agent, goal, ob, rays, g):
        return torch.ops.dgppo.lidar_observe_fov(env._cfg_handle, agent, goal, ob, rays, None, 3, 0, 1, 0.1,
                                                 float("-inf"), _lib.OBSERVE_NOISE | _lib.OBSERVE_FOV, 60.0, g.nodes,
                                                 g.edges, g.states, g.receivers, g.senders)

    with FakeTensorMode():
        g = env.empty_graph((B,), "cpu")
        shapes = [tuple(getattr(g, f).shape) for f in ("nodes", "edges", "states", "receivers", "senders")]
        assert observe(torch.empty(B, n, sd), torch.empty(B, n, sd), torch.empty(B, 2, 16), torch.empty(R_, 2), g) is None
        assert [tuple(getattr(g, f).shape) for f in ("nodes", "edges", "states", "receivers", "senders")] == shapes
        seen = torch.empty(B, n, n, dtype=torch.uint8)
        assert torch.ops.dgppo.agent_fov(env._cfg_handle, torch.empty(B, n, sd), 60.0, seen) is None
        assert tuple(seen.shape) == (B, n, n)
    with pytest.raises(_lib.NativeLibraryError):  # the real kernels have no CPU path
        observe(torch.zeros(B, n, sd), torch.zeros(B, n, sd), torch.zeros(B, 2, 16), torch.zeros(R_, 2),
                env.empty_graph((B,), "cpu"))
    with pytest.raises(_lib.NativeLibraryError):
        torch.ops.dgppo.agent_fov(env._cfg_handle, torch.zeros(B, n, sd), 60.0, torch.zeros(B, n, n, dtype=torch.uint8))


# ---- 4. the env, the engines, the algorithms ---------------------------------------------------------------------------
def test_field_of_view_and_observe_refusals_on_cpu_envs():
    B, n = 2, 3
    for eid, sd in HEADING:
        env = make_env(eid, n, num_obs=2, device="cpu")
        agent, goal, ob = torch.zeros(B, n, sd), torch.zeros(B, n, sd), torch.zeros(B, 2, 16)
        with pytest.raises(ValueError, match="agent_states"):
            env.field_of_view(agent[:, :2], 60.0)
        for bad in (0.0, -5.0, 181.0, float("nan"), None):
            with pytest.raises(ValueError, match="half angle"):
                env.field_of_view(agent, bad)
            if bad is not None:
                with pytest.raises(ValueError, match="half angle"):
                    env.observe((agent, goal, ob), 0, sigma=0.0, dropout=0.0, seed=1, fov=bad)
        with pytest.raises(_lib.NativeLibraryError):  # well-formed calls on CPU tensors: there is no CPU kernel
            env.field_of_view(agent, 60.0)
        with pytest.raises(_lib.NativeLibraryError):
            env.field_of_view(agent, 180.0)
        with pytest.raises(_lib.NativeLibraryError):
            env.observe((agent, goal, ob), 0, sigma=0.0, dropout=0.0, seed=1, fov=60.0)
        bare = make_env(eid, n, num_obs=0, device="cpu")  # no obstacles: field_of_view is served, observe has no LiDAR
        with pytest.raises(_lib.NativeLibraryError):
            bare.field_of_view(agent, 60.0)
        with pytest.raises(ValueError, match="no LiDAR"):
            bare.observe((agent, goal, ob), 0, sigma=0.0, dropout=0.0, seed=1, fov=60.0)
    agent, goal, ob = torch.zeros(B, n, 4), torch.zeros(B, n, 4), torch.zeros(B, 2, 16)
    for eid in NO_HEADING:
        e = make_env(eid, n, num_obs=2, device="cpu")
        with pytest.raises(ValueError, match="no heading"):  # before any launch
            e.field_of_view(agent, 60.0)
        with pytest.raises(ValueError, match="no heading"):
            e.observe((agent, goal, ob), 0, sigma=0.0, dropout=0.0, seed=1, fov=60.0)
        with pytest.raises(ValueError, match="no heading"):
            NoisyLidarRolloutEngine(e, B, 2, "cpu", actor=object(), fov=60.0)
        with pytest.raises(ValueError, match="no heading"):
            SensorRolloutEngine(e, B, 2, "cpu", actor=object(), sensor=None, fov=60.0)
    mpe = make_env("MPESpread", n, num_obs=3, device="cpu")
    with pytest.raises(ValueError, match="no heading"):
        mpe.field_of_view(agent, 60.0)
    with pytest.raises(ValueError, match="no LiDAR"):
        mpe.observe((agent, goal, ob), 0, sigma=0.0, dropout=0.0, seed=1, fov=60.0)
    vmas = make_env("VMASWheel", 3, device="cpu")
    with pytest.raises(NotImplementedError):
        vmas.field_of_view(agent, 60.0)
    with pytest.raises(NotImplementedError):
        vmas.observe((agent, goal, ob), 0, sigma=0.0, dropout=0.0, seed=1, fov=60.0)
    env = make_env("LidarOmniTarget", n, num_obs=2, device="cpu")
    with pytest.raises(ValueError, match="sensor must be a callable"):  # None means identity only with a mask to apply
        SensorRolloutEngine(env, B, 2, "cpu", actor=object(), sensor=None, fov=180.0)


def test_observe_picks_the_op_by_the_cone(monkeypatch):
    env = make_env("LidarOmniTarget", 3, num_obs=2, device="cpu")
    B, n = 2, 3
    state = (torch.zeros(B, n, 7), torch.zeros(B, n, 7), torch.zeros(B, 2, 16))
    from torch.utils._python_dispatch import TorchDispatchMode

    calls = []
    watched = {torch.ops.dgppo.lidar_observe.default: "lidar_observe",
               torch.ops.dgppo.lidar_observe_los.default: "lidar_observe_los",
               torch.ops.dgppo.lidar_observe_fov.default: "lidar_observe_fov"}

    class Record(TorchDispatchMode):  # the op env.observe picks, its flags and angle, without running it
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func in watched:
                name = watched[func]
                calls.append((name, args[11]) + ((args[12],) if name == "lidar_observe_fov" else ()))
                return None
            return func(*args, **(kwargs or {}))

    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    kw = dict(sigma=0.05, dropout=0.1, seed=1)
    with Record():
        env.observe(state, 0, **kw)
        env.observe(state, 0, fov=None, **kw)
        env.observe(state, 0, fov=180, **kw)
        env.observe(state, 0, fov=180.0, occlusion=True, **kw)
        env.observe(state, 0, fov=60, **kw)
        env.observe(state, 0, fov=60.0, occlusion=True, **kw)
        env.observe(state, 0, sigma=0.0, dropout=0.0, seed=1, fov=30.5)
    assert calls == [("lidar_observe", 3), ("lidar_observe", 3), ("lidar_observe", 3), ("lidar_observe_los", 3 | 4),
                     ("lidar_observe_fov", 3 | 8, 60.0), ("lidar_observe_fov", 3 | 4 | 8, 60.0),
                     ("lidar_observe_fov", 8, 30.5)]


def _algo_kwargs(env, **kw):
    return dict(env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                action_dim=env.action_dim, n_agents=env.num_agents, batch_size=8, rnn_step=2, device="cpu", **kw)


@pytest.mark.parametrize("algo", ["dgppo", "informarl", "informarl_lagr"])
def test_algorithms_accept_a_cone_and_refuse_what_cannot_train_under_it(algo):
    for eid, _ in HEADING:
        env = make_env(eid, 3, num_obs=2, device="cpu")
        a = make_algo(algo, **_algo_kwargs(env, lidar_fov=60))
        assert a.sensor is None and a.occlusion is False and a.fov == 60.0 and a.sensed  # on its own it is sensed
        a = make_algo(algo, **_algo_kwargs(env, lidar_fov=45.0, lidar_noise=0.1, lidar_occlusion=True))
        assert a.sensor == (0.1, 0.0) and a.occlusion is True and a.fov == 45.0 and a.sensed
        a = make_algo(algo, **_algo_kwargs(env))
        assert a.fov is None and not a.sensed
        a = make_algo(algo, **_algo_kwargs(env, lidar_fov=180))  # no cone
        assert a.fov is None and not a.sensed
        for bad in (0.0, 200.0, -3.0):
            with pytest.raises(ValueError, match="half angle"):
                make_algo(algo, **_algo_kwargs(env, lidar_fov=bad))
        bare = make_env(eid, 3, num_obs=0, device="cpu")  # --obs 0
        with pytest.raises(ValueError, match="no LiDAR"):
            make_algo(algo, **_algo_kwargs(bare, lidar_fov=60))
    for eid in NO_HEADING:
        e = make_env(eid, 3, num_obs=2, device="cpu")
        with pytest.raises(ValueError, match="no heading"):
            make_algo(algo, **_algo_kwargs(e, lidar_fov=60))
        assert make_algo(algo, **_algo_kwargs(e)).fov is None
    for eid, okw in (("MPESpread", dict(num_obs=3)), ("VMASWheel", {})):
        e = make_env(eid, 3, device="cpu", **okw)
        with pytest.raises(ValueError, match="no LiDAR"):
            make_algo(algo, **_algo_kwargs(e, lidar_fov=60))


def test_hcbfcrpo_refuses_a_cone():
    env = make_env("LidarOmniTarget", 3, num_obs=2, device="cpu")
    for flags in (dict(lidar_fov=60), dict(lidar_fov=60, lidar_noise=0.1), dict(lidar_fov=60, lidar_occlusion=True)):
        with pytest.raises(ValueError, match="get_cost"):
            make_algo("hcbfcrpo", **_algo_kwargs(env, **flags))
    assert make_algo("hcbfcrpo", **_algo_kwargs(env)).fov is None


def _cli(name):
    spec = importlib.util.spec_from_file_location(f"dgppo_{name}_cli_fov", os.path.join(ROOT, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_and_test_parsers_accept_the_flag(tmp_path):
    train = _cli("train")
    p = train.build_parser()
    base = ["--env", "LidarOmniTarget", "-n", "3", "--algo", "dgppo", "--obs", "2"]
    assert p.parse_args(base).lidar_fov is None
    a = p.parse_args(base + ["--lidar-fov", "60"])
    assert a.lidar_fov == 60.0 and a.lidar_noise is None and a.lidar_dropout is None and a.lidar_occlusion is False
    a = p.parse_args(base + ["--lidar-fov", "45.5", "--lidar-occlusion", "--lidar-noise", "0.02"])
    assert a.lidar_fov == 45.5 and a.lidar_occlusion is True and a.lidar_noise == 0.02
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--lidar-fov"])  # a value, not a switch
    # a flag a resumed run may not change: recorded with the run's arguments, compared on --resume
    assert "lidar_fov" not in train.RESUME_FREE
    saved = dict(vars(p.parse_args(base + ["--lidar-fov", "60"])), _world_size=1)
    with open(tmp_path / "train_args.json", "w") as f:
        json.dump(saved, f)
    train.check_resume_args(p.parse_args(base + ["--lidar-fov", "60"]), str(tmp_path), world=1)
    for other in (["--lidar-fov", "45"], []):
        with pytest.raises(SystemExit, match="lidar_fov"):
            train.check_resume_args(p.parse_args(base + other), str(tmp_path), world=1)
    saved = dict(vars(p.parse_args(base)), _world_size=1)
    saved.pop("lidar_fov")  # a run saved before the flag existed trained without it
    with open(tmp_path / "train_args.json", "w") as f:
        json.dump(saved, f)
    train.check_resume_args(p.parse_args(base), str(tmp_path), world=1)
    with pytest.raises(SystemExit, match="lidar_fov"):
        train.check_resume_args(p.parse_args(base + ["--lidar-fov", "60"]), str(tmp_path), world=1)
    tp = _cli("test").build_parser()
    assert tp.parse_args(["--path", "x"]).lidar_fov is None
    a = tp.parse_args(["--path", "x", "--lidar-fov", "60"])
    assert a.lidar_fov == 60.0 and a.lidar_noise is None and a.lidar_occlusion is False
    a = tp.parse_args(["--path", "x", "--lidar-fov", "60", "--lidar-occlusion", "--lidar-dropout", "0.1"])
    assert a.lidar_fov == 60.0 and a.lidar_occlusion is True and a.lidar_dropout == 0.1
