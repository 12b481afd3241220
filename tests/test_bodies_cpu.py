"""LiDAR sees agents, without a GPU: the NumPy reference (tests/bodies_ref.py) on hand-derived known answers, the new
entries' declarations and argument checks (none of which launches), the ops' registration and fake kernels, the refusals
of the `bodies` option through make_algo, both sensor engines, env.observe and env.lidar_scan on device="cpu" envs, the
op each call picks, and the flags of train.py / test.py."""
import ctypes
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

from dgppo_fov_amd import _lib, ops  # noqa: F401  (registers torch.ops.dgppo.*)
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.trainer.rollout import NoisyLidarRolloutEngine, SensorRolloutEngine
from dgppo_fov_amd.utils.sensor import Sensing, bodies_option

import bodies_ref as R
from test_capi import ROOT, declared_functions

F = np.float32
RAYS, RANGE, RHO = 32, 0.5, 0.05
AHEAD = RAYS // 2  # the beam (RANGE, 0)
NONE = F(1e6)
OBSERVE_POINTERS = ("agent", "goal", "obstacles", "ray_dirs", "nodes", "edges", "out_states", "receivers", "senders")
SCAN_POINTERS = ("agent", "obstacles", "ray_dirs", "alpha")
LIDAR = ("LidarSpread", "LidarTarget", "LidarLine", "LidarBicycleTarget", "LidarOmniTarget")


def pair(d, theta=0.0):
    """Two agents: the receiver at the origin, the sender at distance d and bearing theta."""
    agent = np.zeros((1, 2, 4), F)
    agent[0, 1, :2] = d * np.cos(theta), d * np.sin(theta)
    return agent


# ---- 1. the reference's known answers ------------------------------------------------------------------------------------
def test_ray_table_of_the_hand_made_cases():
    tab = R.ray_table_ref(RAYS, RANGE)
    assert tab.dtype == F and tab.shape == (RAYS, 2) and tab[AHEAD, 0] == F(0.5) and tab[AHEAD, 1] == 0


@pytest.mark.parametrize("d,beams", [(0.1, 5), (0.2, 3), (0.3, 1), (0.54, 1)])
def test_sender_dead_ahead(d, beams):
    a = R.body_alpha_ref(pair(d), R.ray_table_ref(RAYS, RANGE), RHO)
    assert a.dtype == F and a.shape == (1, 2, RAYS)
    assert abs(float(a[0, 0, AHEAD]) - (d - RHO) / RANGE) <= 1e-6  # the near surface, as a fraction of the range
    assert int((a[0, 0] <= 1).sum()) == beams and (a[0, 0][a[0, 0] > 1] == NONE).all()
    # the sender sees the receiver on the opposite beam, at the same distance
    assert abs(float(a[0, 1, 0]) - (d - RHO) / RANGE) <= 1e-6 and a[0, 1, AHEAD] == NONE


def test_out_of_range_behind_and_alone():
    tab = R.ray_table_ref(RAYS, RANGE)
    assert (R.body_alpha_ref(pair(0.56), tab, RHO) == NONE).all()  # 0.56 - rho > range
    a = R.body_alpha_ref(pair(0.2, np.pi), tab, RHO)  # behind the receiver: only the beams towards it return
    assert a[0, 0, AHEAD] == NONE and abs(float(a[0, 0, 0]) - 0.3) <= 1e-6
    alone = np.zeros((3, 1, 4), F)
    assert (R.body_alpha_ref(alone, tab, RHO) == NONE).all()  # n == 1
    zero = np.zeros((1, 2), F)  # a zero ray has bb == 0 and returns nothing
    assert (R.body_alpha_ref(pair(0.2), zero, RHO) == NONE).all()


def test_overlapping_discs_return_zero():
    tab = R.ray_table_ref(RAYS, RANGE)
    for d in (0.0, 0.01, 0.049):  # coincident, inside
        a = R.body_alpha_ref(pair(d), tab, RHO)
        assert (a == 0).all() and not np.signbit(a).any(), d
    # cc == 0 built exactly: rho = 0.25, the sender at (0.25, 0): 0.0625 - 0.0625
    a = R.body_alpha_ref(pair(0.25), tab, 0.25)
    assert F(0.25) * F(0.25) - F(0.25) * F(0.25) == 0 and (a == 0).all()
    # just outside: a return at a small positive alpha dead ahead, nothing behind
    a = R.body_alpha_ref(pair(0.2500001), tab, 0.25)
    assert 0 <= a[0, 0, AHEAD] < 1e-6 and a[0, 0, 0] == NONE


def test_grazing_beam_misses():
    """The sender at (0.3, 0.0501): the beam along +x passes 0.0501 > rho from its centre (disc < 0), the next beam
    up (11.25 degrees) passes within rho."""
    tab = R.ray_table_ref(RAYS, RANGE)
    agent = np.zeros((1, 2, 4), F)
    agent[0, 1, :2] = 0.3, 0.0501
    a = R.body_alpha_ref(agent, tab, RHO)
    dx, mx, my = F(0.5), F(0.3), F(0.0501)
    bb = dx * mx
    assert bb * bb - (dx * dx) * ((mx * mx + my * my) - F(RHO) * F(RHO)) < 0
    assert a[0, 0, AHEAD] == NONE and a[0, 0, AHEAD + 1] < 1


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_nan_or_infinite_sender_returns_nothing_and_spoils_nothing(bad):
    tab = R.ray_table_ref(RAYS, RANGE)
    agent = np.zeros((1, 3, 4), F)
    agent[0, 1, 0] = 0.3
    clean = R.body_alpha_ref(agent[:, :2], tab, RHO)
    for col in (0, 1):
        rows = agent.copy()
        rows[0, 2, col] = bad
        a = R.body_alpha_ref(rows, tab, RHO)
        assert not np.isnan(a).any()
        np.testing.assert_array_equal(a[0, :2], clean[0])  # the others' returns off each other are intact
        assert (a[0, 2] == NONE).all()  # and the broken receiver sees nothing


def test_the_obstacle_return_and_its_nan():
    a_body = np.array([0.5, 0.2, 1e6, 0.5, 0.0], F)
    a_obs = np.array([0.2, 0.5, np.nan, np.nan, 1e6], F)
    got = R.nearer_alpha_ref(a_obs, a_body)
    np.testing.assert_array_equal(got[[0, 1, 4]], np.array([0.2, 0.2, 0.0], F))  # the wall hides, the body wins
    assert np.isnan(got[2]) and np.isnan(got[3])  # a NaN a_obs stays NaN
    # through the whole scan: a wall at 0.2 on every beam hides the body at 0.5, a wall at 0.8 does not
    tab = R.ray_table_ref(RAYS, RANGE)
    agent = pair(0.3)
    near = R.scan_bodies_ref(np.full((1, 2, RAYS), 0.2, F), agent, tab, RHO)
    far = R.scan_bodies_ref(np.full((1, 2, RAYS), 0.8, F), agent, tab, RHO)
    assert (near == F(0.2)).all() and abs(float(far[0, 0, AHEAD]) - 0.5) <= 1e-6 and far[0, 0, 0] == F(0.8)


# ---- 2. the C entries ---------------------------------------------------------------------------------------------------
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


def test_header_signatures_and_exports_agree():
    lib = _lib.load()
    for name in ("dgppo_lidar_scan_bodies", "dgppo_lidar_observe_bodies"):
        assert name in declared_functions() and hasattr(lib, name)
    assert _lib.SIGNATURES["dgppo_lidar_scan_bodies"] == _lib.SIGNATURES["dgppo_lidar_scan"]
    assert _lib.SIGNATURES["dgppo_lidar_observe_bodies"] == _lib.SIGNATURES["dgppo_lidar_observe_fov"]
    assert lib.dgppo_abi_version() == 14 == _lib.ABI_VERSION  # new symbols, no new ABI number
    with open(os.path.join(ROOT, "include", "dgppo_hip.h")) as f:
        src = f.read()
    assert re.search(r"#define\s+DGPPO_OBSERVE_BODIES\s+16\b", src) and _lib.OBSERVE_BODIES == 16


def test_argument_checks_do_not_launch():
    lib = _lib.load()
    scan, observe = lib.dgppo_lidar_scan_bodies, lib.dgppo_lidar_observe_bodies
    deg = ctypes.c_float(60.0)
    for eid in LIDAR:
        env = make_env(eid, 3, num_obs=2, device="cpu")
        cfg = ctypes.byref(env.cfg)
        heading, line = eid in ("LidarBicycleTarget", "LidarOmniTarget"), eid == "LidarLine"
        # the scan: dgppo_lidar_scan's refusals
        assert scan(cfg, None, None) == _lib.DGPPO_EINVAL
        for field in SCAN_POINTERS:
            io, keep = _host_io(_lib.LidarScanIO, SCAN_POINTERS)
            setattr(io, field, None)
            assert scan(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, field
        io, keep = _host_io(_lib.LidarScanIO, SCAN_POINTERS, n_env=-1)
        assert scan(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
        assert scan(cfg, ctypes.byref(_lib.LidarScanIO()), None) == 0  # n_env == 0
        # the observe entry: all five bits, the cone only with a heading, LidarLine refused as today
        for flags in range(32):
            io = _lib.LidarObserveIO()
            io.flags = flags
            want = 0 if (heading or not flags & 8) and not line else _lib.DGPPO_EINVAL
            assert observe(cfg, ctypes.byref(io), deg, None) == want, (eid, flags)
        for bad in (32, 48, -1):
            io = _lib.LidarObserveIO()
            io.flags = bad
            assert observe(cfg, ctypes.byref(io), deg, None) == _lib.DGPPO_EINVAL, bad
        if not line:
            for field in OBSERVE_POINTERS:
                io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS, flags=16)
                setattr(io, field, None)
                assert observe(cfg, ctypes.byref(io), deg, None) == _lib.DGPPO_EINVAL, field
        # the three older entries keep refusing the new bit
        for flags in (16, 17, 20, 24):
            io = _lib.LidarObserveIO()
            io.flags = flags
            assert lib.dgppo_lidar_observe(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
            assert lib.dgppo_lidar_observe_los(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
            assert lib.dgppo_lidar_observe_fov(cfg, ctypes.byref(io), deg, None) == _lib.DGPPO_EINVAL
    for eid, kw in (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=0)), ("VMASWheel", {})):
        other = make_env(eid, 3, device="cpu", **kw)
        for n_env in (0, 1):
            io, keep = _host_io(_lib.LidarScanIO, SCAN_POINTERS, n_env=n_env)
            assert scan(ctypes.byref(other.cfg), ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (eid, n_env)
            io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS, n_env=n_env, flags=16)
            assert observe(ctypes.byref(other.cfg), ctypes.byref(io), deg, None) == _lib.DGPPO_EINVAL, (eid, n_env)


# ---- 3. the ops -----------------------------------------------------------------------------------------------------------
def test_ops_registered_and_trace_under_fake_tensors():
    alias = lambda x: re.sub(r"\(a\d+!\)", "(a!)", x)  # noqa: E731
    for new, old in (("lidar_scan_bodies", "lidar_scan"), ("lidar_observe_bodies", "lidar_observe_fov")):
        s = str(getattr(torch.ops.dgppo, new).default._schema)
        assert alias(s.replace(f"dgppo::{new}(", f"dgppo::{old}(")) == alias(
            str(getattr(torch.ops.dgppo, old).default._schema)), s
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n, R_, sd = 2, 3, 32, 4
    from torch._subclasses.fake_tensor import FakeTensorMode

    def observe(agent, goal, ob, rays, g):
        return torch.ops.dgppo.lidar_observe_bodies(env._cfg_handle, agent, goal, ob, rays, None, 3, 0, 1, 0.1,
                                                    float("-inf"), _lib.OBSERVE_NOISE | _lib.OBSERVE_BODIES, 180.0,
                                                    g.nodes, g.edges, g.states, g.receivers, g.senders)

    with FakeTensorMode():
        g = env.empty_graph((B,), "cpu")
        shapes = [tuple(getattr(g, f).shape) for f in ("nodes", "edges", "states", "receivers", "senders")]
        assert observe(torch.empty(B, n, sd), torch.empty(B, n, sd), torch.empty(B, 2, 16), torch.empty(R_, 2), g) is None
        assert [tuple(getattr(g, f).shape) for f in ("nodes", "edges", "states", "receivers", "senders")] == shapes
        alpha = torch.empty(B, n, R_)
        assert torch.ops.dgppo.lidar_scan_bodies(env._cfg_handle, torch.empty(B, n, sd), torch.empty(B, 2, 16),
                                                 torch.empty(R_, 2), alpha) is None
        assert tuple(alpha.shape) == (B, n, R_)
    with pytest.raises(_lib.NativeLibraryError):  # the real kernels have no CPU path
        observe(torch.zeros(B, n, sd), torch.zeros(B, n, sd), torch.zeros(B, 2, 16), torch.zeros(R_, 2),
                env.empty_graph((B,), "cpu"))
    with pytest.raises(_lib.NativeLibraryError):
        torch.ops.dgppo.lidar_scan_bodies(env._cfg_handle, torch.zeros(B, n, sd), torch.zeros(B, 2, 16),
                                          torch.zeros(R_, 2), torch.zeros(B, n, R_))


# ---- 4. refusals before any GPU call ------------------------------------------------------------------------------------
class _Actor:  # what an engine reads of its actor before the first run
    carry_width = 64


def _algo_kwargs(env, **kw):
    return dict(env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                action_dim=env.action_dim, n_agents=env.num_agents, batch_size=8, rnn_step=2, device="cpu", **kw)


ALGOS = ("dgppo", "informarl", "informarl_lagr")
REFUSED = [("MPESpread", dict(num_obs=3), ValueError, "no LiDAR"),
           ("VMASWheel", {}, NotImplementedError, "VMAS"),
           ("LidarSpread", dict(num_obs=0), ValueError, "no LiDAR"),
           ("LidarOmniTarget", dict(num_obs=0), ValueError, "no LiDAR")]


@pytest.mark.parametrize("eid,okw,exc,word", REFUSED, ids=lambda v: v if isinstance(v, str) else None)
def test_envs_without_a_lidar_refuse_bodies_everywhere(eid, okw, exc, word, monkeypatch):
    def no_gpu(*a, **k):
        raise AssertionError("the GPU was asked for")

    monkeypatch.setattr(_lib, "require_gpu", no_gpu)
    env = make_env(eid, 3, device="cpu", **okw)
    B, sd = 2, env.state_dim
    state = (torch.zeros(B, 3, sd), torch.zeros(B, env.num_goals, sd), torch.zeros(B, max(env.n_obs, 1), 16))
    with pytest.raises(exc, match=word):
        bodies_option(env, "test", True)
    assert bodies_option(env, "test", False) is False
    for algo in ALGOS:
        with pytest.raises(exc, match=word):
            make_algo(algo, **_algo_kwargs(env, lidar_bodies=True))
        a = make_algo(algo, **_algo_kwargs(env))
        assert a.bodies is False and not a.sensed
    with pytest.raises(exc, match=word):
        NoisyLidarRolloutEngine(env, B, 2, "cpu", actor=_Actor(), bodies=True)
    with pytest.raises(exc, match=word):
        SensorRolloutEngine(env, B, 2, "cpu", actor=_Actor(), sensor=None, bodies=True)
    with pytest.raises(exc, match=word):
        env.observe(state, 0, sigma=0.0, dropout=0.0, seed=1, bodies=True)
    with pytest.raises(exc, match=word):
        env.lidar_scan(state[0], state[2], bodies=True)


def test_hcbfcrpo_refuses_bodies_in_its_own_words():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    for flags in (dict(lidar_bodies=True), dict(lidar_bodies=True, lidar_noise=0.1)):
        with pytest.raises(ValueError, match="get_cost"):
            make_algo("hcbfcrpo", **_algo_kwargs(env, **flags))
    with pytest.raises(ValueError, match="HCBFCRPO.*lidar_bodies"):
        make_algo("hcbfcrpo", **_algo_kwargs(env, lidar_bodies=True))
    a = make_algo("hcbfcrpo", **_algo_kwargs(env))
    assert a.bodies is False and not a.sensed
    from dgppo_fov_amd.algo import HCBFCRPO

    with pytest.raises(ValueError, match="get_cost"):
        bodies_option(env, "test", True, algo_cls=HCBFCRPO)
    bare = make_env("MPESpread", 3, num_obs=3, device="cpu")  # the algorithm is refused before the env is looked at
    with pytest.raises(ValueError, match="get_cost"):
        make_algo("hcbfcrpo", **_algo_kwargs(bare, lidar_bodies=True))


@pytest.mark.parametrize("algo", ALGOS)
def test_algorithms_and_engines_accept_the_flag(algo):
    for eid in LIDAR:
        env = make_env(eid, 3, num_obs=2, device="cpu")
        a = make_algo(algo, **_algo_kwargs(env, lidar_bodies=True))
        assert a.bodies is True and a.sensed and a.sensing is None and a.sensor is None and a.fov is None  # on its own
        a = make_algo(algo, **_algo_kwargs(env, lidar_bodies=True, lidar_noise=0.1, lidar_occlusion=True))
        assert a.bodies is True and a.sensed and a.sensor == (0.1, 0.0) and a.occlusion is True
        a = make_algo(algo, **_algo_kwargs(env, lidar_noise=0.1))
        assert a.bodies is False and a.sensed
        a = make_algo(algo, **_algo_kwargs(env))
        assert a.bodies is False and not a.sensed


def test_engines_hold_the_flag_and_the_record_is_unchanged():
    env = make_env("LidarOmniTarget", 3, num_obs=2, device="cpu")
    e = NoisyLidarRolloutEngine(env, 2, 2, "cpu", actor=_Actor(), bodies=True)
    assert e.bodies is True and (e.sigma, e.dropout, e.occlusion, e.fov) == (0.0, 0.0, False, None)
    e = NoisyLidarRolloutEngine(env, 2, 2, "cpu", actor=_Actor(), sigma=0.1, fov=60, bodies=True)
    assert e.bodies is True and (e.sigma, e.fov) == (0.1, 60.0)
    assert NoisyLidarRolloutEngine(env, 2, 2, "cpu", actor=_Actor()).bodies is False
    e = SensorRolloutEngine(env, 2, 2, "cpu", actor=_Actor(), sensor=None, bodies=True)  # None: the identity
    alpha = torch.zeros(2, 3, 32)
    assert e.bodies is True and e.sensor(alpha, 0) is alpha and e.sensing is None
    e = SensorRolloutEngine(env, 2, 2, "cpu", actor=_Actor(), sensor=None, bodies=True, occlusion=True)
    assert e.bodies is True and e.occlusion and e.sensor(alpha, 0) is alpha
    assert SensorRolloutEngine(env, 2, 2, "cpu", actor=_Actor(), sensor=lambda a, t: a).bodies is False
    with pytest.raises(ValueError, match="sensor must be a callable"):  # without the flag None still needs a mask
        SensorRolloutEngine(env, 2, 2, "cpu", actor=_Actor(), sensor=None)
    import dataclasses

    assert [f.name for f in dataclasses.fields(Sensing)] == ["sigma", "dropout", "occlusion", "fov"]


# ---- 5. the op each call picks ------------------------------------------------------------------------------------------
class _Record(TorchDispatchMode):
    """The dgppo ops a call dispatches, with every argument, without running them."""

    def __init__(self, calls):
        super().__init__()
        self.calls = calls

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if func.namespace == "dgppo":
            self.calls.append((func._schema.name.split("::")[1], args))
            return None
        return func(*args, **(kwargs or {}))


def _same_args(a, b):
    return len(a) == len(b) and all((x is y) or (not isinstance(x, torch.Tensor) and x == y) or
                                    (isinstance(x, torch.Tensor) and isinstance(y, torch.Tensor)
                                     and x.data_ptr() == y.data_ptr() and x.shape == y.shape) for x, y in zip(a, b))


@pytest.mark.parametrize("eid", ["LidarSpread", "LidarOmniTarget"])
def test_bodies_false_is_todays_dispatch_and_true_picks_the_new_ops(eid, monkeypatch):
    env = make_env(eid, 3, num_obs=2, device="cpu")
    heading = eid == "LidarOmniTarget"
    B, n, sd = 2, 3, env.state_dim
    state = (torch.zeros(B, n, sd), torch.zeros(B, n, sd), torch.zeros(B, 2, 16))
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    out = env.empty_graph((B,), "cpu")
    options = [dict(), dict(occlusion=True)] + ([dict(fov=60.0), dict(fov=45.0, occlusion=True)] if heading else [])
    for opt in options:
        kw = dict(sigma=0.05, dropout=0.1, seed=1, out=out, **opt)
        today, off, on = [], [], []
        with _Record(today):
            env.observe(state, 0, **kw)
        with _Record(off):
            env.observe(state, 0, bodies=False, **kw)
        with _Record(on):
            env.observe(state, 0, bodies=True, **kw)
        assert len(today) == len(off) == len(on) == 1
        assert off[0][0] == today[0][0] and _same_args(off[0][1], today[0][1]), opt
        name, args = on[0]
        assert name == "lidar_observe_bodies" and len(args) == 18
        flags = 3 | 16 | (4 if opt.get("occlusion") else 0) | (8 if "fov" in opt else 0)
        assert args[11] == flags and args[12] == opt.get("fov", 180.0), opt
        told = today[0][1]
        assert _same_args(args[:11], told[:11]) and _same_args(args[13:], told[-5:])  # every other argument is today's
    today, off, on = [], [], []
    with _Record(today):
        a0 = env.lidar_scan(state[0], state[2])
    with _Record(off):
        a1 = env.lidar_scan(state[0], state[2], bodies=False)
    with _Record(on):
        a2 = env.lidar_scan(state[0], state[2], bodies=True)
    assert [c[0] for c in today + off + on] == ["lidar_scan", "lidar_scan", "lidar_scan_bodies"]
    for calls, alpha in ((today, a0), (off, a1), (on, a2)):
        (_, args), = calls
        assert args[0] == env._cfg_handle and args[1] is state[0] and args[2] is state[2] and args[4] is alpha
        assert tuple(alpha.shape) == (B, n, 32)


def test_lidar_line_takes_the_chained_path_with_the_bodies_scan(monkeypatch):
    env = make_env("LidarLine", 3, num_obs=2, device="cpu")
    B, n = 2, 3
    state = (torch.zeros(B, n, 4), torch.zeros(B, env.num_goals, 4), torch.zeros(B, 2, 16))
    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    for bodies, scan in ((False, "lidar_scan"), (True, "lidar_scan_bodies")):
        for occlusion in (False, True):
            calls = []
            with _Record(calls):
                env.observe(state, 0, sigma=0.0, dropout=0.0, seed=1, occlusion=occlusion, bodies=bodies)
            names = [c[0] for c in calls]
            assert names == (["lidar_sight"] if occlusion else []) + [scan, "lidar_hits", "env_get_graph_hits"]


# ---- 6. the command lines -----------------------------------------------------------------------------------------------
def _cli(name):
    spec = importlib.util.spec_from_file_location(f"dgppo_{name}_cli_bodies", os.path.join(ROOT, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_and_test_parsers_accept_the_flag(tmp_path):
    train = _cli("train")
    p = train.build_parser()
    base = ["--env", "LidarSpread", "-n", "3", "--algo", "dgppo", "--obs", "2"]
    assert p.parse_args(base).lidar_bodies is False
    a = p.parse_args(base + ["--lidar-bodies"])
    assert a.lidar_bodies is True and a.lidar_noise is None and a.lidar_occlusion is False and a.lidar_fov is None
    a = p.parse_args(base + ["--lidar-bodies", "--lidar-occlusion", "--lidar-noise", "0.02", "--lidar-dropout", "0.1",
                             "--lidar-fov", "60"])
    assert a.lidar_bodies is True and a.lidar_occlusion is True and (a.lidar_noise, a.lidar_dropout) == (0.02, 0.1)
    assert a.lidar_fov == 60.0
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--lidar-bodies", "1"])  # a switch, not a value
    tp = _cli("test").build_parser()
    assert tp.parse_args(["--path", "x"]).lidar_bodies is False
    a = tp.parse_args(["--path", "x", "--lidar-bodies"])
    assert a.lidar_bodies is True and a.lidar_noise is None and a.lidar_occlusion is False and a.lidar_fov is None
    a = tp.parse_args(["--path", "x", "--lidar-bodies", "--lidar-fov", "60", "--lidar-occlusion", "--lidar-dropout", "0.1",
                       "--lidar-noise", "0.05"])
    assert a.lidar_bodies is True and a.lidar_fov == 60.0 and a.lidar_occlusion is True and a.lidar_dropout == 0.1


def test_resume_may_not_change_the_flag(tmp_path):
    train = _cli("train")
    p = train.build_parser()
    base = ["--env", "LidarSpread", "-n", "3", "--algo", "dgppo", "--obs", "2"]
    assert "lidar_bodies" not in train.RESUME_FREE
    saved = dict(vars(p.parse_args(base + ["--lidar-bodies"])), _world_size=1)
    assert saved["lidar_bodies"] is True  # recorded with the run's arguments (train_args.json, config.yaml: vars(args))
    with open(tmp_path / "train_args.json", "w") as f:
        json.dump(saved, f)
    train.check_resume_args(p.parse_args(base + ["--lidar-bodies"]), str(tmp_path), world=1)
    with pytest.raises(SystemExit, match="lidar_bodies"):
        train.check_resume_args(p.parse_args(base), str(tmp_path), world=1)
    saved = dict(vars(p.parse_args(base)), _world_size=1)
    with open(tmp_path / "train_args.json", "w") as f:
        json.dump(saved, f)
    train.check_resume_args(p.parse_args(base), str(tmp_path), world=1)
    with pytest.raises(SystemExit, match="lidar_bodies"):
        train.check_resume_args(p.parse_args(base + ["--lidar-bodies"]), str(tmp_path), world=1)
    saved.pop("lidar_bodies")  # a run saved before the flag existed trained without it
    with open(tmp_path / "train_args.json", "w") as f:
        json.dump(saved, f)
    train.check_resume_args(p.parse_args(base), str(tmp_path), world=1)
    with pytest.raises(SystemExit, match="lidar_bodies"):
        train.check_resume_args(p.parse_args(base + ["--lidar-bodies"]), str(tmp_path), world=1)
