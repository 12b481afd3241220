"""Sensor in the loop without a GPU: the three C entry points' declarations, struct layouts and argument checks (none
of which launches), the torch ops' registration and fake kernels, ranges_to_alpha, the Python-side refusals on
device="cpu" envs, LidarNoise's identity case, and test.py's flags."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib, ops  # noqa: F401  (registers torch.ops.dgppo.*)
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.trainer.rollout import RolloutEngine, SensorRolloutEngine
from dgppo_fov_amd.utils.sensor import NO_RETURN, LidarNoise, ranges_to_alpha

from test_capi import ROOT, _c_layout, declared_functions

NEW = {"dgppo_lidar_scan": (_lib.LidarScanIO, "dgppo_lidar_scan_io", ("agent", "obstacles", "ray_dirs", "alpha")),
       "dgppo_lidar_hits": (_lib.LidarHitsIO, "dgppo_lidar_hits_io", ("agent", "alpha", "ray_dirs", "hits")),
       "dgppo_env_get_graph_hits": (_lib.EnvGraphHitsIO, "dgppo_env_graph_hits_io",
                                    ("agent", "goal", "hits", "nodes", "edges", "out_states", "receivers", "senders"))}


def test_header_signatures_and_exports_agree():
    lib = _lib.load()
    fns = declared_functions()
    for name, (struct, _, _) in NEW.items():
        assert name in fns and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert args == [ctypes.POINTER(_lib.EnvCfg), ctypes.POINTER(struct), ctypes.c_void_p]
    assert lib.dgppo_abi_version() == 14 == _lib.ABI_VERSION  # new symbols, no new ABI number


@pytest.mark.parametrize("name", sorted(NEW))
def test_ctypes_mirror_matches_c_layout(name):
    struct, cname, _ = NEW[name]
    names = [f[0] for f in struct._fields_]
    got = _c_layout(cname, names)
    assert got[0] == ctypes.sizeof(struct)
    for field, off in zip(names, got[1:]):
        assert getattr(struct, field).offset == off, field


def _host_io(name, n_env=1):
    """An io whose pointers are non-NULL host addresses: only for calls that return before any launch."""
    struct, _, pointers = NEW[name]
    buf = (ctypes.c_float * 4)()
    io = struct()
    for f in pointers:
        setattr(io, f, ctypes.addressof(buf))
    io.n_env = n_env
    return io, buf


@pytest.mark.parametrize("name", sorted(NEW))
def test_argument_checks_do_not_launch(name):
    fn = getattr(_lib.load(), name)
    struct, _, pointers = NEW[name]
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    cfg = ctypes.byref(env.cfg)
    io, keep = _host_io(name)
    assert fn(cfg, None, None) == _lib.DGPPO_EINVAL
    assert fn(None, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    for field in pointers:
        io, keep = _host_io(name)
        setattr(io, field, None)
        assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, field
    io, keep = _host_io(name, n_env=-1)
    assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    assert fn(cfg, ctypes.byref(struct()), None) == 0  # n_env == 0 is answered before any pointer is looked at
    # engines without a LiDAR, whatever the batch: MPE, a Lidar env without obstacles, VMAS
    for eid, kw in (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=0)), ("VMASWheel", {})):
        other = make_env(eid, 3, device="cpu", **kw)
        for n_env in (0, 1):
            io, keep = _host_io(name, n_env=n_env)
            assert fn(ctypes.byref(other.cfg), ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (eid, n_env)
    bad = _lib.EnvCfg()
    ctypes.memmove(ctypes.byref(bad), ctypes.byref(env.cfg), ctypes.sizeof(bad))
    bad.top_k = bad.n_rays + 1
    io, keep = _host_io(name)
    assert fn(ctypes.byref(bad), ctypes.byref(io), None) == _lib.DGPPO_EINVAL


def test_ops_registered_and_trace_under_fake_tensors():
    s = {n: str(getattr(torch.ops.dgppo, n).default._schema) for n in ("lidar_scan", "lidar_hits", "env_get_graph_hits")}
    # inputs are read-only, only the outputs are mutated
    assert re.fullmatch(r"dgppo::lidar_scan\((Sym)?[Ii]nt cfg, Tensor agent, Tensor obstacles, Tensor ray_dirs, "
                        r"Tensor\(a\d!\) alpha\) -> \(\)", s["lidar_scan"]), s["lidar_scan"]
    assert re.fullmatch(r"dgppo::lidar_hits\((Sym)?[Ii]nt cfg, Tensor agent, Tensor alpha, Tensor ray_dirs, "
                        r"Tensor\(a\d!\) hits\) -> \(\)", s["lidar_hits"]), s["lidar_hits"]
    assert re.fullmatch(r"dgppo::env_get_graph_hits\((Sym)?[Ii]nt cfg, Tensor agent, Tensor goal, Tensor hits, "
                        r"Tensor\(a\d!\) nodes, Tensor\(a\d!\) edges, Tensor\(a\d!\) states, Tensor\(a\d!\) receivers, "
                        r"Tensor\(a\d!\) senders\) -> \(\)", s["env_get_graph_hits"]), s["env_get_graph_hits"]
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n, R, k = 2, 3, 32, 8
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        agent, goal = torch.empty(B, n, 4), torch.empty(B, n, 4)
        alpha, hits = torch.empty(B, n, R), torch.empty(B, n, k, 2)
        g = env.empty_graph((B,), "cpu")
        assert torch.ops.dgppo.lidar_scan(env._cfg_handle, agent, torch.empty(B, 2, 16), torch.empty(R, 2), alpha) is None
        assert torch.ops.dgppo.lidar_hits(env._cfg_handle, agent, alpha, torch.empty(R, 2), hits) is None
        assert torch.ops.dgppo.env_get_graph_hits(env._cfg_handle, agent, goal, hits, g.nodes, g.edges, g.states,
                                                  g.receivers, g.senders) is None
    # the real kernels have no CPU path
    with pytest.raises(_lib.NativeLibraryError):
        torch.ops.dgppo.lidar_scan(env._cfg_handle, torch.zeros(B, n, 4), torch.zeros(B, 2, 16), torch.zeros(R, 2),
                                   torch.zeros(B, n, R))


def test_ranges_to_alpha():
    inf, nan = float("inf"), float("nan")
    r = torch.tensor([[0.0, 0.125, 0.5, 0.5000001, -0.1, nan, inf, -inf, 1e30]])
    a = ranges_to_alpha(r, 0.5)
    assert a.dtype == torch.float32 and a.shape == r.shape
    np.testing.assert_array_equal(a.numpy(), np.array([[0.0, 0.25, 1.0, 1e6, 1e6, 1e6, 1e6, 1e6, 1e6]], np.float32))
    assert NO_RETURN == 1e6
    np.testing.assert_array_equal(ranges_to_alpha(torch.tensor([0.3], dtype=torch.float64), 1.5).numpy(),
                                  (np.float32(0.3) / np.float32(1.5)).reshape(1))
    with pytest.raises(ValueError, match="ranges"):
        ranges_to_alpha(torch.tensor([1, 2]), 0.5)
    with pytest.raises(ValueError, match="sense_range"):
        ranges_to_alpha(r, 0.0)


def test_python_side_refusals_on_cpu_envs():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n, R, k = 2, 3, 32, 8
    agent, goal, ob = torch.zeros(B, n, 4), torch.zeros(B, n, 4), torch.zeros(B, 2, 16)
    alpha, hits = torch.zeros(B, n, R), torch.zeros(B, n, k, 2)
    # shapes and dtypes are named
    with pytest.raises(ValueError, match="lidar_scan: agent_states"):
        env.lidar_scan(agent[:, :2], ob)
    with pytest.raises(ValueError, match="lidar_scan: agent_states"):
        env.lidar_scan(agent[0], ob)
    with pytest.raises(ValueError, match="lidar_scan: agent_states must be float32"):
        env.lidar_scan(agent.double(), ob)
    with pytest.raises(ValueError, match="lidar_scan: obstacles"):
        env.lidar_scan(agent, ob[:, :1])
    with pytest.raises(ValueError, match="lidar_scan: obstacles"):
        env.lidar_scan(agent, None)
    with pytest.raises(ValueError, match="lidar_hits: alpha"):
        env.lidar_hits(agent, alpha[..., :-1])
    with pytest.raises(ValueError, match="lidar_hits: alpha must be float32"):
        env.lidar_hits(agent, alpha.double())
    with pytest.raises(ValueError, match="lidar_hits: agent_states"):
        env.lidar_hits(agent[..., :3], alpha)
    with pytest.raises(ValueError, match="get_graph: lidar_data"):
        env.get_graph((agent, goal, None), lidar_data=hits[:, :, :-1])
    with pytest.raises(ValueError, match="get_graph: lidar_data must be float32"):
        env.get_graph((agent, goal, None), lidar_data=hits.double())
    with pytest.raises(ValueError, match="state.agent"):
        env.get_graph((agent[:, :2], goal, None), lidar_data=hits)
    with pytest.raises(ValueError, match="state.obstacle"):
        env.get_graph((agent, goal, ob[:, :1]), lidar_data=hits)
    with pytest.raises(TypeError):
        env.get_graph((agent, goal, None), None, hits)  # keyword-only
    # a well-formed call on CPU tensors: there is no CPU kernel
    for call in (lambda: env.lidar_scan(agent, ob), lambda: env.lidar_hits(agent, alpha),
                 lambda: env.get_graph((agent, goal, None), lidar_data=hits),
                 lambda: env.get_graph((agent, goal, ob), lidar_data=hits)):
        with pytest.raises(_lib.NativeLibraryError):
            call()
    # envs without a LiDAR
    for eid, kw in (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=0))):
        e = make_env(eid, n, device="cpu", **kw)
        with pytest.raises(ValueError, match="no LiDAR"):
            e.lidar_scan(agent, ob)
        with pytest.raises(ValueError, match="no LiDAR"):
            e.lidar_hits(agent, alpha)
        with pytest.raises(ValueError, match="no LiDAR"):
            e.get_graph((agent, goal, None), lidar_data=hits)
        with pytest.raises(ValueError, match="no LiDAR"):
            SensorRolloutEngine(e, B, 2, "cpu", actor=object(), sensor=lambda a, t: a)
    vm = make_env("VMASWheel", 3, device="cpu")
    for call in (lambda: vm.lidar_scan(agent, ob), lambda: vm.lidar_hits(agent, alpha),
                 lambda: vm.get_graph((agent, goal, None), lidar_data=hits)):
        with pytest.raises(NotImplementedError):
            call()
    # the engine's own argument checks
    with pytest.raises(ValueError, match="sensor must be a callable"):
        SensorRolloutEngine(env, B, 2, "cpu", actor=object(), sensor=None)
    with pytest.raises(ValueError, match="needs an actor"):
        SensorRolloutEngine(env, B, 2, "cpu", actor=None, sensor=lambda a, t: a)
    with pytest.raises(ValueError, match="needs an actor"):
        SensorRolloutEngine(env, B, 2, "cpu", actor=object(), mode=RolloutEngine.MODE_RANDOM, sensor=lambda a, t: a)


def test_step_on_a_sensor_only_graph_says_it_has_no_obstacles():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    g = env.empty_graph((2,), "cpu")  # a graph without obstacle records, as get_graph((agent, goal, None), ...) returns
    assert g.env_states.obstacle is None
    with pytest.raises(ValueError, match="carries no obstacles"):
        env._obstacles_of(g)


def test_lidar_noise_identity_and_refusals():
    x = torch.rand(2, 3, 32)
    x[0, 0, 0], x[0, 0, 1] = float("nan"), 1e6
    same = LidarNoise(0.0, 0.0, seed=3)(x, 5)
    assert same is x  # the input bits
    with pytest.raises(_lib.NativeLibraryError):
        LidarNoise(0.01, 0.0, seed=3)(x, 0)
    with pytest.raises(_lib.NativeLibraryError):
        LidarNoise(0.0, 0.5, seed=3)(x, 0)
    for bad in (dict(sigma=-1.0), dict(sigma=float("nan")), dict(dropout=1.5), dict(dropout=-0.1), dict(sense_range=0.0)):
        with pytest.raises(ValueError):
            LidarNoise(**bad)
    # Phi^-1 of the dropout probability, its ends exact
    assert LidarNoise(dropout=0.5)._drop_below == 0.0
    assert LidarNoise(dropout=1.0)._drop_below == float("inf") and LidarNoise(dropout=0.0)._drop_below == -float("inf")
    assert abs(LidarNoise(dropout=0.975)._drop_below - 1.959964) < 1e-5


def test_cli_parser_accepts_the_sensor_flags():
    spec = importlib.util.spec_from_file_location("dgppo_test_cli", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    a = p.parse_args(["--path", "x"])
    assert a.lidar_noise is None and a.lidar_dropout is None
    a = p.parse_args(["--path", "x", "--lidar-noise", "0.02", "--lidar-dropout", "0.1"])
    assert a.lidar_noise == 0.02 and a.lidar_dropout == 0.1
    a = p.parse_args(["--path", "x", "--lidar-dropout", "1"])
    assert a.lidar_noise is None and a.lidar_dropout == 1.0
    with pytest.raises(SystemExit):
        p.parse_args(["--path", "x", "--lidar-noise", "loud"])
