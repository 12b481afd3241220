"""Training under the LiDAR sensor model without a GPU: dgppo_lidar_observe's declaration, struct layout and argument
checks (none of which launches), the torch op's registration and fake kernel, env.observe's and the algorithms'
refusals on device="cpu" envs, and train.py's flags."""
import ctypes
import importlib.util
import os
import re

import pytest
import torch

from dgppo_fov_amd import _lib, ops  # noqa: F401  (registers torch.ops.dgppo.*)
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.trainer.rollout import NoisyLidarRolloutEngine, RolloutEngine

from test_capi import ROOT, _c_layout, declared_functions

POINTERS = ("agent", "goal", "obstacles", "ray_dirs", "nodes", "edges", "out_states", "receivers", "senders")


def test_header_signature_and_export_agree():
    lib = _lib.load()
    assert "dgppo_lidar_observe" in declared_functions() and hasattr(lib, "dgppo_lidar_observe")
    res, args = _lib.SIGNATURES["dgppo_lidar_observe"]
    assert res is ctypes.c_int
    assert args == [ctypes.POINTER(_lib.EnvCfg), ctypes.POINTER(_lib.LidarObserveIO), ctypes.c_void_p]
    assert lib.dgppo_abi_version() == 14 == _lib.ABI_VERSION  # a new symbol, no new ABI number


def test_ctypes_mirror_matches_c_layout():
    names = [f[0] for f in _lib.LidarObserveIO._fields_]
    got = _c_layout("dgppo_lidar_observe_io", names)
    assert got[0] == ctypes.sizeof(_lib.LidarObserveIO)
    for field, off in zip(names, got[1:]):
        assert getattr(_lib.LidarObserveIO, field).offset == off, field


def _host_io(n_env=1):
    """An io whose pointers are non-NULL host addresses: only for calls that return before any launch."""
    buf = (ctypes.c_float * 4)()
    io = _lib.LidarObserveIO()
    for f in POINTERS:
        setattr(io, f, ctypes.addressof(buf))
    io.n_env = n_env
    return io, buf


def test_argument_checks_do_not_launch():
    fn = _lib.load().dgppo_lidar_observe
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    cfg = ctypes.byref(env.cfg)
    io, keep = _host_io()
    assert fn(cfg, None, None) == _lib.DGPPO_EINVAL
    assert fn(None, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    for field in POINTERS:
        io, keep = _host_io()
        setattr(io, field, None)
        assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, field
    for field, bad in (("n_env", -1), ("t", -1), ("env_offset", -1), ("flags", 4)):
        io, keep = _host_io()
        setattr(io, field, bad)
        assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, field
    assert fn(cfg, ctypes.byref(_lib.LidarObserveIO()), None) == 0  # n_env == 0: answered before any pointer is read
    # MPE, a Lidar env without obstacles, VMAS, and the LidarLine variant (env.observe chains the launches for it)
    for eid, kw in (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=0)), ("VMASWheel", {}),
                    ("LidarLine", dict(num_obs=2))):
        other = make_env(eid, 3, device="cpu", **kw)
        for n_env in (0, 1):
            io, keep = _host_io(n_env=n_env)
            assert fn(ctypes.byref(other.cfg), ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (eid, n_env)


def test_op_registered_and_traces_under_fake_tensors():
    s = str(torch.ops.dgppo.lidar_observe.default._schema)
    # inputs are read-only, only the five graph tensors are mutated
    assert re.fullmatch(r"dgppo::lidar_observe\((Sym)?[Ii]nt cfg, Tensor agent, Tensor goal, Tensor obstacles, "
                        r"Tensor ray_dirs, Tensor\? key, (Sym)?[Ii]nt seed, (Sym)?[Ii]nt env_offset, (Sym)?[Ii]nt t, "
                        r"float noise_scale, float drop_below, (Sym)?[Ii]nt flags, Tensor\(a\d+!\) nodes, "
                        r"Tensor\(a\d+!\) edges, Tensor\(a\d+!\) states, Tensor\(a\d+!\) receivers, "
                        r"Tensor\(a\d+!\) senders\) -> \(\)", s), s
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n, R = 2, 3, 32
    from torch._subclasses.fake_tensor import FakeTensorMode

    def call(agent, goal, ob, rays, g):
        return torch.ops.dgppo.lidar_observe(env._cfg_handle, agent, goal, ob, rays, None, 3, 0, 1, 0.1, float("-inf"),
                                             _lib.OBSERVE_NOISE, g.nodes, g.edges, g.states, g.receivers, g.senders)

    with FakeTensorMode():
        g = env.empty_graph((B,), "cpu")
        shapes = [tuple(getattr(g, f).shape) for f in ("nodes", "edges", "states", "receivers", "senders")]
        assert call(torch.empty(B, n, 4), torch.empty(B, n, 4), torch.empty(B, 2, 16), torch.empty(R, 2), g) is None
        assert [tuple(getattr(g, f).shape) for f in ("nodes", "edges", "states", "receivers", "senders")] == shapes
    with pytest.raises(_lib.NativeLibraryError):  # the real kernel has no CPU path
        call(torch.zeros(B, n, 4), torch.zeros(B, n, 4), torch.zeros(B, 2, 16), torch.zeros(R, 2),
             env.empty_graph((B,), "cpu"))


def test_observe_refusals_on_cpu_envs():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n = 2, 3
    agent, goal, ob = torch.zeros(B, n, 4), torch.zeros(B, n, 4), torch.zeros(B, 2, 16)
    kw = dict(sigma=0.05, dropout=0.1, seed=1)
    with pytest.raises(ValueError, match="state.agent"):
        env.observe((agent[:, :2], goal, ob), 0, **kw)
    with pytest.raises(ValueError, match="state.obstacle"):
        env.observe((agent, goal, None), 0, **kw)
    with pytest.raises(ValueError, match="sigma"):
        env.observe((agent, goal, ob), 0, sigma=-1.0, dropout=0.0, seed=1)
    with pytest.raises(ValueError, match="dropout"):
        env.observe((agent, goal, ob), 0, sigma=0.0, dropout=1.5, seed=1)
    with pytest.raises(ValueError, match="t and env_offset"):
        env.observe((agent, goal, ob), -1, **kw)
    with pytest.raises(ValueError, match="tensor seed"):
        env.observe((agent, goal, ob), 0, sigma=0.0, dropout=0.0, seed=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(TypeError):
        env.observe((agent, goal, ob), 0, 0.05, 0.1, 1)  # keyword-only
    with pytest.raises(_lib.NativeLibraryError):  # a well-formed call on CPU tensors: there is no CPU kernel
        env.observe((agent, goal, ob), 0, **kw)
    for eid, okw in (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=0))):
        e = make_env(eid, n, device="cpu", **okw)
        with pytest.raises(ValueError, match="no LiDAR"):
            e.observe((agent, goal, ob), 0, **kw)
        with pytest.raises(ValueError, match="no LiDAR"):
            NoisyLidarRolloutEngine(e, B, 2, "cpu", actor=object(), sigma=0.1)
    with pytest.raises(NotImplementedError):
        make_env("VMASWheel", 3, device="cpu").observe((agent, goal, ob), 0, **kw)
    with pytest.raises(ValueError, match="needs an actor"):
        NoisyLidarRolloutEngine(env, B, 2, "cpu", actor=None, sigma=0.1)
    with pytest.raises(ValueError, match="needs an actor"):
        NoisyLidarRolloutEngine(env, B, 2, "cpu", actor=object(), mode=RolloutEngine.MODE_RANDOM, sigma=0.1)
    with pytest.raises(ValueError, match="sigma"):
        NoisyLidarRolloutEngine(env, B, 2, "cpu", actor=object(), sigma=-0.1)


def _algo_kwargs(env, **kw):
    return dict(env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                action_dim=env.action_dim, n_agents=env.num_agents, batch_size=8, rnn_step=2, device="cpu", **kw)


@pytest.mark.parametrize("algo", ["dgppo", "informarl", "informarl_lagr"])
def test_algorithms_refuse_what_cannot_train_under_the_sensor(algo):
    lidar = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    for eid, okw in (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=0)), ("VMASWheel", {})):
        e = make_env(eid, 3, device="cpu", **okw)
        for flags in (dict(lidar_noise=0.1), dict(lidar_dropout=0.2), dict(lidar_noise=0.0, lidar_dropout=0.0)):
            with pytest.raises(ValueError, match="no LiDAR"):
                make_algo(algo, **_algo_kwargs(e, **flags))
    with pytest.raises(ValueError, match="sigma"):
        make_algo(algo, **_algo_kwargs(lidar, lidar_noise=-0.1))
    for p in (-0.1, 1.5):
        with pytest.raises(ValueError, match="dropout"):
            make_algo(algo, **_algo_kwargs(lidar, lidar_dropout=p))


def test_hcbfcrpo_refuses_the_sensor_flags():
    lidar = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    for flags in (dict(lidar_noise=0.1), dict(lidar_dropout=0.2), dict(lidar_noise=0.0, lidar_dropout=0.0)):
        with pytest.raises(ValueError, match="get_cost"):
            make_algo("hcbfcrpo", **_algo_kwargs(lidar, **flags))


def test_train_parser_accepts_the_sensor_flags():
    spec = importlib.util.spec_from_file_location("dgppo_train_cli", os.path.join(ROOT, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    p = mod.build_parser()
    base = ["--env", "LidarSpread", "-n", "3", "--algo", "dgppo", "--obs", "2"]
    a = p.parse_args(base)
    assert a.lidar_noise is None and a.lidar_dropout is None
    a = p.parse_args(base + ["--lidar-noise", "0.02", "--lidar-dropout", "0.1"])
    assert a.lidar_noise == 0.02 and a.lidar_dropout == 0.1
    a = p.parse_args(base + ["--lidar-dropout", "1"])
    assert a.lidar_noise is None and a.lidar_dropout == 1.0
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--lidar-noise", "loud"])
    # refused before the GPU is touched
    for bad in (["--lidar-noise", "-1"], ["--lidar-dropout", "1.5"]):
        with pytest.raises(SystemExit, match="--lidar-noise must be"):
            mod.train(p.parse_args(base + bad))
    # flags a resumed run may not change
    assert "lidar_noise" not in mod.RESUME_FREE and "lidar_dropout" not in mod.RESUME_FREE
