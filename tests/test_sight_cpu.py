"""Line-of-sight neighbour sensing without a GPU: the NumPy reference (tests/sight_ref.py) on hand-made known answers,
utils.sensor.mask_unseen on CPU tensors, dgppo_lidar_sight's and dgppo_lidar_observe_los's declarations, struct layout
and argument checks (none of which launches), the torch ops' registration and fake kernels, and the refusals and flags
of env.line_of_sight / env.observe / make_algo / train.py / test.py on device="cpu" envs."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib, ops  # noqa: F401  (registers torch.ops.dgppo.*)
from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.trainer.rollout import NoisyLidarRolloutEngine, SensorRolloutEngine
from dgppo_fov_amd.utils.sensor import mask_unseen
from oracle import env as O

import sight_ref as S
from test_capi import ROOT, _c_layout, declared_functions

F = np.float32
OBSERVE_POINTERS = ("agent", "goal", "obstacles", "ray_dirs", "nodes", "edges", "out_states", "receivers", "senders")
SIGHT_POINTERS = ("agent", "obstacles", "visible")


# ---- 1. the reference ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(S.kat_scenes()))
def test_reference_known_answers(name):
    agent, obst, expect = S.kat_scenes()[name]
    got = S.line_of_sight_ref(agent[None], obst[None])[0]
    np.testing.assert_array_equal(got, expect)
    assert got.diagonal().all()


def test_reference_nan_corner_poisons_its_own_edges_only():
    agent, obst, _ = S.kat_scenes()["NaN corner, across a clean edge"]
    valid = S.edge_valid(agent[0, 0], agent[0, 1], agent[1, 0], agent[1, 1], obst[0])
    # edges 0 and 1 touch the NaN corner: invalid, not "blocked"; edge 3 (the bottom side) is crossed; edge 2 is parallel
    np.testing.assert_array_equal(valid, [False, False, False, True])


def test_reference_directions_are_computed_on_their_own_and_agents_do_not_occlude():
    sq = S.square(1.0, 1.0, 0.5)[None]
    # three agents in a row left of the square: the middle one does not hide the outer two from each other
    agent = np.array([[0.1, 1.0], [0.3, 1.0], [0.5, 1.0]], F)
    assert S.line_of_sight_ref(agent[None], sq[None]).all()
    # the mask is the agents' alone: a reset scene's mask is the same with the goals anywhere, and both directions
    # of a pair are evaluated (the matrix need not be symmetric by construction, but is entry-wise defined)
    spec = O.Spec("LidarSpread", 8, 3)
    ag, _, ob = O.env_reset(spec, 7, 32)
    vis = S.line_of_sight_ref(ag, ob)
    inr = S.in_range_ref(spec, ag)
    assert int((~vis & inr).sum()) == 14 and int(inr.sum()) == 420  # blocked / in-range pairs of this scene set
    for b, i, j in np.argwhere(~vis)[:8]:
        one = S.edge_valid(ag[b, i, 0], ag[b, i, 1], ag[b, j, 0], ag[b, j, 1], ob[b])
        assert one.any()


def test_observed_graph_ref_changes_receivers_and_senders_only():
    spec = O.Spec("LidarSpread", 8, 3)
    ag, gl, ob = O.env_reset(spec, 7, 32)
    hits, _ = O.lidar(np.ascontiguousarray(ag[..., :2]), ob, O.ray_table(spec.n_rays, spec.comm_r), spec.top_k)
    true = O.build_graph(spec, ag, gl, hits)
    seen = S.observed_graph_ref(spec, ag, gl, ob, hits)
    for f in ("nodes", "edges", "states"):
        np.testing.assert_array_equal(seen[f], true[f])
    n, pad = spec.n, spec.n_nodes - 1
    vis = S.line_of_sight_ref(ag, ob).reshape(32, n * n)
    for f in ("receivers", "senders"):
        np.testing.assert_array_equal(seen[f][:, n * n:], true[f][:, n * n:])
        np.testing.assert_array_equal(seen[f][:, :n * n][vis], true[f][:, :n * n][vis])
        assert (seen[f][:, :n * n][~vis] == pad).all()
    assert (seen["receivers"] != true["receivers"]).sum() == 14  # the in-range blocked pairs


# ---- 2. mask_unseen -------------------------------------------------------------------------------------------------------
def test_mask_unseen_on_cpu_tensors():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    n, pad = 3, env.n_nodes - 1
    for batch in ((2,), (2, 4)):
        g = env.empty_graph(batch, "cpu")
        g.receivers.copy_(torch.arange(g.receivers.numel(), dtype=torch.int32).view_as(g.receivers) % 7)
        g.senders.copy_(torch.arange(g.senders.numel(), dtype=torch.int32).view_as(g.senders) % 5)
        g.edges.fill_(3.0), g.nodes.fill_(2.0), g.states.fill_(1.0)
        before = {f: getattr(g, f).clone() for f in ("nodes", "edges", "states", "receivers", "senders")}
        visible = torch.ones(batch + (n, n), dtype=torch.bool)
        visible[..., 0, 2] = False
        visible[(1,) + (0,) * (len(batch) - 1) + (2, 1)] = False
        out = mask_unseen(g, visible)
        assert out is g and out.receivers.data_ptr() == g.receivers.data_ptr()  # in place
        hide = ~visible.reshape(batch + (n * n,))
        for f in ("receivers", "senders"):
            got = getattr(g, f)
            assert torch.equal(got[..., n * n:], before[f][..., n * n:])
            assert bool((got[..., :n * n][hide] == pad).all())
            assert torch.equal(got[..., :n * n][~hide], before[f][..., :n * n][~hide])
        for f in ("nodes", "edges", "states"):
            assert torch.equal(getattr(g, f), before[f])
    # a strided view (a time-major buffer's transpose) is edited in place too
    buf = env.empty_graph((4, 2), "cpu")
    buf.receivers.zero_(), buf.senders.zero_()
    tr = env._assemble(*(getattr(buf, f).transpose(0, 1) for f in ("nodes", "edges", "states", "receivers", "senders")),
                       None)
    vis = torch.ones(2, 4, n, n, dtype=torch.bool)
    vis[1, 3, 2, 0] = False
    mask_unseen(tr, vis)
    assert int(buf.receivers[3, 1, 2 * n + 0]) == pad and int((buf.receivers == pad).sum()) == 1
    with pytest.raises(ValueError, match="bool"):
        mask_unseen(g, torch.ones(2, 4, n, n))
    with pytest.raises(ValueError, match="visible must be"):
        mask_unseen(g, torch.ones(2, n, n, dtype=torch.bool))
    with pytest.raises(ValueError, match="visible must be"):
        mask_unseen(g, torch.ones(2, 4, n, n + 1, dtype=torch.bool))


# ---- 3. the C entries ---------------------------------------------------------------------------------------------------
def test_header_signatures_and_exports_agree():
    lib = _lib.load()
    for name, io in (("dgppo_lidar_sight", _lib.LidarSightIO), ("dgppo_lidar_observe_los", _lib.LidarObserveIO)):
        assert name in declared_functions() and hasattr(lib, name)
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int
        assert args == [ctypes.POINTER(_lib.EnvCfg), ctypes.POINTER(io), ctypes.c_void_p]
    assert lib.dgppo_abi_version() == 14 == _lib.ABI_VERSION  # new symbols, no new ABI number
    with open(os.path.join(ROOT, "include", "dgppo_hip.h")) as f:
        assert re.search(r"#define\s+DGPPO_OBSERVE_SIGHT\s+4\b", f.read())
    assert _lib.OBSERVE_SIGHT == 4


def test_ctypes_mirror_matches_c_layout():
    names = [f[0] for f in _lib.LidarSightIO._fields_]
    assert names == ["agent", "agent_stride", "obstacles", "obstacles_stride", "visible", "visible_stride", "n_env"]
    got = _c_layout("dgppo_lidar_sight_io", names)
    assert got[0] == ctypes.sizeof(_lib.LidarSightIO)
    for field, off in zip(names, got[1:]):
        assert getattr(_lib.LidarSightIO, field).offset == off, field


def _host_io(cls, pointers, n_env=1):
    """An io whose pointers are non-NULL host addresses: only for calls that return before any launch."""
    buf = (ctypes.c_float * 4)()
    io = cls()
    for f in pointers:
        setattr(io, f, ctypes.addressof(buf))
    io.n_env = n_env
    return io, buf


UNSUPPORTED = (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=0)), ("VMASWheel", {}))


def test_sight_argument_checks_do_not_launch():
    fn = _lib.load().dgppo_lidar_sight
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    cfg = ctypes.byref(env.cfg)
    io, keep = _host_io(_lib.LidarSightIO, SIGHT_POINTERS)
    assert fn(cfg, None, None) == _lib.DGPPO_EINVAL
    assert fn(None, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    for field in SIGHT_POINTERS:
        io, keep = _host_io(_lib.LidarSightIO, SIGHT_POINTERS)
        setattr(io, field, None)
        assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, field
    io, keep = _host_io(_lib.LidarSightIO, SIGHT_POINTERS, n_env=-1)
    assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    assert fn(cfg, ctypes.byref(_lib.LidarSightIO()), None) == 0  # n_env == 0: answered before any pointer is read
    line = make_env("LidarLine", 3, num_obs=2, device="cpu")  # the variant is served: positions and obstacles only
    assert fn(ctypes.byref(line.cfg), ctypes.byref(_lib.LidarSightIO()), None) == 0
    for eid, kw in UNSUPPORTED:
        other = make_env(eid, 3, device="cpu", **kw)
        for n_env in (0, 1):
            io, keep = _host_io(_lib.LidarSightIO, SIGHT_POINTERS, n_env=n_env)
            assert fn(ctypes.byref(other.cfg), ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (eid, n_env)


def test_observe_los_argument_checks_do_not_launch():
    lib = _lib.load()
    fn = lib.dgppo_lidar_observe_los
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    cfg = ctypes.byref(env.cfg)
    io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS)
    assert fn(cfg, None, None) == _lib.DGPPO_EINVAL
    assert fn(None, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    for flags in (0, 4, 7):
        for field in OBSERVE_POINTERS:
            io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS)
            io.flags = flags
            setattr(io, field, None)
            assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (field, flags)
    for field, bad in (("n_env", -1), ("t", -1), ("env_offset", -1), ("flags", 8), ("flags", 12), ("flags", -1)):
        io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS)
        setattr(io, field, bad)
        assert fn(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (field, bad)
    for flags in (0, 4, 5, 6, 7):  # every accepted flag set; n_env == 0 is answered before any pointer is read
        io = _lib.LidarObserveIO()
        io.flags = flags
        assert fn(cfg, ctypes.byref(io), None) == 0, flags
    # dgppo_lidar_observe keeps refusing the new bit
    io = _lib.LidarObserveIO()
    io.flags = _lib.OBSERVE_SIGHT
    assert lib.dgppo_lidar_observe(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    for eid, kw in UNSUPPORTED + (("LidarLine", dict(num_obs=2)),):  # LidarLine: env.observe masks the chained graph
        other = make_env(eid, 3, device="cpu", **kw)
        for n_env in (0, 1):
            io, keep = _host_io(_lib.LidarObserveIO, OBSERVE_POINTERS, n_env=n_env)
            io.flags = _lib.OBSERVE_SIGHT
            assert fn(ctypes.byref(other.cfg), ctypes.byref(io), None) == _lib.DGPPO_EINVAL, (eid, n_env)


# ---- 4. the ops -----------------------------------------------------------------------------------------------------------
def test_ops_registered_and_trace_under_fake_tensors():
    s = str(torch.ops.dgppo.lidar_observe_los.default._schema)
    old = str(torch.ops.dgppo.lidar_observe.default._schema)
    assert s.replace("dgppo::lidar_observe_los(", "dgppo::lidar_observe(") == old  # lidar_observe's schema
    s = str(torch.ops.dgppo.lidar_sight.default._schema)
    assert re.fullmatch(r"dgppo::lidar_sight\((Sym)?[Ii]nt cfg, Tensor agent, Tensor obstacles, "
                        r"Tensor\(a\d+!\) visible\) -> \(\)", s), s
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n, R = 2, 3, 32
    from torch._subclasses.fake_tensor import FakeTensorMode

    def observe(agent, goal, ob, rays, g):
        return torch.ops.dgppo.lidar_observe_los(env._cfg_handle, agent, goal, ob, rays, None, 3, 0, 1, 0.1,
                                                 float("-inf"), _lib.OBSERVE_NOISE | _lib.OBSERVE_SIGHT, g.nodes,
                                                 g.edges, g.states, g.receivers, g.senders)

    with FakeTensorMode():
        g = env.empty_graph((B,), "cpu")
        shapes = [tuple(getattr(g, f).shape) for f in ("nodes", "edges", "states", "receivers", "senders")]
        assert observe(torch.empty(B, n, 4), torch.empty(B, n, 4), torch.empty(B, 2, 16), torch.empty(R, 2), g) is None
        assert [tuple(getattr(g, f).shape) for f in ("nodes", "edges", "states", "receivers", "senders")] == shapes
        vis = torch.empty(B, n, n, dtype=torch.uint8)
        assert torch.ops.dgppo.lidar_sight(env._cfg_handle, torch.empty(B, n, 4), torch.empty(B, 2, 16), vis) is None
        assert tuple(vis.shape) == (B, n, n)
    with pytest.raises(_lib.NativeLibraryError):  # the real kernels have no CPU path
        observe(torch.zeros(B, n, 4), torch.zeros(B, n, 4), torch.zeros(B, 2, 16), torch.zeros(R, 2),
                env.empty_graph((B,), "cpu"))
    with pytest.raises(_lib.NativeLibraryError):
        torch.ops.dgppo.lidar_sight(env._cfg_handle, torch.zeros(B, n, 4), torch.zeros(B, 2, 16),
                                    torch.zeros(B, n, n, dtype=torch.uint8))


# ---- 5. the env, the engines, the algorithms ---------------------------------------------------------------------------
def test_line_of_sight_and_observe_refusals_on_cpu_envs():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n = 2, 3
    agent, goal, ob = torch.zeros(B, n, 4), torch.zeros(B, n, 4), torch.zeros(B, 2, 16)
    with pytest.raises(ValueError, match="agent_states"):
        env.line_of_sight(agent[:, :2], ob)
    with pytest.raises(ValueError, match="obstacles"):
        env.line_of_sight(agent, ob[:, :1])
    with pytest.raises(_lib.NativeLibraryError):  # a well-formed call on CPU tensors: there is no CPU kernel
        env.line_of_sight(agent, ob)
    kw = dict(sigma=0.0, dropout=0.0, seed=1, occlusion=True)
    with pytest.raises(_lib.NativeLibraryError):
        env.observe((agent, goal, ob), 0, **kw)
    with pytest.raises(ValueError, match="state.obstacle"):
        env.observe((agent, goal, None), 0, **kw)
    for eid, okw in (("MPESpread", dict(num_obs=3)), ("LidarSpread", dict(num_obs=0))):
        e = make_env(eid, n, device="cpu", **okw)
        with pytest.raises(ValueError, match="no LiDAR"):  # before any launch
            e.line_of_sight(agent, ob)
        with pytest.raises(ValueError, match="no LiDAR"):
            e.observe((agent, goal, ob), 0, **kw)
        with pytest.raises(ValueError, match="no LiDAR"):
            NoisyLidarRolloutEngine(e, B, 2, "cpu", actor=object(), occlusion=True)
        with pytest.raises(ValueError, match="no LiDAR"):
            SensorRolloutEngine(e, B, 2, "cpu", actor=object(), sensor=None, occlusion=True)
    vmas = make_env("VMASWheel", 3, device="cpu")
    with pytest.raises(NotImplementedError):
        vmas.line_of_sight(agent, ob)
    with pytest.raises(NotImplementedError):
        vmas.observe((agent, goal, ob), 0, **kw)
    with pytest.raises(ValueError, match="sensor must be a callable"):  # None means identity only with occlusion
        SensorRolloutEngine(env, B, 2, "cpu", actor=object(), sensor=None)


def test_observe_without_occlusion_keeps_the_old_op(monkeypatch):
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n = 2, 3
    state = (torch.zeros(B, n, 4), torch.zeros(B, n, 4), torch.zeros(B, 2, 16))
    from torch.utils._python_dispatch import TorchDispatchMode

    calls = []
    watched = {torch.ops.dgppo.lidar_observe.default: "lidar_observe",
               torch.ops.dgppo.lidar_observe_los.default: "lidar_observe_los"}

    class Record(TorchDispatchMode):  # the op env.observe picks and its flags, without running it
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if func in watched:
                calls.append((watched[func], args[11]))
                return None
            return func(*args, **(kwargs or {}))

    monkeypatch.setattr(_lib, "require_gpu", lambda *a, **k: None)
    with Record():
        env.observe(state, 0, sigma=0.05, dropout=0.1, seed=1)
        env.observe(state, 0, sigma=0.05, dropout=0.1, seed=1, occlusion=False)
        env.observe(state, 0, sigma=0.05, dropout=0.0, seed=1, occlusion=True)
        env.observe(state, 0, sigma=0.0, dropout=0.0, seed=1, occlusion=True)
    assert calls == [("lidar_observe", 3), ("lidar_observe", 3), ("lidar_observe_los", 1 | 4), ("lidar_observe_los", 4)]


def _algo_kwargs(env, **kw):
    return dict(env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                action_dim=env.action_dim, n_agents=env.num_agents, batch_size=8, rnn_step=2, device="cpu", **kw)


@pytest.mark.parametrize("algo", ["dgppo", "informarl", "informarl_lagr"])
def test_algorithms_accept_occlusion_and_refuse_what_cannot_train_under_it(algo):
    lidar = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    a = make_algo(algo, **_algo_kwargs(lidar, lidar_occlusion=True))
    assert a.sensor is None and a.occlusion is True and a.sensed  # occlusion has its own attribute
    a = make_algo(algo, **_algo_kwargs(lidar, lidar_occlusion=True, lidar_noise=0.1))
    assert a.sensor == (0.1, 0.0) and a.occlusion is True
    a = make_algo(algo, **_algo_kwargs(lidar))
    assert a.sensor is None and a.occlusion is False and not a.sensed
    for eid, okw in UNSUPPORTED:
        e = make_env(eid, 3, device="cpu", **okw)
        with pytest.raises(ValueError, match="no LiDAR"):
            make_algo(algo, **_algo_kwargs(e, lidar_occlusion=True))
        assert make_algo(algo, **_algo_kwargs(e)).occlusion is False


def test_hcbfcrpo_refuses_occlusion():
    lidar = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    for flags in (dict(lidar_occlusion=True), dict(lidar_occlusion=True, lidar_noise=0.1)):
        with pytest.raises(ValueError, match="get_cost"):
            make_algo("hcbfcrpo", **_algo_kwargs(lidar, **flags))
    assert make_algo("hcbfcrpo", **_algo_kwargs(lidar)).occlusion is False


def _cli(name):
    spec = importlib.util.spec_from_file_location(f"dgppo_{name}_cli_sight", os.path.join(ROOT, f"{name}.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_train_and_test_parsers_accept_the_flag(tmp_path):
    train = _cli("train")
    p = train.build_parser()
    base = ["--env", "LidarSpread", "-n", "3", "--algo", "dgppo", "--obs", "2"]
    assert p.parse_args(base).lidar_occlusion is False
    a = p.parse_args(base + ["--lidar-occlusion"])
    assert a.lidar_occlusion is True and a.lidar_noise is None and a.lidar_dropout is None
    a = p.parse_args(base + ["--lidar-occlusion", "--lidar-noise", "0.02"])
    assert a.lidar_occlusion is True and a.lidar_noise == 0.02
    with pytest.raises(SystemExit):
        p.parse_args(base + ["--lidar-occlusion", "yes"])  # a switch, not a value
    # a flag a resumed run may not change: recorded with the run's arguments, compared on --resume
    assert "lidar_occlusion" not in train.RESUME_FREE
    import json

    saved = dict(vars(p.parse_args(base)), _world_size=1)
    with open(tmp_path / "train_args.json", "w") as f:
        json.dump(saved, f)
    train.check_resume_args(p.parse_args(base), str(tmp_path), world=1)
    with pytest.raises(SystemExit, match="lidar_occlusion"):
        train.check_resume_args(p.parse_args(base + ["--lidar-occlusion"]), str(tmp_path), world=1)
    saved.pop("lidar_occlusion")  # a run saved before the flag existed trained without it
    with open(tmp_path / "train_args.json", "w") as f:
        json.dump(saved, f)
    train.check_resume_args(p.parse_args(base), str(tmp_path), world=1)
    with pytest.raises(SystemExit, match="lidar_occlusion"):
        train.check_resume_args(p.parse_args(base + ["--lidar-occlusion"]), str(tmp_path), world=1)
    tp = _cli("test").build_parser()
    assert tp.parse_args(["--path", "x"]).lidar_occlusion is False
    a = tp.parse_args(["--path", "x", "--lidar-occlusion"])
    assert a.lidar_occlusion is True and a.lidar_noise is None and a.lidar_dropout is None
    a = tp.parse_args(["--path", "x", "--lidar-occlusion", "--lidar-dropout", "0.1"])
    assert a.lidar_occlusion is True and a.lidar_dropout == 0.1
