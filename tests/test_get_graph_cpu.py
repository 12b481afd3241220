"""env.get_graph without a GPU: the host-side Rectangle.create against the oracle, the C-ABI's struct layout and
argument checks (none of which launches), the torch op's registration and fake kernel, the no-CPU rule, and the
scene files."""
import ctypes
import re

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib, ops  # noqa: F401  (registers torch.ops.dgppo.*)
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.env.obstacle import Rectangle
from oracle import env as O

from test_capi import _c_layout

F = np.float32


def _rect_inputs():
    rng = np.random.default_rng(11)
    pi = np.pi
    special = np.array([0.0, pi / 2, -pi / 2, pi, -pi, 2 * pi, -0.0], F)
    count = 64 + len(special)
    center = rng.uniform(-0.5, 2.5, (count, 2)).astype(F)
    width = rng.uniform(0.05, 1.2, count).astype(F)
    height = rng.uniform(0.05, 1.2, count).astype(F)
    theta = np.concatenate([rng.uniform(-pi, 2 * pi, 64).astype(F), special])
    return center, width, height, theta


def test_make_rectangles_equals_oracle_exactly():
    center, width, height, theta = _rect_inputs()
    ref = O.make_rectangles(center, width, height, theta)
    # the raw host entry point
    out = np.full((len(theta), 16), np.nan, F)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    rc = _lib.load().dgppo_make_rectangles(len(theta), p(center), p(width), p(height), p(theta), p(out))
    assert rc == 0
    assert out.tobytes() == ref.tobytes()  # bit for bit, the sign of zero included
    # Rectangle.create, batched (7, 10) + the 71st alone
    t = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
    rect = Rectangle.create(t(center[:70]).view(7, 10, 2), t(width[:70]).view(7, 10), t(height[:70]).view(7, 10),
                            t(theta[:70]).view(7, 10))
    assert rect.packed.shape == (7, 10, 16) and rect.n == 10
    assert rect.packed.numpy().tobytes() == ref[:70].tobytes()
    one = Rectangle.create(t(center[70]), t(width[70]), t(height[70]), t(theta[70]))
    assert one.packed.numpy().tobytes() == ref[70].tobytes()
    np.testing.assert_array_equal(rect.points.numpy().reshape(70, 8), ref[:70, 8:])
    with pytest.raises(ValueError, match="width"):
        Rectangle.create(t(center[:4]), t(width[:3]), t(height[:4]), t(theta[:4]))
    with pytest.raises(ValueError, match="center"):
        Rectangle.create(torch.tensor(1.0), torch.tensor(1.0), torch.tensor(1.0), torch.tensor(0.0))
    lib = _lib.load()
    assert lib.dgppo_make_rectangles(-1, p(center), p(width), p(height), p(theta), p(out)) == _lib.DGPPO_EINVAL
    assert lib.dgppo_make_rectangles(2, p(center), None, p(height), p(theta), p(out)) == _lib.DGPPO_EINVAL
    assert lib.dgppo_make_rectangles(0, None, None, None, None, None) == 0


def test_env_graph_io_mirror_matches_c_layout():
    names = [f[0] for f in _lib.EnvGraphIO._fields_]
    got = _c_layout("dgppo_env_graph_io", names)
    assert got[0] == ctypes.sizeof(_lib.EnvGraphIO)
    for name, off in zip(names, got[1:]):
        assert getattr(_lib.EnvGraphIO, name).offset == off, name


def _host_io(n_env=1):
    """An io whose pointers are non-NULL host addresses: only for calls that return before any launch."""
    buf = (ctypes.c_float * 4)()
    a = ctypes.addressof(buf)
    io = _lib.EnvGraphIO()
    for f in ("agent", "goal", "third", "ray_dirs", "nodes", "edges", "out_states", "receivers", "senders"):
        setattr(io, f, a)
    io.n_env = n_env
    return io, buf


def test_get_graph_argument_checks_do_not_launch():
    lib = _lib.load()
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    cfg = ctypes.byref(env.cfg)
    io, keep = _host_io()
    assert lib.dgppo_env_get_graph(cfg, None, None) == _lib.DGPPO_EINVAL
    assert lib.dgppo_env_get_graph(None, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    for field in ("agent", "goal", "third", "ray_dirs", "nodes", "edges", "out_states", "receivers", "senders"):
        io, keep = _host_io()
        setattr(io, field, None)
        assert lib.dgppo_env_get_graph(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL, field
    io, keep = _host_io(n_env=-1)
    assert lib.dgppo_env_get_graph(cfg, ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    io, keep = _host_io(n_env=0)
    assert lib.dgppo_env_get_graph(cfg, ctypes.byref(io), None) == 0
    io = _lib.EnvGraphIO()  # n_env == 0 is checked before the pointers
    assert lib.dgppo_env_get_graph(cfg, ctypes.byref(io), None) == 0
    # the VMAS engines are refused whatever the batch
    vm = make_env("VMASWheel", 3, device="cpu")
    io, keep = _host_io()
    assert lib.dgppo_env_get_graph(ctypes.byref(vm.cfg), ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    io, keep = _host_io(n_env=0)
    assert lib.dgppo_env_get_graph(ctypes.byref(vm.cfg), ctypes.byref(io), None) == _lib.DGPPO_EINVAL
    with pytest.raises(NotImplementedError):
        vm.get_graph((torch.zeros(1, 3, 4), torch.zeros(1, 3, 4), None))


def test_op_registered_and_traces_under_fake_tensors():
    schema = str(torch.ops.dgppo.env_get_graph.default._schema)
    assert re.match(r"dgppo::env_get_graph\((Sym)?[Ii]nt cfg, Tensor agent, Tensor goal, Tensor\? third, Tensor ray_dirs,",
                    schema), schema  # inputs are read-only
    assert schema.endswith("-> ()"), schema
    for name in ("nodes", "edges", "states", "receivers", "senders"):
        assert re.search(rf"Tensor\(a\d+!\) {name}\b", schema), (name, schema)
    from torch._subclasses.fake_tensor import FakeTensorMode

    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    with FakeTensorMode():
        B, n, N, E = 4, 3, env.n_nodes, env.n_edges
        torch.ops.dgppo.env_get_graph(env._cfg_handle, torch.empty(B, n, 4), torch.empty(B, n, 4),
                                      torch.empty(B, 2, 16), torch.empty(32, 2), torch.empty(B, N, 7),
                                      torch.empty(B, E, 4), torch.empty(B, N, 4),
                                      torch.empty(B, E, dtype=torch.int32), torch.empty(B, E, dtype=torch.int32))
        torch.ops.dgppo.env_get_graph(env._cfg_handle, torch.empty(B, n, 4), torch.empty(B, n, 4), None,
                                      torch.empty(32, 2), torch.empty(B, N, 7), torch.empty(B, E, 4),
                                      torch.empty(B, N, 4), torch.empty(B, E, dtype=torch.int32),
                                      torch.empty(B, E, dtype=torch.int32))


def _cpu_state(env, B):
    n, sd = env.num_agents, env.state_dim
    agent, goal = torch.rand(B, n, sd), torch.rand(B, env.num_goals, sd)
    if env.ENGINE == _lib.DGPPO_ENGINE_MPE:
        return agent, goal, torch.rand(B, env.n_obs, sd)
    th = torch.rand(B, env.n_obs)
    return agent, goal, Rectangle.create(torch.rand(B, env.n_obs, 2), th * 0.2 + 0.1, th * 0.1 + 0.1, th * 6)


def test_get_graph_on_cpu_raises_native_library_error():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    B, n, N, E = 2, 3, env.n_nodes, env.n_edges
    agent, goal, rect = _cpu_state(env, B)
    with pytest.raises(_lib.NativeLibraryError):
        env.get_graph((agent, goal, rect))
    with pytest.raises(_lib.NativeLibraryError):
        torch.ops.dgppo.env_get_graph(env._cfg_handle, agent, goal, rect.packed, torch.zeros(32, 2),
                                      torch.empty(B, N, 7), torch.empty(B, E, 4), torch.empty(B, N, 4),
                                      torch.empty(B, E, dtype=torch.int32), torch.empty(B, E, dtype=torch.int32))
    # shapes are checked first, and the message names the field
    with pytest.raises(ValueError, match="state.agent"):
        env.get_graph((agent[:, :2], goal, rect))
    with pytest.raises(ValueError, match="state.goal"):
        env.get_graph((agent, goal[..., :3], rect))
    with pytest.raises(ValueError, match="state.goal"):
        env.get_graph((agent, goal[:1], rect))
    with pytest.raises(ValueError, match="state.obstacle"):
        env.get_graph((agent, goal, rect.packed[:, :1]))
    with pytest.raises(ValueError, match="state.obstacle"):
        env.get_graph((agent, goal, None))
    mpe = make_env("MPESpread", 3, num_obs=3, device="cpu")
    with pytest.raises(ValueError, match="state.obs"):
        mpe.get_graph((agent, goal, torch.zeros(B, 2, 4)))
    with pytest.raises(ValueError):
        mpe.get_lidar_data(agent, None)


@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 3, 2), ("LidarOmniTarget", 2, 0), ("MPESpread", 3, 3),
                                       ("MPELine", 3, 2), ("MPETarget", 2, 0)])
def test_scene_round_trip(tmp_path, eid, n, obs):
    from dgppo_fov_amd.utils.scene import load_scene, save_scene

    env = make_env(eid, n, num_obs=obs, device="cpu")
    state = _cpu_state(env, 5)
    if env.n_obs == 0:
        state = (state[0], state[1], None)
    path = str(tmp_path / "scene.npz")
    save_scene(path, env, state)
    with np.load(path, allow_pickle=False) as z:
        third = "obs" if eid.startswith("MPE") else "obstacle"
        assert sorted(z.files) == sorted(["env_id", "agent", "goal", third])
        assert str(z["env_id"]) == type(env).__name__
        assert z["agent"].shape == (5, n, env.state_dim) and z["goal"].shape == (5, env.num_goals, env.state_dim)
        assert z[third].shape == (5, env.n_obs, 4 if third == "obs" else 16)
        assert all(z[k].dtype == np.float32 for k in ("agent", "goal", third))
    back = load_scene(path, env, "cpu")
    assert type(back).__name__ == ("MPEEnvState" if eid.startswith("MPE") else "LidarEnvState")
    assert torch.equal(back[0], state[0]) and torch.equal(back[1], state[1])
    if env.n_obs > 0:
        assert torch.equal(getattr(back[2], "packed", back[2]), getattr(state[2], "packed", state[2]))
    elif not eid.startswith("MPE"):
        assert back[2] is None


def test_scene_shape_mismatch_names_the_array(tmp_path):
    from dgppo_fov_amd.utils.scene import load_scene, save_scene

    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    path = str(tmp_path / "scene.npz")
    save_scene(path, env, _cpu_state(env, 4))
    with pytest.raises(ValueError, match="'agent'"):
        load_scene(path, make_env("LidarSpread", 4, num_obs=2, device="cpu"), "cpu")
    with pytest.raises(ValueError, match="'obstacle'"):
        load_scene(path, make_env("LidarSpread", 3, num_obs=3, device="cpu"), "cpu")
    with pytest.raises(ValueError, match="'obs'"):
        load_scene(path, make_env("MPESpread", 3, num_obs=2, device="cpu"), "cpu")
    with pytest.raises(ValueError, match="agent"):
        save_scene(path, env, (torch.zeros(4, 2, 4),) + tuple(_cpu_state(env, 4))[1:])
