"""VMAS rendering checks that need no GPU: known answers of the float64 reference (tests/vmas_render_ref.py) the GPU
tests compare against, its negative controls, the C entry's refusals (dgppo_render_frames_vmas decides them on the
host, before any launch), the op's schema under fake tensors, the Python surface's refusals, the header text of
render_video, and test.py's --cbf refusal for a VMAS env."""
import ctypes
import importlib.util
import os
import re
import sys

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.env.vmas import vmas_header_lines

import render_ref as R
import vmas_render_ref as V
from test_capi import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WHEEL = dict(engine=V.WHEEL, area_size=2.4, agent_radius=0.03, dist2goal=0.01)
TRANSPORT = dict(engine=V.TRANSPORT, area_size=1.6, agent_radius=0.03, dist2goal=0.01)


def _byte(c):
    return np.floor(255.0 * c + 0.5).astype(np.uint8)


# ---- the reference's known answers -----------------------------------------------------------------------------------
def test_cfg_numbers_are_the_reference_classes():
    for eid, want in (("VMASWheel", WHEEL), ("VMASReverseTransport", TRANSPORT)):
        got = V.cfg_numbers(make_env(eid, 3, device="cpu"))
        assert got["engine"] == want["engine"]
        for k in ("area_size", "agent_radius", "dist2goal"):
            assert got[k] == pytest.approx(want[k], rel=1e-6), (eid, k)


def test_pixel_under_an_agent_centre_is_its_colour():
    st, rec = V.control_scene(V.WHEEL)
    img = V.render_ref(WHEEL, st, rec, 256)
    for i, colour in enumerate(V.AGENT_COLOURS):
        row, col = V.pixel_of(WHEEL, 256, st[i, 0], st[i, 1])
        assert (img[row, col, :3] == _byte(colour)).all(), i
    assert (img[..., 3] == 255).all()
    st[2, :2] = st[1, :2]  # coincident agents: agent 2 is on top
    row, col = V.pixel_of(WHEEL, 256, st[1, 0], st[1, 1])
    assert (V.render_ref(WHEEL, st, rec, 256)[row, col, :3] == _byte(V.C4)).all()


def test_pixel_inside_the_avoid_sector_only_is_white_blended_with_c0():
    st, rec = V.control_scene(V.WHEEL)  # avoid angle 2.5: (-0.8, 0.6) is on the sector's axis, far from everything else
    img = V.render_ref(WHEEL, st, rec, 256)
    row, col = V.pixel_of(WHEEL, 256, -0.8, 0.6)
    assert (img[row, col, :3] == _byte(1.0 + 0.2 * (V.C0 - 1.0))).all()
    row, col = V.pixel_of(WHEEL, 256, 0.8, -0.9)  # outside every primitive
    assert (img[row, col, :3] == 255).all()
    # the sector runs off the view: the corner pixel on its axis side is still inside it
    rec2 = rec.copy()
    rec2[1] = 3 * np.pi / 4
    assert (V.render_ref(WHEEL, st, rec2, 64)[0, 0, :3] == _byte(1.0 + 0.2 * (V.C0 - 1.0))).all()


def test_pixel_under_the_box_centre_is_c3_and_the_goal_shows_through():
    st, rec = V.control_scene(V.TRANSPORT)
    img = V.render_ref(TRANSPORT, st, rec, 512)
    row, col = V.pixel_of(TRANSPORT, 512, st[3, 0], st[3, 1])
    assert (img[row, col, :3] == _byte(V.C3)).all()
    row, col = V.pixel_of(TRANSPORT, 512, rec[0], rec[1])  # the goal: C5 at alpha 0.5 on white
    assert (img[row, col, :3] == _byte(1.0 + 0.5 * (V.C5 - 1.0))).all()
    rec[0:2] = st[3, :2]  # the goal under the box centre: the centre disc (alpha 1, on top) wins
    row, col = V.pixel_of(TRANSPORT, 512, st[3, 0], st[3, 1])
    assert (V.render_ref(TRANSPORT, st, rec, 512)[row, col, :3] == _byte(V.C3)).all()


@pytest.mark.parametrize("S", [33, 97, 256, 512])
def test_an_outline_thinner_than_a_pixel_never_reaches_full_coverage(S):
    """Half-width V / 1440 against h = V / S: the best coverage is 0.5 + S / 1440 < 1 for every S < 720."""
    Vw, h, px, py = V.view(TRANSPORT, S)
    cov = R.coverage(V.d_outline(px, py, 0.1, -0.05, V.BOX, V.BOX, Vw / 1440), h)
    assert 0.0 < cov.max() <= 0.5 + S / 1440 + 1e-12 < 1.0
    img = V.render_ref(TRANSPORT, *V.control_scene(V.TRANSPORT), S, skip_layers={2, 3, 5, 6})
    painted = (img[..., :3] != 255).any(-1)
    assert painted.any() and not (img[painted][:, :3] == _byte(V.C3)).all(-1).any()  # never the full colour


@pytest.mark.parametrize("engine,layer", [(e, k) for e in (V.WHEEL, V.TRANSPORT) for k in V.LAYERS[e]])
def test_reference_without_a_layer_differs(engine, layer):
    """The negative controls are not vacuous: at S = 512 every layer moves some byte by more than 1 LSB."""
    cfg = WHEEL if engine == V.WHEEL else TRANSPORT
    st, rec = V.control_scene(engine)
    full = controls_full(engine).astype(np.int16)
    without = V.render_ref(cfg, st, rec, 512, skip_layers={layer}).astype(np.int16)
    assert np.abs(full - without).max() > 1, (engine, layer)


_FULL = {}


def controls_full(engine):
    if engine not in _FULL:
        cfg = WHEEL if engine == V.WHEEL else TRANSPORT
        _FULL[engine] = V.render_ref(cfg, *V.control_scene(engine), 512)
        _FULL[engine].setflags(write=False)
    return _FULL[engine]


def test_non_finite_inputs_drop_their_primitives_in_the_reference():
    st, rec = V.control_scene(V.WHEEL)
    bad = st.copy()
    bad[3, 0] = np.nan  # the line angle: both halves go
    assert (V.render_ref(WHEEL, bad, rec, 64) == V.render_ref(WHEEL, st, rec, 64, skip_layers={2, 3})).all()
    bad = st.copy()
    bad[1, :] = np.inf
    assert (V.render_ref(WHEEL, bad, rec, 64) == V.render_ref(WHEEL, st, rec, 64, skip_agents={1})).all()


# ---- the C entry -------------------------------------------------------------------------------------------------------
def test_header_declares_the_entry_and_the_signature_is_bound():
    assert "dgppo_render_frames_vmas" in declared_functions()
    res, args = _lib.SIGNATURES["dgppo_render_frames_vmas"]
    assert res is ctypes.c_int and len(args) == 3 and args[1]._type_ is _lib.RenderArgs
    assert hasattr(_lib.load(), "dgppo_render_frames_vmas")
    assert _lib.load().dgppo_abi_version() == 14 and _lib.ABI_VERSION == 14  # an addition


def test_einval_without_a_launch():
    """Argument errors are decided on the host, before any launch: this runs without a GPU."""
    lib = _lib.load()
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)

    def args(**kw):
        a = _lib.RenderArgs()
        a.states, a.obstacles = base, base + 1024  # 64 and 32 bytes are read
        a.out = base + 8192
        a.n_frames, a.frames_per_episode, a.size, a.flags = 1, 1, 8, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    E = _lib.DGPPO_EINVAL
    for eid in ("VMASWheel", "VMASReverseTransport"):
        cfg = ctypes.byref(make_env(eid, 3, device="cpu").cfg)
        assert lib.dgppo_render_frames_vmas(cfg, None, None) == E
        assert lib.dgppo_render_frames_vmas(None, args(), None) == E
        assert lib.dgppo_render_frames_vmas(cfg, args(n_frames=0), None) == 0  # nothing to draw: no launch
        assert lib.dgppo_render_frames_vmas(cfg, args(n_frames=0, states=None, out=None), None) == 0
        for bad in (dict(size=0), dict(size=-3), dict(size=32769), dict(n_frames=-1), dict(frames_per_episode=0),
                    dict(states=None), dict(out=None), dict(obstacles=None), dict(flags=1), dict(flags=-1),
                    dict(states_estride=-1), dict(states_tstride=-16), dict(index_estride=-1), dict(index_tstride=-4),
                    dict(obstacles_estride=-8),
                    dict(size=32768, n_frames=1 << 21),  # more (frame, tile) workgroups than a grid holds
                    dict(out=base), dict(out=base + 60), dict(out=base - 252),  # out overlaps the states
                    dict(out=base + 1024), dict(out=base + 1024 + 28), dict(out=base + 1024 - 252),  # ... the record
                    dict(out=base + 2048, n_frames=2, states_estride=512),  # ... the second episode's states
                    dict(out=base + 4096, n_frames=2, obstacles_estride=768)):  # ... the second episode's record
            assert lib.dgppo_render_frames_vmas(cfg, args(**bad), None) == E, (eid, bad)
    lidar = make_env("LidarSpread", 3, num_obs=2, device="cpu")  # every other engine: dgppo_render_frames
    assert lib.dgppo_render_frames_vmas(ctypes.byref(lidar.cfg), args(), None) == E
    mpe = make_env("MPESpread", 3, num_obs=3, device="cpu")
    assert lib.dgppo_render_frames_vmas(ctypes.byref(mpe.cfg), args(), None) == E


# ---- the op and the Python surface -------------------------------------------------------------------------------------
def test_op_schema_and_fake_tensor_call():
    s = str(torch.ops.dgppo.render_frames_vmas.default._schema)
    assert re.fullmatch(r"dgppo::render_frames_vmas\((Sym)?[Ii]nt cfg, Tensor states, Tensor record, "
                        r"Tensor\(a\d+!\) out\) -> \(\)", s), s
    env = make_env("VMASWheel", 3, device="cpu")
    from torch._subclasses.fake_tensor import FakeTensorMode

    with FakeTensorMode():
        out = torch.empty(2, 3, 16, 16, 4, dtype=torch.uint8)
        assert torch.ops.dgppo.render_frames_vmas(env._cfg_handle, torch.empty(2, 3, 4, 4), torch.empty(2, 1, 8),
                                                  out) is None
        assert tuple(out.shape) == (2, 3, 16, 16, 4)
    with pytest.raises(_lib.NativeLibraryError):  # real CPU tensors: no host path, no fall-back
        torch.ops.dgppo.render_frames_vmas(env._cfg_handle, torch.zeros(2, 4, 4), torch.zeros(2, 1, 8),
                                           torch.empty(2, 16, 16, 4, dtype=torch.uint8))


@pytest.mark.parametrize("eid", ["VMASWheel", "VMASReverseTransport"])
def test_cpu_graph_and_value_layers_are_refused(eid):
    env = make_env(eid, 3, device="cpu")
    g = env.empty_graph((1,), "cpu")
    with pytest.raises(NotImplementedError, match="VMAS"):
        env.render_frames(g, size=16)
    for key in ("field", "cbf", "Vh"):
        with pytest.raises(NotImplementedError, match=f"{key}.*VMAS"):
            env.render_frames(g, size=16, viz_opts={key: None})
    with pytest.raises(NotImplementedError, match="VMAS"):
        env.render_frames(g, size=16, viz_opts={"fov": False})  # ignored: the graph is what is refused


# ---- the header text ---------------------------------------------------------------------------------------------------
def test_wheel_header_lines():
    env = make_env("VMASWheel", 3, device="cpu")
    body, rec = [0.5, 0.1234, 0, 0], [1.0, -0.25, 0, 0, 0, 0, 0, 0]
    assert vmas_header_lines(env, body, rec, [0.0, 0.0], 7) == [
        "omega=+0.123", "kk=0007", "dist_obs=0.750", "dist_goal=-0.500"]
    # the differences wrap past +-pi: 3.0 - (-3.0) = 6.0 -> 6.0 - 2 pi; -3.1 - 3.1 = -6.2 -> 2 pi - 6.2
    got = vmas_header_lines(env, [3.0, -2.0, 0, 0], [-3.0, -3.0, 0, 0, 0, 0, 0, 0], None, 63)
    assert got == ["omega=-2.000", "kk=0063", f"dist_obs={6.0 - 2 * np.pi:.3f}", f"dist_goal={6.0 - 2 * np.pi:.3f}"]
    assert got[2] == "dist_obs=-0.283"
    got = vmas_header_lines(env, [-3.1, 0.0, 0, 0], [3.1, 3.1, 0, 0, 0, 0, 0, 0], None, 0)
    assert got[2:] == ["dist_obs=0.083", "dist_goal=0.083"] and got[0] == "omega=+0.000"
    got = vmas_header_lines(env, [7.0, 0.0, 0, 0], [0.0, 7.0 - 2 * np.pi, 0, 0, 0, 0, 0, 0], None, 1)  # a wound-up angle
    assert got[2] in ("dist_obs=0.000", "dist_obs=-0.000") and got[3] == f"dist_goal={7.0 - 2 * np.pi:.3f}"


def test_transport_header_lines():
    env = make_env("VMASReverseTransport", 3, device="cpu")
    body = [0.1, -0.2, 0, 0]
    rec = [0.4, 0.2, 0.1, 0.0, 0.1, -0.3, -0.2, -0.6]  # goal 0.5 away; obstacles 0.2, 0.1, 0.5 away
    assert vmas_header_lines(env, body, rec, [0.1, -0.2], 12) == [
        "cost=+0.100, -0.200", "kk=0012", "dist_obs=[+0.050, -0.050, +0.350]", "dist_goal=0.500"]


# ---- test.py -----------------------------------------------------------------------------------------------------------
def test_test_py_refuses_cbf_for_a_vmas_env_before_anything_is_loaded(tmp_path, monkeypatch):
    spec = importlib.util.spec_from_file_location("dgppo_entry_test_vmas_render", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    (tmp_path / "config.yaml").write_text("env: VMASWheel\nalgo: dgppo\nnum_agents: 3\nobs: 0\n")  # no models/ at all
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", str(tmp_path), "--video", "--cbf", "0"])
    with pytest.raises(SystemExit, match="--cbf is not built for VMASWheel.*get_graph"):
        mod.main()
    (tmp_path / "config.yaml").write_text("env: LidarSpread\nalgo: dgppo\nnum_agents: 3\nobs: 0\n")
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", str(tmp_path), "--env", "VMASReverseTransport", "--video",
                                      "--cbf", "1"])
    with pytest.raises(SystemExit, match="--cbf is not built for VMASReverseTransport"):
        mod.main()
