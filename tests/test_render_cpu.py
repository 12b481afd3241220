"""Rendering checks that need no GPU: the C-ABI addition (dgppo_render_frames, dgppo_render_args) is declared, bound
and laid out as the header says without a new ABI number; the Python surface refuses a CPU graph instead of falling
back; test.py's parser takes the video options; and the float64 reference (tests/render_ref.py) the GPU tests compare
against paints what the pixel rule says on two shapes with a known answer."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib
from dgppo_fov_amd.env import make_env

import render_ref as R
from test_capi import _c_layout, declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_render_frames_and_signature_is_bound():
    assert "dgppo_render_frames" in declared_functions()
    res, args = _lib.SIGNATURES["dgppo_render_frames"]
    assert res is ctypes.c_int and len(args) == 3 and args[1]._type_ is _lib.RenderArgs
    assert hasattr(_lib.load(), "dgppo_render_frames")


def test_render_args_mirror_matches_c_layout():
    names = [f[0] for f in _lib.RenderArgs._fields_]
    got = _c_layout("dgppo_render_args", names)
    assert got[0] == ctypes.sizeof(_lib.RenderArgs)
    for name, off in zip(names, got[1:]):
        assert getattr(_lib.RenderArgs, name).offset == off, name


def test_abi_version_is_unchanged():
    assert _lib.load().dgppo_abi_version() == 14 and _lib.ABI_VERSION == 14


def test_load_names_a_missing_symbol(monkeypatch):
    monkeypatch.setattr(_lib, "_LIB", None)
    monkeypatch.setitem(_lib.SIGNATURES, "dgppo_not_there", (ctypes.c_int, []))
    with pytest.raises(_lib.NativeLibraryError, match=r"dgppo_not_there.*rebuild \(`make`\)"):
        _lib.load()


def test_einval_without_a_launch():
    """Argument errors are decided on the host, before any launch."""
    lib = _lib.load()
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    cfg = ctypes.byref(env.cfg)
    buf = (ctypes.c_float * 4096)()
    base = ctypes.addressof(buf)

    def args(**kw):
        a = _lib.RenderArgs()
        a.states, a.receivers, a.senders, a.obstacles = base, base, base, base
        a.out = base + 8192
        a.n_frames, a.frames_per_episode, a.size, a.flags = 1, 1, 8, 0
        for k, v in kw.items():
            setattr(a, k, v)
        return ctypes.byref(a)

    E = _lib.DGPPO_EINVAL
    assert lib.dgppo_render_frames(cfg, None, None) == E and lib.dgppo_render_frames(None, args(), None) == E
    assert lib.dgppo_render_frames(cfg, args(n_frames=0), None) == 0  # nothing to draw: no launch
    for bad in (dict(size=0), dict(size=-3), dict(n_frames=-1), dict(frames_per_episode=0), dict(states=None),
                dict(out=None), dict(receivers=None), dict(senders=None), dict(obstacles=None),
                dict(states_estride=-1), dict(index_tstride=-4), dict(obstacles_estride=-16),
                dict(out=base), dict(out=base + 16)):  # the last two: out overlaps the inputs
        assert lib.dgppo_render_frames(cfg, args(**bad), None) == E, bad
    vm = make_env("VMASWheel", 3, device="cpu")
    assert lib.dgppo_render_frames(ctypes.byref(vm.cfg), args(), None) == E


def test_render_frames_on_cpu_raises_instead_of_falling_back():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    g = env.empty_graph((2,), "cpu")
    with pytest.raises(_lib.NativeLibraryError):
        env.render_frames(g, size=16)
    with pytest.raises(_lib.NativeLibraryError):
        torch.ops.dgppo.render_frames(env._cfg_handle, g.states, g.receivers, g.senders, None,
                                      torch.empty(2, 16, 16, 4, dtype=torch.uint8), 0)
    with pytest.raises(NotImplementedError, match="not built"):
        env.render_frames(g, size=16, viz_opts={"cbf": 0})
    with pytest.raises(NotImplementedError, match="VMAS"):
        vm = make_env("VMASWheel", 3, device="cpu")
        vm.render_frames(vm.empty_graph((1,), "cpu"), size=16)
    assert "render_frames" in str(torch.ops.dgppo.render_frames.default._schema)


def test_test_py_parser_accepts_the_video_options(monkeypatch):
    spec = importlib.util.spec_from_file_location("dgppo_entry_test_render", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}
    monkeypatch.setattr(mod, "test", lambda a: seen.update(vars(a)))
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", "x", "--video", "--max-videos", "2"])
    mod.main()
    assert seen["video"] is True and seen["max_videos"] == 2 and seen["dpi"] == 100 and seen["no_video"] is False
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", "x", "--no-video"])
    mod.main()
    assert seen["video"] is False and seen["max_videos"] == 5 and seen["no_video"] is True  # the default: no video


def test_reference_circle_area():
    """An isolated circle's summed coverage times h^2 is its area within 1 % at S = 200."""
    L, S, r = 1.5, 200, 0.05
    px, py, h = R.pixel_centres(L, S)
    cov = R.coverage(R.d_circle(px, py, 0.7312, 0.4057, r), h)
    assert abs(cov.sum() * h * h - np.pi * r * r) <= 0.01 * np.pi * r * r


def test_reference_zero_length_edge_is_a_dot():
    """An edge whose two endpoints coincide paints a disc of radius L / 720: no NaN, and exactly the circle's image."""
    L, S = 1.5, 240
    px, py, h = R.pixel_centres(L, S)
    d = R.d_edge(px, py, 0.6, 0.9, 0.6, 0.9, L / 720)
    assert np.isfinite(d).all()
    np.testing.assert_allclose(d, R.d_circle(px, py, 0.6, 0.9, L / 720), rtol=0, atol=1e-12)
    cfg = dict(engine=R.ENGINE_MPE, n=1, n_goals=1, n_obs=0, n_nodes=3, area_size=L, car_radius=0.05, obs_radius=0.05,
               fov_angle_deg=0.0, fov_rmax=0.0)
    st = np.array([[0.6, 0.9, 0, 0], [0.6, 0.9, 0, 0], [0, 0, 0, 0]])
    img = R.render_ref(cfg, st, [0], [1], None, S, skip_layers={4})
    assert img.dtype == np.uint8 and (img[..., 3] == 255).all()
    row, col = int(S - 0.9 / h), int(0.6 / h)
    assert (img[row, col, :3] < 255).any() and (img[0, 0, :3] == 255).all()
    painted = (img[..., :3] != 255).any(-1).sum() * h * h  # alpha 0.5 on white changes every covered pixel
    assert painted <= np.pi * (L / 720 + h) ** 2 * 1.5
