"""Field-layer checks that need no GPU: the float64 restatement of the rule (tests/field_ref.py) stays within its own
bar when evaluated in fp32; the C-ABI addition (dgppo_render_frames_field, dgppo_render_field) is declared, bound,
laid out as the header says and validated on the host without a new ABI number; sweep_states against NumPy indexing;
FieldLayer's validation; the palette; test.py's parser."""
import ctypes
import importlib.util
import os
import sys

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib
from dgppo_fov_amd.algo import DGPPO, HCBFCRPO, InforMARL, InforMARLLagr
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.utils import field as F

import field_ref as FR
from test_capi import _c_layout, declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTENT = (0.013, 1.487, 0.021, 1.379)
GX, GY, L = 9, 7, 1.5


def _axes():
    return np.linspace(EXTENT[0], EXTENT[1], GX), np.linspace(EXTENT[2], EXTENT[3], GY)


# ---- the reference within its own bar ------------------------------------------------------------------------------
@pytest.mark.parametrize("S", (50, 96))
def test_fp32_evaluation_of_the_rule_is_within_one_lsb_of_float64(S):
    xs, ys = _axes()
    val = FR.analytic_field(xs, ys)
    half = float(np.abs(val).max())
    pal = F.palette(14)
    i64, undecided, inside = FR.field_background(val, EXTENT, half, pal, L, S)
    i32, _, _ = FR.field_background(val, EXTENT, half, pal, L, S, dtype=np.float32)
    b64, b32 = FR.to_bytes(i64).astype(np.int16), FR.to_bytes(i32).astype(np.int16)
    diff = np.abs(b64 - b32).max(axis=-1)
    share = float(undecided.sum()) / float(inside.sum())
    print(f"S={S}: undecided {share:.2%}, max decided diff {int(diff[~undecided].max())} LSB")
    assert inside.sum() > 0.8 * S * S
    assert share <= 0.01
    assert diff[~undecided].max() <= 1
    # the scene is not vacuous: most bands are used and the zero line is there
    bands = np.unique(np.floor((val.astype(np.float64) + half) / (2 * half) * 14).clip(0, 13))
    assert len(bands) >= 10
    no_line = FR.to_bytes(FR.field_background(val, EXTENT, half, pal, L, S, line=False)[0]).astype(np.int16)
    no_bands = FR.to_bytes(FR.field_background(val, EXTENT, half, pal, L, S, bands=False)[0]).astype(np.int16)
    assert np.abs(b64 - no_line).max() > 50 and np.abs(b64 - no_bands).max() > 50  # both parts move bytes
    assert (b64[~inside][:, :3] == 255).all()  # outside the extent: white


def test_reference_constant_field_has_no_line_and_nan_cells_are_unpainted():
    xs, ys = _axes()
    pal = F.palette(14)
    img, _, inside = FR.field_background(np.full((GY, GX), 0.25, np.float32), EXTENT, 1.0, pal, L, 50)
    b = FR.to_bytes(img)
    band = int(np.floor((0.25 + 1.0) / 2.0 * 14))
    want = np.floor(255.0 * (1 + 0.9 * (pal[band].astype(np.float64) - 1)) + 0.5).astype(np.uint8)
    assert (b[inside][:, :3] == want).all()
    val = FR.analytic_field(xs, ys)
    val[3, 4] = np.nan
    img, _, inside = FR.field_background(val, EXTENT, 1.2, pal, L, 96)
    b = FR.to_bytes(img)
    h = L / 96
    col, row = np.meshgrid(np.arange(96), np.arange(96))
    px, py = (col + 0.5) * h, (96 - row - 0.5) * h
    hole = (px > xs[3]) & (px < xs[5]) & (py > ys[2]) & (py < ys[4])
    assert hole.sum() > 100 and (b[hole][:, :3] == 255).all()
    assert (b[inside & ~hole][:, :3] != 255).any(axis=-1).all()


# ---- ABI -----------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_bound_and_exported_without_a_new_abi_number():
    assert "dgppo_render_frames_field" in declared_functions()
    res, args = _lib.SIGNATURES["dgppo_render_frames_field"]
    assert res is ctypes.c_int and len(args) == 4 and args[2]._type_ is _lib.RenderField
    lib = _lib.load()
    assert hasattr(lib, "dgppo_render_frames_field")
    assert lib.dgppo_abi_version() == 14 and _lib.ABI_VERSION == 14


def test_render_field_mirror_matches_c_layout():
    names = [f[0] for f in _lib.RenderField._fields_]
    got = _c_layout("dgppo_render_field", names)
    assert got[0] == ctypes.sizeof(_lib.RenderField)
    for name, off in zip(names, got[1:]):
        assert getattr(_lib.RenderField, name).offset == off, name
    args = [f[0] for f in _lib.RenderArgs._fields_]
    assert _c_layout("dgppo_render_args", args)[0] == ctypes.sizeof(_lib.RenderArgs)  # unchanged


def test_einval_without_a_launch():
    """Every argument error is decided on the host, before any launch (host pointers, NULL stream)."""
    lib = _lib.load()
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    cfg = ctypes.byref(env.cfg)
    buf = (ctypes.c_float * 8192)()
    base = ctypes.addressof(buf)
    out = base + 16384
    keep = []

    def args(**kw):
        a = _lib.RenderArgs()
        a.states, a.receivers, a.senders, a.obstacles = base, base, base, base
        a.out = out
        a.n_frames, a.frames_per_episode, a.size, a.flags = 1, 1, 8, 0
        for k, v in kw.items():
            setattr(a, k, v)
        keep.append(a)
        return ctypes.byref(a)

    def field(**kw):
        f = _lib.RenderField()
        f.values, f.palette = base + 4096, base + 8192
        f.gx, f.gy, f.bands = 4, 3, 14
        f.extent[:] = [0.0, 1.5, 0.0, 1.5]
        f.half_range, f.alpha, f.line_halfwidth = 1.0, 0.9, 1.5 / 480
        for k, v in kw.items():
            if k == "extent":
                f.extent[:] = v
            else:
                setattr(f, k, v)
        keep.append(f)
        return ctypes.byref(f)

    E, call = _lib.DGPPO_EINVAL, lib.dgppo_render_frames_field
    assert call(cfg, args(n_frames=0), field(), None) == 0  # a valid field, nothing to draw: no launch
    assert call(cfg, args(n_frames=0), None, None) == 0
    assert call(None, args(), field(), None) == E and call(cfg, None, field(), None) == E
    nan, inf = float("nan"), float("inf")
    for bad in (dict(values=None), dict(palette=None), dict(gx=1), dict(gy=1), dict(gx=0), dict(gy=-2),
                dict(bands=1), dict(bands=33), dict(bands=0),
                dict(extent=[0.0, nan, 0.0, 1.5]), dict(extent=[0.0, 1.5, -inf, 1.5]), dict(extent=[1.5, 1.5, 0.0, 1.5]),
                dict(extent=[0.0, 1.5, 1.0, 0.5]),
                dict(half_range=0.0), dict(half_range=-1.0), dict(half_range=nan), dict(half_range=inf),
                dict(values=out), dict(values=out - 16), dict(values=out + 8 * 8 * 4 - 4)):  # values overlap out
        assert call(cfg, args(), field(**bad), None) == E, bad
    # everything dgppo_render_frames rejects is rejected with a valid field too
    for bad in (dict(size=0), dict(n_frames=-1), dict(frames_per_episode=0), dict(states=None), dict(out=None),
                dict(receivers=None), dict(obstacles=None), dict(states_estride=-1), dict(out=base), dict(out=base + 16)):
        assert call(cfg, args(**bad), field(), None) == E, bad
    vm = make_env("VMASWheel", 3, device="cpu")
    assert call(ctypes.byref(vm.cfg), args(), field(), None) == E


def test_ops_are_registered_and_refuse_cpu_tensors():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    g = env.empty_graph((2,), "cpu")
    assert "render_frames_field" in str(torch.ops.dgppo.render_frames_field.default._schema)
    layer = F.FieldLayer(torch.zeros(2, 3, 4), np.linspace(0, 1.5, 4), np.linspace(0, 1.5, 3), 1.0)
    with pytest.raises(_lib.NativeLibraryError):
        env.render_frames(g, size=16, viz_opts={"field": layer})
    for key in ("cbf", "Vh"):  # the reference's keys stay unbuilt, with a field or without
        with pytest.raises(NotImplementedError, match="not built"):
            env.render_frames(g, size=16, viz_opts={key: 0, "field": layer})


# ---- get_Vh's presence ---------------------------------------------------------------------------------------------
def test_get_vh_is_public_where_the_reference_has_it():
    assert callable(DGPPO.get_Vh) and callable(HCBFCRPO.get_Vh)
    for cls in (InforMARL, InforMARLLagr):
        obj = cls.__new__(cls)
        assert not hasattr(obj, "get_Vh")
        with pytest.raises(ValueError, match=cls.__name__):
            F.value_field(obj, None, 0, 0, torch.zeros(2), torch.zeros(2))


# ---- sweep_states --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("eid,n,obs,Fr", [("LidarSpread", 3, 2, 2), ("LidarSpread", 3, 2, 1), ("MPESpread", 3, 3, 2),
                                          ("LidarOmniTarget", 3, 0, 1)])
def test_sweep_states_against_numpy_indexing(eid, n, obs, Fr):
    env = make_env(eid, n, num_obs=obs, device="cpu")
    gen = torch.Generator().manual_seed(5)
    sd, ng = env.state_dim, env.num_goals
    agent, goal = torch.rand(Fr, n, sd, generator=gen), torch.rand(Fr, ng, sd, generator=gen)
    third = None
    if obs:
        third = torch.rand(Fr, obs, env._obstacle_fields() or sd, generator=gen)
    xs, ys = torch.tensor([0.1, 0.5, 0.9, 1.3]), torch.tensor([0.2, 0.7, 1.2])
    a0, g0 = agent.clone(), goal.clone()
    a, g, t = F.sweep_states(env, (agent, goal, third), 1, xs, ys)
    assert torch.equal(agent, a0) and torch.equal(goal, g0)  # the inputs are not written
    want = np.broadcast_to(a0.numpy()[:, None, None], (Fr, 3, 4, n, sd)).copy()
    want[:, :, :, 1, 0] = xs.numpy()[None, None, :]
    want[:, :, :, 1, 1] = ys.numpy()[None, :, None]
    assert a.shape == (Fr * 12, n, sd) and np.array_equal(a.numpy(), want.reshape(Fr * 12, n, sd))
    assert np.array_equal(g.numpy(), np.repeat(g0.numpy(), 12, axis=0)) and g.shape == (Fr * 12, ng, sd)
    if obs:
        assert np.array_equal(t.numpy(), np.repeat(third.numpy(), 12, axis=0))
    else:
        assert t is None
    assert g.stride(-1) == 1 and g.stride(-2) == sd
    if Fr == 1:
        assert g.stride(0) == 0  # views per frame, no copy


def test_sweep_states_rejects_bad_arguments_and_vmas():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    agent, goal, ob = torch.zeros(1, 3, 4), torch.zeros(1, 3, 4), torch.zeros(1, 2, 16)
    xs = ys = torch.linspace(0, 1.5, 3)
    for bad in (3, -1, 1.0, None):
        with pytest.raises(ValueError, match="agent"):
            F.sweep_states(env, (agent, goal, ob), bad, xs, ys)
    with pytest.raises(ValueError, match=r"state\.agent"):
        F.sweep_states(env, (agent[:, :2], goal, ob), 0, xs, ys)
    with pytest.raises(ValueError, match=r"state\.goal"):
        F.sweep_states(env, (agent, goal[..., :3], ob), 0, xs, ys)
    with pytest.raises(ValueError, match=r"state\.obstacle"):
        F.sweep_states(env, (agent, goal, ob[:, :1]), 0, xs, ys)
    with pytest.raises(ValueError, match="xs"):
        F.sweep_states(env, (agent, goal, ob), 0, xs.view(1, 3), ys)
    with pytest.raises(ValueError, match="ys"):
        F.sweep_states(env, (agent, goal, ob), 0, xs, ys.double())
    vm = make_env("VMASWheel", 3, device="cpu")
    with pytest.raises(NotImplementedError, match="VMAS"):
        F.sweep_states(vm, (agent, goal, None), 0, xs, ys)


def test_grid_axes():
    env = make_env("LidarSpread", 3, num_obs=2, device="cpu")
    xs, ys = F.grid_axes(env, 8)
    want = torch.linspace(0, env.area_size, 8)
    assert torch.equal(xs, want) and torch.equal(ys, want) and xs.dtype == torch.float32


# ---- FieldLayer ----------------------------------------------------------------------------------------------------
def test_field_layer_validation():
    v = torch.zeros(2, 3, 4)
    xs, ys = np.linspace(0.0, 1.5, 4), np.linspace(0.1, 1.4, 3)
    ok = F.FieldLayer(v, xs, ys, 2.0, label="x")
    assert ok.extent == (0.0, 1.5, 0.1, 1.4) and ok.bands == 14 and ok.half_range == 2.0
    assert F.FieldLayer(v, torch.tensor(xs, dtype=torch.float32), torch.tensor(ys, dtype=torch.float32), 1.0).bands == 14
    sub = ok.sliced(slice(1, 2))
    assert sub.values.shape == (1, 3, 4) and sub.half_range == 2.0 and sub.label == "x" and sub.extent == ok.extent
    bent = xs.copy()
    bent[1] += 1e-3
    for kw in (dict(xs=bent), dict(xs=xs[::-1].copy()), dict(xs=xs[:1]), dict(ys=np.array([0.0, np.nan, 1.0])),
               dict(xs=np.linspace(0, 1.5, 5)), dict(bands=1), dict(bands=33), dict(half_range=0.0),
               dict(half_range=-1.0), dict(half_range=float("nan")), dict(half_range=float("inf")),
               dict(values=v.double()), dict(values=v.transpose(1, 2)), dict(values=torch.zeros(4))):
        a = dict(values=v, xs=xs, ys=ys, half_range=1.0)
        a.update(kw)
        with pytest.raises(ValueError):
            F.FieldLayer(**a)
    near = xs.copy()
    near[1] += 1e-6 * 1.5  # within 1e-5 of the span: uniform
    F.FieldLayer(v, near, ys, 1.0)


def test_centred_half_range():
    xs, ys = np.linspace(0.0, 1.5, 4), np.linspace(0.0, 1.5, 3)
    assert F.FieldLayer.centred(torch.zeros(3, 4), xs, ys).half_range == 1.0
    v = torch.tensor([[0.5, -2.5, float("nan"), 1.0]] * 3)
    assert F.FieldLayer.centred(v, xs, ys).half_range == 2.5
    v[0, 0] = float("inf")
    assert F.FieldLayer.centred(v, xs, ys, "lbl").half_range == 2.5
    assert F.FieldLayer.centred(torch.full((3, 4), float("nan")), xs, ys).half_range == 1.0


# ---- palette -------------------------------------------------------------------------------------------------------
def test_palette_against_the_four_colours():
    want = {"blue": (0.325, 0.586, 0.775), "light_blue": (0.990, 1.0, 1.0), "red": (0.844, 0.421, 0.336),
            "light_red": (1.0, 0.996, 0.990)}
    got = F.burd_colours()
    for k, c in want.items():
        assert np.abs(np.asarray(got[k]) - np.asarray(c)).max() <= 1e-3, (k, got[k])
    c = {k: np.asarray(v) for k, v in got.items()}
    for K in (2, 14, 32):
        p = F.palette(K)
        assert p.shape == (K, 3) and p.dtype == np.float32
        for b in range(K):
            t = (b + 0.5) / K
            w = c["light_red"] + 2 * t * (c["red"] - c["light_red"]) if t < 0.5 else \
                c["blue"] + (2 * t - 1) * (c["light_blue"] - c["blue"])
            assert np.abs(p[b] - w).max() <= 1e-6
    p = F.palette(14)
    assert p[0, 0] > p[0, 2] > 0.9 and p[6, 0] > p[6, 2] + 0.4  # negative: light red ... red
    assert p[7, 2] > p[7, 0] + 0.4 and p[13].min() > 0.9  # positive: blue ... light blue
    for K in (1, 33):
        with pytest.raises(ValueError):
            F.palette(K)


# ---- parser --------------------------------------------------------------------------------------------------------
def test_test_py_parser_accepts_cbf(monkeypatch):
    spec = importlib.util.spec_from_file_location("dgppo_entry_test_field", os.path.join(ROOT, "test.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    seen = {}
    monkeypatch.setattr(mod, "test", lambda a: seen.update(vars(a)))
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", "x", "--video", "--cbf", "2"])
    mod.main()
    assert seen["cbf"] == 2 and seen["cbf_grid"] == 32 and seen["video"] is True
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", "x", "--cbf", "0", "--cbf-grid", "8"])
    mod.main()
    assert seen["cbf"] == 0 and seen["cbf_grid"] == 8
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", "x"])
    mod.main()
    assert seen["cbf"] is None
