"""The field layer on the GPU (dgppo_render_frames_field, csrc/render.hip) against the float64 restatement of its rule
(tests/field_ref.py), and what feeds it: algo.get_Vh against the float64 network oracle, value_field against the NumPy
env oracle.

Parity bar (tests/test_render_gpu.py's): every byte within 1 LSB of the reference and at most 1 % of the RGB bytes
different at all, alpha 255 -- on the DECIDED pixels: where the band coordinate s or the grid coordinates u, v lie
within 1e-3 of an integer, fp32 and float64 may pick the neighbouring band or cell, and those pixels (at most 1 % of
the inside ones) are left out.  tests/test_field_cpu.py measures an fp32 NumPy evaluation of the rule against float64
under the same bar: 0 LSB on the decided pixels, 0.13 % / 0.15 % undecided at S = 50 / 96."""
import glob
import os
import sys

import numpy as np
import pytest
import torch
import yaml

from dgppo_fov_amd.algo import make_algo
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.nn.layers import GraphBatch
from dgppo_fov_amd.trainer.rollout import RolloutEngine
from dgppo_fov_amd.utils import field as F
from oracle import env as O
from oracle import nets_t as NT

import field_ref as FR
import render_ref as R
import test_render_gpu as TR
from test_nets_gpu import _close

pytestmark = pytest.mark.gpu

EXTENT = (0.013, 1.487, 0.021, 1.379)
GX, GY = 9, 7
SIZES = (50, 96)


def axes(extent=EXTENT, gx=GX, gy=GY):
    return np.linspace(extent[0], extent[1], gx), np.linspace(extent[2], extent[3], gy)


def analytic(bs, extent=EXTENT, gx=GX, gy=GY):
    """The analytic field with another phase per frame -> float32 (*bs, gy, gx)."""
    xs, ys = axes(extent, gx, gy)
    out = np.empty(tuple(bs) + (gy, gx), dtype=np.float32)
    for k, idx in enumerate(np.ndindex(*bs)):
        out[idx] = FR.analytic_field(xs, ys, phase=0.37 * k)
    return out


def layer_of(values, dev, extent=EXTENT, **kw):
    xs, ys = axes(extent, values.shape[-1], values.shape[-2])
    return F.FieldLayer.centred(torch.from_numpy(values).to(dev), xs, ys, **kw)


def reference(env, graph, S, values, layer, **kw):
    """render_field_ref on host copies of every frame -> (uint8 (*bs, S, S, 4), undecided (*bs, S, S), inside)."""
    cfg = R.cfg_numbers(env)
    st, rc, sn = TR._host(graph.states), TR._host(graph.receivers), TR._host(graph.senders)
    ob = TR._host(TR._obstacles(env, graph))
    bs = st.shape[:-2]
    out = np.empty(bs + (S, S, 4), dtype=np.uint8)
    und, ins = np.empty(bs + (S, S), dtype=bool), np.empty(bs + (S, S), dtype=bool)
    pal = F.palette(layer.bands)
    for idx in np.ndindex(*bs):
        out[idx], und[idx], ins[idx] = FR.render_field_ref(cfg, st[idx], rc[idx], sn[idx], None if ob is None else
                                                           ob[idx], S, values[idx], layer.extent, layer.half_range,
                                                           pal, **kw)
    return out, und, ins


def assert_parity(img, ref, undecided, inside, what=""):
    img = TR._host(img) if isinstance(img, torch.Tensor) else img
    assert img.shape == ref.shape and img.dtype == np.uint8, (what, img.shape, ref.shape)
    decided = ~undecided
    diff = np.abs(img.astype(np.int16) - ref.astype(np.int16))[..., :3][decided]
    frac = float((diff != 0).mean())
    share = float(undecided.sum()) / max(1.0, float(inside.sum()))
    print(f"{what}: max |diff| {int(diff.max())} LSB, differing decided RGB bytes {frac:.2e}, undecided {share:.2%}")
    assert diff.max() <= 1, (what, int(diff.max()))
    assert frac <= 0.01, (what, frac)
    assert share <= 0.01, (what, share)
    assert (img[..., 3] == 255).all(), what


# ---- layer parity ------------------------------------------------------------------------------------------------
CONFIGS = [("LidarSpread", 3, 2), ("MPESpread", 3, 3)]


@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("cfg", CONFIGS, ids=["LidarSpread-n3-o2", "MPESpread-n3-o3"])
def test_parity(cuda, cfg, S):
    env, graph = TR.frames(*cfg)
    values = analytic((2, 3))
    layer = layer_of(values, cuda)
    img = env.render_frames(graph, size=S, viz_opts={"field": layer})
    torch.cuda.synchronize()
    assert img.shape == (2, 3, S, S, 4) and img.dtype == torch.uint8 and img.device == graph.states.device
    ref, und, ins = reference(env, graph, S, values, layer)
    assert_parity(img, ref, und, ins, f"{cfg} S={S}")
    plain = TR._host(env.render_frames(graph, size=S))
    assert (np.abs(TR._host(img).astype(np.int16) - plain).reshape(6, -1).max(axis=1) > 50).all()  # the field is there


@pytest.mark.parametrize("control", ["bands", "line", "swapped"])
def test_reference_without_a_part_differs(cuda, control):
    """Negative controls: the reference without the bands, without the zero line, and with every frame given
    another frame's field is more than 1 LSB away from the image in every frame."""
    env, graph = TR.frames("LidarSpread", 3, 2)
    values = analytic((2, 3))
    layer = layer_of(values, cuda)
    img = TR._host(env.render_frames(graph, size=50, viz_opts={"field": layer})).astype(np.int16)
    if control == "swapped":
        moved = np.roll(values.reshape(6, GY, GX), 1, axis=0).reshape(values.shape)
        other, _, _ = reference(env, graph, 50, moved, layer)
    else:
        other, _, _ = reference(env, graph, 50, values, layer, **{control: False})
    per_frame = np.abs(img - other.astype(np.int16)).reshape(6, -1).max(axis=1)
    assert (per_frame > 1).all(), (control, per_frame)


# ---- edge cases ----------------------------------------------------------------------------------------------------
def test_two_by_two_grid(cuda):
    env, graph = TR.frames("LidarSpread", 3, 2)
    values = analytic((2, 3), gx=2, gy=2)
    layer = layer_of(values, cuda)
    img = env.render_frames(graph, size=50, viz_opts={"field": layer})
    assert_parity(img, *reference(env, graph, 50, values, layer), "2 x 2 grid")


@pytest.mark.parametrize("S", SIZES)
def test_extent_inside_the_arena_leaves_the_outside_alone(cuda, S):
    env, graph = TR.frames("LidarSpread", 3, 2)
    extent = (0.31, 1.13, 0.42, 0.97)
    values = analytic((2, 3), extent)
    layer = layer_of(values, cuda, extent)
    img = env.render_frames(graph, size=S, viz_opts={"field": layer})
    ref, und, ins = reference(env, graph, S, values, layer)
    assert_parity(img, ref, und, ins, f"inner extent S={S}")
    plain = env.render_frames(graph, size=S)
    outside = torch.from_numpy(~ins).to(cuda)
    assert 0.6 < float(outside.float().mean()) < 0.9
    assert torch.equal(img[outside], plain[outside])
    assert not torch.equal(img[~outside], plain[~outside])


def test_extent_larger_than_the_arena(cuda):
    env, graph = TR.frames("MPESpread", 3, 3)
    extent = (-0.397, 2.119, -0.293, 1.931)  # no pixel centre of S = 50 on a grid line
    values = analytic((2, 3), extent)
    layer = layer_of(values, cuda, extent)
    img = env.render_frames(graph, size=50, viz_opts={"field": layer})
    ref, und, ins = reference(env, graph, 50, values, layer)
    assert ins.all()
    assert_parity(img, ref, und, ins, "outer extent")


def test_nan_node_leaves_its_four_cells_unpainted(cuda):
    env, graph = TR.frames("LidarSpread", 3, 2)
    values = analytic((2, 3))
    values[0, 1, 3, 4] = np.nan
    values[1, 0, 0, 0] = np.inf
    layer = layer_of(values, cuda)
    assert np.isfinite(layer.half_range)
    img = env.render_frames(graph, size=96, viz_opts={"field": layer})
    torch.cuda.synchronize()  # the call returns
    ref, und, ins = reference(env, graph, 96, values, layer)
    assert_parity(img, ref, und, ins, "NaN node")
    xs, ys = axes()
    px, py, _ = R.pixel_centres(env.area_size, 96)
    hole = torch.from_numpy((px > xs[3]) & (px < xs[5]) & (py > ys[2]) & (py < ys[4])).to(cuda)
    plain = env.render_frames(graph, size=96)
    assert int(hole.sum()) > 100 and torch.equal(img[0, 1][hole], plain[0, 1][hole])
    assert not torch.equal(img[0, 0][hole], plain[0, 0][hole])
    corner = torch.from_numpy((px < xs[1]) & (py < ys[1]) & ins[1, 0]).to(cuda)
    assert int(corner.sum()) > 20 and torch.equal(img[1, 0][corner], plain[1, 0][corner])


def test_constant_field_has_no_line(cuda):
    env, graph = TR.frames("LidarSpread", 3, 2)
    values = np.full((2, 3, GY, GX), 0.25, dtype=np.float32)
    values[1] = 0.0  # exactly zero everywhere: |val| / |grad| is 0 / 0, and still no line
    xs, ys = axes()
    layer = F.FieldLayer(torch.from_numpy(values).to(cuda), xs, ys, 1.0, bands=13)  # 13: s = 8.125 and 6.5, mid-band
    img = env.render_frames(graph, size=50, viz_opts={"field": layer})
    ref, und, ins = reference(env, graph, 50, values, layer)
    assert_parity(img, ref, und, ins, "constant field")
    plain = TR._host(env.render_frames(graph, size=50))
    pal = F.palette(13).astype(np.float64)
    for b, band in ((0, 8), (1, 6)):
        want = np.floor(255.0 * (1 + 0.9 * (pal[band] - 1)) + 0.5)
        free = ins[b] & (plain[b, ..., :3] == 255).all(axis=-1)  # inside pixels no scene shape touches
        assert free.sum() > 500
        assert (np.abs(TR._host(img)[b][free][:, :3] - want) <= 1).all()


# ---- no regression, views, reuse -------------------------------------------------------------------------------------
def test_render_frames_without_a_field_is_the_raw_op(cuda):
    env, graph = TR.frames("LidarSpread", 3, 2)
    ob = TR._obstacles(env, graph)[:, 0]
    out = torch.empty(2, 3, 50, 50, 4, dtype=torch.uint8, device=cuda)
    torch.ops.dgppo.render_frames(env._cfg_handle, graph.states, graph.receivers, graph.senders, ob, out, 1)
    assert torch.equal(env.render_frames(graph, size=50), out)
    assert torch.equal(env.render_frames(graph, size=50, viz_opts={"field": None}), out)
    TR.assert_parity(out, TR.frames_reference("LidarSpread", 3, 2, 50), "no field")


def test_strided_rollout_view_reuse_and_determinism(cuda):
    env, eng, roll = TR.rollout()
    g = roll.graph
    assert g.states.shape[:2] == (3, 5) and not g.states.is_contiguous()
    values = analytic((3, 5))
    layer = layer_of(values, cuda)
    img = env.render_frames(g, size=50, viz_opts={"field": layer})
    dense = env._assemble(g.nodes.contiguous(), g.edges.contiguous(), g.states.contiguous(), g.receivers.contiguous(),
                          g.senders.contiguous(), eng.obstacles.clone())
    assert torch.equal(img, env.render_frames(dense, size=50, viz_opts={"field": layer}))
    ref, und, ins = reference(env, dense, 50, values, layer)
    assert_parity(img[1], ref[1], und[1], ins[1], "rollout view, episode 1")
    out = torch.full((3, 5, 50, 50, 4), 7, dtype=torch.uint8, device=cuda)
    got = env.render_frames(g, size=50, viz_opts={"field": layer}, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, img)
    assert torch.equal(env.render_frames(g, size=50, viz_opts={"field": layer}), img)  # two launches, identical bytes
    with pytest.raises(ValueError, match="field"):
        env.render_frames(g, size=50, viz_opts={"field": layer.sliced(slice(0, 2))})
    with pytest.raises(ValueError, match="FieldLayer"):
        env.render_frames(g, size=50, viz_opts={"field": values})


def test_op_schema_faketensor_and_argument_errors(cuda):
    env, graph = TR.frames("LidarSpread", 3, 2)
    ob = TR._obstacles(env, graph)[:, 0]
    out = torch.empty(2, 3, 50, 50, 4, dtype=torch.uint8, device=cuda)
    values = analytic((2, 3))
    layer = layer_of(values, cuda)
    pal = F.palette_tensor(14, cuda)
    op = torch.ops.dgppo.render_frames_field
    head = (env._cfg_handle, graph.states, graph.receivers, graph.senders, ob)

    def tail(values=layer.values, palette=pal, extent=list(layer.extent), half=layer.half_range, out=out):
        return (values, palette, extent, half, 0.9, env.area_size / 480.0, out, 1)

    torch.library.opcheck(op.default, head + tail(), test_utils=("test_schema", "test_faketensor"))
    op(*head, *tail())
    assert torch.equal(out, env.render_frames(graph, size=50, viz_opts={"field": layer}))
    with pytest.raises(ValueError, match="values"):
        op(*head, *tail(values=layer.values[..., ::2]))
    with pytest.raises(ValueError, match="values"):
        op(*head, *tail(values=layer.values[0]))
    with pytest.raises(ValueError, match="palette"):
        op(*head, *tail(palette=pal[:, :2]))
    with pytest.raises(ValueError, match="extent"):
        op(*head, *tail(extent=[0.0, 1.0, 0.0]))
    with pytest.raises(ValueError, match="out must be"):
        op(*head, *tail(out=out[:, :2]))
    for bad in (dict(palette=pal[:1]), dict(half=0.0), dict(half=float("nan")), dict(extent=[1.0, 1.0, 0.0, 1.0])):
        with pytest.raises(ValueError, match="DGPPO_EINVAL"):
            op(*head, *tail(**bad))


# ---- get_Vh ----------------------------------------------------------------------------------------------------------
def _algo(name, env, cuda, **kw):
    return make_algo(name, env=env, node_dim=env.node_dim, edge_dim=env.edge_dim, state_dim=env.state_dim,
                     action_dim=env.action_dim, n_agents=env.num_agents, batch_size=64, rnn_step=2, seed=2, device=cuda,
                     **kw)


def _host_graph(env, graph):
    gb = GraphBatch.from_graph(graph, env)
    return {k: getattr(gb, k).cpu().numpy() for k in ("nodes", "edges", "receivers", "senders")}


@pytest.mark.parametrize("eid,n,obs", [("LidarSpread", 3, 2), ("LidarOmniTarget", 3, 1)])
def test_get_vh_dgppo_against_the_float64_oracle(cuda, eid, n, obs):
    env = make_env(eid, n, num_obs=obs, device=cuda)
    algo = _algo("dgppo", env, cuda)
    B = 4
    g = env.reset(key=13, n_env=B)
    h = np.random.default_rng(3).standard_normal((B, 1, n, 1, 64)).astype(np.float32) * 0.5
    vh = algo.get_Vh(g, torch.from_numpy(h).to(cuda), algo.params)
    torch.cuda.synchronize()
    assert vh.shape == (B, n, env.n_cost) and vh.dtype == torch.float32
    ref = NT.vh(NT.to_t(algo.Vh.flax()), _host_graph(env, g), h.reshape(B, n, 64), n)
    _close(vh.cpu().numpy(), ref.detach().numpy().reshape(B, n, -1), what="get_Vh")
    assert torch.equal(algo.get_Vh(g, torch.from_numpy(h).to(cuda)), vh)
    with pytest.raises(AssertionError, match="params"):
        algo.get_Vh(g, torch.from_numpy(h).to(cuda), {"policy": None})


def test_get_vh_hcbfcrpo_is_the_env_cost(cuda):
    env = make_env("LidarSpread", 3, num_obs=2, device=cuda)
    algo = _algo("hcbfcrpo", env, cuda)
    g = env.reset(key=14, n_env=4)
    assert torch.equal(algo.get_Vh(g), env.get_cost(g)) and torch.equal(algo.get_Vh(g, None, None), env.get_cost(g))
    assert not hasattr(_algo("informarl", env, cuda), "get_Vh")


# ---- value_field -----------------------------------------------------------------------------------------------------
def _rollout(env, algo, cuda, B=2, T=2):
    eng = RolloutEngine(env, B, T, cuda, actor=algo.actor, mode=RolloutEngine.MODE_DET)
    roll = eng.run(23)
    torch.cuda.synchronize()
    return eng, roll


def _moved(roll, episode, t, agent, xs, ys, n, ng):
    """Host (agent, goal) rows of frame t with `agent` at every grid node, row-major over (j, i)."""
    st = TR._host(roll.graph.states)[episode, t]
    G = len(xs) * len(ys)
    a = np.repeat(st[None, :n], G, axis=0).copy()
    gx, gy = np.meshgrid(xs, ys)
    a[:, agent, 0], a[:, agent, 1] = gx.reshape(-1), gy.reshape(-1)
    return a, np.repeat(st[None, n:n + ng], G, axis=0)


def test_value_field_hcbfcrpo_is_the_oracle_cost_of_the_moved_state(cuda):
    eid, n, obs, T, episode, agent = "LidarSpread", 3, 2, 2, 1, 1
    env = make_env(eid, n, num_obs=obs, max_step=T, device=cuda)
    algo = _algo("hcbfcrpo", env, cuda)
    eng, roll = _rollout(env, algo, cuda, T=T)
    xs, ys = torch.tensor([0.2, 0.75, 1.3]), torch.tensor([0.4, 1.1])
    field = F.value_field(algo, roll, episode, agent, xs, ys)
    torch.cuda.synchronize()
    assert field.shape == (T, 2, 3, env.n_cost) and field.dtype == torch.float32
    spec = O.Spec(eid, n, obs)
    ob = TR._host(eng.obstacles)[episode]
    for t in range(T):
        a, _ = _moved(roll, episode, t, agent, xs.numpy(), ys.numpy(), n, n)
        third = np.repeat(ob[None], 6, axis=0)
        hits, _ = O.lidar(a[..., :2], third, O.ray_table(spec.n_rays, spec.comm_r), spec.top_k)
        cost = O.get_cost_lidar(spec, a, hits)
        np.testing.assert_array_equal(field[t].cpu().numpy().reshape(6, -1), cost[:, agent], err_msg=f"t={t}")
    assert len(np.unique(field.cpu().numpy())) > 3  # the grid moves the cost


def test_value_field_dgppo(cuda):
    eid, n, obs, T, episode, agent = "LidarSpread", 3, 2, 2, 1, 1
    env = make_env(eid, n, num_obs=obs, max_step=T, device=cuda)
    algo = _algo("dgppo", env, cuda)
    eng, roll = _rollout(env, algo, cuda, T=T)
    x0, y0 = (float(v) for v in roll.graph.states[episode, 0, agent, :2])
    xs, ys = torch.tensor([x0, 0.75, 1.3]), torch.tensor([y0, 1.1])
    field = F.value_field(algo, roll, episode, agent, xs, ys)
    torch.cuda.synchronize()
    assert field.shape == (T, 2, 3, env.n_cost)
    spec = O.Spec(eid, n, obs)
    ob = TR._host(eng.obstacles)[episode]
    p = NT.to_t(algo.Vh.flax())
    carry = TR._host(roll.rnn_states)[episode]  # (T, 1, n, 1, 64)
    for t in range(T):
        a, gl = _moved(roll, episode, t, agent, xs.numpy(), ys.numpy(), n, n)
        host = O.initial_graph(spec, a, gl, np.repeat(ob[None], 6, axis=0))
        ref = NT.vh(p, host, np.repeat(carry[t].reshape(1, n, 64), 6, axis=0), n).detach().numpy().reshape(6, n, -1)
        _close(field[t].cpu().numpy().reshape(6, -1), ref[:, agent], what=f"value_field t={t}")
    # node (0, 0) of frame 0 is the agent's own position: the unmodified rollout graph
    g = roll.graph
    own = env._assemble(g.nodes[episode, 0:1], g.edges[episode, 0:1], g.states[episode, 0:1], g.receivers[episode, 0:1],
                        g.senders[episode, 0:1], eng.obstacles[episode:episode + 1])
    vh = algo.get_Vh(own, roll.rnn_states[episode, 0:1])
    _close(field[0, 0, 0].cpu().numpy(), vh[0, agent].cpu().numpy(), what="own position")
    # one frame per chunk and all frames at once: the same bits
    one = F.value_field(algo, roll, episode, agent, xs, ys, max_graph_bytes=1)
    assert torch.equal(one, field) and torch.equal(F.value_field(algo, roll, episode, agent, xs, ys, 1 << 40), field)


# ---- render_video ----------------------------------------------------------------------------------------------------
def test_render_video_with_a_field(cuda, tmp_path, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    env, eng, roll = TR.rollout()
    T, S = 5, 50
    values = analytic((T,))
    values[3:] *= 3.0  # a per-chunk half_range would colour the last frames differently
    layer = layer_of(values, cuda, label="h = -max Vh, agent 0")
    unsafe = (roll.costs >= 0.0).any(dim=-1)[1]
    calls = []
    inner = env.render_frames
    monkeypatch.setattr(env, "render_frames", lambda *a, **k: calls.append(k["viz_opts"]["field"]) or inner(*a, **k))
    p1 = env.render_video(roll, tmp_path / "chunked.gif", unsafe, {"field": layer}, dpi=5, episode=1,
                          max_frame_bytes=2 * S * S * 4)
    assert len(calls) == 3 and [c.values.shape[0] for c in calls] == [2, 2, 1]
    assert all(c.half_range == layer.half_range for c in calls)
    p2 = env.render_video(roll, tmp_path / "whole.gif", unsafe, {"field": layer}, dpi=5, episode=1)
    monkeypatch.setattr(env, "render_frames", inner)
    p3 = env.render_video(roll, tmp_path / "plain.gif", unsafe, dpi=5, episode=1)
    with Image.open(p1) as a, Image.open(p2) as b, Image.open(p3) as c:
        assert a.n_frames == T and b.n_frames == T and c.n_frames == T
        assert a.size == (S, S + S // 8) and b.size == a.size and c.size == a.size
        for t in range(T):
            a.seek(t), b.seek(t), c.seek(t)
            fa, fb, fc = (np.asarray(im.convert("RGB")) for im in (a, b, c))
            assert np.array_equal(fa, fb), t
            assert not np.array_equal(fa[S // 8:], fc[S // 8:]), t
    with pytest.raises(ValueError, match="FieldLayer"):
        env.render_video(roll, tmp_path / "x.gif", unsafe, {"field": layer.sliced(slice(0, 2))}, dpi=5, episode=1)
    for key in ("cbf", "Vh"):
        with pytest.raises(NotImplementedError, match="not built"):
            env.render_video(roll, tmp_path / "x.gif", unsafe, {key: None, "field": layer}, dpi=5, episode=1)


# ---- CLI -------------------------------------------------------------------------------------------------------------
def test_cli_cbf_writes_one_gif_and_the_same_metrics(cuda, tmp_path, monkeypatch, capsys):
    pytest.importorskip("PIL")
    test_py, train_py = TR._entry("test"), TR._entry("train")
    argv = ["train.py", "--env", "LidarOmniTarget", "-n", "3", "--algo", "dgppo", "--obs", "2", "--steps", "2",
            "--n-env-train", "8", "--batch-size", "256", "--n-env-test", "4", "--eval-interval", "1",
            "--save-interval", "2", "--log-dir", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", argv)
    train_py.main()
    (run,) = glob.glob(os.path.join(str(tmp_path), "LidarOmniTarget", "dgppo", "seed0_*"))
    base = ["test.py", "--path", run, "--epi", "2", "--max-step", "8"]
    metrics = lambda out: [ln for ln in out.splitlines() if ln.startswith(("epi: ", "reward: "))]  # noqa: E731
    capsys.readouterr()
    monkeypatch.setattr(sys, "argv", base + ["--cbf", "0"])  # without --video: no effect
    test_py.main()
    plain = metrics(capsys.readouterr().out)
    assert len(plain) == 3 and not os.path.exists(os.path.join(run, "videos"))
    video = ["--video", "--max-videos", "1", "--dpi", "10"]
    monkeypatch.setattr(sys, "argv", base + video + ["--cbf", "0", "--cbf-grid", "8"])
    test_py.main()
    assert metrics(capsys.readouterr().out) == plain
    gifs = glob.glob(os.path.join(run, "videos", "*", "*"))
    assert len(gifs) == 1 and gifs[0].endswith(".gif")
    from PIL import Image

    with Image.open(gifs[0]) as im:
        assert im.n_frames == 8 and im.size == (100, 112)
        rgb = np.asarray(im.convert("RGB"))[12:].reshape(-1, 3)
    assert (rgb != 255).any(axis=-1).mean() > 0.9  # the field fills the scene
    for bad in ("3", "-1"):
        monkeypatch.setattr(sys, "argv", base + video + ["--cbf", bad])
        with pytest.raises(SystemExit, match="agent index"):
            test_py.main()
    # a run whose algorithm has no get_Vh: refused before anything is loaded
    other = tmp_path / "informarl_run"
    other.mkdir()
    with open(os.path.join(run, "config.yaml")) as f:
        cfg = {}
        for d in yaml.safe_load_all(f):
            cfg.update(d or {})
    cfg["algo"] = "informarl"
    with open(other / "config.yaml", "w") as f:
        yaml.safe_dump(cfg, f)
    monkeypatch.setattr(sys, "argv", ["test.py", "--path", str(other), "--epi", "2", "--max-step", "8"] + video +
                        ["--cbf", "0"])
    with pytest.raises(SystemExit, match="get_Vh"):
        test_py.main()
    assert len(glob.glob(os.path.join(run, "videos", "*", "*"))) == 1
