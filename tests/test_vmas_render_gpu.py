"""VMASEnv.render_frames / render_video on the GPU (dgppo_render_frames_vmas, the VMAS form of csrc/render.hip's
kernel) against the float64 brute-force restatement in tests/vmas_render_ref.py.

Parity bar: the renderer's own (tests/test_render_gpu.py assert_parity): every byte within 1 LSB of the reference and
at most 1 % of the RGB bytes different at all.  The arithmetic is that renderer's fp32 arithmetic on the same four
distances plus one fabs and one subtraction (the outline), and cos / sin of three angles taken once per primitive in
fp32 (relative error 1e-7 on coordinates of at most 2.4, a 1e-4 share of the finest pixel pitch used here), so the
bar's room is the same; the negative controls show that no layer fits inside it."""
import functools
import glob
import os
import sys

import numpy as np
import pytest
import torch

from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.trainer.rollout import RolloutEngine

import vmas_render_ref as V
from test_render_gpu import _entry, _host, assert_parity

pytestmark = pytest.mark.gpu

KINDS = ["VMASWheel", "VMASReverseTransport"]
SIZES = (33, 97, 256)  # one pixel past a 32 x 32 tile; an odd size (4 x 4 tiles, the last partial); 8 x 8 whole tiles


def graph_of(env, states, record):
    """A graph whose states (B[, T], 4, 4) and record (B, 1, 8) are the given ones (the renderer reads nothing else)."""
    g = env.empty_graph(tuple(states.shape[:-2]), states.device)
    return env._assemble(g.nodes, g.edges, states, g.receivers, g.senders, record)


def reference(env, graph, S, record=None, **kw):
    """render_ref on host copies of every frame of `graph` -> uint8 (*batch, S, S, 4)."""
    cfg, st = V.cfg_numbers(env), _host(graph.states)
    rec = _host(graph.env_states.record if record is None else record)
    bs = st.shape[:-2]
    out = np.empty(bs + (S, S, 4), dtype=np.uint8)
    for idx in np.ndindex(*bs):
        out[idx] = V.render_ref(cfg, st[idx], rec[idx[0]].reshape(-1)[:8], S, **kw)
    return out


@functools.lru_cache(maxsize=None)
def frames(kind):
    """(env, (2, 3) graph): env.reset(key=7, n_env=2) plus 2 random-action steps, stacked along T."""
    dev = torch.device("cuda:0")
    env = make_env(kind, 3, device=dev)
    g = [env.reset(key=7, n_env=2)]
    gen = torch.Generator(device="cpu").manual_seed(11)
    for _ in range(2):
        a = (torch.rand(2, 3, env.action_dim, generator=gen) * 2 - 1).to(dev)
        g.append(env.step(g[-1], a).graph)
    graph = graph_of(env, torch.stack([x.states for x in g], dim=1), g[0].env_states.record)
    torch.cuda.synchronize()
    return env, graph


@functools.lru_cache(maxsize=None)
def frames_reference(kind, S):
    env, graph = frames(kind)
    ref = reference(env, graph, S)
    ref.setflags(write=False)
    return ref


# ---- parity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_parity(cuda, kind, S):
    env, graph = frames(kind)
    img = env.render_frames(graph, size=S)
    torch.cuda.synchronize()
    assert img.shape == (2, 3, S, S, 4) and img.dtype == torch.uint8 and img.device == graph.states.device
    ref = frames_reference(kind, S)
    assert_parity(img, ref, f"{kind} S={S}")
    assert (ref[..., :3] != 255).any(axis=(2, 3, 4)).all()  # no empty frame


def test_dpi_sets_the_size_and_fov_is_ignored(cuda):
    env, graph = frames("VMASWheel")
    img = env.render_frames(graph, dpi=5, viz_opts={"fov": False})
    assert img.shape == (2, 3, 50, 50, 4) and torch.equal(img, env.render_frames(graph, size=50))


# ---- hand-made states ------------------------------------------------------------------------------------------
def test_hand_made_wheel_states(cuda):
    """Line angles 0, pi / 2, -3 and a wound-up 7.0; goal / avoid angles on either side of +-pi; an agent on the view's
    corner, one outside the view, two coincident."""
    env = make_env("VMASWheel", 3, device=cuda)
    half = 1.02 * 1.2
    agents = [[[half, half], [1.5, 0.0], [0.3, -0.4]], [[-0.5, 0.5], [0.2, 0.7], [0.2, 0.7]],
              [[-half, -half], [0.0, -1.0], [0.01, -1.0]], [[0.9, 0.0], [0.0, 0.0], [-2.0, 3.0]]]
    st = torch.zeros(4, 4, 4)
    st[:, :3, :2] = torch.tensor(agents)
    st[:, 3, 0] = torch.tensor([0.0, np.pi / 2, -3.0, 7.0])
    rec = torch.zeros(4, 1, 8)
    rec[:, 0, 0] = torch.tensor([3.1, -3.1, np.pi, 3.3])  # goal
    rec[:, 0, 1] = torch.tensor([-3.1, 3.1, -np.pi, -3.3])  # avoid
    g = graph_of(env, st.to(cuda), rec.to(cuda))
    for S in (33, 97):
        img = env.render_frames(g, size=S)
        torch.cuda.synchronize()
        ref = reference(env, g, S)
        assert_parity(img, ref, f"hand-made Wheel S={S}")
        assert (ref[0, 0, S - 1, :3] != 255).any()  # the corner agent reaches the corner pixel
    assert (ref[3, 48, 48, :3] == np.floor(255 * V.C1 + 0.5)).all()  # S = 97: agent 1 over the line at the origin


def test_hand_made_transport_states(cuda):
    """The box half outside the view, an obstacle centred outside it, the goal under the box centre."""
    env = make_env("VMASReverseTransport", 3, device=cuda)
    st = torch.zeros(3, 4, 4)
    st[:, 3, :2] = torch.tensor([[0.8, 0.0], [0.1, -0.05], [-0.75, 0.79]])
    st[:, :3, :2] = st[:, 3:4, :2] + torch.tensor([[0.1, 0.1], [-0.2, 0.05], [0.0, -0.25]])
    rec = torch.zeros(3, 1, 8)
    rec[:, 0] = torch.tensor([[0.4, 0.4, 0.9, 0.9, -0.5, -0.5, 0.0, 0.85], [0.1, -0.05, 0.5, 0.5, -0.5, 0.5, 0.3, -0.5],
                              [-0.75, 0.79, -2.0, 0.0, 0.0, 0.0, 0.81, -0.81]])
    g = graph_of(env, st.to(cuda), rec.to(cuda))
    for S in (33, 97, 256):
        img = env.render_frames(g, size=S)
        torch.cuda.synchronize()
        assert_parity(img, reference(env, g, S), f"hand-made Transport S={S}")


# ---- negative controls: every layer is seen ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def control_frame(kind):
    dev = torch.device("cuda:0")
    env = make_env(kind, 3, device=dev)
    st, rec = V.control_scene(int(env.cfg.engine))
    g = graph_of(env, torch.from_numpy(st)[None].to(dev), torch.from_numpy(rec).view(1, 1, 8).to(dev))
    img = _host(env.render_frames(g, size=512))
    return env, st, rec, img


@pytest.mark.parametrize("kind,layer", [(k, lay) for k, e in zip(KINDS, (V.WHEEL, V.TRANSPORT)) for lay in V.LAYERS[e]])
def test_reference_without_a_layer_fails_parity(cuda, kind, layer):
    env, st, rec, img = control_frame(kind)
    cfg = V.cfg_numbers(env)
    if layer == 1:
        assert_parity(img[0], V.render_ref(cfg, st, rec, 512), f"{kind} control scene")
    without = V.render_ref(cfg, st, rec, 512, skip_layers={layer})
    with pytest.raises(AssertionError):
        assert_parity(img[0], without, f"{kind} without layer {layer}")
    assert np.abs(img[0].astype(np.int16) - without.astype(np.int16)).max() > 1


# ---- non-finite inputs -------------------------------------------------------------------------------------------
def test_non_finite_wheel_inputs_drop_their_primitives(cuda):
    """A NaN line angle (both halves of the line), an inf agent row (its disc), a NaN avoid angle (the sector)."""
    env, graph = frames("VMASWheel")
    states, record = graph.states.clone(), graph.env_states.record[:, 0].clone()
    states[0, 1, 3, 0] = float("nan")
    states[1, 2, 1, :] = float("inf")
    record[1, 0, 1] = float("nan")
    bad = graph_of(env, states, record)
    img = env.render_frames(bad, size=97)
    torch.cuda.synchronize()
    good, cfg = frames_reference("VMASWheel", 97), V.cfg_numbers(env)
    st, rec = _host(graph.states), _host(graph.env_states.record)[:, 0, 0]
    ref = good.copy()
    ref[0, 1] = V.render_ref(cfg, st[0, 1], rec[0], 97, skip_layers={2, 3})
    for t in range(3):
        ref[1, t] = V.render_ref(cfg, st[1, t], rec[1], 97, skip_layers={1}, skip_agents={1} if t == 2 else ())
    for idx in ((0, 1), (1, 0), (1, 2)):
        assert np.abs(ref[idx].astype(np.int16) - good[idx]).max() > 1, idx  # what was dropped was visible
    assert (ref[0, 0] == good[0, 0]).all() and (ref[0, 2] == good[0, 2]).all()
    assert_parity(img, ref, "Wheel non-finite")
    assert (reference(env, bad, 97) == ref).all()  # the reference drops the same primitives by itself


def test_non_finite_transport_inputs_drop_their_primitives(cuda):
    """An inf box row (outline and centre), a NaN agent coordinate, a NaN obstacle coordinate and a NaN goal."""
    env, graph = frames("VMASReverseTransport")
    states, record = graph.states.clone(), graph.env_states.record[:, 0].clone()
    states[0, 0, 3, 1] = float("inf")
    states[0, 2, 0, 0] = float("nan")
    record[1, 0, 4] = float("nan")  # obstacle 1
    record[1, 0, 1] = float("-inf")  # goal
    bad = graph_of(env, states, record)
    img = env.render_frames(bad, size=97)
    torch.cuda.synchronize()
    ref, good = reference(env, bad, 97), frames_reference("VMASReverseTransport", 97)
    for idx in ((0, 0), (0, 2), (1, 0), (1, 1), (1, 2)):
        assert np.abs(ref[idx].astype(np.int16) - good[idx]).max() > 1, idx
    assert (ref[0, 1] == good[0, 1]).all()
    assert_parity(img, ref, "Transport non-finite")


# ---- strides, reuse, determinism -------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rollout(kind, B=3, T=5):
    dev = torch.device("cuda:0")
    env = make_env(kind, 3, max_step=T, device=dev)
    eng = RolloutEngine(env, B, T, dev)
    gen = torch.Generator(device="cpu").manual_seed(3)
    eng.actions.copy_((torch.rand(eng.actions.shape, generator=gen) * 2 - 1).to(dev))
    roll = eng.run(21)
    torch.cuda.synchronize()
    return env, eng, roll


@pytest.mark.parametrize("kind", KINDS)
def test_strided_rollout_view_is_read_in_place(cuda, kind, monkeypatch):
    env, eng, roll = rollout(kind)
    g = roll.graph
    assert g.states.shape[:2] == (3, 5) and not g.states.is_contiguous()
    seen = []
    op = torch.ops.dgppo.render_frames_vmas
    monkeypatch.setattr(torch.ops.dgppo, "render_frames_vmas",
                        lambda cfg, st, rec, out: seen.append((st.data_ptr(), st.stride())) or op(cfg, st, rec, out))
    img = env.render_frames(g, size=50)
    assert seen == [(g.states.data_ptr(), g.states.stride())]  # no copy: the view itself reaches the op
    dense = graph_of(env, g.states.contiguous(), eng.obstacles.clone())
    assert torch.equal(img, env.render_frames(dense, size=50))
    assert_parity(img, reference(env, dense, 50), f"{kind} rollout view")
    out = torch.full((3, 5, 50, 50, 4), 7, dtype=torch.uint8, device=cuda)
    got = env.render_frames(g, size=50, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(out, img)
    assert torch.equal(env.render_frames(g, size=50), img)  # two launches, identical bytes
    with pytest.raises(ValueError):
        env.render_frames(g, size=50, out=out[:, :4])


def test_op_schema_faketensor_and_argument_errors(cuda):
    env, graph = frames("VMASWheel")
    rec = graph.env_states.record[:, 0]
    out = torch.empty(2, 3, 50, 50, 4, dtype=torch.uint8, device=cuda)
    args = (env._cfg_handle, graph.states, rec, out)
    torch.library.opcheck(torch.ops.dgppo.render_frames_vmas.default, args, test_utils=("test_schema", "test_faketensor"))
    torch.ops.dgppo.render_frames_vmas(*args)
    assert torch.equal(out, env.render_frames(graph, size=50))
    with pytest.raises(ValueError, match="contiguous"):
        torch.ops.dgppo.render_frames_vmas(env._cfg_handle, graph.states.transpose(-1, -2), rec, out)
    with pytest.raises(ValueError, match="out must be"):
        torch.ops.dgppo.render_frames_vmas(env._cfg_handle, graph.states, rec, out[:, :2])
    with pytest.raises(ValueError, match="record must be"):
        torch.ops.dgppo.render_frames_vmas(env._cfg_handle, graph.states, rec[:1], out)
    lidar = make_env("LidarSpread", 3, num_obs=2, device=cuda)
    with pytest.raises(ValueError, match="DGPPO_EINVAL"):  # the entry takes the two VMAS engines only
        torch.ops.dgppo.render_frames_vmas(lidar._cfg_handle, graph.states, rec, out)


# ---- render_video -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_render_video_chunks_and_gif(cuda, tmp_path, monkeypatch, kind):
    Image = pytest.importorskip("PIL.Image")
    env, eng, roll = rollout(kind)
    T, S = 5, 50
    calls = []
    inner = env.render_frames
    monkeypatch.setattr(env, "render_frames", lambda *a, **k: calls.append(1) or inner(*a, **k))
    unsafe = (roll.costs >= 0.0).any(dim=-1)[1]
    p1 = env.render_video(roll, tmp_path / "chunked.mp4", unsafe, dpi=5, episode=1, max_frame_bytes=2 * S * S * 4)
    assert p1.endswith("chunked.gif") and os.path.exists(p1) and len(calls) == 3  # 2 + 2 + 1 frames
    calls.clear()
    p2 = env.render_video(roll, tmp_path / "whole.gif", unsafe, dpi=5, episode=1)
    assert len(calls) == 1
    with Image.open(p1) as a, Image.open(p2) as b:
        assert a.n_frames == T and b.n_frames == T
        assert a.size == (S, S + S // 8) and b.size == a.size
        for t in range(T):
            a.seek(t), b.seek(t)
            assert np.array_equal(np.asarray(a.convert("RGB")), np.asarray(b.convert("RGB"))), t
    with pytest.raises(NotImplementedError, match="VMAS"):
        env.render_video(roll, tmp_path / "x.gif", unsafe, viz_opts={"Vh": None}, dpi=5)


# ---- CLI ----------------------------------------------------------------------------------------------------------
def test_cli_video_writes_one_gif_and_the_same_metrics(cuda, tmp_path, monkeypatch, capsys):
    pytest.importorskip("PIL")
    test_py, train_py = _entry("test"), _entry("train")
    argv = ["train.py", "--env", "VMASWheel", "-n", "3", "--algo", "dgppo", "--obs", "0", "--steps", "2",
            "--n-env-train", "8", "--batch-size", "256", "--n-env-test", "4", "--eval-interval", "1",
            "--save-interval", "2", "--log-dir", str(tmp_path)]
    monkeypatch.setattr(sys, "argv", argv)
    train_py.main()
    (run,) = glob.glob(os.path.join(str(tmp_path), "VMASWheel", "dgppo", "seed0_*"))
    base = ["test.py", "--path", run, "--epi", "2", "--max-step", "8"]
    metrics = lambda out: [ln for ln in out.splitlines() if ln.startswith(("epi: ", "reward: "))]  # noqa: E731
    capsys.readouterr()
    monkeypatch.setattr(sys, "argv", base)
    test_py.main()
    plain = metrics(capsys.readouterr().out)
    assert len(plain) == 3 and not os.path.exists(os.path.join(run, "videos"))  # the default: no video
    monkeypatch.setattr(sys, "argv", base + ["--video", "--max-videos", "1", "--dpi", "10"])
    test_py.main()
    assert metrics(capsys.readouterr().out) == plain
    gifs = glob.glob(os.path.join(run, "videos", "*", "*"))
    assert len(gifs) == 1 and gifs[0].endswith(".gif") and "_n3_epi00_reward" in os.path.basename(gifs[0])
    from PIL import Image

    with Image.open(gifs[0]) as im:
        assert im.n_frames == 8 and im.size == (100, 112)
    monkeypatch.setattr(sys, "argv", base + ["--video", "--cbf", "0"])
    with pytest.raises(SystemExit, match="--cbf is not built for VMASWheel"):
        test_py.main()
