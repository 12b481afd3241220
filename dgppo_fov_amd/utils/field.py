"""Scalar fields over the arena: the learned constraint value Vh as a picture.

`sweep_states` moves one agent of an env state over a grid, `value_field` evaluates `algo.get_Vh` on the graphs of
those states for every frame of a rollout episode (the reference's get_bb_Vh, trainer/utils.py:160-190, with this
project's batched `env.get_graph`), and a `FieldLayer` hands such a field to `env.render_frames` /
`env.render_video` as `viz_opts={"field": layer}`: the banded, zero-lined layer 0 of the rasteriser
(csrc/render.hip; DESIGN.md "Rendering").  Plain torch plumbing: the kernels are get_graph's, the networks' and the
rasteriser's."""
from __future__ import annotations

import colorsys
import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

from .. import _lib

# the reference's BuRd colour map (plot.py:113-126) as (h, s, l) triples
_HSL = {"blue": (0.57, 0.5, 0.55), "light_blue": (0.5, 1.0, 0.995), "red": (0.028, 0.62, 0.59),
        "light_red": (0.098, 1.0, 0.995)}
FIELD_ALPHA = 0.9  # the bands' alpha on white
DEFAULT_BANDS = 14  # the reference's 15 contourf levels


def burd_colours() -> dict:
    """name -> straight sRGB (r, g, b) of the four BuRd anchors."""
    return {k: colorsys.hls_to_rgb(h, l, s) for k, (h, s, l) in _HSL.items()}


def palette(bands: int = DEFAULT_BANDS) -> np.ndarray:
    """(bands, 3) float32: band b is the reversed BuRd map at t = (b + 0.5) / bands -- light red -> red below the
    middle, blue -> light blue above it, so negative values are red and positive ones blue."""
    if not 2 <= int(bands) <= _lib.RENDER_MAX_BANDS:
        raise ValueError(f"bands must be in [2, {_lib.RENDER_MAX_BANDS}], got {bands}")
    c = {k: np.asarray(v, dtype=np.float64) for k, v in burd_colours().items()}
    out = np.empty((int(bands), 3), dtype=np.float64)
    for b in range(int(bands)):
        t = (b + 0.5) / int(bands)
        if t < 0.5:
            out[b] = c["light_red"] + 2 * t * (c["red"] - c["light_red"])
        else:
            out[b] = c["blue"] + (2 * t - 1) * (c["light_blue"] - c["blue"])
    return out.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _palette_on(bands: int, device: str) -> torch.Tensor:
    return torch.from_numpy(palette(bands)).to(device)


def palette_tensor(bands: int, device) -> torch.Tensor:
    """The palette as a device tensor (one per (bands, device), kept for the life of the process)."""
    return _palette_on(int(bands), str(torch.device(device)))


def _axis(a, name: str) -> np.ndarray:
    a = np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)
    if a.ndim != 1 or a.shape[0] < 2:
        raise ValueError(f"FieldLayer: {name} must be a 1-D axis with at least 2 nodes")
    if not np.isfinite(a).all():
        raise ValueError(f"FieldLayer: {name} must be finite")
    span = a[-1] - a[0]
    if not span > 0:
        raise ValueError(f"FieldLayer: {name} must increase ({name}[-1] > {name}[0])")
    if np.abs(np.diff(a) - span / (a.shape[0] - 1)).max() > 1e-5 * span:
        raise ValueError(f"FieldLayer: {name} must be uniform (to 1e-5 of its span)")
    return a


@dataclass
class FieldLayer:
    """A scalar field per frame for `viz_opts["field"]`: values float32 (*batch, Gy, Gx), contiguous, on the graph's
    device, node (j, i) at (xs[i], ys[j]); xs / ys uniform axes; K = `bands` hard-edged bands over
    [-half_range, half_range]; `label` is written in render_video's header."""
    values: torch.Tensor
    xs: object
    ys: object
    half_range: float
    bands: int = DEFAULT_BANDS
    label: str = ""

    def __post_init__(self):
        v = self.values
        if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.dim() < 2 or not v.is_contiguous():
            raise ValueError("FieldLayer: values must be a contiguous float32 (*batch, Gy, Gx) tensor")
        xs, ys = _axis(self.xs, "xs"), _axis(self.ys, "ys")
        if tuple(v.shape[-2:]) != (ys.shape[0], xs.shape[0]):
            raise ValueError(f"FieldLayer: values (..., {v.shape[-2]}, {v.shape[-1]}) do not match the axes "
                             f"(Gy = {ys.shape[0]}, Gx = {xs.shape[0]})")
        self.extent = (float(xs[0]), float(xs[-1]), float(ys[0]), float(ys[-1]))
        self.half_range = float(self.half_range)
        if not (math.isfinite(self.half_range) and self.half_range > 0):
            raise ValueError(f"FieldLayer: half_range must be finite and > 0, got {self.half_range}")
        self.bands = int(self.bands)
        if not 2 <= self.bands <= _lib.RENDER_MAX_BANDS:
            raise ValueError(f"FieldLayer: bands must be in [2, {_lib.RENDER_MAX_BANDS}], got {self.bands}")
        self.label = str(self.label)

    @classmethod
    def centred(cls, values: torch.Tensor, xs, ys, label: str = "", bands: int = DEFAULT_BANDS) -> "FieldLayer":
        """half_range = max |values| over the finite entries, 1.0 when that is 0: the reference's centered_norm
        (trainer/utils.py:152-158), zero in the middle of the colour map."""
        a = values.detach().abs()
        a = a[torch.isfinite(a)]
        m = float(a.max()) if a.numel() else 0.0
        return cls(values, xs, ys, m if m > 0 else 1.0, bands, label)

    def sliced(self, sl) -> "FieldLayer":
        """The layer of the frames `sl` of the leading batch axis (same axes, half_range, bands and label)."""
        return FieldLayer(self.values[sl], self.xs, self.ys, self.half_range, self.bands, self.label)


def grid_axes(env, G: int = 32):
    """(xs, ys): G nodes from 0 to the arena's side on both axes."""
    a = torch.linspace(0.0, float(env.area_size), int(G), dtype=torch.float32)
    return a, a.clone()


def sweep_states(env, state, agent: int, xs: torch.Tensor, ys: torch.Tensor):
    """`state` (an env state tuple with batch (F,), as env.state_rows accepts) with agent `agent` moved over the grid:
    the state tuple with batch F * Gy * Gx, row-major over (f, j, i), whose agent row `agent` has columns 0 and 1
    replaced by (xs[i], ys[j]); every other column and row is kept.  With F == 1 the goal and obstacle rows are
    zero-stride views, otherwise copies.  Works on CPU tensors (there is no kernel here)."""
    if env.ENGINE in env._VMAS_ENGINES:
        raise NotImplementedError("VMAS envs: sweep_states is not supported (get_graph of given states is not: the env "
                                  "record carries contact-physics state)")
    a, goal, third, F = env.state_rows(state, "sweep_states: state")
    n = env.num_agents
    if not isinstance(agent, (int, np.integer)) or not 0 <= int(agent) < n:
        raise ValueError(f"sweep_states: agent must be an index in [0, {n}), got {agent!r}")
    for name, t in (("xs", xs), ("ys", ys)):
        if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.shape[0] < 1 or t.dtype != torch.float32:
            raise ValueError(f"sweep_states: {name} must be a float32 (G,) tensor")
    Gx, Gy = int(xs.shape[0]), int(ys.shape[0])
    G = Gy * Gx
    moved = a.float().unsqueeze(1).unsqueeze(1).repeat(1, Gy, Gx, 1, 1)  # (F, Gy, Gx, n, sd), a copy
    moved[:, :, :, int(agent), 0] = xs.to(a.device).view(1, 1, Gx)
    moved[:, :, :, int(agent), 1] = ys.to(a.device).view(1, Gy, 1)

    def over_grid(t):
        if t is None:
            return None
        t = t.unsqueeze(1).expand((F, G) + tuple(t.shape[1:]))
        return t[0] if F == 1 else t.reshape((F * G,) + tuple(t.shape[2:]))

    return moved.view((F * G,) + tuple(a.shape[1:])), over_grid(goal), over_grid(third)


def _graph_bytes(env, algo) -> int:
    """Bytes of one transient graph of the sweep with its carry rows."""
    N, E = env.n_nodes, env.n_edges
    carry = env.num_agents * getattr(algo, "rnn_layers", 1) * getattr(algo, "n_carries", 1) * 64
    return 4 * (N * (env.node_dim + env.state_dim + 1) + E * (env.edge_dim + 2) + 2 * carry)


def value_field(algo, rollout, episode: int, agent: int, xs: torch.Tensor, ys: torch.Tensor,
                max_graph_bytes: int = 1 << 30) -> torch.Tensor:
    """Vh of agent `agent` had it stood at every node of the grid, for every frame of rollout.graph[episode]: float32
    (T, Gy, Gx, n_cost) = algo.get_Vh(env.get_graph(sweep_states(...)), carry)[..., agent, :] with the other agents,
    the goals, the obstacles and the carry (rollout.rnn_states[episode, t], repeated over the grid) fixed.  Frames are
    taken in chunks whose transient graphs stay within max_graph_bytes."""
    if not callable(getattr(algo, "get_Vh", None)):
        raise ValueError(f"{type(algo).__name__} has no get_Vh: there is no constraint value to draw")
    env = algo._env
    g = rollout.graph
    if g.states.dim() != 4:
        raise ValueError("value_field: rollout.graph must have batch shape (B, T)")
    T, n, ng, O = int(g.states.shape[1]), env.num_agents, env.num_goals, env.n_obs
    Gx, Gy = int(xs.shape[0]), int(ys.shape[0])
    G = Gy * Gx
    states = g.states[episode]  # (T, N, sd)
    if O == 0:
        third = None
    elif env._obstacle_fields() > 0:
        third = env._obstacles_of(g)[episode]  # (T, O, 16), expanded over T
    else:
        third = states[:, n + ng:n + ng + O]
    rnn = rollout.rnn_states
    per = max(1, int(max_graph_bytes) // (G * _graph_bytes(env, algo)))
    out = torch.empty((T, Gy, Gx, env.n_cost), dtype=torch.float32, device=states.device)
    for t0 in range(0, T, per):
        t1 = min(T, t0 + per)
        F = t1 - t0
        base = (states[t0:t1, :n], states[t0:t1, n:n + ng], None if third is None else third[t0:t1])
        graph = env.get_graph(sweep_states(env, base, agent, xs, ys))
        carry = None
        if rnn is not None:
            c = rnn[episode, t0:t1]
            carry = c.unsqueeze(1).expand((F, G) + tuple(c.shape[1:])).reshape((F * G,) + tuple(c.shape[1:]))
        vh = algo.get_Vh(graph, carry)
        out[t0:t1] = vh[:, int(agent), :].view(F, Gy, Gx, -1)
    return out
