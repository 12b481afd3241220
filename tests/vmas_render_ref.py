"""NumPy float64 brute-force restatement of the VMAS pictures (DESIGN.md "Rendering", the VMAS view and the two layer
tables; helper, not a test).  Every primitive on every pixel, no tiles, no culling, with the shape functions and the
coverage rule of tests/render_ref.py.

View: the square of side V = m * area_size about the origin, m = 1.02 (Wheel) / 1.01 (Transport), h = V / S, pixel
(row, col) samples p = (-V/2 + (col + 0.5) h, V/2 - (row + 0.5) h).  A 2 pt line has half-width V / 720, a patch's
1 pt outline V / 1440.  A primitive with a non-finite input contributes nothing.

Layers, bottom to top (`skip_layers` leaves some out: the tests' negative controls):
  VMASWheel                                                         VMASReverseTransport
  1  avoid sector, radius 2.4, half-angle 15 deg   C0 0.2           1  arena outline [-hw, hw]^2             C3 1
  2  line, positive half (1.0 x 0.05 about +0.5 u) C5 1             2  goal disc, radius 0.01                C5 0.5
  3  line, negative half                           C3 1             3  obstacle discs 0..2, radius 0.15      C0 0.7
  4  goal ray, origin -> 2 (cos g, sin g)          C5 0.2           4  box outline 0.6 x 0.6                 C3 1
  5  agents 0, 1, 2 (2 on top), radius 0.03        C2 C1 C4 1       5  agents 0, 1, 2                        C2 C1 C4 1
                                                                    6  box centre disc, radius 0.005         C3 1
"""
import numpy as np

import render_ref as R

WHEEL, TRANSPORT = 4, 5  # DGPPO_ENGINE_VMAS_WHEEL / _TRANSPORT
C0, C1, C2, C3, C4, C5 = (np.array([(c >> 16) & 255, (c >> 8) & 255, c & 255], dtype=np.float64) / 255.0
                          for c in (0x1f77b4, 0xff7f0e, 0x2ca02c, 0xd62728, 0x9467bd, 0x8c564b))
AGENT_COLOURS = (C2, C1, C4)
LAYERS = {WHEEL: (1, 2, 3, 4, 5), TRANSPORT: (1, 2, 3, 4, 5, 6)}
LINE_LENGTH, LINE_WIDTH, SECTOR_R, SECTOR_HALF_DEG = 2.0, 0.05, 2.4, 15.0
BOX, OBS_R = 0.6, 0.15


def cfg_numbers(env):
    c = env.cfg
    return dict(engine=int(c.engine), area_size=float(c.area_size), agent_radius=float(c.car_radius),
                dist2goal=float(c.dist2goal))


def view(cfg, S):
    """(V, h, px, py) of an S x S image."""
    V = (1.02 if cfg["engine"] == WHEEL else 1.01) * cfg["area_size"]
    h = V / S
    col, row = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    return V, h, -V / 2 + (col + 0.5) * h, V / 2 - (row + 0.5) * h


def pixel_of(cfg, S, x, y):
    """(row, col) of the pixel whose square holds the world point (x, y)."""
    V, h, _, _ = view(cfg, S)
    return int(np.floor((V / 2 - y) / h)), int(np.floor((x + V / 2) / h))


def d_outline(px, py, cx, cy, w, hgt, half_width):
    return np.abs(R.d_rect(px, py, cx, cy, w, hgt, 1.0, 0.0)) - half_width


def render_ref(cfg, states, record, S, skip_layers=(), skip_agents=()):
    """One frame: states (4, 4) (agents 0..2, then the body row), record (8,) or (1, 8) -> uint8 (S, S, 4).
    `skip_agents`: agents whose disc is left out."""
    st = np.asarray(states, dtype=np.float64)
    rec = np.asarray(record, dtype=np.float64).reshape(-1)
    V, h, px, py = view(cfg, S)
    img = np.ones((S, S, 3), dtype=np.float64)

    def paint(d, colour, alpha):
        w = (alpha * R.coverage(d, h))[..., None]
        img[...] = img + w * (colour - img)

    def ok(*v):
        return bool(np.all(np.isfinite(v)))

    def agents():
        for i in range(3):
            if i not in skip_agents and ok(st[i, 0], st[i, 1]):
                paint(R.d_circle(px, py, st[i, 0], st[i, 1], cfg["agent_radius"]), AGENT_COLOURS[i], 1.0)

    if cfg["engine"] == WHEEL:
        goal, avoid, a = rec[0], rec[1], st[3, 0]
        if 1 not in skip_layers and ok(avoid):
            paint(R.d_wedge(px, py, 0.0, 0.0, np.cos(avoid), np.sin(avoid), np.deg2rad(SECTOR_HALF_DEG), SECTOR_R),
                  C0, 0.2)
        for layer, sign, colour in ((2, 1.0, C5), (3, -1.0, C3)):
            if layer not in skip_layers and ok(a):
                c, s = np.cos(a), np.sin(a)
                paint(R.d_rect(px, py, sign * 0.25 * LINE_LENGTH * c, sign * 0.25 * LINE_LENGTH * s, 0.5 * LINE_LENGTH,
                               LINE_WIDTH, c, s), colour, 1.0)
        if 4 not in skip_layers and ok(goal):
            paint(R.d_edge(px, py, 0.0, 0.0, LINE_LENGTH * np.cos(goal), LINE_LENGTH * np.sin(goal), V / 720), C5, 0.2)
        if 5 not in skip_layers:
            agents()
    else:
        box = st[3, :2]
        if 1 not in skip_layers:
            paint(d_outline(px, py, 0.0, 0.0, cfg["area_size"], cfg["area_size"], V / 1440), C3, 1.0)
        if 2 not in skip_layers and ok(rec[0], rec[1]):
            paint(R.d_circle(px, py, rec[0], rec[1], cfg["dist2goal"]), C5, 0.5)
        if 3 not in skip_layers:
            for o in range(3):
                if ok(rec[2 + 2 * o], rec[3 + 2 * o]):
                    paint(R.d_circle(px, py, rec[2 + 2 * o], rec[3 + 2 * o], OBS_R), C0, 0.7)
        if 4 not in skip_layers and ok(*box):
            paint(d_outline(px, py, box[0], box[1], BOX, BOX, V / 1440), C3, 1.0)
        if 5 not in skip_layers:
            agents()
        if 6 not in skip_layers and ok(*box):
            paint(R.d_circle(px, py, box[0], box[1], 0.5 * cfg["dist2goal"]), C3, 1.0)
    out = np.full((S, S, 4), 255, dtype=np.uint8)
    out[..., :3] = np.floor(255.0 * img + 0.5).astype(np.uint8)
    return out


def control_scene(engine):
    """A hand-made frame (states (4, 4), record (8,)) on which no layer of the engine's table hides another: leaving
    any one of them out moves some byte by more than 1 LSB at S = 512, where the smallest primitive, the 0.005 disc,
    spans more than two pixels (the negative controls of the CPU and GPU tests)."""
    if engine == WHEEL:
        states = [[0.5, -0.5, 0, 0], [-0.6, 0.3, 0, 0], [0.2, 0.8, 0, 0], [0.4, 0.1, 0, 0]]
        record = [-2.0, 2.5, 0, 0, 0, 0, 0, 0]
    else:
        states = [[0.2, 0.0, 0, 0], [0.0, -0.2, 0, 0], [0.25, -0.2, 0, 0], [0.1, -0.05, 0, 0]]
        record = [-0.4, 0.45, 0.5, 0.5, -0.5, -0.5, 0.55, -0.45]
    return np.array(states, dtype=np.float32), np.array(record, dtype=np.float32)
