"""NumPy float32 restatement of line-of-sight neighbour sensing (include/dgppo_hip.h, dgppo_lidar_sight).

For an ordered pair (receiver i, sender j), i != j, P / Q = columns 0, 1 of agent rows i / j: blocked[i, j] is true iff
some edge of some obstacle is `valid` by the per-edge expressions of oracle.env.raytrace_alpha with (sx, sy) = P and
(ex, ey) = Q, restated below edge by edge (raytrace_alpha itself returns only the minimum over edges).  NaN and det ==
0 make an EDGE invalid (every comparison with the NaN / infinite quotient fails).  visible = ~blocked, diagonal True.
Everything else (specs, resets, rectangles, graphs) is oracle.env's.
"""
import numpy as np

from oracle import env as O

F = np.float32


def edge_valid(sx, sy, ex, ey, rec):
    """(..., 4) bool: `valid` of Rectangle.raytracing for each of the 4 edges.  sx..ey (...,), rec (..., 16)."""
    out = []
    with np.errstate(all="ignore"):
        for e in range(4):
            x3, y3 = rec[..., 8 + 2 * e], rec[..., 9 + 2 * e]
            e4 = (e - 1) % 4  # points[[-1, 0, 1, 2]]
            x4, y4 = rec[..., 8 + 2 * e4], rec[..., 9 + 2 * e4]
            det = (sx - ex) * (y4 - y3) - (sy - ey) * (x4 - x3)
            det = np.sign(det) * np.clip(np.abs(det), F(1e-7), F(1e7))
            alpha = ((y4 - y3) * (sx - x3) - (x4 - x3) * (sy - y3)) / det
            beta = (-(sy - ey) * (sx - x3) + (sx - ex) * (sy - y3)) / det
            assert alpha.dtype == F and beta.dtype == F
            out.append((alpha <= 1) & (alpha >= 0) & (beta <= 1) & (beta >= 0))
    return np.stack(out, -1)


def line_of_sight_ref(agent, obst):
    """agent (B, n, sd) float32 (columns 0, 1 read), obst (B, O, 16) float32 -> visible (B, n, n) bool."""
    agent, obst = np.asarray(agent, F), np.asarray(obst, F)
    B, n = agent.shape[:2]
    px, py = agent[:, :, None, None, 0], agent[:, :, None, None, 1]  # receiver i: (B, n, 1, 1)
    qx, qy = agent[:, None, :, None, 0], agent[:, None, :, None, 1]  # sender j:   (B, 1, n, 1)
    valid = edge_valid(px, py, qx, qy, obst[:, None, None, :, :])  # (B, n, n, O, 4)
    blocked = valid.any(axis=(-1, -2))
    return ~blocked | np.eye(n, dtype=bool)[None]


def in_range_ref(spec, agent):
    """(B, n, n) bool: the agent-agent mask of oracle.env.build_graph (distance < comm_radius, diagonal False)."""
    ap = np.asarray(agent, F)[..., :2]
    d = O.norm2d(ap[:, :, None, 0] - ap[:, None, :, 0], ap[:, :, None, 1] - ap[:, None, :, 1])
    d = d + (np.eye(spec.n, dtype=F) * F(spec.comm_r + 1))[None]
    return d < F(spec.comm_r)


def mask_unseen_ref(spec, graph, visible):
    """build_graph's dict with the unseen pairs' leading agent-agent edges sent to the pad node (copies)."""
    n, pad = spec.n, spec.n_nodes - 1
    out = dict(graph)
    hide = ~visible.reshape(visible.shape[0], n * n)
    for f in ("receivers", "senders"):
        a = graph[f].copy()
        a[:, :n * n] = np.where(hide, np.int32(pad), a[:, :n * n])
        out[f] = a
    return out


def observed_graph_ref(spec, agent, goal, obst, hits):
    """The observed graph under occlusion: oracle.env.build_graph on `hits` (B, n, k, 2) plus the mask."""
    return mask_unseen_ref(spec, O.build_graph(spec, agent, goal, hits), line_of_sight_ref(agent, obst))


def square(cx, cy, side, theta=0.0):
    """One axis-aligned (or rotated) square's record, (16,) float32, by oracle.env.make_rectangles."""
    return O.make_rectangles(np.array([[cx, cy]], F), np.array([side], F), np.array([side], F), np.array([theta], F))[0]


def kat_scenes():
    """The hand-made known-answer scenes: name -> (agent (n, 2), obst (O, 16), expected visible (n, n)).  The square
    has its centre at (1, 1) and side 0.5 (corners at 0.75 / 1.25)."""
    sq = square(1.0, 1.0, 0.5)[None]
    T, Fl = True, False
    both = np.array([[T, Fl], [Fl, T]])
    seen = np.ones((2, 2), bool)
    # corners: 0 (1.25, 1.25), 1 (0.75, 1.25), 2 (0.75, 0.75), 3 (1.25, 0.75); edge e runs from corner e to corner e - 1.
    # A NaN in corner 0 poisons edges 0 (right side) and 1 (top); edges 2 (left) and 3 (bottom) stay clean.
    nan_sq = sq.copy()
    nan_sq[0, 8] = np.nan
    return {
        "either side of the square": (np.array([[0.5, 1.0], [1.5, 1.0]], F), sq, both),
        "ends short of the square": (np.array([[0.2, 1.0], [0.7, 1.0]], F), sq, seen),
        # vertical through the square: parallel to its left and right sides (det == 0 there), cut by top and bottom
        "through, parallel to two sides": (np.array([[1.0, 0.5], [1.0, 1.5]], F), sq, both),
        # on the line of the bottom side (y = 0.75) but left of the square
        "collinear with a side, outside": (np.array([[0.2, 0.75], [0.6, 0.75]], F), sq, seen),
        "one agent inside the square": (np.array([[1.0, 1.0], [1.6, 1.1]], F), sq, both),
        "coincident agents": (np.array([[1.0, 1.0], [1.0, 1.0]], F), sq, seen),
        # the NaN corner poisons its own two edges only: a segment across a clean edge is still blocked, and one
        # that could only cross the NaN edges is visible
        "NaN corner, across a clean edge": (np.array([[1.0, 0.7], [1.0, 0.8]], F), nan_sq, both),  # the bottom
        "NaN corner, across a NaN edge": (np.array([[1.0, 1.2], [1.0, 1.3]], F), nan_sq, seen),  # the top
    }
