"""NumPy float32 restatement of field-of-view neighbour sensing (include/dgppo_hip.h, dgppo_agent_fov).

For an ordered pair (receiver i, sender j), i != j, receiver row (x, y, c, s, ...) -- columns 2, 3 the heading's cosine
and sine, used as given -- in the operation order of oracle.env.get_cost_omni's `lx`, `ly`, `nrm`, `h_a` lines:

    dx = x_j - x_i;  dy = y_j - y_i
    lx = c * dx + s * dy;  ly = (-s) * dx + c * dy;  nrm = sqrt(lx * lx + ly * ly)
    in_fov[i, j] = (cb * (nrm + 1e-8) - lx) <= 0,      cb = cos(fp32(deg) * fp32(pi / 180)) (oracle.env.omni_cos_fov)

The diagonal is True without a test; NaN makes a pair unseen (the comparison is False); coincident agents have nrm = lx
= 0 and are seen exactly when cb <= 0 (the formula's quirk, kept); no range test.  `mistake=` builds the wrong masks the
tests must be able to tell from the right one.  Everything else (specs, resets, graphs, costs) is oracle.env's.
"""
import types

import numpy as np

from oracle import env as O

F = np.float32
MISTAKES = ("sender_heading", "swapped", "no_eps", "strict")


def cone_cos(deg):
    """cb of a half angle in degrees: oracle.env.omni_cos_fov's float32 product and shared fp32 cosine."""
    return O.omni_cos_fov(types.SimpleNamespace(params={"fov_angle_deg": deg}))


def fov_margin(agent, deg, mistake=None):
    """h (B, n, n) float32 = cb * (nrm + 1e-8) - lx for every ordered pair (the diagonal included, untested)."""
    agent = np.asarray(agent, F)
    assert mistake is None or mistake in MISTAKES
    recv, send = agent[:, :, None, :], agent[:, None, :, :]  # receiver i: (B, n, 1, sd), sender j: (B, 1, n, sd)
    if mistake == "swapped":
        recv, send = send, recv
    head = send if mistake == "sender_heading" else recv
    cb = cone_cos(deg)
    with np.errstate(all="ignore"):
        dx = send[..., 0] - recv[..., 0]
        dy = send[..., 1] - recv[..., 1]
        c, s_ = head[..., 2], head[..., 3]
        lx = c * dx + s_ * dy
        ly = (-s_) * dx + c * dy
        nrm = O.norm2d(lx, ly)
        h = cb * (nrm if mistake == "no_eps" else nrm + F(1e-8)) - lx
    h = np.broadcast_to(h, agent.shape[:1] + (agent.shape[1],) * 2)
    assert h.dtype == F
    return h


def field_of_view_ref(agent, deg, mistake=None):
    """agent (B, n, sd) float32 (columns 0..3 read), deg -> in_fov (B, n, n) bool."""
    h = fov_margin(agent, deg, mistake)
    with np.errstate(invalid="ignore"):
        seen = h < 0 if mistake == "strict" else h <= 0
    return seen | np.eye(h.shape[1], dtype=bool)[None]


def in_range_ref(spec, agent):
    """(B, n, n) bool: the agent-agent mask of oracle.env.build_graph (distance < comm_radius, diagonal False)."""
    ap = np.asarray(agent, F)[..., :2]
    d = O.norm2d(ap[:, :, None, 0] - ap[:, None, :, 0], ap[:, :, None, 1] - ap[:, None, :, 1])
    d = d + (np.eye(spec.n, dtype=F) * F(spec.comm_r + 1))[None]
    return d < F(spec.comm_r)


def mask_unseen_ref(spec, graph, seen):
    """build_graph's dict with the unseen pairs' leading agent-agent edges sent to the pad node (copies)."""
    n, pad = spec.n, spec.n_nodes - 1
    out = dict(graph)
    hide = ~seen.reshape(seen.shape[0], n * n)
    for f in ("receivers", "senders"):
        a = graph[f].copy()
        a[:, :n * n] = np.where(hide, np.int32(pad), a[:, :n * n])
        out[f] = a
    return out


def row(x, y, c=1.0, s=0.0, sd=7):
    """One agent row (sd,) float32: position, heading (c, s), zeros behind."""
    r = np.zeros(sd, F)
    r[:4] = x, y, c, s
    return r


def kat_scenes(sd=7):
    """The hand-made known answers: name -> (agent (2, sd), deg, expected in_fov (2, 2)).  Agent 0 is the receiver under
    test, at (1, 1) (once at the origin) with heading (1, 0) unless the name says otherwise; agent 1, the sender, has
    heading (1, 0) unless given, so where it sits ahead of agent 0 it has agent 0 behind it."""
    T, Fl = True, False
    nan = np.full(sd, np.nan, F)

    def pair(a, b):
        return np.stack([a, b])

    return {
        # deg = 0.001: cb == 1.0f exactly, so dead ahead h = (d + 1e-8) - d in fp32
        "hairline cone, dead ahead at 0.25: h == 0, seen (<= not <)":
            (pair(row(1, 1, sd=sd), row(1.25, 1, sd=sd)), 0.001, [[T, T], [Fl, T]]),
        "hairline cone, dead ahead at 1e-6: h == 1.0000008e-08, unseen (the 1e-8)":
            (pair(row(0, 0, sd=sd), row(1e-6, 0, sd=sd)), 0.001, [[T, Fl], [Fl, T]]),  # at the origin: fp32 keeps 1e-6
        # deg = 90: cb == -4.371139e-08, not 0
        "half plane, exactly abeam: seen":
            (pair(row(1, 1, sd=sd), row(1, 1.5, sd=sd)), 90.0, [[T, T], [T, T]]),
        "half plane, dead behind: unseen":
            (pair(row(1, 1, sd=sd), row(0.5, 1, sd=sd)), 90.0, [[T, Fl], [T, T]]),
        "coincident at 90: seen (cb <= 0)":
            (pair(row(1, 1, sd=sd), row(1, 1, 0.0, 1.0, sd=sd)), 90.0, [[T, T], [T, T]]),
        "coincident at 60: unseen (cb > 0)":
            (pair(row(1, 1, sd=sd), row(1, 1, 0.0, 1.0, sd=sd)), 60.0, [[T, Fl], [Fl, T]]),
        "NaN receiver row: its row and column are False off the diagonal":
            (pair(nan, row(1.2, 1, -1.0, 0.0, sd=sd)), 120.0, [[T, Fl], [Fl, T]]),
        "zero heading at 90: sees everyone (cb <= 0)":
            (pair(row(1, 1, 0.0, 0.0, sd=sd), row(0.5, 1.3, sd=sd)), 90.0, [[T, T], [T, T]]),
        "zero heading at 60: sees no one":
            (pair(row(1, 1, 0.0, 0.0, sd=sd), row(1.3, 1, sd=sd)), 60.0, [[T, Fl], [Fl, T]]),
    }

