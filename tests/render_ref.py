"""NumPy float64 brute-force restatement of the rendering pixel rule (DESIGN.md "Rendering"; helper, not a test).

Every primitive is evaluated on every pixel, no culling, no tiles: the world square [0, L]^2 maps onto S x S pixels
of pitch h = L / S, pixel (row, col) samples p = ((col + 0.5) h, (S - row - 0.5) h), a shape of signed distance d(p)
covers clamp(0.5 - d / h, 0, 1) of the pixel, and the shapes are composited in painter's order on straight sRGB
values, c += alpha * cov * (colour - c) from white; the byte is floor(255 c + 0.5), A = 255.

Layers, bottom to top (`skip_layers` leaves some out: the tests' negative controls):
  1  MPE obstacle circles (state rows [n + n_goals, n + n_goals + O))      #8a0000  alpha 1
  2  FoV wedges of agents 0 .. n-2 (Omni engine, fov=True)                  #0068ff  alpha 0.15
  3  edges 0 .. E-1 (capsules sender -> receiver, half-width L / 720)       #2fdd00 from a goal, else #333333; alpha 0.5
  4  goal circles n_goals-1 .. 0, then agent circles n-1 .. 0               #2fdd00 / #0068ff  alpha 1
  5  Lidar obstacle rectangles                                              #8a0000  alpha 1
"""
import numpy as np

RED, BLUE, GREEN, GREY = (np.array(c, dtype=np.float64) / 255.0 for c in
                          ((0x8a, 0, 0), (0, 0x68, 0xff), (0x2f, 0xdd, 0), (0x33, 0x33, 0x33)))
ENGINE_LIDAR, ENGINE_BICYCLE, ENGINE_MPE, ENGINE_OMNI = 0, 1, 2, 3


def cfg_numbers(env):
    """The cfg numbers the renderer reads, from a MultiAgentEnv."""
    c = env.cfg
    return dict(engine=int(c.engine), n=int(c.n_agents), n_goals=int(c.n_goals) or int(c.n_agents), n_obs=int(c.n_obs),
                n_nodes=int(c.n_nodes), area_size=float(c.area_size), car_radius=float(c.car_radius),
                obs_radius=float(c.obs_radius), fov_angle_deg=float(c.fov_angle_deg), fov_rmax=float(c.fov_rmax))


def pixel_centres(L, S):
    h = L / S
    col, row = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    return (col + 0.5) * h, (S - row - 0.5) * h, h


def d_circle(px, py, cx, cy, r):
    return np.hypot(px - cx, py - cy) - r


def d_rect(px, py, cx, cy, w, hgt, cos, sin):
    dx, dy = px - cx, py - cy
    qx = np.abs(cos * dx + sin * dy) - w / 2
    qy = np.abs(-sin * dx + cos * dy) - hgt / 2
    return np.hypot(np.maximum(qx, 0), np.maximum(qy, 0)) + np.minimum(np.maximum(qx, qy), 0)


def d_edge(px, py, ax, ay, bx, by, hw):
    pax, pay, bax, bay = px - ax, py - ay, bx - ax, by - ay
    t = np.clip((pax * bax + pay * bay) / max(bax * bax + bay * bay, 1e-12), 0, 1)
    return np.hypot(pax - t * bax, pay - t * bay) - hw


def d_wedge(px, py, cx, cy, hx, hy, beta, r):
    nrm = max(np.hypot(hx, hy), 1e-12)
    hx, hy = hx / nrm, hy / nrm
    dx, dy = px - cx, py - cy
    u, v = dx * hx + dy * hy, np.abs(dx * hy - dy * hx)
    sb, cb = np.sin(beta), np.cos(beta)
    ln = np.hypot(u, v) - r
    k = np.clip(v * sb + u * cb, 0, r)
    m = np.hypot(v - k * sb, u - k * cb)
    return np.maximum(ln, m * np.sign(cb * v - sb * u))


def coverage(d, h):
    return np.clip(0.5 - d / h, 0, 1)


def render_ref(cfg, states, receivers, senders, obstacles, S, fov=True, skip_layers=(), skip_nodes=()):
    """One frame: states (N, sd), receivers / senders (E,), obstacles (O, 16) or None -> uint8 (S, S, 4).
    `skip_nodes`: node rows whose primitives (circle, wedge, edges) are left out."""
    st = np.asarray(states, dtype=np.float64)
    rc, sn = np.asarray(receivers).astype(np.int64), np.asarray(senders).astype(np.int64)
    n, ng, O, N, L = cfg["n"], cfg["n_goals"], cfg["n_obs"], cfg["n_nodes"], cfg["area_size"]
    px, py, h = pixel_centres(L, S)
    img = np.ones((S, S, 3), dtype=np.float64)
    skip_nodes = set(int(i) for i in skip_nodes)

    def paint(d, colour, alpha):
        w = (alpha * coverage(d, h))[..., None]
        img[...] = img + w * (colour - img)

    def ok(*v):
        return bool(np.all(np.isfinite(v)))

    if 1 not in skip_layers and cfg["engine"] == ENGINE_MPE:
        for i in range(n + ng, n + ng + O):
            if i not in skip_nodes and ok(st[i, 0], st[i, 1]):
                paint(d_circle(px, py, st[i, 0], st[i, 1], cfg["obs_radius"]), RED, 1.0)
    if 2 not in skip_layers and cfg["engine"] == ENGINE_OMNI and fov:
        for i in range(n - 1):
            if i not in skip_nodes and ok(*st[i, :4]):
                paint(d_wedge(px, py, st[i, 0], st[i, 1], st[i, 2], st[i, 3], np.deg2rad(cfg["fov_angle_deg"]),
                              cfg["fov_rmax"]), BLUE, 0.15)
    if 3 not in skip_layers:
        for r, s in zip(rc, sn):
            if not (0 <= r < N - 1 and 0 <= s < N - 1) or r in skip_nodes or s in skip_nodes:
                continue
            if ok(st[s, 0], st[s, 1], st[r, 0], st[r, 1]):
                paint(d_edge(px, py, st[s, 0], st[s, 1], st[r, 0], st[r, 1], L / 720),
                      GREEN if n <= s < n + ng else GREY, 0.5)
    if 4 not in skip_layers:
        for i in list(range(n + ng - 1, n - 1, -1)) + list(range(n - 1, -1, -1)):
            if i not in skip_nodes and ok(st[i, 0], st[i, 1]):
                paint(d_circle(px, py, st[i, 0], st[i, 1], cfg["car_radius"]), GREEN if i >= n else BLUE, 1.0)
    if 5 not in skip_layers and cfg["engine"] != ENGINE_MPE and O > 0:
        ob = np.asarray(obstacles, dtype=np.float64)
        for o in ob:
            if ok(o[0], o[1], o[2], o[3], o[5], o[6]):
                paint(d_rect(px, py, o[0], o[1], o[2], o[3], o[5], o[6]), RED, 1.0)
    out = np.full((S, S, 4), 255, dtype=np.uint8)
    out[..., :3] = np.floor(255.0 * img + 0.5).astype(np.uint8)
    return out
