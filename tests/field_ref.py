"""NumPy restatement of the field layer's pixel rule (DESIGN.md "Rendering", layer 0; helper, not a test).

`field_background` paints the layer on white: a pixel centre p has grid coordinates u = (px - x0) / dx, v = (py - y0) /
dy, dx = (x1 - x0) / (Gx - 1); it is inside when 0 <= u <= Gx - 1 and 0 <= v <= Gy - 1, its cell is i = clamp(floor u,
0, Gx - 2) (j likewise); outside pixels and cells with a non-finite node stay white; val is the bilinear interpolation
(x first, then y) and grad val the cell's analytic gradient in world units; s = (val + half) / (2 half) K, band b =
clamp(floor s, 0, K - 1), c += 0.9 (palette[b] - c); then, where |grad| L > 1e-6 half, the black zero line of coverage
clamp(0.5 - (|val| / |grad| - L / 480) / h, 0, 1).  float64 by default; dtype=np.float32 evaluates the same rule in
fp32 (what a kernel can do at best).

`undecided`: inside pixels whose s, u or v lies within 1e-3 of an integer -- there fp32 and float64 may legitimately
pick the neighbouring band or cell.

`render_field_ref` composites that background and then repeats render_ref's layer loop (layers 1-5) on it."""
import numpy as np

import render_ref as R

ALPHA = 0.9
UNDECIDED = 1e-3


def analytic_field(xs, ys, phase=0.0):
    """sin(3.1 x + 0.4 + phase) cos(2.3 y - 0.7) + 0.15 on the grid, float32 (Gy, Gx)."""
    x, y = np.meshgrid(np.asarray(xs, np.float64), np.asarray(ys, np.float64))
    return (np.sin(3.1 * x + 0.4 + phase) * np.cos(2.3 * y - 0.7) + 0.15).astype(np.float32)


def field_background(values, extent, half_range, palette, L, S, dtype=np.float64, bands=True, line=True):
    """values (Gy, Gx) -> (img (S, S, 3) of `dtype`, undecided (S, S) bool, inside (S, S) bool)."""
    T = dtype
    val = np.asarray(values).astype(T)
    Gy, Gx = val.shape
    pal = np.asarray(palette).astype(T)
    K = pal.shape[0]
    x0, x1, y0, y1 = (T(e) for e in extent)
    half, Lt = T(half_range), T(L)
    h = Lt / T(S)
    col, row = np.meshgrid(np.arange(S).astype(T), np.arange(S).astype(T))
    px, py = (col + T(0.5)) * h, (T(S) - row - T(0.5)) * h
    dx, dy = (x1 - x0) / T(Gx - 1), (y1 - y0) / T(Gy - 1)
    u, v = (px - x0) / dx, (py - y0) / dy
    inside = (u >= 0) & (u <= Gx - 1) & (v >= 0) & (v <= Gy - 1)
    fi, fj = np.clip(np.floor(u), 0, Gx - 2), np.clip(np.floor(v), 0, Gy - 2)
    i, j = fi.astype(np.int64), fj.astype(np.int64)
    v00, v10, v01, v11 = val[j, i], val[j, i + 1], val[j + 1, i], val[j + 1, i + 1]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        finite = np.isfinite(v00) & np.isfinite(v10) & np.isfinite(v01) & np.isfinite(v11)
        tx, ty = (u - fi).astype(T), (v - fj).astype(T)
        lo, hi = v00 + tx * (v10 - v00), v01 + tx * (v11 - v01)
        f = lo + ty * (hi - lo)
        gx, gy = ((v10 - v00) + ty * ((v11 - v01) - (v10 - v00))) / dx, (hi - lo) / dy
        s = (f + half) / (T(2) * half) * T(K)
        painted = inside & finite
        band = np.clip(np.floor(np.where(painted, s, 0)), 0, K - 1).astype(np.int64)
        img = np.ones((S, S, 3), dtype=T)
        if bands:
            img = np.where(painted[..., None], img + T(ALPHA) * (pal[band] - img), img)
        gn = np.sqrt(gx * gx + gy * gy)
        on = painted & (gn * Lt > T(1e-6) * half)
        d = np.abs(f) / np.where(on, gn, 1)
        w = np.where(on, np.clip(T(0.5) - (d - Lt / T(480)) / h, 0, 1), 0).astype(T)
        if line:
            img = img - w[..., None] * img

        def near(a):
            return np.abs(a - np.round(a)) < UNDECIDED

        undecided = painted & (near(s) | near(u) | near(v))
    return img.astype(T), undecided, inside


def to_bytes(img):
    out = np.full(img.shape[:2] + (4,), 255, dtype=np.uint8)
    out[..., :3] = np.floor(255.0 * img.astype(np.float64) + 0.5).astype(np.uint8)
    return out


def render_field_ref(cfg, states, receivers, senders, obstacles, S, values, extent, half_range, palette, fov=True,
                     bands=True, line=True):
    """One frame: the field, then render_ref's layers 1-5 on it -> (uint8 (S, S, 4), undecided, inside (S, S))."""
    st = np.asarray(states, dtype=np.float64)
    rc, sn = np.asarray(receivers).astype(np.int64), np.asarray(senders).astype(np.int64)
    n, ng, O, N, L = cfg["n"], cfg["n_goals"], cfg["n_obs"], cfg["n_nodes"], cfg["area_size"]
    px, py, h = R.pixel_centres(L, S)
    img, undecided, inside = field_background(values, extent, half_range, palette, L, S, bands=bands, line=line)

    def paint(d, colour, alpha):
        w = (alpha * R.coverage(d, h))[..., None]
        img[...] = img + w * (colour - img)

    def ok(*v):
        return bool(np.all(np.isfinite(v)))

    if cfg["engine"] == R.ENGINE_MPE:
        for i in range(n + ng, n + ng + O):
            if ok(st[i, 0], st[i, 1]):
                paint(R.d_circle(px, py, st[i, 0], st[i, 1], cfg["obs_radius"]), R.RED, 1.0)
    if cfg["engine"] == R.ENGINE_OMNI and fov:
        for i in range(n - 1):
            if ok(*st[i, :4]):
                paint(R.d_wedge(px, py, st[i, 0], st[i, 1], st[i, 2], st[i, 3], np.deg2rad(cfg["fov_angle_deg"]),
                                cfg["fov_rmax"]), R.BLUE, 0.15)
    for r, s in zip(rc, sn):
        if not (0 <= r < N - 1 and 0 <= s < N - 1):
            continue
        if ok(st[s, 0], st[s, 1], st[r, 0], st[r, 1]):
            paint(R.d_edge(px, py, st[s, 0], st[s, 1], st[r, 0], st[r, 1], L / 720),
                  R.GREEN if n <= s < n + ng else R.GREY, 0.5)
    for i in list(range(n + ng - 1, n - 1, -1)) + list(range(n - 1, -1, -1)):
        if ok(st[i, 0], st[i, 1]):
            paint(R.d_circle(px, py, st[i, 0], st[i, 1], cfg["car_radius"]), R.GREEN if i >= n else R.BLUE, 1.0)
    if cfg["engine"] != R.ENGINE_MPE and O > 0:
        for o in np.asarray(obstacles, dtype=np.float64):
            if ok(o[0], o[1], o[2], o[3], o[5], o[6]):
                paint(R.d_rect(px, py, o[0], o[1], o[2], o[3], o[5], o[6]), R.RED, 1.0)
    return to_bytes(img), undecided, inside
