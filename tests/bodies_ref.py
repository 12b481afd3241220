"""LiDAR sees agents, restated in NumPy float32: the yardstick of dgppo_lidar_scan_bodies / dgppo_lidar_observe_bodies.

Written from the definition in include/dgppo_hip.h, never from a kernel: one rounded float32 operation per statement, in
the definition's order, so a kernel compiled without contraction gives the same bits.  For receiver i, beam (dx, dy) from
(sx, sy) and every other agent j in increasing j at (cx, cy), rho the body radius:

    mx = cx - sx;  my = cy - sy;  cc = (mx mx + my my) - rho rho;  aa = dx dx + dy dy;  bb = dx mx + dy my
    disc = bb bb - aa cc
    t_j = 0 if cc <= 0, else t = (bb - sqrt(disc)) / aa if bb > 0 and disc >= 0 and 0 <= t <= 1, else 1e6
    a_body = min_j t_j (1e6 when n == 1);   alpha = a_obs if a_obs is NaN, else a_body if a_body < a_obs, else a_obs

Every comparison is false on NaN, so a NaN or infinite row returns nothing and a_body is never NaN."""
import numpy as np

F = np.float32
NO_RETURN = F(1e6)


def ray_table_ref(n_rays: int, sense_range: float) -> np.ndarray:
    """(R, 2) beams of length sense_range at R angles from -pi in steps of 2 pi / R: for the hand-made cases only (ray
    R / 2 is exactly (sense_range, 0)); the GPU tests take the env's own table."""
    th = -np.pi + 2.0 * np.pi * np.arange(n_rays) / n_rays
    return (np.stack([np.cos(th), np.sin(th)], -1) * sense_range).astype(F)


def body_alpha_ref(agent: np.ndarray, ray_dirs: np.ndarray, rho) -> np.ndarray:
    """a_body (B, n, R) of agent rows (B, n, >= 2) and beams (R, 2)."""
    agent, ray_dirs = np.asarray(agent, F), np.asarray(ray_dirs, F)
    B, n = agent.shape[:2]
    R = ray_dirs.shape[0]
    rho = F(rho)
    rr = rho * rho
    dx, dy = ray_dirs[None, None, :, 0], ray_dirs[None, None, :, 1]  # (1, 1, R)
    dxx = dx * dx
    dyy = dy * dy
    aa = dxx + dyy
    sx, sy = agent[:, :, None, 0], agent[:, :, None, 1]  # (B, n, 1): the receivers
    best = np.full((B, n, R), NO_RETURN, F)
    with np.errstate(all="ignore"):
        for j in range(n):
            cx, cy = agent[:, j, None, None, 0], agent[:, j, None, None, 1]  # (B, 1, 1): sender j
            mx = cx - sx
            my = cy - sy
            mxx = mx * mx
            myy = my * my
            m2 = mxx + myy
            cc = m2 - rr
            px = dx * mx
            py = dy * my
            bb = px + py
            b2 = bb * bb
            ac = aa * cc
            disc = b2 - ac
            root = np.sqrt(disc)
            num = bb - root
            t = num / aa
            hit = (bb > 0) & (disc >= 0) & (t >= 0) & (t <= 1)
            tj = np.where(np.broadcast_to(cc <= 0, hit.shape), F(0), np.where(hit, t, NO_RETURN)).astype(F)
            tj[:, j, :] = NO_RETURN  # j == i is not a body of the receiver's
            best = np.where(tj < best, tj, best)
    assert best.dtype == F and not np.isnan(best).any()
    return best


def nearer_alpha_ref(a_obs: np.ndarray, a_body: np.ndarray) -> np.ndarray:
    """Step 4: the obstacle NaN propagates, else the nearer of the two returns."""
    a_obs, a_body = np.asarray(a_obs, F), np.asarray(a_body, F)
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(a_obs), a_obs, np.where(a_body < a_obs, a_body, a_obs)).astype(F)


def scan_bodies_ref(a_obs: np.ndarray, agent: np.ndarray, ray_dirs: np.ndarray, rho) -> np.ndarray:
    """alpha (B, n, R) of lidar_scan(bodies=True): `a_obs` (B, n, R) the obstacle-only scan of the same state."""
    return nearer_alpha_ref(a_obs, body_alpha_ref(agent, ray_dirs, rho))
