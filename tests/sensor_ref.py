"""NumPy restatements for the sensor tests: the scan-to-hits rule in four lines, and alpha rows the ray cast never
produces."""
import numpy as np

F = np.float32


def hits_ref(agent, alpha, ray_tab, k):
    """(B, n, k, 2): the k smallest alphas per agent by a stable argsort (NaN last, -0 == +0, ties by ray index), each
    as start + (end - start) * alpha with end = start + ray, every operation rounded to float32."""
    with np.errstate(all="ignore"):
        order = np.argsort(alpha, axis=-1, kind="stable")[..., :k]
        start = agent[:, :, None, :2].astype(F)
        pts = (start + ((start + ray_tab[None, None]).astype(F) - start).astype(F) * alpha[..., None]).astype(F)
        return np.take_along_axis(pts, order[..., None], axis=2)


def hand_made_alpha(R, n, seed):
    """(7, n, R) float32; env b holds, for every agent: 0 all equal, 1 -0.0 next to +0.0 among positives, 2 negative
    values, 3 NaNs scattered, 4 all 1e6, 5 random with ties, 6 one of each kind per agent."""
    rng = np.random.default_rng(seed)
    a = np.empty((7, n, R), F)
    a[0] = F(0.25)
    a[1] = rng.uniform(0.0, 1.0, (n, R)).astype(F)
    a[1, :, ::2] = F(0.0)
    a[1, :, ::4] = F(-0.0)
    a[2] = rng.uniform(-2.0, 1.0, (n, R)).astype(F)
    a[3] = rng.uniform(0.0, 1.0, (n, R)).astype(F)
    a[3][rng.random((n, R)) < 0.4] = np.nan
    a[3, 0] = np.nan  # a whole row of NaN: the first k rays, in order
    a[4] = F(1e6)
    a[5] = rng.integers(0, 4, (n, R)).astype(F) / F(4)
    a[6] = rng.choice(np.array([0.0, -0.0, 0.5, -0.5, 1e6, np.nan, np.inf, -np.inf], F), size=(n, R))
    return a
