"""NumPy restatements of the update path's small primitives (csrc/nn.hip, csrc/gru.hip) and the four comparison
classes the primitive tests use (helper, not a test; tests/test_prim_ref_cpu.py checks it, tests/test_primitives_gpu.py
compares the kernels with it).

Every reference is written from the formulas of oracle/nets.py / oracle/nets_t.py and the flax definitions (GRUCell,
LSTMCell, LayerNorm with fast variance), never from a kernel, and takes `dt`: np.float64 is the reference proper,
np.float32 the same statements in single precision (`ref32` of the project's rule).  The backward statements are
hand-derived; the CPU file holds them against torch.autograd in float64.

Comparison classes (each returns the worst error / bound ratio and raises AssertionError above 1):
  bits      pure moves and selections: the int32 views are equal
  exact     reductions of integer-valued floats whose partial sums stay below 2^24: any summation order is exact in
            fp32, so the result equals the float64 sum exactly
  sums      reductions of random floats: |got - ref64| <= 1e-5 sum|x_i| (+ the slack of ambiguous gates); this is
            d 2^-24 sum|x| of a summation tree of depth d <= 160
  close     everything else: |got - ref64| <= 1e-5 scale + 8 |ref32 - ref64|, scale = 1 + |ref64| or, where the
            reference is a sum with cancellation, the sum of its summands' magnitudes
The TanhNormal clip branches use `close` with ref32 = None (no floor) and the summand scale: a float32 restatement
written like the kernel would carry the kernel's own cancellation and excuse it.
"""
import math

import numpy as np
from scipy import special

from oracle import nets as O

F64, F32 = np.float64, np.float32
# The clip threshold is a float32 constant in the reference program (and in the kernel); atanh amplifies its rounding
# by 1 / (1 - t^2) = 500, so the float64 restatement takes the float32 value, not 0.999.
THRESH = float(F32(O.THRESH))
AMB = 1e-5  # gates closer than this (relative to the scale of the gated quantity) may fall either way in fp32
MAX_AMB_FRAC = 1e-3


# ---- comparison classes ---------------------------------------------------------------------------------------
def check_bits(got, ref, what=""):
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.itemsize == 4 and ref.itemsize == 4, (what, got.shape, ref.shape)
    bad = got.view(np.int32) != ref.view(np.int32)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} words differ, first at {np.argwhere(bad)[0]}"
    return 0.0


def check_exact(got, ref64, what=""):
    got = np.asarray(got).astype(F64)
    ref64 = np.asarray(ref64, F64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    bad = got != ref64
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} exact sums differ, worst by "
                           f"{np.abs(got - ref64).max()}")
    return 0.0


def _ratio(err, bound, what):
    assert not np.isnan(err).any(), f"{what}: NaN in the result"
    r = float((err / bound).max()) if err.size else 0.0
    assert r <= 1.0, f"{what}: worst error {float(err.max()):.3e} is {r:.3g} x its bound"
    return r


def check_sums(got, ref64, sum_abs, slack=0.0, what=""):
    """sum_abs: sum of |summand| per output; slack: sum of |summand| over ambiguous gates per output."""
    got, ref64 = np.asarray(got).astype(F64), np.asarray(ref64, F64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    bound = 1e-5 * np.asarray(sum_abs, F64) + np.asarray(slack, F64) + 1e-30
    return _ratio(np.abs(got - ref64), np.broadcast_to(bound, got.shape), what)


def check_close(got, ref64, ref32=None, scale=None, keep=None, what=""):
    """keep: boolean mask of the elements compared (False: an ambiguous gate), at least 99.9 % of them."""
    got, ref64 = np.asarray(got).astype(F64), np.asarray(ref64, F64)
    assert got.shape == ref64.shape, (what, got.shape, ref64.shape)
    scale = 1.0 + np.abs(ref64) if scale is None else np.broadcast_to(np.asarray(scale, F64), ref64.shape)
    floor = 0.0 if ref32 is None else 8.0 * np.abs(np.asarray(ref32).astype(F64) - ref64)
    err, bound = np.abs(got - ref64), 1e-5 * scale + floor + 1e-30
    if keep is not None:
        keep = np.broadcast_to(keep, got.shape)
        assert (~keep).sum() <= MAX_AMB_FRAC * max(keep.size, 1000), f"{what}: {int((~keep).sum())} ambiguous gates"
        err, bound = err[keep], bound[keep]
    return _ratio(err, bound, what)


def amb_ok(amb):
    """At most 0.1 % of a case's elements may sit on an ambiguous gate (tiny cases: at most one in 1000 slots)."""
    return int(np.sum(amb)) <= MAX_AMB_FRAC * max(np.size(amb), 1000)


# ---- elementwise helpers in the working precision ----------------------------------------------------------------
def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softplus(x):
    return np.logaddexp(x, x.dtype.type(0))


def _tanh_fldj(x):
    """oracle.nets.tanh_fldj in the precision of x: 2 (log 2 - x - softplus(-2 x))."""
    return 2 * (x.dtype.type(math.log(2.0)) - x - _softplus(-2 * x))


def _normal_logpdf(x, mu, sd):
    """oracle.nets.normal_logpdf in the precision of its arguments."""
    z = (x - mu) / sd
    return -z * z / 2 - np.log(sd) - sd.dtype.type(0.5 * math.log(2 * math.pi))


def _as(dt, *xs):
    return [None if x is None else np.asarray(x).astype(dt) for x in xs]


# ---- LayerNorm (+ReLU) -------------------------------------------------------------------------------------------
def layernorm_fwd(x, scale, bias, relu, eps=1e-6, dt=F64):
    """flax LayerNorm (fast variance, oracle.nets.layernorm) then relu: (y, pre, mean, rstd, y_scale, rstd_scale).
    The fast variance E[x^2] - mean^2 is a sum with cancellation and rstd = (var + eps)^-1/2 amplifies its error by
    rstd^3 / 2, so the scales carry the summands' magnitudes through that derivative (and through x - mean for y)."""
    x, scale, bias = _as(dt, x, scale, bias)
    pre = O.layernorm(x, dict(scale=scale, bias=bias), eps=dt(eps))
    mean = x.mean(-1)
    ex2 = (x * x).mean(-1)
    var = np.maximum(dt(0), ex2 - mean * mean)
    rstd = 1 / np.sqrt(var + dt(eps))
    rstd_scale = 1 + rstd + rstd ** 3 / 2 * (ex2 + mean * mean)
    y_scale = 1 + np.abs(pre) + np.abs(scale) * ((np.abs(x) + np.abs(mean)[:, None]) * rstd[:, None]
                                                 + np.abs(x - mean[:, None]) * (rstd_scale - 1 - rstd)[:, None])
    return (O.relu(pre) if relu else pre), pre, mean, rstd, y_scale, rstd_scale


def layernorm_bwd(x, dy, scale, mean, rstd, gate=None, dt=F64):
    """Backward of y = xh scale + bias, xh = (x - mean) rstd with the row statistics given (the forward's);
    gate (bool, y > 0) applies the ReLU backward first.  Returns dx, dscale, dbias and the summand magnitudes of the
    two parameter sums and of dx."""
    x, dy, scale, mean, rstd = _as(dt, x, dy, scale, mean, rstd)
    g = dy if gate is None else np.where(gate, dy, dt(0))
    xh = (x - mean[:, None]) * rstd[:, None]
    gx = g * scale
    m1, m2 = gx.mean(-1, keepdims=True), (gx * xh).mean(-1, keepdims=True)
    dx = rstd[:, None] * (gx - m1 - xh * m2)
    dx_scale = np.abs(rstd[:, None]) * (np.abs(gx) + np.abs(gx).mean(-1, keepdims=True)
                                        + np.abs(xh) * np.abs(gx * xh).mean(-1, keepdims=True))
    return dx, (g * xh).sum(0), g.sum(0), np.abs(g * xh).sum(0), np.abs(g).sum(0), dx_scale


# ---- column sums -------------------------------------------------------------------------------------------------
def colsum_rows(buf, rows, cols, ld, grp=0, gstride=0):
    """The (rows, cols) matrix dgppo_colsum reads from the flat buffer: row r starts at r ld, or with grp > 0 at
    (r // grp) gstride + (r % grp) ld."""
    buf = np.ascontiguousarray(buf).reshape(-1)
    it, view = buf.itemsize, np.lib.stride_tricks.as_strided
    if grp <= 0:
        return view(buf, (rows, cols), (ld * it, it), writeable=False)
    groups = -(-rows // grp)
    return view(buf, (groups, grp, cols), (gstride * it, ld * it, it), writeable=False).reshape(groups * grp, cols)[:rows]


def colsum(x, out0, alpha, beta, dt=F64):
    """alpha colsum(x) + beta out0 (beta = 0: out0 is not read); also the summand magnitudes."""
    x, out0 = _as(dt, x, out0)
    s = x.sum(0) if x.shape[0] else np.zeros(x.shape[1], dt)
    prev = dt(beta) * out0 if beta != 0 else np.zeros_like(s)
    return dt(alpha) * s + prev, abs(alpha) * np.abs(x).sum(0) + np.abs(prev)


# ---- losses ------------------------------------------------------------------------------------------------------
def ppo_loss(log_pi, log_pi_old, adv, entropy, clip_eps, coef_ent, dt=F64):
    """oracle.nets.ppo_policy_loss with its gradients: stats = [mean max(l1, l2), mean entropy, clip_frac,
    mean |ratio - 1|], dlog_pi, dentropy, the per-element |summands| of stats 0 / 1 / 3 and the ambiguous gates
    (ratio within AMB of a clip edge, where fp32 may clip or not)."""
    lp, lpo, A, ent = _as(dt, log_pi, log_pi_old, adv, entropy)
    n = lp.size
    ratio = np.exp(lp - lpo)
    lo, hi = dt(1) - dt(clip_eps), dt(1) + dt(clip_eps)
    l1, l2 = -ratio * A, -np.clip(ratio, lo, hi) * A
    _, info = O.ppo_policy_loss(lp, lpo, A, ent, clip_eps=dt(clip_eps), coef_ent=dt(coef_ent))
    stats = np.array([np.maximum(l1, l2).mean(), info["entropy"], info["clip_frac"],
                      2 * info["total_variation_dist"]], dt)
    inside = (ratio >= lo) & (ratio <= hi)
    # d max(l1, l2) / d log_pi: l1 carries -A ratio, the clipped l2 carries it only inside the clip (ties: both do)
    g = np.where(inside | (l1 > l2), -A * ratio, dt(0))
    amb = (np.abs(ratio - lo) <= AMB) | (np.abs(ratio - hi) <= AMB)
    mags = np.stack([np.abs(np.maximum(l1, l2)), np.abs(ent), np.abs(ratio - 1)])
    return dict(stats=stats, dlog_pi=g / dt(n), dentropy=np.full(n, -dt(coef_ent) / dt(n), dt), mags=mags, amb=amb,
                clipped=(l2 > l1))


def l2_loss(pred, target, dt=F64):
    """optax.l2_loss mean: 0.5 mean (pred - target)^2, its gradient, the summands."""
    p, t = _as(dt, pred, target)
    d = p - t
    return (dt(0.5) * d * d).mean(), d / dt(d.size), dt(0.5) * d * d


# ---- TanhNormal --------------------------------------------------------------------------------------------------
def hazard(z):
    """lambda(z) = phi(z) / Phi(z) = d/dz log Phi(z), without cancellation: sqrt(2/pi) / erfcx(-z / sqrt 2)."""
    z = np.asarray(z)
    return z.dtype.type(math.sqrt(2 / math.pi)) / special.erfcx(-z / z.dtype.type(math.sqrt(2)))


def hazard_cancelling_f32(z):
    """The form exp(log phi(z) - log Phi(z)) evaluated in float32 with the tail series for log Phi below -10: both
    terms are about -z^2 / 2, so the subtraction cancels (the negative control's lambda)."""
    z = F32(z)
    z2 = z * z
    s = F32(1) - F32(1) / z2 + F32(3) / (z2 * z2) - F32(15) / (z2 * z2 * z2)
    c = F32(0.91893853320467274)
    log_ndtr = F32(-0.5) * z2 - np.log(-z) - c + np.log(s) if z <= -10 else \
        np.log(F32(0.5) * F32(special.erfc(F64(-z) * math.sqrt(0.5))))
    return np.exp((F32(-0.5) * z * z - c) - log_ndtr, dtype=F32)


def std_raw_for(sd, std_shift, std_min):
    """float32 std_raw whose softplus(std_raw + shift) + std_min is (close to) sd."""
    return (np.log(np.expm1(np.asarray(sd, F64) - std_min)) - std_shift).astype(F32)


def tanh_normal(mean, std_raw, std_shift, std_min, action, entropy_eps=None, n_agents=1, dlog_pi=None,
                dentropy=None, dt=F64):
    """Independent(TanhTransformed(Normal(mean, softplus(std_raw + shift) + std_min))) at the given actions
    (rows, A), as oracle.nets.tanh_normal_log_prob / tanh_normal_entropy, plus the gradients with respect to mean and
    std_raw for the upstream dlog_pi / dentropy (rows).  Returns a dict; `*_mag` are summand magnitudes, `clip` marks
    the elements on a clip branch."""
    mu, sraw, a = _as(dt, mean, std_raw, action)
    rows, A = mu.shape
    sraw = sraw + dt(std_shift)
    sd = _softplus(sraw) + dt(std_min)
    t = dt(THRESH)
    inv_t, log_eps = np.arctanh(t), np.log(dt(1) - t)
    v = np.clip(a, -t, t)
    left, right = v <= -t, v >= t
    x = np.arctanh(np.where(left | right, dt(0), v))
    z = (x - mu) / sd
    w, u = (-inv_t - mu) / sd, (mu - inv_t) / sd
    with np.errstate(all="ignore"):
        # the clipped mass: log Phi of w on the left, of u on the right; its derivative is the hazard lambda
        q = np.where(left, w, np.where(right, u, dt(0)))
        lq, lam = special.log_ndtr(q), hazard(q)
        lp_el = np.where(left | right, lq - log_eps, _normal_logpdf(x, mu, sd) - _tanh_fldj(x))
        lp_mag = np.where(left | right, np.abs(lq) + abs(log_eps),
                          z * z / 2 + np.abs(np.log(sd)) + 1 + np.abs(_tanh_fldj(x)))
        dmu = np.where(left, -lam / sd, np.where(right, lam / sd, z / sd))
        dsd = np.where(left | right, -lam * q / sd, (z * z - 1) / sd)
        # q = (-+atanh(t) - -+mean) / sd is itself a difference that cancels near q = 0: its summands' magnitudes
        dsd_mag = np.where(left | right, lam * (inv_t + np.abs(mu)) / sd / sd, (z * z + 1) / sd)
    out = dict(std=sd, log_pi=lp_el.sum(-1), log_pi_mag=lp_mag.sum(-1), clip=left | right)
    dmu_e = dsd_e = np.zeros_like(mu)
    if entropy_eps is not None:
        eps = np.asarray(entropy_eps).astype(dt).reshape(n_agents, A)[np.arange(rows) % n_agents]
        ys = mu + sd * eps
        ent_el = dt(0.5) + dt(0.5 * math.log(2 * math.pi)) + np.log(sd) + _tanh_fldj(ys)
        out["entropy"] = ent_el.sum(-1)
        out["entropy_mag"] = (2 + np.abs(np.log(sd)) + np.abs(_tanh_fldj(ys))).sum(-1)
        dmu_e = -2 * np.tanh(ys)
        dsd_e = 1 / sd + dmu_e * eps
    glp = np.zeros(rows, dt) if dlog_pi is None else np.asarray(dlog_pi).astype(dt)
    gen = np.zeros(rows, dt) if dentropy is None else np.asarray(dentropy).astype(dt)
    glp, gen = glp[:, None], gen[:, None]
    sg = _sigmoid(sraw)
    out["dmean"] = glp * dmu + gen * dmu_e
    out["dmean_mag"] = np.abs(glp * dmu) + np.abs(gen * dmu_e)
    out["dstd_raw"] = (glp * dsd + gen * dsd_e) * sg
    out["dstd_raw_mag"] = (np.abs(glp) * dsd_mag + np.abs(gen * dsd_e)) * sg
    return out


def tanh_normal_action(mean, std_raw, std_shift, std_min, noise=None, dt=F64):
    """mode(): tanh(mean); sample: tanh(mean + sd noise)."""
    mu, sraw, noise = _as(dt, mean, std_raw, noise)
    sd = _softplus(sraw + dt(std_shift)) + dt(std_min)
    return np.tanh(mu if noise is None else mu + sd * noise)


# ---- GRU / LSTM cells from their gate pre-activations -----------------------------------------------------------------
def gru_cell(gi, gh, bhn, h, dt=F64):
    """flax GRUCell (oracle.nets.gru_cell) from gi = x Wi + bi (rows, 3H: r | z | n) and gh = h Wh (no bias; the n
    gate's hidden bias is bhn): r = s(gi_r + gh_r), z = s(gi_z + gh_z), n = tanh(gi_n + r (gh_n + bhn)),
    h' = (1 - z) n + z h."""
    gi, gh, bhn, h = _as(dt, gi, gh, bhn, h)
    H = h.shape[-1]
    r = _sigmoid(gi[:, :H] + gh[:, :H])
    z = _sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
    n = np.tanh(gi[:, 2 * H:] + r * (gh[:, 2 * H:] + bhn))
    return (1 - z) * n + z * h, (r, z, n)


def gru_cell_bwd(gi, gh, bhn, h, dh_new, dt=F64, mutate=None):
    """(dgi, dgh, dh) of gru_cell for the upstream dh_new; dh is the direct path dh_new z only (the path through gh
    is the caller's GEMM).  mutate="dn_r" writes dn r where dn belongs (a negative control)."""
    gi, gh, bhn, h, g = _as(dt, gi, gh, bhn, h, dh_new)
    H = h.shape[-1]
    _, (r, z, n) = gru_cell(gi, gh, bhn, h, dt)
    hn = gh[:, 2 * H:] + bhn
    dn_pre = g * (1 - z) * (1 - n * n)
    dz_pre = g * (h - n) * z * (1 - z)
    dr_pre = dn_pre * hn * r * (1 - r)
    dgi = np.concatenate([dr_pre, dz_pre, dn_pre * r if mutate == "dn_r" else dn_pre], -1)
    dgh = np.concatenate([dr_pre, dz_pre, dn_pre * r], -1)
    return dgi, dgh, g * z


def lstm_cell(g, c_prev, dt=F64):
    """flax LSTMCell (oracle.nets_t.lstm_cell) from the summed pre-activations g (rows, 4H: i | f | g | o):
    returns (activated gates, c', h'); c_prev None: zeros."""
    g, c_prev = _as(dt, g, c_prev)
    H = g.shape[-1] // 4
    i, f, o = _sigmoid(g[:, :H]), _sigmoid(g[:, H:2 * H]), _sigmoid(g[:, 3 * H:])
    gg = np.tanh(g[:, 2 * H:3 * H])
    c = i * gg if c_prev is None else f * c_prev + i * gg
    return np.concatenate([i, f, gg, o], -1), c, o * np.tanh(c)


def lstm_cell_bwd(act, c_prev, c, dh, dc, dt=F64):
    """(dg pre-activation gradients, dc_prev) from the activated gates, c', dL/dh' and dL/dc' (None: 0)."""
    act, c_prev, c, dh, dc = _as(dt, act, c_prev, c, dh, dc)
    H = c.shape[-1]
    i, f, gg, o = act[:, :H], act[:, H:2 * H], act[:, 2 * H:3 * H], act[:, 3 * H:]
    tc = np.tanh(c)
    dcc = dh * o * (1 - tc * tc) + (0 if dc is None else dc)
    cp = np.zeros_like(c) if c_prev is None else c_prev
    dg = np.concatenate([dcc * gg * i * (1 - i), dcc * cp * f * (1 - f), dcc * i * (1 - gg * gg),
                         dh * tc * o * (1 - o)], -1)
    return dg, dcc * f


# ---- whole-sequence GRU ------------------------------------------------------------------------------------------
def gru_seq(gi, Wh, bhn, h0, dt=F64):
    """gi (S, L, n, 3H) -- sequence s, step t, agent i -- and carries (S n, H): hs (S, L, n, H), hT (S n, H)."""
    gi, Wh, bhn, h0 = _as(dt, gi, Wh, bhn, h0)
    S, L, n, G3 = gi.shape
    H = G3 // 3
    h = np.zeros((S * n, H), dt) if h0 is None else h0
    hs = np.empty((S, L, n, H), dt)
    for t in range(L):
        h, _ = gru_cell(gi[:, t].reshape(S * n, G3), h @ Wh, bhn, h, dt)
        hs[:, t] = h.reshape(S, n, H)
    return hs, h


def gru_seq_bwd(gi, Wh, bhn, h0, hs, dhs, dt=F64):
    """Backward through time for the upstream dhs (S, L, n, H) on every step's output: dgi, dgh (S, L, n, 3H),
    dh0 (S n, H), dbhn (H) = the column sum of dgh's n block, and that sum's summand magnitudes."""
    gi, Wh, bhn, h0, hs, dhs = _as(dt, gi, Wh, bhn, h0, hs, dhs)
    S, L, n, G3 = gi.shape
    H = G3 // 3
    dgi, dgh = np.empty_like(gi), np.empty_like(gi)
    dh = np.zeros((S * n, H), dt)
    for t in range(L - 1, -1, -1):
        hp = hs[:, t - 1].reshape(S * n, H) if t > 0 else (np.zeros((S * n, H), dt) if h0 is None else h0)
        a, b, direct = gru_cell_bwd(gi[:, t].reshape(S * n, G3), hp @ Wh, bhn, hp, dhs[:, t].reshape(S * n, H) + dh, dt)
        dgi[:, t], dgh[:, t] = a.reshape(S, n, G3), b.reshape(S, n, G3)
        dh = direct + b @ Wh.T
    dnr = dgh[..., 2 * H:].reshape(-1, H)
    return dgi, dgh, dh, dnr.sum(0), np.abs(dnr).sum(0)


# ---- agent mean, ReLU backward, clip ----------------------------------------------------------------------------------
def agent_mean(x, dt=F64):
    """(G, n, F) -> (G, F) and the summand magnitudes."""
    x = np.asarray(x).astype(dt)
    return x.mean(1), np.abs(x).mean(1)


def agent_mean_bwd(dy, n, mask=None):
    """float32, bit for bit: dx[g, i] = dy[g] / n, zeroed where the mask (G, n, F) is not > 0 (NaN included)."""
    dy = np.asarray(dy, F32)
    dx = np.repeat((dy / F32(n))[:, None, :], n, 1)
    return dx if mask is None else np.where(np.asarray(mask) > 0, dx, F32(0))


def relu_bwd(dy, y):
    return np.where(np.asarray(y) > 0, np.asarray(dy, F32), F32(0))


def clip_min0(x):
    x = np.asarray(x, F32)
    return np.where(x < 0, F32(0), x)  # jnp.clip(x, a_min=0): -0.0 and NaN pass through


# ---- minibatch gather ----------------------------------------------------------------------------------------------
def gather_env_steps(src, envs, shift=None):
    """src (B, T, ...)[envs]; shift = (e, t): that one row comes from env envs[e] + 1 (a negative control)."""
    out = np.asarray(src)[np.asarray(envs)].copy()
    if shift is not None:
        e, t = shift
        out[e, t] = np.asarray(src)[(envs[e] + 1) % src.shape[0], t]
    return out


# ---- advantages ------------------------------------------------------------------------------------------------------
def _norm_t(x, dt):
    return (x - x.mean(1, keepdims=True)) / (x.std(1, keepdims=True) + dt(1e-8))


def shaped_l(rewards, costs, w, dt=F64):
    r, c = _as(dt, rewards, costs)
    pos = np.maximum(c, dt(0)).sum(-1).sum(-1)
    return -r + dt(w) * pos, np.abs(r) + abs(w) * pos


def informarl_adv(Ql, Vl, n, dt=F64):
    Ql, Vl = _as(dt, Ql, Vl)
    return -np.repeat(_norm_t(Ql - Vl[:, :-1], dt)[:, :, None], n, -1)


def lagr_adv(Ql, Vl, Qh, Vh, lagr, dt=F64):
    Ql, Vl, Qh, Vh, lagr = _as(dt, Ql, Vl, Qh, Vh, lagr)
    Al, Ah = _norm_t(Ql - Vl[:, :-1], dt), _norm_t(Qh - Vh[:, :-1], dt)
    return -Al[:, :, None] - (Ah * lagr).mean(-1), Ah, np.abs(Al)[:, :, None] + np.abs(Ah * lagr).mean(-1)


def lagr_update(lagr, log_pi, log_pi_old, Vh, Ah, gamma, lr, dt=F64):
    """oracle.nets.lagr_update on flat rows: log_pi (rows, n), Vh / Ah (rows, n, nh); also the summand magnitudes."""
    lagr, lp, lpo, Vh, Ah = _as(dt, lagr, log_pi, log_pi_old, Vh, Ah)
    terms = Vh * (dt(1) - dt(gamma)) + np.exp(lp - lpo)[..., None] * Ah
    new = np.maximum(lagr + terms.mean(0) * dt(lr), dt(0))
    return new, np.abs(lagr) + abs(lr) * (np.abs(Vh * (dt(1) - dt(gamma)))
                                          + np.abs(np.exp(lp - lpo)[..., None] * Ah)).mean(0)


def dgppo_adv(Ql, Vl, Vh, dt_env, alpha, cbf_eps, cbf_weight, dt=F64):
    """oracle.nets.merged_cbf_advantages per env: A (B, T, n), the per-env count of safe (t, agent) pairs, the
    ambiguous `safe` gates (CBF derivative within AMB of 0 relative to its terms) and A's summand magnitudes."""
    Ql, Vl, Vh = _as(dt, Ql, Vl, Vh)
    T = Ql.shape[1]
    Al = _norm_t(Ql - Vl[:, :T], dt)
    deriv = (Vh[:, 1:] - Vh[:, :T]) / dt(dt_env) + dt(alpha) * Vh[:, :T]
    mag = np.abs(Vh[:, 1:] - Vh[:, :T]) / dt(dt_env) + np.abs(dt(alpha) * Vh[:, :T])
    safe = (deriv <= 0).all(-1)
    amb = (np.abs(deriv) <= AMB * mag).any(-1)
    acbf = np.maximum(deriv + dt(cbf_eps), dt(0)).max(-1) * dt(cbf_weight)
    A = -(np.where(safe, Al[:, :, None], dt(0)) + acbf)
    A_mag = np.abs(Al)[:, :, None] + (mag.max(-1) + abs(cbf_eps)) * abs(cbf_weight)
    return A, safe.sum((1, 2)).astype(dt), amb, A_mag


# ---- inputs shared by the CPU checks (gate ambiguity caps) and the GPU cases ---------------------------------------
PPO_NS = (1, 255, 131072, 131377)
PPO_CLIP, PPO_COEF = 0.25, 1e-2


def ppo_inputs(n, seed=0):
    """float32 (log_pi, log_pi_old, adv, entropy): element k's ratio is inside (k % 8 in 0, 1), above (2, 3) or below
    (4, 5) the clip with A > 0 on even and A < 0 on odd k; k % 8 == 6: ratio exactly 1; k % 8 == 7: A = 0."""
    rng = np.random.default_rng(1000 + n + seed)
    k = np.arange(n) % 8
    lo = np.select([k < 2, k < 4, k < 6], [0.8, 1.3, 0.3], 1.0)
    hi = np.select([k < 2, k < 4, k < 6], [1.2, 2.0, 0.7], 1.0)
    ratio = rng.uniform(lo, hi)
    old = rng.standard_normal(n).astype(F32)
    new = np.where(k == 6, old, (old + np.log(ratio)).astype(F32)).astype(F32)
    adv = (np.abs(rng.standard_normal(n)) + 0.1) * np.where(k % 2 == 0, 1.0, -1.0)
    adv = np.where(k == 7, 0.0, adv).astype(F32)
    return new, old, adv, rng.standard_normal(n).astype(F32)


ADV_CASES = [(T, n, nh) for T in (1, 2, 257) for n in (1, 5) for nh in (1, 3)]
ADV_B = 3
ADV_DT, ADV_ALPHA, ADV_EPS, ADV_W = 0.03, 1.0, 0.02, 0.1


def adv_inputs(T, n, nh, seed=0):
    """float32 rollout values of ADV_B envs; the last env's Ql - Vl is the constant 0.5 (exact in fp32 for every
    summation order: the std is exactly 0)."""
    rng = np.random.default_rng(2000 + 100 * T + 10 * n + nh + seed)
    B = ADV_B
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    d = dict(Ql=f(B, T), Vl=f(B, T + 1), Qh=f(B, T, n, nh), Vh=f(B, T + 1, n, nh) * F32(0.3),
             lagr=np.abs(f(n, nh)), rewards=f(B, T), costs=f(B, T, n, nh))
    d["Ql"][-1], d["Vl"][-1] = 1.5, 1.0
    return d


Z_GRID = (6.0, 0.0, -3.0, -9.9, -10.0, -10.1, -12.0, -30.0, -100.0, -1000.0, -1e4)
Z_SD = (0.5, 0.5, 0.5, 0.1, 0.1, 0.1, 0.1, 0.05, 0.02, 5e-3, 5e-4)
STD_SHIFT, STD_MIN = math.log(math.exp(0.5) - 1.0), 1e-5  # the actor's std_dev_init 0.5 and std_dev_min


def clip_grid():
    """(mean, std_raw, action), each (2 len(Z_GRID), 1) float32: row 2k sits on the left clip (a = -1) with
    (-atanh(t) - mean) / sd = Z_GRID[k], row 2k + 1 on the right clip (a = 0.999f) with (mean - atanh(t)) / sd =
    Z_GRID[k], up to the float32 rounding of mean and std_raw (the reference recomputes z from the rounded inputs)."""
    z, sd = np.repeat(np.array(Z_GRID), 2), np.repeat(np.array(Z_SD), 2)
    side = np.tile(np.array([-1.0, 1.0]), len(Z_GRID))
    mean = side * (math.atanh(THRESH) + z * sd)
    act = np.where(side < 0, F32(-1.0), F32(0.999))
    return mean.astype(F32)[:, None], std_raw_for(sd, STD_SHIFT, STD_MIN)[:, None], act.astype(F32)[:, None]
