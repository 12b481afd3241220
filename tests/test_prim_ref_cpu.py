"""Checks of tests/prim_ref.py that need no GPU, and of the host side of the primitives' entry points.

1. Every hand-derived backward reference agrees with torch.autograd in float64 on the oracle's forward (oracle/nets_t.py)
   to 1e-10, and phi / Phi with mpmath at 50 digits on the z grid of the TanhNormal clip cases.
2. Negative controls: each comparison class of prim_ref, run on (reference, mutated reference), fails.
3. The GPU cases' seeds keep the float64 reference's ambiguous gates below 0.1 %.
4. Every covered entry point returns DGPPO_EINVAL for each argument its host code rejects (invalid calls only: nothing
   launches), and the workspace-size helpers follow min(512, ceil(rows / 64)).
"""
import ctypes
import math

import numpy as np
import pytest
import torch

import prim_ref as P
from dgppo_fov_amd import _lib
from oracle import nets_t as R

T64 = torch.float64


def _t(a, grad=True):
    return torch.tensor(np.asarray(a, np.float64), dtype=T64, requires_grad=grad)


def _agree(got, want, what, tol=1e-10):
    want = want.detach().numpy() if torch.is_tensor(want) else np.asarray(want)
    err = np.abs(np.asarray(got) - want).max()
    assert err <= tol * (1 + np.abs(want).max()), (what, err)


def _selectors(H, names):
    """Dense kernels that pick block k of a (rows, len(names) H) input: the oracle's cells then see x Wi + bi = gi."""
    eye = np.eye(H)
    out = {}
    for k, name in enumerate(names):
        sel = np.zeros((len(names) * H, H))
        sel[k * H:(k + 1) * H] = eye
        out[name] = dict(kernel=_t(sel, False))
    return out


# ---- 1. references against autograd ---------------------------------------------------------------------------------
def _gru_params(rng, H):
    Wh = rng.standard_normal((H, 3 * H)) / math.sqrt(H)
    bhn = rng.standard_normal(H) * 0.3
    p = _selectors(H, ("ir", "iz", "in"))
    Wh_t, bhn_t = _t(Wh), _t(bhn)
    p["hr"], p["hz"] = dict(kernel=Wh_t[:, :H]), dict(kernel=Wh_t[:, H:2 * H])
    p["hn"] = dict(kernel=Wh_t[:, 2 * H:], bias=bhn_t)
    return Wh, bhn, p, Wh_t, bhn_t


def test_gru_cell_reference_matches_oracle_and_autograd():
    rng = np.random.default_rng(0)
    rows, H = 9, 7
    Wh, bhn, p, Wh_t, bhn_t = _gru_params(rng, H)
    gi, h, dhn = rng.standard_normal((rows, 3 * H)), rng.standard_normal((rows, H)), rng.standard_normal((rows, H))
    gi_t, h_t = _t(gi), _t(h)
    out = R.gru_cell(p, h_t, gi_t)
    hn, _ = P.gru_cell(gi, h @ Wh, bhn, h)
    _agree(hn, out, "h'")
    (out * _t(dhn, False)).sum().backward()
    dgi, dgh, dh = P.gru_cell_bwd(gi, h @ Wh, bhn, h, dhn)
    _agree(dgi, gi_t.grad, "dgi")
    _agree(dh + dgh @ Wh.T, h_t.grad, "dh")
    _agree(h.T @ dgh, Wh_t.grad, "dgh through dWh")  # rows > H and h of full rank: pins dgh
    _agree(dgh[:, 2 * H:].sum(0), bhn_t.grad, "dbhn")


@pytest.mark.parametrize("with_h0", [False, True])
def test_gru_seq_reference_matches_autograd(with_h0):
    rng = np.random.default_rng(1)
    S, L, n, H = 3, 4, 2, 5
    Wh, bhn, p, Wh_t, bhn_t = _gru_params(rng, H)
    gi, dhs = rng.standard_normal((S, L, n, 3 * H)), rng.standard_normal((S, L, n, H))
    h0 = rng.standard_normal((S * n, H)) if with_h0 else None
    gi_t = _t(gi)
    h0_t = _t(h0) if with_h0 else torch.zeros(S * n, H, dtype=T64, requires_grad=True)
    h, outs = h0_t, []
    for t in range(L):
        h = R.gru_cell(p, h, gi_t[:, t].reshape(S * n, 3 * H))
        outs.append(h.reshape(S, n, H))
    hs_t = torch.stack(outs, 1)
    hs, hT = P.gru_seq(gi, Wh, bhn, h0)
    _agree(hs, hs_t, "hs")
    _agree(hT, h, "hT")
    (hs_t * _t(dhs, False)).sum().backward()
    dgi, dgh, dh0, dbhn, _ = P.gru_seq_bwd(gi, Wh, bhn, h0, hs, dhs)
    _agree(dgi, gi_t.grad, "dgi")
    _agree(dh0, h0_t.grad, "dh0")
    _agree(dbhn, bhn_t.grad, "dbhn")
    hprev = np.concatenate([(np.zeros((S, 1, n, H)) if h0 is None else h0.reshape(S, 1, n, H)), hs[:, :-1]], 1)
    _agree(np.einsum("slnh,slng->hg", hprev, dgh), Wh_t.grad, "dgh through dWh")


@pytest.mark.parametrize("null_c,null_dc", [(False, False), (True, True)])
def test_lstm_cell_reference_matches_oracle_and_autograd(null_c, null_dc):
    rng = np.random.default_rng(2)
    rows, H = 6, 5
    p = _selectors(H, ("ii", "if", "ig", "io"))
    for k in ("hi", "hf", "hg", "ho"):
        p[k] = dict(kernel=torch.zeros(H, H, dtype=T64), bias=torch.zeros(H, dtype=T64))
    g, c0 = rng.standard_normal((rows, 4 * H)), rng.standard_normal((rows, H))
    dh, dc = rng.standard_normal((rows, H)), rng.standard_normal((rows, H))
    g_t, c_t = _t(g), _t(np.zeros_like(c0) if null_c else c0)
    c2_t, h2_t = R.lstm_cell(p, c_t, torch.zeros(rows, H, dtype=T64), g_t)
    act, c2, h2 = P.lstm_cell(g, None if null_c else c0)
    _agree(c2, c2_t, "c'")
    _agree(h2, h2_t, "h'")
    ((h2_t * _t(dh, False)).sum() + (0 if null_dc else (c2_t * _t(dc, False)).sum())).backward()
    dg, dcp = P.lstm_cell_bwd(act, None if null_c else c0, c2, dh, None if null_dc else dc)
    _agree(dg, g_t.grad, "dg")
    _agree(dcp, c_t.grad, "dc_prev")


@pytest.mark.parametrize("relu", [0, 1])
def test_layernorm_reference_matches_autograd(relu):
    rng = np.random.default_rng(3)
    rows, F = 11, 13
    x, dy = rng.standard_normal((rows, F)) * 2 + 0.5, rng.standard_normal((rows, F))
    sc, bi = 1 + 0.3 * rng.standard_normal(F), 0.2 * rng.standard_normal(F)
    x_t, sc_t, bi_t = _t(x), _t(sc), _t(bi)
    pre_t = R.layernorm(x_t, dict(scale=sc_t, bias=bi_t))
    y_t = torch.relu(pre_t) if relu else pre_t
    y, pre, mean, rstd = P.layernorm_fwd(x, sc, bi, relu)[:4]
    _agree(y, y_t, "y")
    (y_t * _t(dy, False)).sum().backward()
    dx, ds, db, *_ = P.layernorm_bwd(x, dy, sc, mean, rstd, gate=(y > 0) if relu else None)
    _agree(dx, x_t.grad, "dx")
    _agree(ds, sc_t.grad, "dscale")
    _agree(db, bi_t.grad, "dbias")


def test_tanh_normal_reference_matches_autograd(monkeypatch):
    monkeypatch.setattr(R, "THRESH", P.THRESH)
    rng = np.random.default_rng(4)
    rows, A, n_agents = 12, 3, 3
    mu, sraw = rng.standard_normal((rows, A)), rng.standard_normal((rows, A))
    act = rng.uniform(-0.99, 0.99, (rows, A))
    act[0, 0], act[1, 1], act[2, 2], act[3, 0] = -1.0, 1.0, -P.THRESH, P.THRESH  # clip branches at moderate z
    eps = rng.standard_normal((n_agents, A))
    glp, gen = rng.standard_normal(rows), rng.standard_normal(rows)
    mu_t, sraw_t = _t(mu), _t(sraw)
    sd_t = torch.nn.functional.softplus(sraw_t + P.STD_SHIFT) + P.STD_MIN
    lp_t = R.tanh_normal_log_prob(act, mu_t, sd_t)
    ent_t = R.tanh_normal_entropy(mu_t, sd_t, np.tile(eps, (rows // n_agents, 1)))
    ref = P.tanh_normal(mu, sraw, P.STD_SHIFT, P.STD_MIN, act, eps, n_agents, glp, gen)
    assert ref["clip"].sum() == 4
    _agree(ref["log_pi"], lp_t, "log_pi")
    _agree(ref["entropy"], ent_t, "entropy")
    ((lp_t * _t(glp, False)).sum() + (ent_t * _t(gen, False)).sum()).backward()
    _agree(ref["dmean"], mu_t.grad, "dmean")
    _agree(ref["dstd_raw"], sraw_t.grad, "dstd_raw")


def test_loss_references_match_autograd():
    lp, lpo, adv, ent = (np.asarray(a, np.float64) for a in P.ppo_inputs(255))
    lp_t, ent_t = _t(lp), _t(ent)
    loss_t = R.ppo_loss(lp_t, _t(lpo, False), _t(adv, False), ent_t, clip_eps=P.PPO_CLIP, coef_ent=P.PPO_COEF)
    loss_t.backward()
    ref = P.ppo_loss(lp, lpo, adv, ent, P.PPO_CLIP, P.PPO_COEF)
    _agree(ref["stats"][0] - P.PPO_COEF * ref["stats"][1], loss_t, "loss")
    _agree(ref["dlog_pi"], lp_t.grad, "dlog_pi")
    _agree(ref["dentropy"], ent_t.grad, "dentropy")
    assert ref["clipped"].sum() > 0 and ref["stats"][2] == ref["clipped"].mean()
    p_t = _t(lp)
    (0.5 * (p_t - _t(lpo, False)) ** 2).mean().backward()
    loss, dpred, _ = P.l2_loss(lp, lpo)
    _agree(dpred, p_t.grad, "l2 dpred")
    _agree(loss, 0.5 * ((lp - lpo) ** 2).mean(), "l2 loss")


def test_hazard_matches_mpmath_on_the_z_grid():
    import mpmath as mp

    with mp.workdps(50):
        for z in P.Z_GRID:
            want = mp.npdf(z) / mp.ncdf(z)
            got = P.hazard(np.float64(z))
            assert abs(mp.mpf(float(got)) - want) <= mp.mpf(1e-13) * abs(want), (z, got, want)


def test_advantage_references_match_oracle():
    from oracle import nets as O

    for T, n, nh in P.ADV_CASES:
        d = P.adv_inputs(T, n, nh)
        A, safe_cnt, _, _ = P.dgppo_adv(d["Ql"], d["Vl"], d["Vh"], P.ADV_DT, P.ADV_ALPHA, P.ADV_EPS, P.ADV_W)
        A_o, frac, _ = O.merged_cbf_advantages(d["Ql"], d["Vl"], d["Vh"], n, P.ADV_DT, P.ADV_ALPHA, P.ADV_EPS, P.ADV_W)
        _agree(A, A_o, "dgppo A", 1e-13)
        _agree(safe_cnt.sum() / (P.ADV_B * T * n), frac, "safe fraction", 1e-13)
        assert np.isfinite(A).all()  # the constant row: std exactly 0, no NaN
        _agree(P.informarl_adv(d["Ql"], d["Vl"], n), O.informarl_advantages(d["Ql"], d["Vl"], n), "informarl", 1e-13)
        assert np.all(P.informarl_adv(d["Ql"], d["Vl"], n)[-1] == 0)
        Al, Ah, _ = P.lagr_adv(d["Ql"], d["Vl"], d["Qh"], d["Vh"], d["lagr"])
        Al_o, Ah_o = O.lagr_advantages(d["Ql"], d["Vl"], d["Qh"], d["Vh"], d["lagr"])
        _agree(Al, Al_o, "lagr A", 1e-13)
        _agree(Ah, Ah_o, "lagr Ah", 1e-13)
        _agree(P.shaped_l(d["rewards"], d["costs"], 0.7)[0], O.informarl_shaped_l(d["rewards"], d["costs"], 0.7), "l",
               1e-13)
        lp, lpo = d["Ql"][:, :, None] * np.ones(n), d["Vl"][:, :T, None] * np.ones(n)
        new, _ = P.lagr_update(d["lagr"], lp.reshape(-1, n), lpo.reshape(-1, n), d["Vh"][:, :T].reshape(-1, n, nh),
                               d["Qh"].reshape(-1, n, nh), 0.99, 0.5)
        _agree(new, O.lagr_update(d["lagr"], lp, lpo, d["Vh"][:, :T], d["Qh"], 0.99, 0.5), "lagr update", 1e-13)


# ---- 2. negative controls ----------------------------------------------------------------------------------------
def _fails(fn, *a, **k):
    with pytest.raises(AssertionError):
        fn(*a, **k)


def test_sum_comparisons_catch_dropped_duplicated_and_zeroed_rows():
    rng = np.random.default_rng(5)
    rows, cols, rpb = 32769, 64, 65
    xi = rng.integers(-8, 9, (rows, cols)).astype(np.float64)
    xf = rng.standard_normal((rows, cols))
    for x, check in ((xi, lambda m, r, x: P.check_exact(m.astype(np.float32), r)),
                     (xf, lambda m, r, x: P.check_sums(m.astype(np.float32), r, np.abs(x).sum(0)))):
        ref = x.sum(0)
        assert check(ref, ref, x) <= 1.0
        _fails(check, ref - x[12345], ref, x)  # one row dropped
        _fails(check, ref + x[777], ref, x)  # one row counted twice
        _fails(check, ref - x[(rows - 1) // rpb * rpb:].sum(0), ref, x)  # the last partial block zeroed
    assert np.abs(xi).sum(0).max() < 2 ** 24


def test_close_comparison_catches_gate_order_and_dn_r():
    rng = np.random.default_rng(6)
    rows, H = 5, 7
    gi, gh = rng.standard_normal((rows, 3 * H)), rng.standard_normal((rows, 3 * H))
    bhn, h, dhn = rng.standard_normal(H), rng.standard_normal((rows, H)), rng.standard_normal((rows, H))
    ref, _ = P.gru_cell(gi, gh, bhn, h)
    ref32, _ = P.gru_cell(gi, gh, bhn, h, dt=np.float32)
    assert ref32.dtype == np.float32 and P.check_close(ref32, ref, ref32) <= 1.0
    perm = np.concatenate([np.arange(H, 2 * H), np.arange(H), np.arange(2 * H, 3 * H)])  # z | r | n
    _fails(P.check_close, P.gru_cell(gi[:, perm], gh[:, perm], bhn, h)[0], ref, ref32)
    dgi, _, _ = P.gru_cell_bwd(gi, gh, bhn, h, dhn)
    dgi32, _, _ = P.gru_cell_bwd(gi, gh, bhn, h, dhn, dt=np.float32)
    assert P.check_close(dgi32, dgi, dgi32) <= 1.0
    _fails(P.check_close, P.gru_cell_bwd(gi, gh, bhn, h, dhn, mutate="dn_r")[0], dgi, dgi32)


def test_bits_comparison_catches_a_row_from_the_next_env():
    rng = np.random.default_rng(7)
    src = rng.standard_normal((6, 4, 10)).astype(np.float32)
    envs = np.array([5, 0, 0, 3])
    ref = P.gather_env_steps(src, envs)
    assert P.check_bits(ref.copy(), ref) == 0.0
    _fails(P.check_bits, P.gather_env_steps(src, envs, shift=(2, 1)), ref)
    nan = np.array([np.nan, -0.0], np.float32)
    _fails(P.check_bits, np.array([np.nan, 0.0], np.float32), nan)  # -0.0 against 0.0
    assert P.check_bits(nan.copy(), nan) == 0.0  # NaN payloads compare as bits


def test_clip_comparison_catches_the_cancelling_lambda():
    z = -1000.0
    lam = float(P.hazard(np.float64(z)))
    assert P.check_close(np.float32(lam), lam, scale=abs(lam)) <= 1.0
    bad = P.hazard_cancelling_f32(z)
    assert abs(bad - lam) / lam > 1e-4  # the emulated float32 form loses three digits here
    _fails(P.check_close, bad, lam, scale=abs(lam))
    for zz in (-10.1, -30.0, -1e4):  # the series form lambda = -z / s stays within 1e-6 in float32
        z32 = np.float32(zz)
        z2 = z32 * z32
        s = np.float32(1) - np.float32(1) / z2 + np.float32(3) / (z2 * z2) - np.float32(15) / (z2 * z2 * z2)
        ref = float(P.hazard(np.float64(z32)))
        assert abs(float(-z32 / s) - ref) <= (2e-5 if zz > -12 else 1e-6) * ref, zz


# ---- 3. the GPU cases' gates ---------------------------------------------------------------------------------------
def test_case_seeds_keep_ambiguous_gates_below_the_cap():
    for n in P.PPO_NS:
        ref = P.ppo_loss(*P.ppo_inputs(n), P.PPO_CLIP, P.PPO_COEF)
        assert P.amb_ok(ref["amb"]), n
    for T, n, nh in P.ADV_CASES:
        d = P.adv_inputs(T, n, nh)
        amb = P.dgppo_adv(d["Ql"], d["Vl"], d["Vh"], P.ADV_DT, P.ADV_ALPHA, P.ADV_EPS, P.ADV_W)[2]
        assert P.amb_ok(amb), (T, n, nh)
    mean, sraw, act = P.clip_grid()
    ref = P.tanh_normal(mean, sraw, P.STD_SHIFT, P.STD_MIN, act)
    assert ref["clip"].all()
    sd = ref["std"][:, 0]
    z = np.where(act[:, 0] < 0, -math.atanh(P.THRESH) - mean[:, 0], mean[:, 0] - math.atanh(P.THRESH)) / sd
    assert np.abs(z - np.repeat(P.Z_GRID, 2)).max() <= 2e-3 * (1 + np.abs(z)).max() and (z[6:8] > -10).all() \
        and (z[10:12] < -10).all()  # -9.9 and -10.1 stay on their sides of the kernel's branch at -10


# ---- 4. argument validation and workspace sizes ----------------------------------------------------------------------
_BUF = (ctypes.c_float * 64)()
PTR = ctypes.addressof(_BUF)  # a non-null address; no call below gets as far as reading it

# name -> (valid positional arguments, [(index, rejected value), ...]); the stream argument (last) stays 0
_CALLS = {
    "dgppo_relu_bwd": ([PTR, PTR, 4, 0], [(0, 0), (1, 0), (2, -1)]),
    "dgppo_clip_min0": ([PTR, PTR, 4, 0], [(0, 0), (1, 0), (2, -1)]),
    "dgppo_lstm_cell_fwd": ([4, 8, PTR, PTR, PTR, PTR, 0], [(0, -1), (1, 0), (2, 0), (4, 0), (5, 0)]),
    "dgppo_lstm_cell_bwd": ([4, 8, PTR, PTR, PTR, PTR, PTR, PTR, PTR, 0], [(0, -1), (1, 0), (2, 0), (4, 0), (5, 0), (7, 0)]),
    "dgppo_layernorm_fwd": ([PTR] * 6 + [4, 64, 1, 1e-6, 0], [(i, 0) for i in range(6)] + [(6, -1), (7, 0)]),
    "dgppo_layernorm_bwd": ([PTR] * 9 + [4, 64, 1, PTR, 0],
                            [(i, 0) for i in range(9)] + [(9, -1), (10, 0), (12, 0)]),
    "dgppo_colsum": ([PTR, 4, 8, 8, 0, 0, PTR, 1.0, 0.0, PTR, 0], [(0, 0), (1, -1), (2, 0), (6, 0), (9, 0)]),
    "dgppo_gru_fwd": ([PTR] * 5 + [4, 8, 0], [(i, 0) for i in range(5)] + [(5, -1), (6, 0)]),
    "dgppo_gru_bwd": ([PTR] * 8 + [4, 8, 0], [(i, 0) for i in range(8)] + [(8, -1), (9, 0)]),
    "dgppo_agent_mean_fwd": ([PTR, PTR, 4, 2, 8, 16, 0], [(0, 0), (1, 0), (2, -1), (3, 0), (4, 0)]),
    "dgppo_agent_mean_bwd": ([PTR, PTR, 4, 2, 8, 16, 0], [(0, 0), (1, 0), (2, -1), (3, 0), (4, 0)]),
    "dgppo_agent_mean_bwd_masked": ([PTR, PTR, PTR, 4, 2, 8, 16, 0], [(0, 0), (2, 0), (3, -1), (4, 0), (5, 0)]),
    "dgppo_ppo_loss": ([PTR] * 4 + [4, 0.25, 0.01] + [PTR] * 4 + [0],
                       [(i, 0) for i in (0, 1, 2, 3, 7, 8, 9, 10)] + [(4, 0), (4, -3)]),
    "dgppo_l2_loss": ([PTR, PTR, 4, PTR, PTR, PTR, 0], [(0, 0), (1, 0), (2, 0), (3, 0), (4, 0), (5, 0)]),
    "dgppo_cost_shaped_loss": ([PTR, PTR, 0.5, PTR, 2, 3, 2, 1, 0],
                               [(0, 0), (1, 0), (3, 0), (4, -1), (5, 0), (6, 0), (7, 0)]),
    "dgppo_informarl_advantages": ([PTR, PTR, PTR, 2, 3, 2, 0], [(0, 0), (1, 0), (2, 0), (3, -1), (4, 0), (5, 0)]),
    "dgppo_lagr_advantages": ([PTR] * 7 + [2, 3, 2, 1, 0], [(i, 0) for i in range(7)] + [(7, -1), (8, 0), (9, 0), (10, 0)]),
    "dgppo_lagr_update": ([PTR] * 6 + [4, 2, 1, 0.99, 0.1, 0], [(i, 0) for i in range(5)] + [(6, 0), (7, 0), (8, 0)]),
}


@pytest.mark.parametrize("name", sorted(_CALLS))
def test_entry_points_reject_invalid_arguments(name):
    fn = getattr(_lib.load(), name)
    valid, rejected = _CALLS[name]
    assert len(valid) == len(fn.argtypes)
    for idx, bad in rejected:
        args = list(valid)
        args[idx] = bad
        assert fn(*args) == _lib.DGPPO_EINVAL, (name, idx, bad)


def _struct_rejects(fn, make, rejected):
    assert fn(None, None) == _lib.DGPPO_EINVAL
    for field, bad in rejected:
        a = make()
        for f, v in zip(field, bad) if isinstance(field, tuple) else ((field, bad),):
            setattr(a, f, v)
        assert fn(ctypes.byref(a), None) == _lib.DGPPO_EINVAL, (field, bad)


def test_struct_entry_points_reject_invalid_arguments():
    lib = _lib.load()

    def tn():
        a = _lib.TanhNormalArgs()
        a.rows, a.A, a.mode, a.n_agents = 4, 2, 2, 1
        a.mean = a.std_raw = a.action = a.noise = a.dmean = a.dstd_raw = a.entropy_eps = PTR
        return a
    _struct_rejects(lib.dgppo_tanh_normal, tn,
                    [("rows", -1), ("A", 0), ("mean", 0), ("std_raw", 0), ("mode", -1), ("mode", 3), ("action", 0),
                     (("mode", "noise"), (1, 0)), ("dstd_raw", 0), ("n_agents", 0)])

    def gae():
        a = _lib.GaeArgs()
        a.B, a.T, a.n_agents, a.n_h = 2, 8, 2, 1
        a.hs = a.l = a.Vh = a.Vl = a.Qh = a.Ql = PTR
        a.gamma = 0.99
        setattr(a, "lambda", 0.95)
        return a
    _struct_rejects(lib.dgppo_gae, gae,
                    [("B", -1), ("T", 0), ("T", 1025), ("n_agents", 0), ("n_h", 0), ("hs", 0), ("l", 0), ("Vh", 0),
                     ("Vl", 0), ("Qh", 0), ("Ql", 0), (("n_agents", "n_h"), (64, 4)),  # K = 256
                     (("T", "n_agents", "n_h"), (1024, 20, 1))])  # 180 KB of LDS staging > 160 KB

    def adv():
        a = _lib.AdvArgs()
        a.B, a.T, a.n_agents, a.n_h = 2, 8, 2, 1
        a.Ql = a.Vl = a.Vh = a.A = a.safe_count = PTR
        return a
    _struct_rejects(lib.dgppo_dgppo_advantages, adv,
                    [("B", -1), ("T", 0), ("n_agents", 0), ("n_h", 0), ("Ql", 0), ("Vl", 0), ("Vh", 0), ("A", 0),
                     ("safe_count", 0)])

    def seq():
        a = _lib.GruSeqArgs()
        a.Q, a.L, a.n_agents, a.H = 6, 2, 3, 64
        a.gi = a.Wh = a.bhn = a.hs = a.dhs = a.dgi = a.dgh = PTR
        return a
    common = [("Q", -1), ("L", 0), ("n_agents", 0), ("H", 32), ("gi", 0), ("Wh", 0), ("bhn", 0), ("hs", 0), ("Q", 7)]
    _struct_rejects(lib.dgppo_gru_seq_fwd, seq, common)
    _struct_rejects(lib.dgppo_gru_seq_bwd, seq, common + [("dhs", 0), ("dgi", 0), ("dgh", 0)])
    assert lib.dgppo_gru_set_form(2) == _lib.DGPPO_EINVAL


def test_gather_env_steps_rejects_invalid_arguments():
    fn = _lib.load().dgppo_gather_env_steps
    F = (_lib.GatherField * 9)()
    for f in F:
        f.src, f.dst, f.row_elems, f.src_tstride, f.src_estride = PTR, PTR, 4, 4, 16
    for args in ((F, 0, PTR, 2, 3), (F, 9, PTR, 2, 3), (None, 1, PTR, 2, 3), (F, 1, None, 2, 3), (F, 1, PTR, -1, 3),
                 (F, 1, PTR, 2, 0)):
        assert fn(*args, None) == _lib.DGPPO_EINVAL, args[1:]
    for field, bad in (("src", 0), ("dst", 0), ("row_elems", 0)):
        G = (_lib.GatherField * 2)()
        for f in G:
            f.src, f.dst, f.row_elems = PTR, PTR, 4
        setattr(G[1], field, bad)
        assert fn(G, 2, PTR, 2, 3, None) == _lib.DGPPO_EINVAL, field


def test_workspace_sizes():
    lib = _lib.load()
    for rows in (1, 63, 64, 65, 2048, 2049, 32768, 32769, 65555, 10 ** 6):
        nb = min(512, -(-rows // 64))
        for w in (1, 64, 257):
            assert lib.dgppo_colsum_workspace_floats(rows, w) == nb * w
            assert lib.dgppo_layernorm_bwd_workspace_floats(rows, w) == nb * 2 * w
    assert lib.dgppo_loss_workspace_floats() == 512 * 8
