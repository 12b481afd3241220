"""Every csrc/nn.hip / csrc/gru.hip primitive of the update path, called directly at its launch edges (second passes of
the grid-stride and persistent loops, partial and empty row blocks, every host path) and compared with the float64
restatements of tests/prim_ref.py under its four comparison classes (bits, exact sums, random-float sums, the
project's rule 1e-5 scale + 8 |ref32 - ref64|).

Conventions of every case: outputs start as NaN, accumulating outputs from random non-zero values; every buffer has
64 guard floats on both sides that must come back unchanged; no NaN may remain inside an output's extent; one
torch.cuda.synchronize() per case; the case prints its wall time and its worst error relative to its bound.

Summation depths d of the random-float reductions (the bound is d 2^-24 sum|x| <= 1e-5 sum|x| for d <= 160):
  colsum, rows <= 2048       128 sequential + 16 (LDS) + 1 (beta)                                   = 145
  colsum, rows = 32,769      65 per thread (cols > 256; fewer below) + 32 + 16 + 1                     = 114
  LayerNorm dscale / dbias   9 per lane (F = 64, 65,555 rows) or 33 per wave (generic) + 16 + 32 + 16 + 1  <= 98
  ppo / l2 stats             2 per thread + 6 (wave) + 3 (block) + 8 + 6 (partials)                 = 25
  GRU dbhn partials          2 blocks x 3 steps x 4 rows per lane + 3 (LDS), then summed in float64     = 27
  agent mean                 n - 1
dgppo_lagr_update sums 70,001 rows with 274 sequential adds per thread (d = 282): it is compared under the project's
rule with the summand scale, not as a random-float reduction.
"""
import time

import numpy as np
import pytest
import torch

import prim_ref as P
from dgppo_fov_amd import _lib
from dgppo_fov_amd.nn import kernels as K

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
GUARD, SENT = 64, 7777.0  # 64 floats keep the payload's 16-byte alignment


class Case:
    def __init__(self, dev, name):
        self.dev, self.name, self.bufs, self.worst, self.t0 = dev, name, [], 0.0, time.perf_counter()

    def _alloc(self, n, off):
        full = torch.full((GUARD + off + n + GUARD,), SENT, dtype=torch.float32, device=self.dev)
        self.bufs.append((full, GUARD + off, n))
        return full[GUARD + off:GUARD + off + n]

    def inp(self, arr, off=0):
        """A guarded device copy of a 4-byte array (off: floats of misalignment)."""
        arr = np.ascontiguousarray(arr)
        v = self._alloc(arr.size, off)
        if arr.size:
            v.copy_(torch.from_numpy(arr.reshape(-1).view(F32)))
        return (v.view(torch.int32) if arr.dtype == np.int32 else v).view(arr.shape)

    def out(self, shape, init=None, off=0, dtype=torch.float32):
        """A guarded output: NaN everywhere, or `init` for an accumulating one."""
        shape = tuple(int(s) for s in np.atleast_1d(shape))
        v = self._alloc(int(np.prod(shape)), off)
        if init is None:
            v.fill_(float("nan"))
        else:
            v.copy_(torch.from_numpy(np.ascontiguousarray(init, F32).reshape(-1)))
        return (v.view(torch.int32) if dtype == torch.int32 else v).view(shape)

    def sync(self):
        torch.cuda.synchronize()
        for full, lo, n in self.bufs:
            assert bool((full[:lo] == SENT).all()) and bool((full[lo + n:] == SENT).all()), f"{self.name}: guard overwritten"

    def get(self, t, nan_ok=False):
        a = t.cpu().numpy()
        assert nan_ok or not np.isnan(a.view(F32)).any(), f"{self.name}: NaN left in an output"
        return a

    def add(self, ratio):
        self.worst = max(self.worst, ratio)

    def done(self):
        print(f"[prim] {self.name}: {time.perf_counter() - self.t0:.2f} s, worst error / bound {self.worst:.3g}")


# ---- LayerNorm -----------------------------------------------------------------------------------------------------
LN_FWD = [(r, 64, 0) for r in (1, 15, 17, 65555)] + [(r, F, 0) for F in (1, 63, 65, 192) for r in (1, 5, 4099)] + \
    [(r, 64, 1) for r in (1, 5, 4099)]
LN_BWD = LN_FWD[:4] + [(2049, 64, 0), (32769, 64, 0)] + LN_FWD[4:]


def _ln_inputs(rows, F, seed=0):
    rng = np.random.default_rng(3000 + rows + 7 * F + seed)
    x = (rng.standard_normal((rows, F)) * 2 + 0.5).astype(F32)
    x[min(rows - 1, 3)] = 0.5  # a zero-variance row (mean and E[x^2] exact in fp32)
    sc = (1 + 0.3 * rng.standard_normal(F)).astype(F32)
    bi = (0.2 * rng.standard_normal(F)).astype(F32)
    return rng, x, sc, bi


@pytest.mark.parametrize("rows,F,off", LN_FWD)
def test_layernorm_fwd(cuda, rows, F, off):
    c = Case(cuda, f"layernorm_fwd rows={rows} F={F} off={off}")
    _, x, sc, bi = _ln_inputs(rows, F)
    xd, scd, bid = c.inp(x, off), c.inp(sc), c.inp(bi)
    outs = []
    for relu in (0, 1):
        y, mean, rstd = c.out((rows, F), off=off), c.out(rows), c.out(rows)
        K.layernorm_fwd(xd, scd, bid, y, mean, rstd, relu=bool(relu))
        outs.append((y, mean, rstd))
    c.sync()
    for relu, got in zip((0, 1), outs):
        r64, r32 = P.layernorm_fwd(x, sc, bi, relu), P.layernorm_fwd(x, sc, bi, relu, dt=F32)
        for g, k, scale, what in zip(got, (0, 2, 3), (r64[4], None, r64[5]), ("y", "mean", "rstd")):
            c.add(P.check_close(c.get(g), r64[k], r32[k], scale=scale, what=f"{what} relu={relu}"))
        if F >= 63:  # the constant row is exact in fp32: mean 0.5, variance 0, y = bias
            k = min(rows - 1, 3)
            assert c.get(got[1])[k] == 0.5
            P.check_bits(c.get(got[0])[k], np.maximum(bi, 0) if relu else bi, "y of the constant row")
    c.done()


@pytest.mark.parametrize("rows,F,off", LN_BWD)
def test_layernorm_bwd(cuda, rows, F, off):
    c = Case(cuda, f"layernorm_bwd rows={rows} F={F} off={off}")
    rng, x, sc, bi = _ln_inputs(rows, F)
    dy = rng.standard_normal((rows, F)).astype(F32)
    ds0, db0 = rng.standard_normal(F).astype(F32), rng.standard_normal(F).astype(F32)
    y64, _, mean64, rstd64 = P.layernorm_fwd(x, sc, bi, 1)[:4]
    y, mean, rstd = y64.astype(F32), mean64.astype(F32), rstd64.astype(F32)  # the backward's inputs, fp32 values
    xd, yd, dyd, scd, md, rd = c.inp(x, off), c.inp(y, off), c.inp(dy, off), c.inp(sc), c.inp(mean), c.inp(rstd)
    outs = []
    for relu in (0, 1):
        dx, ds, db = c.out((rows, F), off=off), c.out(F, ds0), c.out(F, db0)
        K.layernorm_bwd(xd, yd, dyd, scd, md, rd, dx, ds, db, relu=bool(relu))
        outs.append((dx, ds, db))
    c.sync()
    for relu, (dx, ds, db) in zip((0, 1), outs):
        gate = (y > 0) if relu else None  # y is an input: its gate is not ambiguous
        r64 = P.layernorm_bwd(x, dy, sc, mean, rstd, gate)
        r32 = P.layernorm_bwd(x, dy, sc, mean, rstd, gate, dt=F32)
        c.add(P.check_close(c.get(dx), r64[0], r32[0], scale=1 + r64[5], what=f"dx relu={relu}"))
        c.add(P.check_sums(c.get(ds), ds0 + r64[1], np.abs(ds0) + r64[3], what=f"dscale relu={relu}"))
        c.add(P.check_sums(c.get(db), db0 + r64[2], np.abs(db0) + r64[4], what=f"dbias relu={relu}"))
    c.done()


@pytest.mark.parametrize("rows,F,off", [(32769, 64, 0), (65555, 64, 0), (4099, 65, 0), (4099, 64, 1)])
def test_layernorm_bwd_exact_sums(cuda, rows, F, off):
    """Integer dy and x in [-8, 8] with mean = 0, rstd = 1 passed in: xh = x, every product and partial sum is an
    integer below 2^24 (65,555 x 64), so dscale / dbias must be exact in any summation order."""
    c = Case(cuda, f"layernorm_bwd exact rows={rows} F={F} off={off}")
    rng = np.random.default_rng(rows + F)
    x = rng.integers(-8, 9, (rows, F)).astype(F32)
    dy = rng.integers(-8, 9, (rows, F)).astype(F32)
    y = rng.integers(-2, 3, (rows, F)).astype(F32)  # the ReLU gate
    ds0, db0 = rng.integers(-8, 9, F).astype(F32), rng.integers(-8, 9, F).astype(F32)
    sc = np.ones(F, F32)
    dx, ds, db = c.out((rows, F), off=off), c.out(F, ds0), c.out(F, db0)
    K.layernorm_bwd(c.inp(x, off), c.inp(y, off), c.inp(dy, off), c.inp(sc), c.inp(np.zeros(rows, F32)),
                    c.inp(np.ones(rows, F32)), dx, ds, db, relu=True)
    c.sync()
    g = np.where(y > 0, dy, 0).astype(F64)
    P.check_exact(c.get(ds), ds0 + (g * x).sum(0), "dscale")
    P.check_exact(c.get(db), db0 + g.sum(0), "dbias")
    c.get(dx)
    c.done()


# ---- colsum --------------------------------------------------------------------------------------------------------
COLS = (1, 17, 64, 99, 256, 257, 300)
AB = ((1.0, 0.0), (0.5, 1.0), (1.0, -2.0))


@pytest.mark.parametrize("rows", [0, 1, 16, 17, 2048, 2049, 32769, 1024])
def test_colsum(cuda, rows):
    """Every host path (direct pass up to 2048 rows without groups, partials above or with groups, rows = 0), cols on
    both sides of 256, ld > cols, grp = 3 with gstride = 5 ld, the three (alpha, beta); random floats (sums class) and
    integers in [-8, 8] (exact class; 1024 x 64 is the shape of the GRU's dbhn partials)."""
    c = Case(cuda, f"colsum rows={rows}")
    rng = np.random.default_rng(rows)
    runs, k = [], 0
    for cols in (64,) if rows == 1024 else (17, 64, 257) if rows > 4096 else COLS:  # 32,769 rows: three widths
        for lay in range(3):
            if lay == 2 and rows > 4096 and cols > 64:
                continue  # the grouped layout of 32,769 x 257 would need 57 MB
            ld = cols if lay == 0 else cols + 3
            grp, gs = (3, 5 * ld) if lay == 2 else (0, 0)
            size = ((rows + 2) // 3) * gs + 3 * ld if grp else rows * ld + 3
            for ints in (False, True):
                alpha, beta = AB[k % 3]
                k += 1
                buf = (rng.integers(-8, 9, size) if ints else rng.standard_normal(size)).astype(F32)
                out0 = (rng.integers(-8, 9, cols) if ints else rng.standard_normal(cols)).astype(F32)
                out = c.out(cols, None if beta == 0 else out0)  # beta = 0 must not read the NaN-filled out
                K.colsum(c.inp(buf), rows, cols, out, ld=ld, grp=grp, gs=gs, alpha=alpha, beta=beta)
                runs.append((buf, out0, out, cols, ld, grp, gs, alpha, beta, ints))
    c.sync()
    for buf, out0, out, cols, ld, grp, gs, alpha, beta, ints in runs:
        ref, mag = P.colsum(P.colsum_rows(buf, rows, cols, ld, grp, gs), out0, alpha, beta)
        what = f"cols={cols} ld={ld} grp={grp} alpha={alpha} beta={beta}"
        if ints:
            c.add(P.check_exact(c.get(out), ref, what))
        else:
            c.add(P.check_sums(c.get(out), ref, mag, what=what))
    c.done()


# ---- losses --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", P.PPO_NS)
def test_ppo_loss(cuda, n):
    c = Case(cuda, f"ppo_loss n={n}")
    lp, lpo, adv, ent = P.ppo_inputs(n)
    dlp, den, stats = c.out(n), c.out(n), c.out(4)
    K.ppo_loss(c.inp(lp), c.inp(lpo), c.inp(adv), c.inp(ent), P.PPO_CLIP, P.PPO_COEF, dlp, den, stats)
    c.sync()
    r64 = P.ppo_loss(lp, lpo, adv, ent, P.PPO_CLIP, P.PPO_COEF)
    r32 = P.ppo_loss(lp, lpo, adv, ent, P.PPO_CLIP, P.PPO_COEF, dt=F32)
    amb = r64["amb"]
    assert P.amb_ok(amb)
    c.add(P.check_close(c.get(dlp) * n, r64["dlog_pi"] * n, r32["dlog_pi"].astype(F64) * n, keep=~amb, what="dlog_pi"))
    c.add(P.check_close(c.get(den) * n, r64["dentropy"] * n, r32["dentropy"].astype(F64) * n, what="dentropy"))
    st = c.get(stats)
    slack = (np.abs(adv.astype(F64)) * P.PPO_CLIP * amb).sum() / n  # an ambiguous clip moves max(l1, l2) by < |A| eps
    for q, k in ((0, 0), (1, 1), (3, 2)):
        c.add(P.check_sums(st[q], r64["stats"][q], r64["mags"][k].sum() / n, slack if q == 0 else 0.0, f"stats[{q}]"))
    count = float(r64["clipped"].sum())
    if amb.any():
        assert abs(st[2] * n - count) <= amb.sum() + 1e-5 * count
    else:  # the count is an integer below 2^24: exact, then one fp32 product with 1 / n
        assert st[2] == F32(count) * (F32(1) / F32(n)), (st[2], count)
    c.done()


@pytest.mark.parametrize("n", P.PPO_NS)
def test_l2_loss(cuda, n):
    c = Case(cuda, f"l2_loss n={n}")
    rng = np.random.default_rng(n)
    pred, tgt = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    dpred, loss = c.out(n), c.out(1)
    K.l2_loss(c.inp(pred), c.inp(tgt), dpred, loss)
    c.sync()
    l64, d64, terms = P.l2_loss(pred, tgt)
    _, d32, _ = P.l2_loss(pred, tgt, dt=F32)
    c.add(P.check_close(c.get(dpred) * n, d64 * n, d32.astype(F64) * n, what="dpred"))
    c.add(P.check_sums(c.get(loss)[0], l64, terms.sum() / n, what="loss"))
    c.done()


# ---- TanhNormal ----------------------------------------------------------------------------------------------------
def _tn_args(c, rows, A, mode, n_agents, mean, sraw, noise=None, action=None, eps=None, glp=None, gen=None,
             skip=()):
    a = _lib.TanhNormalArgs()
    a.rows, a.A, a.mode, a.n_agents = rows, A, mode, n_agents
    a.std_shift, a.std_min = P.STD_SHIFT, P.STD_MIN
    outs, keep = {}, [c.inp(mean), c.inp(sraw)]
    a.mean, a.std_raw = K._p(keep[0]), K._p(keep[1])
    for name, arr in (("noise", noise), ("action", action), ("entropy_eps", eps), ("dlog_pi", glp), ("dentropy", gen)):
        if arr is not None and name not in skip:
            keep.append(c.inp(arr))
            setattr(a, name, K._p(keep[-1]))
    for name, shape in (("action_out", (rows, A)), ("std_out", (rows, A)), ("log_pi", rows), ("entropy", rows),
                        ("dmean", (rows, A)), ("dstd_raw", (rows, A))):
        if name not in skip and not (name == "action_out" and mode == 2):
            outs[name] = c.out(shape)
            setattr(a, name, K._p(outs[name]))
    return a, outs, keep


def _tn_inputs(rows, A, n_agents, seed=0):
    rng = np.random.default_rng(4000 + rows + A + seed)
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    return dict(mean=f(rows, A), sraw=f(rows, A), noise=f(rows, A), eps=f(n_agents, A), glp=f(rows), gen=f(rows),
                action=rng.uniform(-0.9, 0.9, (rows, A)).astype(F32))


def _tn_check(c, d, outs, mode, n_agents, skip=()):
    got = {k: c.get(v) for k, v in outs.items()}
    if mode <= 1 and "action_out" in got:
        noise = d["noise"] if mode == 1 else None
        c.add(P.check_close(got["action_out"], P.tanh_normal_action(d["mean"], d["sraw"], P.STD_SHIFT, P.STD_MIN, noise),
                            P.tanh_normal_action(d["mean"], d["sraw"], P.STD_SHIFT, P.STD_MIN, noise, dt=F32),
                            what="action"))
        action = got["action_out"]  # log_pi is the density of the kernel's own fp32 action
    elif mode <= 1:
        return  # without action_out the evaluated action is not observable: only NaN / guards were checked
    else:
        action = d["action"]
    eps = None if "entropy_eps" in skip else d["eps"]
    kw = dict(entropy_eps=eps, n_agents=n_agents, dlog_pi=None if "dlog_pi" in skip else d["glp"],
              dentropy=None if "dentropy" in skip else d["gen"])
    r64 = P.tanh_normal(d["mean"], d["sraw"], P.STD_SHIFT, P.STD_MIN, action, **kw)
    r32 = P.tanh_normal(d["mean"], d["sraw"], P.STD_SHIFT, P.STD_MIN, action, dt=F32, **kw)
    for k, rk in (("std_out", "std"), ("log_pi", "log_pi"), ("entropy", "entropy"), ("dmean", "dmean"),
                  ("dstd_raw", "dstd_raw")):
        if k in got:
            if k == "entropy" and eps is None:
                assert (got[k] == 0).all()  # no fixed draw: the entropy output is 0
                continue
            scale = 1 + r64[rk + "_mag"] if rk + "_mag" in r64 else None
            c.add(P.check_close(got[k], r64[rk], r32[rk], scale=scale, what=k))


@pytest.mark.parametrize("mode,A,rows,n_agents", [(2, 3, 257, 3), (2, 1, 2097229, 1), (0, 3, 257, 1), (1, 3, 257, 3),
                                                  (1, 1, 1, 1), (2, 3, 1, 1), (0, 1, 257, 3)])
def test_tanh_normal(cuda, mode, A, rows, n_agents):
    c = Case(cuda, f"tanh_normal mode={mode} A={A} rows={rows} n_agents={n_agents}")
    d = _tn_inputs(rows, A, n_agents)
    a, outs, keep = _tn_args(c, rows, A, mode, n_agents, d["mean"], d["sraw"], d["noise"], d["action"], d["eps"],
                             d["glp"], d["gen"])
    K.tanh_normal(a, cuda)
    c.sync()
    _tn_check(c, d, outs, mode, n_agents)
    c.done()


@pytest.mark.parametrize("skip", ["action_out", "std_out", "log_pi", "entropy", "entropy_eps", "dlog_pi", "dentropy",
                                  "dmean"])
def test_tanh_normal_optional_pointers(cuda, skip):
    """Each optional pointer null in turn (dmean null: no backward, dstd_raw stays untouched).  A null output pointer
    changes no other output, a null input only those that read it: they are bit-identical to the full call's."""
    mode, A, rows, n_agents = (2 if skip == "dmean" else 1), 3, 257, 3
    c = Case(cuda, f"tanh_normal without {skip}")
    d = _tn_inputs(rows, A, n_agents, seed=1)
    ins = (d["mean"], d["sraw"], d["noise"], d["action"], d["eps"], d["glp"], d["gen"])
    a, outs, keep = _tn_args(c, rows, A, mode, n_agents, *ins, skip=(skip,))
    K.tanh_normal(a, cuda)
    a_full, full, keep_full = _tn_args(c, rows, A, mode, n_agents, *ins)
    K.tanh_normal(a_full, cuda)
    c.sync()
    if skip == "dmean":
        assert torch.isnan(outs.pop("dstd_raw")).all()
    same = {"entropy_eps": ("action_out", "std_out", "log_pi"), "dlog_pi": ("action_out", "std_out", "log_pi", "entropy"),
            "dentropy": ("action_out", "std_out", "log_pi", "entropy")}.get(skip, tuple(outs))
    for k in same:
        if k in outs:
            P.check_bits(c.get(outs[k]), c.get(full[k]), f"{k} with {skip} null")
    _tn_check(c, d, outs, mode, n_agents, skip=(skip,))
    c.done()


def test_tanh_normal_clip_branches(cuda):
    """Stored actions on both clips with z = (-+atanh(t) - mean) / sd on P.Z_GRID (std_min = 1e-5 makes large |z|
    reachable): log_pi, dmean and dstd_raw within 1e-5 of their summand scale, without a float32 floor.

    dstd_raw = -lambda q / sd is scaled by lambda (atanh(t) + |mean|) / sd^2: q is itself a difference that cancels
    near q = 0.

    Measured on an MI355X, relative error of dmean (both sides alike).  With lambda = exp(log phi - log Phi) in the
    tail (before): z = -30: 2.3e-5, -100: 2.9e-4, -1000: 1.5e-3, -1e4: 0.70.  With the tail series -z / s: at most
    1.1e-6 for z <= -10; the grid's maximum is 4.3e-6 at z = -9.9 (the erfc branch, unchanged)."""
    c = Case(cuda, "tanh_normal clip grid")
    mean, sraw, act = P.clip_grid()
    rows = mean.shape[0]
    glp = np.ones(rows, F32)
    a, outs, keep = _tn_args(c, rows, 1, 2, 1, mean, sraw, action=act, glp=glp, skip=("entropy",))
    K.tanh_normal(a, cuda)
    c.sync()
    r = P.tanh_normal(mean, sraw, P.STD_SHIFT, P.STD_MIN, act, dlog_pi=glp)
    got = {k: c.get(outs[k]) for k in ("log_pi", "dmean", "dstd_raw")}
    rel = {k: np.abs(got[k].reshape(rows) - r[k].reshape(rows)) / r[k + "_mag"].reshape(rows) for k in got}
    for i, z in enumerate(np.repeat(P.Z_GRID, 2)):
        print(f"[prim] clip z={z:g} side={'LR'[i % 2]}: rel err log_pi {rel['log_pi'][i]:.2e} "
              f"dmean {rel['dmean'][i]:.2e} dstd_raw {rel['dstd_raw'][i]:.2e}")
    print("[prim] clip grid max rel err: " + ", ".join(f"{k} {v.max():.2e}" for k, v in rel.items()))
    for k in got:
        c.add(P.check_close(got[k].reshape(rows), r[k].reshape(rows), scale=r[k + "_mag"].reshape(rows), what=k))
    c.done()


# ---- GRU / LSTM cells ----------------------------------------------------------------------------------------------
CELL_SHAPES = [(r, H) for r in (1, 5, 32781) for H in (1, 7, 64)]


@pytest.mark.parametrize("rows,H", CELL_SHAPES)
def test_gru_cell(cuda, rows, H):
    c = Case(cuda, f"gru_fwd/bwd rows={rows} H={H}")
    rng = np.random.default_rng(rows + H)
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    gi, gh, bhn, h, dhn, dh0 = f(rows, 3 * H), f(rows, 3 * H), f(H), f(rows, H), f(rows, H), f(rows, H)
    gid, ghd, bd, hd = c.inp(gi), c.inp(gh), c.inp(bhn), c.inp(h)
    hn, dgi, dgh, dh = c.out((rows, H)), c.out((rows, 3 * H)), c.out((rows, 3 * H)), c.out((rows, H), dh0)
    K.gru_fwd(gid, ghd, bd, hd, hn)
    K.gru_bwd(gid, ghd, bd, hd, c.inp(dhn), dgi, dgh, dh)
    c.sync()
    c.add(P.check_close(c.get(hn), P.gru_cell(gi, gh, bhn, h)[0], P.gru_cell(gi, gh, bhn, h, dt=F32)[0], what="h'"))
    r64, r32 = P.gru_cell_bwd(gi, gh, bhn, h, dhn), P.gru_cell_bwd(gi, gh, bhn, h, dhn, dt=F32)
    c.add(P.check_close(c.get(dgi), r64[0], r32[0], what="dgi"))
    c.add(P.check_close(c.get(dgh), r64[1], r32[1], what="dgh"))
    c.add(P.check_close(c.get(dh), dh0 + r64[2], dh0 + r32[2], scale=1 + np.abs(dh0) + np.abs(r64[2]), what="dh"))
    c.done()


@pytest.mark.parametrize("rows,H", CELL_SHAPES)
def test_lstm_cell(cuda, rows, H):
    c = Case(cuda, f"lstm_cell rows={rows} H={H}")
    rng = np.random.default_rng(rows + 3 * H)
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    g, c0, dh, dc = f(rows, 4 * H), f(rows, H), f(rows, H), f(rows, H)
    variants = [(True, True, True)] if rows > 1000 else [(True, True, True), (False, True, True), (True, False, True),
                                                         (True, True, False), (False, False, False)]
    runs = []
    for has_c, has_dc, has_dcp in variants:
        gd = c.inp(g)  # activated in place
        c0d = c.inp(c0) if has_c else None
        c2, h2 = c.out((rows, H)), c.out((rows, H))
        K.lstm_cell_fwd(rows, H, gd, c0d, c2, h2)
        dg, dcp = c.out((rows, 4 * H)), (c.out((rows, H)) if has_dcp else None)
        # the backward reads the forward's own activated gates and c'
        K.lstm_cell_bwd(rows, H, gd, c0d, c2, c.inp(dh), c.inp(dc) if has_dc else None, dg, dcp)
        runs.append((has_c, has_dc, gd, c2, h2, dg, dcp))
    c.sync()
    for has_c, has_dc, gd, c2, h2, dg, dcp in runs:
        what = f"c_prev={has_c} dc={has_dc}"
        r64, r32 = P.lstm_cell(g, c0 if has_c else None), P.lstm_cell(g, c0 if has_c else None, dt=F32)
        act, cc = c.get(gd), c.get(c2)
        for got, k, name in ((act, 0, "gates"), (cc, 1, "c'"), (c.get(h2), 2, "h'")):
            c.add(P.check_close(got, r64[k], r32[k], what=f"{name} {what}"))
        # backward of the kernel's own fp32 gates and c' (its inputs), in float64 and float32
        b64 = P.lstm_cell_bwd(act, c0 if has_c else None, cc, dh, dc if has_dc else None)
        b32 = P.lstm_cell_bwd(act, c0 if has_c else None, cc, dh, dc if has_dc else None, dt=F32)
        c.add(P.check_close(c.get(dg), b64[0], b32[0], what=f"dg {what}"))
        if dcp is not None:
            c.add(P.check_close(c.get(dcp), b64[1], b32[1], what=f"dc_prev {what}"))
    c.done()


# ---- whole-sequence GRU ----------------------------------------------------------------------------------------------
def _seq_case(Q, n, L, with_h0):
    rng = np.random.default_rng(Q + L)
    S = Q // n
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    gi, Wh, bhn = f(S, L, n, 192) * F32(0.5), f(64, 192) / F32(8), f(64) * F32(0.1)
    h0, dhs = (f(Q, 64) if with_h0 else None), f(S, L, n, 64)
    ref = {}
    for dt in (F64, F32):
        hs, hT = P.gru_seq(gi, Wh, bhn, h0, dt)
        ref[dt] = (hs, hT) + P.gru_seq_bwd(gi, Wh, bhn, h0, hs, dhs, dt)
    return gi, Wh, bhn, h0, dhs, ref


@pytest.mark.parametrize("Q,n,L", [(16408, 8, 3), (16389, 3, 2), (24, 8, 1)])
@pytest.mark.parametrize("with_h0", [False, True])
def test_gru_seq(cuda, Q, n, L, with_h0):
    """Both B-operand forms; the first two shapes have 1026 / 1025 row blocks (> the 1024 persistent workgroups, so
    workgroups 0 and 1 loop) and a partial last block.  gi is laid out independently as (Q / n, L, n, 192)."""
    c = Case(cuda, f"gru_seq Q={Q} n={n} L={L} h0={with_h0}")  # (its wall time includes the float64 / float32 BPTT)
    gi, Wh, bhn, h0, dhs, ref = _seq_case(Q, n, L, with_h0)
    S, nblk = Q // n, K.gru_seq_blocks(Q)
    assert nblk == min(1024, -(-Q // 16))
    gid, Whd, bd, dhsd = c.inp(gi), c.inp(Wh), c.inp(bhn), c.inp(dhs)
    h0d = c.inp(h0) if with_h0 else None
    lib, runs = _lib.load(), []
    try:
        for form in (1, 0):
            assert lib.dgppo_gru_set_form(form) == 0
            hs, hT = c.out((S, L, n, 64)), c.out((Q, 64))
            K.gru_seq(True, Q, L, n, gid, Whd, bd, h0d, hs, hT=hT)
            dgi, dgh = c.out((S, L, n, 192)), c.out((S, L, n, 192))
            dh0, part = c.out((Q, 64)), c.out((nblk, 64))
            K.gru_seq(False, Q, L, n, gid, Whd, bd, h0d, hs, dhs=dhsd, dgi=dgi, dgh=dgh, dh0=dh0, dbhn_part=part)
            runs.append((form, hs, hT, dgi, dgh, dh0, part))
    finally:
        lib.dgppo_gru_set_form(1)
    c.sync()
    r64, r32 = ref[F64], ref[F32]
    for form, *outs in runs:
        for got, k, name in zip(outs[:5], range(5), ("hs", "hT", "dgi", "dgh", "dh0")):
            c.add(P.check_close(c.get(got), r64[k], r32[k], what=f"{name} form={form}"))
        c.add(P.check_sums(c.get(outs[5]).astype(F64).sum(0), r64[5], r64[6], what=f"dbhn form={form}"))
    c.done()


# ---- agent mean ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n,F", [(1, 1, 1), (5, 3, 65), (32781, 4, 64)])
def test_agent_mean(cuda, G, n, F):
    """Graph stride 2 n F: the n rows between two graphs are never read (NaN in x) nor written (dx keeps its NaN).
    Integer inputs: with n a power of two the forward is exact; n = 3 is held to the sums bound."""
    c = Case(cuda, f"agent_mean G={G} n={n} F={F}")
    rng = np.random.default_rng(G + n + F)
    x = np.full((G, 2 * n, F), np.nan, F32)
    x[:, :n] = rng.integers(-8, 9, (G, n, F)) if n != 3 else rng.standard_normal((G, n, F))
    dy = rng.standard_normal((G, F)).astype(F32)
    mask = rng.standard_normal((G, n, F)).astype(F32)
    flat = mask.reshape(-1)
    for i, v in enumerate((0.0, -0.0, -1.5, np.nan)):
        flat[i::7][:max(1, flat.size // 50)] = v
    y, dx, dxm, dxu = c.out((G, F)), c.out((G, 2 * n, F)), c.out((G, 2 * n, F)), c.out((G, 2 * n, F))
    dyd = c.inp(dy)
    K.agent_mean_fwd(c.inp(x), y, G, n, F, 2 * n * F)
    K.agent_mean_bwd(dyd, dx, G, n, F, 2 * n * F)
    K.agent_mean_bwd(dyd, dxm, G, n, F, 2 * n * F, mask=c.inp(mask))
    _lib.check(_lib.load().dgppo_agent_mean_bwd(K._p(dyd), K._p(dxu), G, n, F, 2 * n * F, K._stream(dyd)), "bwd")
    c.sync()
    ref, mag = P.agent_mean(x[:, :n])
    if n != 3:
        c.add(P.check_exact(c.get(y), ref, "mean"))
    else:
        c.add(P.check_sums(c.get(y), ref, mag, what="mean"))
    for got, m in ((dx, None), (dxm, mask), (dxu, None)):
        g = c.get(got, nan_ok=True)
        assert np.isnan(g[:, n:]).all(), "rows between two graphs were written"
        c.add(P.check_bits(g[:, :n], P.agent_mean_bwd(dy, n, m), "dx"))
    c.done()


# ---- ReLU backward, clip -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2097157])
def test_relu_bwd_and_clip_min0(cuda, n):
    c = Case(cuda, f"relu_bwd / clip_min0 n={n}")
    rng = np.random.default_rng(n)
    y, dy = rng.standard_normal(n).astype(F32), rng.standard_normal(n).astype(F32)
    for i, v in enumerate((-0.0, np.nan, 0.0)):  # n = 1: y = -0.0
        y[i::11][:max(1, n // 100)] = v
    dyd, out = c.out(n, dy), c.out(n)
    K.relu_bwd_(dyd, c.inp(y))
    K.clip_min0(c.inp(y), out)
    c.sync()
    c.add(P.check_bits(c.get(dyd), P.relu_bwd(dy, y), "relu_bwd"))
    c.add(P.check_bits(c.get(out, nan_ok=True), P.clip_min0(y), "clip_min0"))
    c.done()


# ---- gather_env_steps ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_sel,T,B", [(0, 7, 4), (1, 7, 4), (10, 103, 6), (7, 1, 9)])
def test_gather_env_steps(cuda, n_sel, T, B):
    """One 8-field call: 810-float rows (scalar moves), 768-float rows (16-byte moves), int32 rows of NaN payloads and
    INT_MIN, a (B, T) scalar field, a time-major view, a 768-float field one float off alignment (scalar moves again),
    4- and 3-float rows; envs unsorted with repeats; 1030 output rows end in a partial block."""
    c = Case(cuda, f"gather_env_steps n_sel={n_sel} T={T} B={B}")
    rng = np.random.default_rng(n_sel + T)
    envs = rng.integers(0, B, n_sel).astype(np.int64)
    if n_sel >= 3:
        envs[:3] = (B - 1, 0, B - 1)
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    ints = rng.integers(-2 ** 31, 2 ** 31, (B, T, 12), dtype=np.int64).astype(np.int32)
    ints[..., 0], ints[..., 1], ints[..., 2] = -2 ** 31, 0x7FC00001, -4194303  # INT_MIN, NaN payloads (+, -)
    host = [f(B, T, 810), f(B, T, 768), ints, f(B, T), f(T, B, 20), f(B, T, 768), f(B, T, 4), f(B, T, 3)]
    src = [c.inp(a, off=1 if i == 5 else 0) for i, a in enumerate(host)]
    src[4], host[4] = src[4].permute(1, 0, 2), host[4].transpose(1, 0, 2)
    dst = [c.out((n_sel,) + a.shape[1:], dtype=torch.int32 if a.dtype == np.int32 else torch.float32) for a in host]
    envd = torch.from_numpy(envs).to(cuda)
    torch.ops.dgppo.gather_env_steps(src, dst, envd)
    with pytest.raises((ValueError, RuntimeError)):
        torch.ops.dgppo.gather_env_steps(src + src[:1], dst + dst[:1], envd)
    c.sync()
    for i, (a, d) in enumerate(zip(host, dst)):
        # (the int32 field holds NaN bit patterns on purpose: a NaN sentinel left there differs from them as bits)
        c.add(P.check_bits(c.get(d, nan_ok=a.dtype == np.int32), P.gather_env_steps(a, envs), f"field {i}"))
    c.done()


# ---- advantages ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,n,nh", P.ADV_CASES)
def test_advantage_kernels(cuda, T, n, nh):
    """T = 1 (zero variance everywhere), T = 2, T = 257 (the stride loop over t); the last env's Ql - Vl is constant:
    std exactly 0, advantages 0 and not NaN."""
    c = Case(cuda, f"advantages T={T} n={n} nh={nh}")
    d, B = P.adv_inputs(T, n, nh), P.ADV_B
    dd = {k: c.inp(v) for k, v in d.items()}
    A, safe = c.out((B, T, n)), c.out(B)
    K.dgppo_advantages(dd["Ql"], dd["Vl"], dd["Vh"], A, safe, P.ADV_DT, P.ADV_ALPHA, P.ADV_EPS, P.ADV_W)
    Ai = c.out((B, T, n))
    K.informarl_advantages(dd["Ql"], dd["Vl"], Ai)
    Al, Ah = c.out((B, T, n)), c.out((B, T, n, nh))
    K.lagr_advantages(dd["Ql"], dd["Vl"], dd["Qh"], dd["Vh"], dd["lagr"], Al, Ah)
    sl = c.out((B, T))
    K.cost_shaped_loss(dd["rewards"], dd["costs"], 0.7, sl)
    c.sync()
    args = (d["Ql"], d["Vl"], d["Vh"], P.ADV_DT, P.ADV_ALPHA, P.ADV_EPS, P.ADV_W)
    r64, r32 = P.dgppo_adv(*args), P.dgppo_adv(*args, dt=F32)
    amb = r64[2]
    assert P.amb_ok(amb)
    gA = c.get(A)
    c.add(P.check_close(gA, r64[0], r32[0], scale=1 + r64[3], keep=~amb, what="dgppo A"))
    gs = c.get(safe)
    if amb.any():
        assert (np.abs(gs - r64[1]) <= amb.sum((1, 2))).all()
    else:
        c.add(P.check_exact(gs, r64[1], "safe_count"))
    gi_ = c.get(Ai)
    c.add(P.check_close(gi_, P.informarl_adv(d["Ql"], d["Vl"], n), P.informarl_adv(d["Ql"], d["Vl"], n, dt=F32),
                        what="informarl A"))
    assert (gi_[-1] == 0).all() and (gi_[:, :, :1] == gi_).all()  # std exactly 0 -> 0; the same value for every agent
    l64 = P.lagr_adv(d["Ql"], d["Vl"], d["Qh"], d["Vh"], d["lagr"])
    l32 = P.lagr_adv(d["Ql"], d["Vl"], d["Qh"], d["Vh"], d["lagr"], dt=F32)
    c.add(P.check_close(c.get(Al), l64[0], l32[0], scale=1 + l64[2], what="lagr A"))
    c.add(P.check_close(c.get(Ah), l64[1], l32[1], what="lagr Ah"))
    s64, smag = P.shaped_l(d["rewards"], d["costs"], 0.7)
    c.add(P.check_close(c.get(sl), s64, P.shaped_l(d["rewards"], d["costs"], 0.7, dt=F32)[0], scale=1 + smag, what="l"))
    c.done()


@pytest.mark.parametrize("rows,n,nh", [(1, 1, 1), (257, 5, 3), (70001, 5, 3), (70001, 1, 1)])
def test_lagr_update(cuda, rows, n, nh):
    c = Case(cuda, f"lagr_update rows={rows} n={n} nh={nh}")
    rng = np.random.default_rng(rows + n)
    f = lambda *s: rng.standard_normal(s).astype(F32)  # noqa: E731
    lp, lpo, Vh, Ah = f(rows, n), f(rows, n), f(rows, n, nh), f(rows, n, nh)
    lp = (lpo + F32(0.2) * lp).astype(F32)
    # small multipliers: some of the 15 updates cross 0 and are clipped; a lone multiplier starts at 1 and stays open
    lagr0 = np.abs(f(n, nh)) * F32(0.05) + F32(n * nh == 1)
    lagr, lmean = c.out((n, nh), lagr0), c.out(1)
    K.lagr_update(c.inp(lp), c.inp(lpo), c.inp(Vh), c.inp(Ah), lagr, lmean, rows, 0.99, 0.5)
    c.sync()
    r64, mag = P.lagr_update(lagr0, lp, lpo, Vh, Ah, 0.99, 0.5)
    r32, _ = P.lagr_update(lagr0, lp, lpo, Vh, Ah, 0.99, 0.5, dt=F32)
    c.add(P.check_close(c.get(lagr), r64, r32, scale=1 + mag, what="lagr"))
    c.add(P.check_close(c.get(lmean)[0], r64.mean(), r32.mean(), scale=1 + mag.mean(), what="lagr mean"))
    c.done()
