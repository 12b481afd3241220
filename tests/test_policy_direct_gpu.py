"""The fused policy step of csrc/policy.hip, called directly through the C ABI on synthetic graphs and held to the
float64 reference of tests/policy_ref.py across what dgppo_policy_step_supported accepts: every agent count 1..16,
action widths 1..4, the narrow / node-table / wide instantiations with both sides of the node-table bound, raw rows
narrower than 4 and wider than 8, edge rows of 4..10 columns, one and two layers, slot orders other than the envs',
repeated senders, cand == -1, slots whose edge targets another receiver, receivers without a valid candidate in the
first and the last row group, fewer graphs than a group, an all-agent graph, log_pi == NULL, and both clip branches
of the TanhNormal tail down to z = -1e4.

Every output sits between guard words that must come back untouched; the graph strides are wider than the rows and
their pads hold NaN (edges_gstride stays a multiple of 4 floats: the narrow kernel loads edge rows as 16-byte vectors).
Comparison: the `close` rule of tests/prim_ref.py with scale 1 + |ref64| for the carry and the action; log_pi is the
reference's at the action the kernel returned, so no clip branch is ambiguous and every element is compared; the work
buffer of dgppo_policy_prepare by `sums` against its summand magnitudes.  Which kernel a case runs is not asked here:
tests/test_policy_ref_cpu.py pins the table's coverage on the CPU."""
import ctypes

import numpy as np
import pytest
import torch

import policy_ref as PR
import prim_ref as P
from dgppo_fov_amd import _lib
from dgppo_fov_amd.nn import kernels as K

pytestmark = pytest.mark.gpu

CASES = {c.key: c for c in PR.cases()}
GUARD, SENT = 256, 0x7FC0DEAD  # guard words on both sides of an output; the sentinel is a NaN as a float
T64, T32 = PR.T64, PR.T32


class Buf:
    """(rows, width) float32 output inside guard words."""

    def __init__(self, dev, rows, width):
        self.rows, self.width = rows, width
        self.flat = torch.full((2 * GUARD + rows * width,), SENT, dtype=torch.int32, device=dev)
        self.ptr = self.flat.data_ptr() + 4 * GUARD

    def read(self, what):
        h = self.flat.cpu().numpy()
        assert (h[:GUARD] == SENT).all() and (h[len(h) - GUARD:] == SENT).all(), f"{what}: guard words overwritten"
        return np.ascontiguousarray(h[GUARD:len(h) - GUARD]).view(np.float32).reshape(self.rows, self.width)


class Bench:
    """The device image of a case's inputs and a dgppo_policy_step_args pointing at it."""

    def __init__(self, dev, c, d):
        self.dev, self.c, self.keep = dev, c, []
        G, n, E = c.Gn, c.n, d["E"]
        p = d["params"]
        a = self.a = _lib.PolicyStepArgs()
        a.G, a.N, a.E, a.n_agents, a.C, a.D0, a.A, a.n_layers, a.H, a.ED = G, c.N, E, n, c.C, c.D0, c.A, c.L, PR.H, c.ED
        a.cand = self.put(d["cand"])
        a.nodes_gstride, a.edges_gstride, a.idx_gstride = c.N * c.D0 + 3, E * c.ED + 8, E + 5
        a.nodes = self.strided(d["x"], a.nodes_gstride, float("nan"))
        a.edges = self.strided(d["ef"], a.edges_gstride, float("nan"))
        # index pads: in range, and naming receiver 0 / sender 0, so that a kernel reading them computes wrong rows
        a.receivers = self.strided(d["receivers"], a.idx_gstride, 0)
        a.senders = self.strided(d["senders"], a.idx_gstride, 0)
        for l, ly in enumerate(p["layers"]):
            r = a.layer[l]
            for f in ("Wq", "bq", "Wkt", "bk", "Wcat", "Wu", "bu"):
                setattr(r, f, self.put(ly[f]))
            r.Wex = self.put(ly["Wex"]) if ly["Wex"] is not None else None
            r.D, r.F = ly["D"], ly["F"]
        for f in ("head_W0", "head_b0", "ln0_s", "ln0_b", "head_W1", "head_b1", "ln1_s", "ln1_b", "gru_Wi", "gru_bi",
                  "gru_Wh", "gru_bhn", "Ws", "bs", "Wm", "bm", "Wsd", "bsd"):
            setattr(a, f, self.put(p[f]))
        a.std_shift, a.std_min = P.STD_SHIFT, P.STD_MIN
        assert a.std_shift == PR.STD_SHIFT and a.std_min == PR.STD_MIN  # the float32 values the reference takes
        a.h_in = self.put(d["h_in"])
        self.noise = self.put(d["noise"])
        self.work = Buf(dev, 2 * PR.QK_ROWS, PR.QK_COLS)
        a.work = self.work.ptr
        assert _lib.load().dgppo_policy_work_floats() == 2 * PR.QK_ROWS * PR.QK_COLS
        assert _lib.load().dgppo_policy_step_supported(ctypes.byref(a)) == 1, c.key

    def put(self, arr):
        t = torch.as_tensor(np.ascontiguousarray(arr)).to(self.dev)
        self.keep.append(t)
        return t.data_ptr()

    def strided(self, arr, gstride, fill):
        arr = np.asarray(arr)
        arr = arr.reshape(arr.shape[0], -1)
        assert gstride > arr.shape[1]
        buf = np.full((arr.shape[0], gstride), fill, arr.dtype)
        buf[:, :arr.shape[1]] = arr
        return self.put(buf)

    def prepare(self):
        K._chk(_lib.load().dgppo_policy_prepare(ctypes.byref(self.a), _lib.stream_handle(self.dev)),
               "dgppo_policy_prepare")
        torch.cuda.synchronize()
        return self.work.read("work").reshape(2, PR.QK_ROWS, PR.QK_COLS)

    def step(self, mode, noise=None, seed=None, stream=0, log_pi=True, what=""):
        """One launch into fresh guarded outputs: (h_out, action, log_pi or None) on the host."""
        a, rows = self.a, self.c.Gn * self.c.n
        h, act, lp = Buf(self.dev, rows, PR.HID), Buf(self.dev, rows, self.c.A), Buf(self.dev, rows, 1)
        a.mode, a.h_out, a.action, a.log_pi = mode, h.ptr, act.ptr, lp.ptr if log_pi else None
        a.noise, a.noise_seed, a.noise_stream = noise, seed, stream
        K._chk(_lib.load().dgppo_policy_step(ctypes.byref(a), _lib.stream_handle(self.dev)), "dgppo_policy_step")
        torch.cuda.synchronize()
        got_lp = lp.read(what + " log_pi")[:, 0]
        if not log_pi:
            assert (got_lp.view(np.int32) == SENT).all(), f"{what}: log_pi written without being passed"
        return h.read(what + " h_out"), act.read(what + " action"), got_lp if log_pi else None


def check_work(c, d, work, what):
    """dgppo_policy_prepare's output over a NaN fill: the layers in use hold the reference in every entry (zeros
    exactly), the half of an unused second layer still holds the fill."""
    w64, mag = PR.expected_work(d["params"])
    got = work[:c.L]
    r = P.check_sums(got, w64, mag, what=f"{what} work")
    assert (got[mag == 0] == 0).all(), f"{what}: work entries outside the products are not zero"
    if c.L == 1:
        assert (work[1].view(np.int32) == SENT).all(), f"{what}: one layer, but the second half of work was written"
    return r


# ---- the domain sweep -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", list(CASES))
def test_policy_step_domain(cuda, key):
    c = CASES[key]
    d = PR.inputs(c)
    r64, r32 = PR.expected(c)
    b = Bench(cuda, c, d)
    ratios = dict(work=check_work(c, d, b.prepare(), key))
    for mode in (0, 1):
        what = f"{key} mode {mode}"
        h, act, lp = b.step(mode, noise=b.noise if mode else None, what=what)
        nz = d["noise"] if mode else None
        rh = P.check_close(h, r64["h_out"], r32["h_out"], what=what + " h_out")
        ra = P.check_close(act, PR.action(r64, nz, T64), PR.action(r32, nz, T32), what=what + " action")
        # log_pi of the kernel's own action: the branch is the action's, whatever rounding decided it
        l64, l32 = PR.log_pi(r64, act, T64), PR.log_pi(r32, act, T32)
        rl = P.check_close(lp, l64["log_pi"], l32["log_pi"], what=what + " log_pi")
        ratios[mode] = (rh, ra, rl)
        if mode == 1:  # without log_pi: the same carry and action bits, nothing written for log_pi
            h2, act2, _ = b.step(1, noise=b.noise, log_pi=False, what=what + " (log_pi NULL)")
            P.check_bits(h2, h, what + " h_out without log_pi")
            P.check_bits(act2, act, what + " action without log_pi")
    print(f"[policy] {key:18s} {c.inst:10s} work {ratios['work']:.3f} | "
          + " | ".join(f"mode {m}: h_out {ratios[m][0]:.3f} action {ratios[m][1]:.3f} log_pi {ratios[m][2]:.3f}"
                       for m in (0, 1)))


# ---- the clip branches of the fused tail -----------------------------------------------------------------------------------
@pytest.mark.parametrize("A", [4, 1])
def test_policy_step_clip_branches(cuda, A):
    """Wm = Wsd = 0 make mean = bm and std_raw = bsd exactly; they walk prim_ref.clip_grid() (std_min 1e-5, z down to
    -1e4, both forms of log Phi), A grid rows of one side per launch, neighbours in |z| together so that the row's
    summed scale stays that of its terms.  Per-row noise of +-1e8 drives the rows onto the right and the left clip
    (action exactly +-1).  log_pi by `close` without a float32 floor, scale the summands' magnitudes: the rule and
    the z grid of test_tanh_normal_clip_branches."""
    mean, sraw, _ = P.clip_grid()
    c = PR.Case("clip", 3, 8, 7, 5, A, G=2)
    d = dict(PR.make_inputs(c))
    p = d["params"] = dict(d["params"])
    p["Wm"], p["Wsd"] = np.zeros((PR.HID, A), np.float32), np.zeros((PR.HID, A), np.float32)
    rows = c.Gn * c.n
    noise = np.where(np.arange(rows)[:, None] % 2 == 0, np.float32(-1e8), np.float32(1e8)) * np.ones((1, A), np.float32)
    if A > 1:
        noise[2:4, 1::2] *= -1  # rows whose action dims sit on different clips
    seen, worst = set(), 0.0
    for side in (0, 1):
        ks = list(range(side, mean.shape[0], 2))
        for i in range(0, len(ks), A):
            idx = (ks[i:i + A] + [ks[-1]] * A)[:A]
            p["bm"], p["bsd"] = mean[idx, 0].copy(), sraw[idx, 0].copy()
            b = Bench(cuda, c, d)
            b.prepare()
            _, act, lp = b.step(1, noise=b.put(noise), what=f"clip A={A} rows {idx}")
            assert (np.abs(act) == 1.0).all() and (np.sign(act) == np.sign(noise)).all()
            r = P.tanh_normal(np.broadcast_to(p["bm"], (rows, A)), np.broadcast_to(p["bsd"], (rows, A)), PR.STD_SHIFT,
                              PR.STD_MIN, act)
            assert r["clip"].all()
            ratio = P.check_close(lp, r["log_pi"], None, scale=r["log_pi_mag"], what=f"clip A={A} rows {idx} log_pi")
            worst = max(worst, ratio)
            # the z each (row, dim) sat at, for the coverage check below
            sd = r["std"]
            t = np.arctanh(P.THRESH)
            z = np.where(act < 0, (-t - p["bm"]) / sd, (p["bm"] - t) / sd)
            seen |= {(side, k) for k in idx if np.isclose(z[:, idx.index(k)], P.Z_GRID[k // 2], rtol=1e-3, atol=1e-3).any()}
            print(f"[policy] clip A={A} grid rows {idx}: z {np.unique(np.round(z, 1))[:8]} ratio {ratio:.3f}")
    assert seen == {(k % 2, k) for k in range(mean.shape[0])}, "a grid row never sat on its clip"
    assert min(P.Z_GRID) <= -10 < max(P.Z_GRID)
    print(f"[policy] clip A={A}: worst log_pi error / bound {worst:.3f}")


# ---- noise drawn in the kernel -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["n1", "n4"])
def test_policy_step_in_kernel_noise_A1_A4(cuda, key):
    """A = 1 and A = 4 (the envs give 2 and 3, tests/test_rollout_gpu.py): the launch drawing its noise from
    (noise_seed, noise_stream) gives the bits of the launch fed the buffer dgppo_normal writes for that stream."""
    c = CASES[key]
    assert c.A == {"n1": 1, "n4": 4}[key]
    b = Bench(cuda, c, PR.inputs(c))
    b.prepare()
    rows = c.Gn * c.n
    for seed, sid in ((0x1234_5678_9ABC, (5 << 32) | 7), (1 << 40, ((1 << 30) - 1) << 32 | 127)):
        key_t = torch.tensor([seed], dtype=torch.int64, device=cuda)
        noise = torch.empty((rows, c.A), device=cuda)
        K.normal_(noise, stream_id=sid, seed_tensor=key_t)
        ref = b.step(1, noise=noise.data_ptr(), what="buffer")
        got = b.step(1, seed=key_t.data_ptr(), stream=sid, what="seed")
        for x, y, what in zip(ref, got, ("h_out", "action", "log_pi")):
            P.check_bits(x, y, f"{key} {what} seed {seed:#x} stream {sid:#x}")
        assert np.isfinite(got[1]).all() and len(np.unique(got[1])) > rows * c.A // 2
