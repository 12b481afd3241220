"""Raw-array reference of the fused policy step at the C-ABI level: dgppo_policy_prepare and dgppo_policy_step
(helper, not a test; tests/test_policy_ref_cpu.py checks it, tests/test_policy_direct_gpu.py compares the kernel with it).

The chain -- GraphTransformer layers in the per-edge form over the valid candidates, MLP head, GRU cell, ScaleHid, the
mean / std Denses and the clipped TanhNormal log-prob -- is written from oracle/nets_t.py and the parameter layouts
that include/dgppo_hip.h documents, never from the kernel; every statement takes a torch dtype: float64 is the
reference, float32 the `ref32` of the `close` rule of tests/prim_ref.py.  The log-prob is prim_ref.tanh_normal (the
float32 value of the clip threshold included).

Graphs come from attn_ref.make_graph (layouts agent_first / spread / free / dup, its masked slots and cand == -1);
empty_receivers() takes every candidate from chosen receivers.  Inputs follow attn_ref.make_inputs: raw node rows and
the first layer's Wu / bu are multiples of 1/8 with magnitude <= 2, so the layer-1 features relu(x_raw Wu0 + bu0) of
the never-receiving nodes are exact in fp32 in any summation order and their gates are unambiguous.

Also here: expected_work() (the query-key products dgppo_policy_prepare writes, with the summand magnitudes),
instantiation() (a restatement of the three-way kernel choice of dgppo_policy_step's host code; the library does not
report which kernel ran) and the case table of the GPU file, whose coverage the CPU file pins through instantiation().
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np
import torch

import attn_ref as A
import prim_ref as P
from oracle import nets_t as R

T64, T32 = torch.float64, torch.float32
H, ROWS, CP, HID = 3, 16, 32, 64          # heads, rows per workgroup, candidate slots, hidden width
MAX_D0, NARROW_D0, MAX_ED, PRE_MAX = 12, 8, 10, 160
QK_ROWS, QK_COLS = 33, 100                # per layer: rows 0..D-1 and the bias row 32; [QT_0 | QT_1 | QT_2 | beta | 0]
LAYOUTS = ("agent_first", "spread", "free", "dup")
# what the kernel is handed: the float32 values of the actor's std_dev_init shift and std_dev_min
STD_SHIFT, STD_MIN = float(np.float32(P.STD_SHIFT)), float(np.float32(P.STD_MIN))


# ---- the host code's decisions ----------------------------------------------------------------------------------------
def supported(n, C, D0, A_, ED, N, n_layers, dims, wex=(True, True), Hh=H):
    """dgppo_policy_step_supported: dims = ((D, F), (D, F)) of the two layer records, wex whether each has Wex."""
    if not (1 <= n <= ROWS and 1 <= C <= CP and 1 <= D0 <= MAX_D0 and 1 <= A_ <= 4 and Hh == H and 4 <= ED <= MAX_ED):
        return False
    if N < n:
        return False
    if ED > 4 and not all(wex[:min(max(n_layers, 0), 2)]):
        return False
    if n_layers == 2:
        return dims[0] == (D0, 32) and dims[1] == (32, 64)
    if n_layers == 1:
        return dims[0] == (D0, 64)
    return False


def instantiation(n, N, D0, ED, n_layers):
    """Which policy_step_kernel dgppo_policy_step launches: "wide" (raw rows past 8 columns or edge rows past 4),
    "node_table" (narrow, two layers, between 1 and 160 / (16 // n) never-receiving nodes per graph: their layer-1
    features are computed once per node) or "narrow"."""
    if D0 > NARROW_D0 or ED > 4:
        return "wide"
    gpg = ROWS // n
    if n_layers == 2 and N > n and gpg * (N - n) <= PRE_MAX:
        return "node_table"
    return "narrow"


# ---- cases --------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    key: str
    n: int
    N: int
    C: int
    D0: int
    A: int
    ED: int = 4
    L: int = 2
    layout: str = "agent_first"
    G: int = 0            # 0: two full row groups and a partial one
    seed: int = 0

    @property
    def gpg(self):
        return ROWS // self.n

    @property
    def Gn(self):
        return self.G or 2 * self.gpg + 1

    @property
    def inst(self):
        return instantiation(self.n, self.N, self.D0, self.ED, self.L)

    @property
    def dims(self):
        return ((self.D0, 32), (32, 64)) if self.L == 2 else ((self.D0, 64),)

    @property
    def dead(self):
        """Receivers left without a valid candidate: one in the first row group, one in the last."""
        return sorted({(0, self.n - 1), (self.Gn - 1, self.n - 1)})


def cases():
    cs = []
    # every agent count (n = 5, 6, 7: dead rows in the 16-row group; n >= 9: one graph per workgroup), the action
    # widths, the layouts, one and two layers, raw rows narrower than 4
    d0s = (1, 2, 3, 4, 5, 6, 7, 8, 3, 5, 7, 8, 1, 4, 6, 8)
    for n in range(1, 17):
        layout = LAYOUTS[(n + 2) % 4]  # spread at n = 3, 7, 11, 15
        if layout == "spread":
            N, C = A.spread_shape(n, 2)
        else:
            N, C = n + 5, min(n + 4, CP)
        cs.append(Case(f"n{n}", n, N, C, d0s[n - 1], 1 + (n - 1) % 4, L=1 if n % 3 == 0 else 2, layout=layout))
    # wide because of the raw rows (ED == 4: no Wex) and because of the edge rows (narrow D0), and both
    cs += [Case("wide_D9", 4, 9, 8, 9, 2), Case("wide_D12_L1", 5, 10, 9, 12, 3, L=1),
           Case("wide_D10_n16", 16, 21, 20, 10, 4), Case("wide_D11_free", 2, 7, 6, 11, 1, layout="free"),
           Case("wide_ED5", 3, 8, 7, 5, 2, ED=5), Case("wide_ED7_L1", 6, 11, 10, 8, 1, ED=7, L=1),
           Case("wide_ED9_dup", 7, 12, 11, 2, 4, ED=9, layout="dup"), Case("wide_ED6_n8", 8, 13, 12, 7, 3, ED=6),
           Case("wide_D10_ED10", 3, 8, 7, 10, 2, ED=10), Case("wide_ED10_n16_A1", 16, 21, 20, 4, 1, ED=10, layout="free")]
    # the node-table boundary gpg (N - n) <= 160 at gpg = 2, 5 and 1, C = 32 so that the candidates reach far into
    # the table; a table whose last MFMA tile is partial
    for n, nnr in ((8, 80), (8, 81), (3, 32), (3, 33), (16, 160), (16, 161)):
        cs.append(Case(f"table_n{n}_nnr{nnr}", n, n + nnr, CP, (7, 8, 5)[n % 3], 2, layout="free" if n == 8 else "agent_first"))
    cs.append(Case("table_partial_tile", 5, 12, 12, 6, 3, layout="dup"))
    # an all-agent graph (N == n): no never-receiving node, the narrow kernel
    cs.append(Case("N_eq_n", 4, 4, 4, 5, 2))
    # fewer graphs than one group holds
    cs += [Case("G1_n3", 3, 8, 7, 7, 2, G=1), Case("G2_n2_L1", 2, 7, 6, 4, 3, G=2, L=1)]
    assert len({c.key for c in cs}) == len(cs)
    return cs


# ---- inputs -------------------------------------------------------------------------------------------------------------
def empty_receivers(g, N, rows):
    """Take every candidate from the receivers (graph, agent) of `rows`: their slots' edges now target the pad N."""
    n, C = g["cand"].shape
    for gi, i in rows:
        g["receivers"][gi, i * C:(i + 1) * C] = N
    return g


def make_params(c: Case, rng):
    """float32 parameter arrays in the layouts of include/dgppo_hip.h."""
    p = dict(layers=[])
    for l, (D, F) in enumerate(c.dims):
        sq = (1.0 if l == 0 else 0.5) / math.sqrt(D)
        ly = dict(D=D, F=F, Wq=A._nrm(rng, (D, H * F), sq), bq=A._nrm(rng, (H * F,), 0.1),
                  Wkt=A._nrm(rng, (H, F, D), sq), bk=A._nrm(rng, (H * F,), 0.1),
                  Wcat=A._nrm(rng, (H * (D + 5), F), 1.0 / math.sqrt(D + 5)),
                  Wex=A._nrm(rng, (H * (c.ED - 4), F), 0.3) if c.ED > 4 else None)
        if l == 0:
            ly["Wu"], ly["bu"] = A._q8(rng, (D, F)), A._q8(rng, (F,))
        else:
            ly["Wu"], ly["bu"] = A._nrm(rng, (D, F), 1.0 / math.sqrt(D)), A._nrm(rng, (F,), 0.3)
        p["layers"].append(ly)
    for l in (0, 1):
        p[f"head_W{l}"], p[f"head_b{l}"] = A._nrm(rng, (HID, HID), 0.125), A._nrm(rng, (HID,), 0.1)
        p[f"ln{l}_s"], p[f"ln{l}_b"] = 1 + A._nrm(rng, (HID,), 0.1), A._nrm(rng, (HID,), 0.1)
    p["gru_Wi"], p["gru_bi"] = A._nrm(rng, (HID, 3 * HID), 0.125), A._nrm(rng, (3 * HID,), 0.1)
    p["gru_Wh"], p["gru_bhn"] = A._nrm(rng, (HID, 3 * HID), 0.125), A._nrm(rng, (HID,), 0.1)
    p["Ws"], p["bs"] = A._nrm(rng, (HID, HID), 0.125), A._nrm(rng, (HID,), 0.1)
    p["Wm"], p["bm"] = A._nrm(rng, (HID, c.A), 0.25), A._nrm(rng, (c.A,), 0.1)
    p["Wsd"], p["bsd"] = A._nrm(rng, (HID, c.A), 0.25), A._nrm(rng, (c.A,), 0.1)
    return p


def make_inputs(c: Case, named=False):
    """float32 / int32 numpy inputs of a case (packed; the GPU file lays them out with its strides)."""
    G = c.Gn
    g = A.make_graph(G, c.n, c.N, c.C, c.layout, seed=c.seed, named=named)
    empty_receivers(g, c.N, c.dead)
    rng = np.random.default_rng([13, c.seed, G, c.n, c.N, c.C, c.D0, c.ED, c.A, c.L])
    d = dict(g)
    d["sidx"] = A.sender_table(g["cand"], g["receivers"], g["senders"])
    d["x"] = A._q8(rng, (G, c.N, c.D0))
    d["ef"] = A._nrm(rng, (G, g["E"], c.ED))
    d["h_in"] = A._nrm(rng, (G * c.n, HID), 0.5)
    d["noise"] = A._nrm(rng, (G * c.n, c.A))
    d["params"] = make_params(c, rng)
    return d


@functools.lru_cache(maxsize=None)
def inputs(c: Case):
    return make_inputs(c)


# ---- the reference --------------------------------------------------------------------------------------------------------
def _t(a, dt):
    return A._t(a, dt)


def gt_layer(ly, x_all, ef, cand, sidx, n, dt):
    """One GraphTransformer layer (oracle.nets_t.graph_transformer) for the agent rows: x_all (G, N, D) the input row
    of every node, the edge list the valid candidates (sidx >= 0) of each receiver.  Returns (G, n, F) and, for each
    receiver row, the attention-weighted sum's weight total (1, or 0 for a receiver without a valid candidate)."""
    G, D, F = x_all.shape[0], ly["D"], ly["F"]
    Rn = G * n
    w = {k: _t(v, dt) for k, v in ly.items() if isinstance(v, np.ndarray)}
    g, i, s = torch.nonzero(sidx >= 0, as_tuple=True)
    seg, snd, e = g * n + i, sidx[g, i, s], cand[i, s]
    xr, xs, efe = x_all[:, :n].reshape(Rn, D), x_all[g, snd], ef[g, e]
    q = (xr @ w["Wq"] + w["bq"]).reshape(Rn, H, F)
    k = torch.einsum("ed,hfd->ehf", xs, w["Wkt"]) + w["bk"].reshape(H, F)
    wv, we = w["Wcat"][:H * D].reshape(H, D, F), w["Wcat"][H * D:H * D + 4 * H].reshape(H, 4, F)
    bv = w["Wcat"][H * D + 4 * H:].reshape(H, F)
    v = torch.einsum("ed,hdf->ehf", xs, wv) + bv
    em = torch.einsum("ej,hjf->ehf", efe[:, :4], we)
    if "Wex" in w:
        em = em + torch.einsum("ej,hjf->ehf", efe[:, 4:], w["Wex"].reshape(H, -1, F))
    lg = (q[seg] * k).sum(-1) / math.sqrt(F)
    a = R.segment_softmax(lg, seg, Rn) if len(seg) else lg
    agg = torch.zeros(Rn, F, dtype=dt).index_add(0, seg, (a[:, :, None] * (v + em)).mean(1))
    tot = torch.zeros(Rn, H, dtype=dt).index_add(0, seg, a)
    return torch.relu(xr @ w["Wu"] + w["bu"] + agg).reshape(G, n, F), tot, lg


def _head_tree(p, dt):
    t = {f"Dense_{l}": dict(kernel=_t(p[f"head_W{l}"], dt), bias=_t(p[f"head_b{l}"], dt)) for l in (0, 1)}
    t.update({f"LayerNorm_{l}": dict(scale=_t(p[f"ln{l}_s"], dt), bias=_t(p[f"ln{l}_b"], dt)) for l in (0, 1)})
    return t


def _gru_tree(p, dt):
    wi, bi, wh = _t(p["gru_Wi"], dt), _t(p["gru_bi"], dt), _t(p["gru_Wh"], dt)
    t = {}
    for j, gate in enumerate("rzn"):
        t["i" + gate] = dict(kernel=wi[:, HID * j:HID * j + HID], bias=bi[HID * j:HID * j + HID])
        t["h" + gate] = dict(kernel=wh[:, HID * j:HID * j + HID])
    t["hn"]["bias"] = _t(p["gru_bhn"], dt)
    return t


@torch.no_grad()
def step(c: Case, d, dt=T64):
    """dgppo_policy_step up to the distribution: h_out (G n, 64), mean and std_raw (G n, A), numpy arrays in dt, and
    the per-layer weight totals / logits."""
    p, n, G = d["params"], c.n, c.Gn
    x, ef, cand, sidx = _t(d["x"], dt), _t(d["ef"], dt), _t(d["cand"], dt), _t(d["sidx"], dt)
    y, tot0, lg0 = gt_layer(p["layers"][0], x, ef, cand, sidx, n, dt)
    tots, lgs = [tot0], [lg0]
    if c.L == 2:
        l0 = p["layers"][0]
        rest = torch.relu(x[:, n:] @ _t(l0["Wu"], dt) + _t(l0["bu"], dt))  # nodes that never receive: no aggregate
        y, tot1, lg1 = gt_layer(p["layers"][1], torch.cat([y, rest], 1), ef, cand, sidx, n, dt)
        tots.append(tot1), lgs.append(lg1)
    z = R.mlp_head(y.reshape(G * n, HID), _head_tree(p, dt))
    h2 = R.gru_cell(_gru_tree(p, dt), _t(d["h_in"], dt), z)
    s = h2 @ _t(p["Ws"], dt) + _t(p["bs"], dt)
    mean = s @ _t(p["Wm"], dt) + _t(p["bm"], dt)
    sraw = s @ _t(p["Wsd"], dt) + _t(p["bsd"], dt)
    return dict(h_out=h2.numpy(), mean=mean.numpy(), std_raw=sraw.numpy(), tot=[t.numpy() for t in tots],
                max_logit=max([float(l.abs().max()) if l.numel() else 0.0 for l in lgs]))


def np_dt(dt):
    return np.float64 if dt == T64 else np.float32


def action(r, noise, dt=T64, std_shift=STD_SHIFT, std_min=STD_MIN):
    """mode 0 (noise None): tanh(mean); mode 1: tanh(mean + std noise)."""
    return P.tanh_normal_action(r["mean"], r["std_raw"], std_shift, std_min, noise, dt=np_dt(dt))


def log_pi(r, act, dt=T64, std_shift=STD_SHIFT, std_min=STD_MIN):
    """The clipped TanhNormal log-prob of the distribution of `r` at the given actions (G n, A): prim_ref.tanh_normal's
    dict (log_pi, its summand magnitudes log_pi_mag, clip)."""
    return P.tanh_normal(r["mean"], r["std_raw"], std_shift, std_min, act, dt=np_dt(dt))


@functools.lru_cache(maxsize=None)
def expected(c: Case):
    """(float64, float32) references of a case, computed once per process and shared."""
    d = inputs(c)
    return step(c, d, T64), step(c, d, T32)


def floor_excess(r64, r32, name):
    """Fraction of an output's elements whose floor term 8 |ref32 - ref64| passes 1e-3 of the scale 1 + |ref64|."""
    a64 = np.asarray(r64[name], np.float64)
    fl = 8.0 * np.abs(np.asarray(r32[name]).astype(np.float64) - a64)
    return float((fl > 1e-3 * (1.0 + np.abs(a64))).mean())


# ---- dgppo_policy_prepare ------------------------------------------------------------------------------------------------
def expected_work(params):
    """(n_layers, 33, 100) float64 and the same shape of summand magnitudes: per layer, rows k < D hold
    [Wq_h Wkt_h (columns 32 h + d, d < D) | Wq_h bk_h (column 96 + h)] of input column k, row 32 the same products of
    bq; every other entry is zero."""
    out, mag = [], []
    for ly in params["layers"]:
        D, F = ly["D"], ly["F"]
        wq = np.concatenate([ly["Wq"], np.zeros((QK_ROWS - 1 - D, H * F)), ly["bq"][None]], 0).astype(np.float64)
        wq = wq.reshape(QK_ROWS, H, F)
        wkt, bk = ly["Wkt"].astype(np.float64), ly["bk"].astype(np.float64).reshape(H, F)
        w, m = np.zeros((QK_ROWS, QK_COLS)), np.zeros((QK_ROWS, QK_COLS))
        for h in range(H):
            w[:, 32 * h:32 * h + D] = wq[:, h] @ wkt[h]
            m[:, 32 * h:32 * h + D] = np.abs(wq[:, h]) @ np.abs(wkt[h])
            w[:, 96 + h] = wq[:, h] @ bk[h]
            m[:, 96 + h] = np.abs(wq[:, h]) @ np.abs(bk[h])
        out.append(w), mag.append(m)
    return np.stack(out), np.stack(mag)


# ---- the oracle's view (tests/test_policy_ref_cpu.py) -----------------------------------------------------------------------
def to_flax(params, ED):
    """The actor's flax parameter tree (float64 numpy leaves) of the raw arrays, as GraphTransformer.flax lays it out."""
    f = lambda a: np.asarray(a, np.float64)  # noqa: E731
    gnn = []
    for ly in params["layers"]:
        D, F = ly["D"], ly["F"]
        wcat = f(ly["Wcat"])
        wv, we, bv = wcat[:H * D], wcat[H * D:H * D + 4 * H], wcat[H * D + 4 * H:]
        k3 = we.reshape(H, 4, F).transpose(1, 0, 2).reshape(4, H * F)
        if ED > 4:
            k3 = np.concatenate([k3, f(ly["Wex"]).reshape(H, ED - 4, F).transpose(1, 0, 2).reshape(ED - 4, H * F)], 0)
        gnn.append({"Dense_0": dict(kernel=f(ly["Wq"]), bias=f(ly["bq"])),
                    "Dense_1": dict(kernel=f(ly["Wkt"]).transpose(2, 0, 1).reshape(D, H * F), bias=f(ly["bk"])),
                    "Dense_2": dict(kernel=wv.reshape(H, D, F).transpose(1, 0, 2).reshape(D, H * F), bias=bv.reshape(-1)),
                    "Dense_3": dict(kernel=k3),
                    "Dense_4": dict(kernel=f(ly["Wu"]), bias=f(ly["bu"]))})
    head = {f"Dense_{l}": dict(kernel=f(params[f"head_W{l}"]), bias=f(params[f"head_b{l}"])) for l in (0, 1)}
    head.update({f"LayerNorm_{l}": dict(scale=f(params[f"ln{l}_s"]), bias=f(params[f"ln{l}_b"])) for l in (0, 1)})
    gru = {}
    for j, gate in enumerate("rzn"):
        gru["i" + gate] = dict(kernel=f(params["gru_Wi"])[:, HID * j:HID * j + HID], bias=f(params["gru_bi"])[HID * j:HID * j + HID])
        gru["h" + gate] = dict(kernel=f(params["gru_Wh"])[:, HID * j:HID * j + HID])
    gru["hn"]["bias"] = f(params["gru_bhn"])
    return dict(gnn=gnn, head=head, gru=gru, ScaleHid=dict(kernel=f(params["Ws"]), bias=f(params["bs"])),
                OutputDenseMean=dict(kernel=f(params["Wm"]), bias=f(params["bm"])),
                OutputDenseStdTrans=dict(kernel=f(params["Wsd"]), bias=f(params["bsd"])))
