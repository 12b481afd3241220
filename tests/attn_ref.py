"""Per-edge reference of the GraphTransformer attention entry points at the C-ABI level (helper, not a test;
tests/test_attn_ref_cpu.py checks it, tests/test_attn_direct_gpu.py compares the kernels with it).

Raw arrays in, the kernels' output arrays out: dgppo_gnn_sender_table, dgppo_gnn_attn_fwd / _bwd (both query forms,
the three sender modes), dgppo_gnn_layer_fwd (qb, attn, xcat, Y, zmean, the value tail) and dgppo_gnn_edge_wsum /
_edge_da.  Written from oracle/nets_t.py (segment_softmax over the list of valid edges, graph_transformer's message
and update, mlp_head, gru_cell) and the formulas of include/dgppo_hip.h, never from a kernel; every statement takes a
torch dtype: float64 is the reference, float32 the `ref32` of the `close` rule of tests/prim_ref.py.  The backward is
torch.autograd on sum(xcat * dxcat) + sum(attn * da_add).

Also here: the seeded synthetic graph generator (every index in range: senders in [0, N), receivers in [0, N] with
N the envs' pad for a masked edge, cand in [-1, E)), the input generator (raw rows and pre_W / pre_b on multiples of
1/8 with magnitude <= 2, so every pre-activation relu(x_raw pre_W + pre_b) is exact in fp32 in any summation order
and its gate is unambiguous), the comparator, and the case table of the GPU file.

Scales of the `close` rule: 1 + |ref64| for attn, qb, Y and the tail output; for sums with cancellation (xcat, zmean,
every gradient) the sum of the summands' magnitudes, carried from the leaves: a gradient's magnitude is its formula
with every factor replaced by its magnitude and every difference by a sum.
"""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass, replace

import numpy as np
import torch

import prim_ref as P
from oracle import nets_t as R

T64, T32 = torch.float64, torch.float32
KH, KD0, ROWS = 3, 8, 16  # heads of the tuned kernels, widest raw row, receiver rows per workgroup


# ---- synthetic graphs -------------------------------------------------------------------------------------------------
def spread_shape(n, k):
    """(N, C) of the Spread layout: agents, goals, k own hits per agent and a pad node."""
    return 2 * n + n * k + 1, 2 * n + k


def make_graph(G, n, N, C, layout="agent_first", seed=0, extra=3, named=False):
    """cand (n, C), receivers / senders (G, E) int32 with E = n C + extra, and the structure the graph holds.

    Slot c of receiver i is edge i C + c.  layout `agent_first`: slot c < n holds agent c, slots >= n distinct
    non-agent senders (what every env emits); `spread`: agent_first with slots n .. 2n - 1 the goals n .. 2n - 1 and
    the rest the receiver's own nodes 2n + i k ..; `free`: each receiver's slots permuted independently; `dup`: some
    receivers hold one agent and one non-agent sender twice.  A masked slot's edge has another receiver (the pad N or
    another agent) and any sender; cand == -1 masks slots whose edge does target the receiver.  named: the candidate
    table names every edge and a masked edge's receiver is always the pad (the graph is then one the oracle's
    receivers / senders form computes the same attention on)."""
    assert layout in ("agent_first", "spread", "free", "dup") and n >= 1 and N >= n and C >= 1
    rng = np.random.default_rng([seed, G, n, N, C, ("agent_first", "spread", "free", "dup").index(layout)])
    E, Rn = n * C + extra, G * n
    S = rng.integers(0, N, (G, n, C))
    V = rng.random((G, n, C)) < 0.7
    can = np.zeros((n, C), bool)  # slots that can hold a valid sender under the layout
    na = min(n, C)
    can[:, :na] = True
    S[:, :, :na] = np.arange(na)
    for g in range(G):
        for i in range(n):
            if C <= n or N == n:
                continue
            if layout == "spread":
                k = C - 2 * n
                assert k >= 1 and N == 2 * n + n * k + 1
                S[g, i, n:2 * n] = np.arange(n, 2 * n)
                S[g, i, 2 * n:] = 2 * n + i * k + np.arange(k)
                can[i, n:] = True
            else:
                m = min(C - n, N - n)
                S[g, i, n:n + m] = rng.permutation(np.arange(n, N))[:m]
                can[i, n:n + m] = True
    V &= can[None]
    flags = set()
    # cand == -1: one slot of every receiver but the one that must keep all C
    rows = [("one", 0), ("zero", 1), ("all", 2)]
    i_all = (2 % Rn) % n if Rn >= 3 else -1
    cand = np.arange(n * C, dtype=np.int32).reshape(n, C)
    neg = np.zeros((n, C), bool)
    if named:
        extra, E = 0, n * C
    if C >= 3 and not named:
        for i in range(n):
            if i != i_all:
                neg[i, (3 * i + 1) % C] = True
                flags.add("cand_neg")
    cand[neg] = -1
    usable = can & ~neg
    if G >= 1 and usable[:, 0].all():  # agent 0 sends to every receiver of the last graph (a self edge at i = 0)
        V[G - 1, :, 0] = True
        flags |= {"sends_to_all", "self_edge"}
    special = {}
    for name, r in rows:
        if r >= Rn:
            continue
        g, i = divmod(r, n)
        special[(g, i)] = name
        if name == "zero":
            V[g, i] = False
            flags.add("zero")
        elif name == "one":
            V[g, i] = False
            cs = np.flatnonzero(usable[i])
            if len(cs):
                V[g, i, cs[-1]] = True
                flags.add("one")
        elif usable[i].all():
            V[g, i] = True
            flags.add("all")
    if layout == "free":
        for g in range(G):
            for i in range(n):
                cs = np.flatnonzero(~neg[i])
                pm = rng.permutation(cs)
                S[g, i, cs], V[g, i, cs] = S[g, i, pm], V[g, i, pm]
        flags.add("free")
    if layout == "dup":
        for g in range(G):
            for i in range(n):
                if (g, i) in special:
                    continue
                cs = np.flatnonzero(usable[i, :na])
                if len(cs) >= 2 and (g + i) % 2 == 0:  # one agent on two valid candidates
                    S[g, i, cs[1]] = S[g, i, cs[0]]
                    V[g, i, cs[:2]] = True
                    flags.add("dup_agent")
                cs = np.flatnonzero(usable[i, n:]) + n
                if len(cs) >= 2:  # one non-agent sender on two valid candidates
                    S[g, i, cs[1]] = S[g, i, cs[0]]
                    V[g, i, cs[:2]] = True
                    flags.add("dup_other")
    send = rng.integers(0, N, (G, E)).astype(np.int32)
    recv = rng.integers(0, N + 1, (G, E)).astype(np.int32)  # the `extra` edges: no candidate names them
    if extra:
        flags.add("unnamed_edges")
    for i in range(n):
        for c in range(C):
            e = i * C + c
            send[:, e] = S[:, i, c]
            other = N if (c % 2 == 0 or n == 1 or named) else (i + 1) % n  # a masked edge: the pad, or another agent's edge
            recv[:, e] = np.where(V[:, i, c] | neg[i, c], i, other)
    if (~V & can[None] & ~neg[None]).any():
        flags.add("recv_mismatch")
    return dict(cand=cand, receivers=recv, senders=send, E=E, flags=flags)


def sender_table(cand, receivers, senders):
    """sidx (G, n, C): senders[g, cand[i, c]] where cand[i, c] >= 0 and that edge's receiver is i, else -1."""
    cand, receivers, senders = (np.asarray(a).astype(np.int64) for a in (cand, receivers, senders))
    n = cand.shape[0]
    e = np.maximum(cand, 0)
    ok = (cand >= 0)[None] & (receivers[:, e] == np.arange(n)[None, :, None])
    return np.where(ok, senders[:, e], -1).astype(np.int32)


# ---- cases -------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    """One call of dgppo_gnn_attn_fwd / _bwd (entry "attn") or dgppo_gnn_layer_fwd ("layer").  mode: full | full_dx
    (full mode, the backward asked for dx) | raw (agent mode, D0 == D rows used directly) | pre (agent mode through
    pre_W / pre_b)."""
    key: str
    G: int
    n: int
    N: int
    C: int
    D: int
    F: int = 32
    H: int = 3
    D0: int = 0
    mode: str = "full"
    layout: str = "agent_first"
    hot: float = 0.0          # > 0: the largest |logit|
    sidx: bool = True
    qform: bool = False       # q with bk instead of beta
    pad: bool = False         # padded graph strides, [qt | beta] and [dqt | dbeta] sharing one buffer
    da_add: bool = True
    entry: str = "attn"
    otf: int = -1             # dgppo_gnn_set_graph_otf before the forward (-1: leave)
    outs: str = "all"         # layer: which outputs the call passes
    n_out: int = 0            # layer: the value tail's width (0: no tail)
    seed: int = 0

    @property
    def agent(self):
        return self.mode in ("raw", "pre")

    @property
    def Dx(self):  # row width of x
        return self.D0 if self.agent else self.D


def _q8(rng, shape):
    return (rng.integers(-16, 17, shape) / 8.0).astype(np.float32)


def _nrm(rng, shape, s=1.0):
    return (s * rng.standard_normal(shape)).astype(np.float32)


def make_inputs(c: Case):
    """float32 / int32 numpy inputs of a case (packed; the GPU file lays them out with the case's strides)."""
    g = make_graph(c.G, c.n, c.N, c.C, c.layout, seed=c.seed)
    rng = np.random.default_rng([7, c.seed, c.G, c.n, c.N, c.C, c.D, c.H])
    Rn, H, D, F = c.G * c.n, c.H, c.D, c.F
    d = dict(g)
    d["sidx"] = sender_table(g["cand"], g["receivers"], g["senders"])
    d["x"] = _q8(rng, (c.G, c.N, c.Dx))
    d["ef"] = _nrm(rng, (c.G, g["E"], 4))
    if c.agent:
        d["xa"] = _nrm(rng, (c.G, c.n, D))
    if c.mode == "pre":
        d["pre_W"], d["pre_b"] = _q8(rng, (c.D0, D)), _q8(rng, (D,))
        if c.seed == 1 and c.N > c.n:  # the structure cases: a wholly dead never-receiver row (exact zeros included)
            d["pre_b"] = -np.abs(d["pre_b"])
            d["x"][:, c.n] = 0.0
    d["scale"] = float(np.float32(1.0 / math.sqrt(F)))
    if c.entry == "layer":
        d["QBW"] = _nrm(rng, (D + 1, H * D + H), 0.5 / math.sqrt(D + 1))
        d["Wcat"] = _nrm(rng, (H * (D + 5), F), 1.0 / math.sqrt(D + 5))
        d["Wu"], d["bu"] = _nrm(rng, (D, F), 1.0 / math.sqrt(D)), _nrm(rng, (F,), 0.3)
        if c.n_out:
            t = {}
            for l in (0, 1):
                t[f"W{l}"], t[f"b{l}"] = _nrm(rng, (64, 64), 0.125), _nrm(rng, (64,), 0.1)
                t[f"ln{l}_s"], t[f"ln{l}_b"] = 1 + _nrm(rng, (64,), 0.1), _nrm(rng, (64,), 0.1)
            t["Wi"], t["bi"] = _nrm(rng, (64, 192), 0.125), _nrm(rng, (192,), 0.1)
            t["Wh"], t["bhn"] = _nrm(rng, (64, 192), 0.125), _nrm(rng, (64,), 0.1)
            t["Wo"], t["bo"] = _nrm(rng, (64, c.n_out), 0.125), _nrm(rng, (c.n_out,), 0.1)
            t["h_in"] = _nrm(rng, (Rn, 64), 0.5)
            d["tail"] = t
    else:
        d["qt"] = _nrm(rng, (Rn, H * D), 0.5)
        if c.qform:
            d["q"], d["bk"] = _nrm(rng, (Rn, H * F), 0.5), _nrm(rng, (H * F,), 0.5)
        else:
            d["beta"], d["bk"] = _nrm(rng, (Rn, H)), _nrm(rng, (H * F,), 0.5)
        d["dxcat"] = _nrm(rng, (Rn, H * (D + 5)))
        if c.da_add:
            d["da_add"] = _nrm(rng, (Rn, H, c.C))
        d["dx0"] = _q8(rng, (c.G, c.N, D)) if c.mode == "full_dx" else None   # prefill of the accumulating outputs
        d["dxa0"] = _q8(rng, (c.G, c.n, D)) if c.agent else None
    if c.hot and c.entry == "attn":  # scale the query side so that the largest |logit| is c.hot
        with torch.no_grad():
            lg = _logits(c, {k: _t(v, T64) for k, v in d.items() if isinstance(v, np.ndarray)}, d["scale"], T64)[0]
        f = np.float32(c.hot / max(float(lg.abs().max()), 1e-30)) if lg.numel() else np.float32(1)
        for k in ("qt", "q", "beta"):
            if k in d:
                d[k] = (d[k] * f).astype(np.float32)
    return d


# ---- the reference -------------------------------------------------------------------------------------------------------
def _t(a, dt):
    a = torch.as_tensor(np.asarray(a))
    return a.to(dt) if a.is_floating_point() else a.long()


def _features(c: Case, t, dt):
    """Sender features of every node (G, N, D)."""
    if not c.agent:
        return t["x"]
    raw = t["x"][:, c.n:]
    rest = torch.relu(raw @ t["pre_W"] + t["pre_b"]) if c.mode == "pre" else raw
    return torch.cat([t["xa"], rest], 1)


def _edges(c: Case, t):
    """The valid candidates as an edge list: graph, receiver, slot, receiver row, sender, edge id."""
    g, i, s = torch.nonzero(t["sidx"] >= 0, as_tuple=True)
    return g, i, s, g * c.n + i, t["sidx"][g, i, s], t["cand"][i, s]


def _logits(c: Case, t, scale, dt):
    g, i, s, seg, snd, e = _edges(c, t)
    xs = _features(c, t, dt)[g, snd]
    if torch.is_grad_enabled() and not xs.requires_grad:
        xs = xs.clone().requires_grad_(True)  # the backward asks for dL / d(each candidate's sender row)
    qt = t["qt"].reshape(c.G * c.n, c.H, c.D)
    beta = t["beta"] if "beta" in t else (t["q"].reshape(-1, c.H, c.F) * t["bk"].reshape(c.H, c.F)).sum(-1)
    return ((qt[seg] * xs[:, None, :]).sum(-1) + beta[seg]) * scale, xs


def _core(c: Case, t, scale, dt):
    """attn (Rn, H, C), xcat (Rn, H (D + 5)) and the per-edge pieces: oracle.nets_t.graph_transformer's softmax and
    aggregation over the valid candidates, with the value / edge / bias terms kept apart as [xbar | ebar | sig]."""
    Rn, H, D = c.G * c.n, c.H, c.D
    g, i, s, seg, snd, e = _edges(c, t)
    lg, xs = _logits(c, t, scale, dt)
    a = R.segment_softmax(lg, seg, Rn) if len(seg) else lg
    ef = t["ef"][g, e]
    z = lambda *sh: torch.zeros(sh, dtype=dt)  # noqa: E731
    xbar = z(Rn, H, D).index_add(0, seg, a[:, :, None] * xs[:, None, :])
    ebar = z(Rn, H, 4).index_add(0, seg, a[:, :, None] * ef[:, None, :])
    sig = z(Rn, H).index_add(0, seg, a)
    attn = z(Rn, H, c.C).index_put((seg[:, None], torch.arange(H)[None, :], s[:, None]), a)
    xcat = torch.cat([xbar.reshape(Rn, -1), ebar.reshape(Rn, -1), sig], 1)
    xmag = torch.cat([z(Rn, H, D).index_add(0, seg, a[:, :, None] * xs.abs()[:, None, :]).reshape(Rn, -1),
                      z(Rn, H, 4).index_add(0, seg, a[:, :, None] * ef.abs()[:, None, :]).reshape(Rn, -1), sig], 1)
    return attn, xcat, xmag, dict(seg=seg, a=a, xs=xs, ef=ef, g=g, snd=snd, slot=s)


def _tensors(c: Case, d, dt, grad=()):
    t = {}
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            t[k] = _t(v, dt)
            if k in grad:
                t[k].requires_grad_(True)
    return t


@torch.no_grad()
def attn_fwd(c: Case, d, dt=T64):
    t = _tensors(c, d, dt)
    attn, xcat, xmag, _ = _core(c, t, _scale(d, dt), dt)
    return dict(attn=attn, xcat=xcat, xcat_mag=xmag)


def _scale(d, dt):
    return torch.tensor(d["scale"], dtype=T32).to(dt)  # the float32 the kernel is handed, in the working precision


def attn_bwd(c: Case, d, dt=T64):
    """dqt, dbeta, dq, and dx (full_dx) or dxa with [dpre_W | dpre_b] (agent modes), by autograd; float64 also returns
    the magnitudes (`*_mag`)."""
    leaves = ["qt"] + (["x"] if c.mode == "full_dx" else []) + (["xa"] if c.agent else []) + \
        (["pre_W", "pre_b"] if c.mode == "pre" else [])
    t = _tensors(c, d, dt, grad=leaves + (["beta"] if "beta" in d else []))
    Rn, H, D, F = c.G * c.n, c.H, c.D, c.F
    if "beta" not in t:  # dL/d(q . bk) through a leaf of its own: dq = dbeta_h bk_h
        t["beta"] = (t["q"].reshape(-1, H, F) * t["bk"].reshape(H, F)).sum(-1).detach().requires_grad_(True)
    sc = _scale(d, dt)
    attn, xcat, _, e = _core(c, t, sc, dt)
    loss = (xcat * t["dxcat"]).sum()
    if "da_add" in t:
        loss = loss + (attn * t["da_add"]).sum()
    names = leaves + ["beta"]
    gr = torch.autograd.grad(loss, [t[k] for k in names] + [e["xs"]], allow_unused=True)
    per_edge = gr[-1]  # dL / d(the sender row as candidate (g, i, slot) reads it)
    gr = {k: (torch.zeros_like(t[k]) if v is None else v) for k, v in zip(names, gr)}
    out = dict(dqt=gr["qt"], dbeta=gr["beta"], dq=(gr["beta"][:, :, None] * t["bk"].reshape(H, F)).reshape(Rn, H * F))
    if c.mode == "full_dx":
        out["dx"] = gr["x"] + t["dx0"]
    if c.agent:
        out["dxa"] = gr["xa"] + t["dxa0"]
    if c.mode == "pre":
        out["dpre"] = torch.cat([gr["pre_W"].reshape(-1), gr["pre_b"]])
    if dt != T64:
        return out
    out["_edges"] = dict(g=e["g"], i=e["seg"] - e["g"] * c.n, slot=e["slot"], snd=e["snd"],
                         con=torch.zeros_like(e["xs"]) if per_edge is None else per_edge)
    # magnitudes: da = dxbar . x + debar . ef + dsig + da_add, dl = a (da - sum_c a da) scale, dqt = sum_c dl x,
    # dbeta = sum_c dl, sender gradient = sum_h a dxbar + dl qt, pre gradient = [x_raw | 1]^T (gate * sender gradient)
    with torch.no_grad():
        seg, a, xs, ef = e["seg"], e["a"], e["xs"].abs(), e["ef"].abs()
        gx = t["dxcat"].abs()
        dxbar, debar, dsig = gx[:, :H * D].reshape(Rn, H, D), gx[:, H * D:H * D + 4 * H].reshape(Rn, H, 4), gx[:, -H:]
        da = (dxbar[seg] * xs[:, None]).sum(-1) + (debar[seg] * ef[:, None]).sum(-1) + dsig[seg]
        if "da_add" in t:
            da = da + t["da_add"].abs()[seg, :, e["slot"]]
        dot = torch.zeros(Rn, H, dtype=dt).index_add(0, seg, a * da)
        dl = a * (da + dot[seg]) * sc
        qt = t["qt"].abs().reshape(Rn, H, D)
        out["dqt_mag"] = torch.zeros(Rn, H, D, dtype=dt).index_add(0, seg, dl[:, :, None] * xs[:, None]).reshape(Rn, -1)
        out["dbeta_mag"] = torch.zeros(Rn, H, dtype=dt).index_add(0, seg, dl)
        out["dq_mag"] = (out["dbeta_mag"][:, :, None] * t["bk"].abs().reshape(H, F)).reshape(Rn, H * F)
        con = (a[:, :, None] * dxbar[seg] + dl[:, :, None] * qt[seg]).sum(1)  # (edges, D)
        node = e["g"] * c.N + e["snd"]
        dnode = torch.zeros(c.G * c.N, D, dtype=dt).index_add(0, node, con).reshape(c.G, c.N, D)
        if c.mode == "full_dx":
            out["dx_mag"] = dnode + t["dx0"].abs()
        if c.agent:
            out["dxa_mag"] = dnode[:, :c.n] + t["dxa0"].abs()
        if c.mode == "pre":
            raw = t["x"].reshape(c.G * c.N, -1).abs()[node]
            gate = ((_features(c, t, dt).reshape(c.G * c.N, D)[node] > 0) & (e["snd"] >= c.n)[:, None]).to(dt)
            dz = con * gate
            out["dpre_mag"] = torch.cat([(raw.T @ dz).reshape(-1), dz.sum(0)])
    return out


@torch.no_grad()
def layer_fwd(c: Case, d, dt=T64):
    """qb = [x_i 1] QBW, attention as attn_fwd, Y = relu(xcat Wcat / H + x_i Wu + bu), zmean, the value tail."""
    t = _tensors(c, d, dt)
    Rn, H, D = c.G * c.n, c.H, c.D
    xi = (t["xa"] if c.agent else t["x"][:, :c.n]).reshape(Rn, D)
    qb = torch.cat([xi, torch.ones(Rn, 1, dtype=dt)], 1) @ t["QBW"]
    t["qt"], t["beta"] = qb[:, :H * D], qb[:, H * D:]
    attn, xcat, xmag, _ = _core(c, t, _scale(d, dt), dt)
    Y = torch.relu(xcat @ t["Wcat"] / H + xi @ t["Wu"] + t["bu"])
    Ymag = xmag @ t["Wcat"].abs() / H + xi.abs() @ t["Wu"].abs() + t["bu"].abs()
    out = dict(qb=qb, attn=attn, xcat=xcat, xcat_mag=xmag, Y=Y, zmean=Y.reshape(c.G, c.n, -1).mean(1),
               zmean_mag=Ymag.reshape(c.G, c.n, -1).mean(1))
    if c.n_out:
        w = {k: _t(v, dt) for k, v in d["tail"].items()}
        head = {f"Dense_{l}": dict(kernel=w[f"W{l}"], bias=w[f"b{l}"]) for l in (0, 1)}
        head.update({f"LayerNorm_{l}": dict(scale=w[f"ln{l}_s"], bias=w[f"ln{l}_b"]) for l in (0, 1)})
        gru = {}
        for j, gate in enumerate("rzn"):
            gru["i" + gate] = dict(kernel=w["Wi"][:, 64 * j:64 * j + 64], bias=w["bi"][64 * j:64 * j + 64])
            gru["h" + gate] = dict(kernel=w["Wh"][:, 64 * j:64 * j + 64])
        gru["hn"]["bias"] = w["bhn"]
        h2 = R.gru_cell(gru, w["h_in"], R.mlp_head(Y, head))
        out["tail"] = R.dense(h2, dict(kernel=w["Wo"], bias=w["bo"]))
    return out


def edge_wsum(attn, cand, sidx, efx, dt=T64):
    """out (Rn, H EX) = sum over the valid candidates of attn[r, h, c] efx[g, cand[i, c]]; and its magnitudes."""
    attn, efx, sidx, cand = _t(attn, dt), _t(efx, dt), _t(sidx, dt), _t(cand, dt)
    G, n, C = sidx.shape
    ex = efx[:, cand.clamp(min=0)]  # (G, n, C, EX)
    w = attn.reshape(G, n, -1, C) * (sidx >= 0)[:, :, None, :]
    out = torch.einsum("gnhc,gncj->gnhj", w, ex)
    return out.reshape(G * n, -1), torch.einsum("gnhc,gncj->gnhj", w.abs(), ex.abs()).reshape(G * n, -1)


def edge_da(dxx, cand, sidx, efx, H, dt=T64):
    """da_add (Rn, H, C) = dxx[r, h] . efx[g, cand[i, c]] on the valid candidates, else 0; and its magnitudes."""
    dxx, efx, sidx, cand = _t(dxx, dt), _t(efx, dt), _t(sidx, dt), _t(cand, dt)
    G, n, C = sidx.shape
    ex, ok = efx[:, cand.clamp(min=0)], (sidx >= 0)[:, :, None, :]
    gx = dxx.reshape(G, n, H, -1)
    z = torch.zeros((), dtype=dt)  # a masked candidate's entry is +0.0 exactly
    return (torch.where(ok, torch.einsum("gnhj,gncj->gnhc", gx, ex), z).reshape(G * n, H, C),
            torch.where(ok, torch.einsum("gnhj,gncj->gnhc", gx.abs(), ex.abs()), z).reshape(G * n, H, C))


# ---- comparison ------------------------------------------------------------------------------------------------------------
def _np(x):
    return x.detach().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


@dataclass
class Expect:
    """One output of a case: the float64 reference, the same statements in float32, the scale of the `close` rule
    (None: 1 + |ref64|) and the elements compared by bits instead (against float32(ref64))."""
    ref64: np.ndarray
    ref32: np.ndarray
    scale: object = None
    bits: object = None

    def scale_arr(self):
        return 1.0 + np.abs(self.ref64) if self.scale is None else np.asarray(self.scale, np.float64)

    def floor_excess(self):
        """Fraction of the elements whose floor term 8 |ref32 - ref64| passes 1e-3 of the scale."""
        fl = 8.0 * np.abs(self.ref32.astype(np.float64) - self.ref64)
        return float((fl > 1e-3 * self.scale_arr() + 1e-30).mean()) if fl.size else 0.0


def compare(got, ex: Expect, what=""):
    """The project's `close` rule (prim_ref.check_close) off the `bits` elements, int32 equality on them."""
    got = np.asarray(got)
    assert got.shape == ex.ref64.shape and got.dtype == np.float32, (what, got.shape, ex.ref64.shape, got.dtype)
    if ex.bits is None:
        return P.check_close(got, ex.ref64, ex.ref32, ex.scale_arr(), what=what)
    b = np.broadcast_to(ex.bits, got.shape)
    P.check_bits(got[b], ex.ref64.astype(np.float32)[b], what=what + " (bits)")
    return P.check_close(got[~b], ex.ref64[~b], ex.ref32[~b], ex.scale_arr()[~b], what=what)


def _zero_rows(d):
    return (d["sidx"] < 0).all(-1).reshape(-1)  # receivers with no valid candidate


def _expect(c, d, fn, spec):
    r64, r32 = fn(c, d, T64), fn(c, d, T32)
    zr = _zero_rows(d)
    out = {}
    for name, (mag, bits) in spec.items():
        if name not in r64:
            continue
        a64 = _np(r64[name])
        b = None
        if bits == "attn":
            b = (a64 == 0.0) | (a64 == 1.0)
        elif bits == "zero_rows":
            b = np.broadcast_to(zr[:, None], a64.shape)
        out[name] = Expect(a64, _np(r32[name]), None if mag is None else _np(r64[mag]), b)
    return out


@functools.lru_cache(maxsize=None)
def inputs(c: Case):
    return make_inputs(c)


@functools.lru_cache(maxsize=None)
def expected(c: Case, what: str):
    """{output name: Expect} of a case; what: fwd | bwd | layer.  Computed once per process and shared."""
    d = inputs(c)
    if what == "fwd":
        return _expect(c, d, attn_fwd, dict(attn=(None, "attn"), xcat=("xcat_mag", "zero_rows")))
    if what == "layer":
        return _expect(c, d, layer_fwd, dict(qb=(None, None), attn=(None, "attn"), xcat=("xcat_mag", "zero_rows"),
                                             Y=(None, None), zmean=("zmean_mag", None), tail=(None, None)))
    return _expect(c, d, attn_bwd, {k: (k + "_mag", None) for k in ("dqt", "dbeta", "dq", "dx", "dxa", "dpre")})


def bwd_attn_input(c: Case):
    return _np(attn_fwd(c, inputs(c), T64)["attn"]).astype(np.float32)


# ---- the GPU case table ----------------------------------------------------------------------------------------------------
def _pre(key, G, n, C, D0=5, D=32, F=64, extra_nodes=4, **kw):
    return Case(key, G, n, n + extra_nodes, C, D, F=F, D0=D0, mode="pre", **kw)


def _full(key, G, n, C, D=7, F=32, extra_nodes=4, **kw):
    return Case(key, G, n, n + extra_nodes, C, D, F=F, **kw)


def attn_cases():
    cs = []
    # rows per workgroup of the row-block pair: idle rows at n = 7 and 9, a partial last block, fewer graphs than
    # a block; n = 17: a 16-row block straddles graphs (the backward then takes a fallback)
    for n in (1, 2, 3, 5, 7, 8, 9, 16, 17):
        gpb = max(ROWS // n, 1)
        for G in sorted({1, gpb - 1, gpb, gpb + 1, 3 * gpb + 1} - {0}):
            cs.append(_pre(f"rows_pre_n{n}_G{G}", G, n, 6) if n % 2 else _full(f"rows_full_n{n}_G{G}", G, n, 6, D=5))
    # candidate widths
    for C in (1, 4, 5, 8, 9, 16, 17, 31, 32):
        cs.append(_full(f"C{C}_full", 7, 3, C, extra_nodes=max(4, C)))
        cs.append(_pre(f"C{C}_pre", 7, 3, C, extra_nodes=max(4, C)))
    # sender widths: full mode (DM 8), the DM 16 instantiations, raw rows, agent mode D0
    for D in (1, 3, 4, 5, 8, 10, 16):
        cs.append(_full(f"D{D}_full", 7, 3, 9, D=D))
    for D0 in (1, 5, 8):
        cs.append(_pre(f"D0{D0}_pre", 7, 3, 9, D0=D0))
    for D in (10, 12):  # pre_W narrower than the 32-wide instantiation it runs in
        cs.append(_pre(f"D{D}_pre", 7, 3, 9, D=D, F=32))
    for D in (4, 8):
        cs.append(Case(f"raw_D{D}", 7, 3, 7, 9, D, D0=D, mode="raw"))
    cs.append(Case("raw_D8_N_eq_n", 7, 3, 3, 5, 8, D0=8, mode="raw"))  # no never-receivers
    cs.append(_pre("pre_N_eq_n", 7, 3, 5, extra_nodes=0))
    # strides and the query form with q
    cs += [_pre("pad_pre", 5, 5, 9, pad=True), _full("pad_full", 5, 5, 9, pad=True),
           _pre("q_pre", 5, 5, 9, qform=True), _full("q_full", 5, 5, 9, qform=True, F=17),
           _full("noadd_full", 5, 5, 9, da_add=False)]
    # fallbacks: H in {1, 2} at every CP, no sender table, D = 40 (DM 64), full-mode dx (the block backward's image)
    for C in (4, 9, 24, 33):
        cs.append(_pre(f"h2_C{C}_pre", 5, 3, C, H=2, extra_nodes=max(4, C)))
        cs.append(_full(f"h2_C{C}_full", 5, 3, C, H=2, extra_nodes=max(4, C)))
    cs += [_full("h1_full", 5, 3, 9, H=1, qform=True), _pre("nosidx_pre", 5, 3, 9, sidx=False),
           _full("nosidx_full", 5, 3, 9, sidx=False), _pre("D40_pre", 5, 3, 9, D=40),
           _pre("D40_C72_pre", 3, 4, 72, D=40, extra_nodes=80, pad=True),  # backward past 64 KB of LDS
           Case("D40_full", 5, 3, 7, 9, 40, F=64)]
    for C in (8, 16, 32, 64, 72):
        cs.append(Case(f"dx_C{C}", 5, 3, 3 + max(C, 4), C, 7, mode="full_dx", pad=C == 16))
    cs.append(Case("dx_D32", 5, 3, 12, 9, 32, mode="full_dx"))
    # persistent grids: more blocks of graphs than workgroups (the caps are 768 / 1536 row-block, 256 for the D = 32
    # graph backward, 2048 block and wave), so a workgroup's LDS images and accumulators live through several blocks
    cs += [_pre("persist_2r_pre", 800, 16, 6), _full("persist_2r_full", 1600, 16, 6, D=5),
           _pre("persist_graph_pre", 300, 5, 36, extra_nodes=40),
           Case("persist_wave_raw", 8200, 8, 12, 6, 8, D0=8, mode="raw", H=2),
           Case("persist_block_dx", 4200, 16, 20, 6, 5, mode="full_dx", H=2)]
    # graph forms (C > 32): every row staged, the Spread layout with the receiver's own rows on the fly and staged,
    # the D <= 8 and D = 32 backward
    for C in (33, 36, 61):
        cs.append(_full(f"graph_C{C}_full", 3, 5, C, extra_nodes=C + 3))
        cs.append(_pre(f"graph_C{C}_pre", 3, 5, C, extra_nodes=C + 3))
    N, C = spread_shape(2, 30)  # 30 own rows per receiver: past the 16 on-the-fly slots, every row staged
    cs.append(Case("graph_spread_n2", 3, 2, N, C, 32, F=64, D0=5, mode="pre", layout="spread"))
    cs.append(Case("graph_spread_n2_full", 3, 2, N, C, 7, layout="spread"))
    N, C = spread_shape(9, 15)  # C = 33 with 15 own rows: the on-the-fly form, and the same call with it switched off
    for otf in (1, 0):
        cs.append(Case(f"graph_spread_otf{otf}", 2, 9, N, C, 32, F=64, D0=5, mode="pre", layout="spread", otf=otf))
    cs.append(Case("graph_raw", 3, 5, 45, 36, 8, D0=8, mode="raw"))
    # structure: the agent_first graph with every structure flag, and its hot variant, per family
    fam = dict(row_pre=_pre("", 7, 3, 9, extra_nodes=9), row_full=_full("", 7, 3, 9, extra_nodes=9),
               row16=_full("", 7, 3, 9, D=10, extra_nodes=9), block_wave_pre=_pre("", 7, 3, 9, H=2, extra_nodes=9),
               block_wave_full=_full("", 7, 3, 9, H=2, extra_nodes=9),
               block_dx=Case("", 7, 3, 12, 9, 7, mode="full_dx"),
               block_agent=_pre("", 3, 4, 72, D=40, extra_nodes=80),  # C > 64: the block backward in agent mode
               graph_pre=_pre("", 3, 5, 36, extra_nodes=40),
               graph_full=_full("", 3, 5, 36, extra_nodes=40))
    for name, c in fam.items():
        cs.append(replace(c, key=f"struct_{name}", seed=1))
        cs.append(replace(c, key=f"hot_{name}", seed=1, hot=60.0))
        for layout in ("free", "dup"):
            cs.append(replace(c, key=f"{layout}_{name}", layout=layout, seed=2))
    assert len({c.key for c in cs}) == len(cs)
    return cs


def layer_cases():
    cs = []
    L = lambda key, G, n, C, mode="full", **kw: (  # noqa: E731
        _pre(key, G, n, C, entry="layer", **kw) if mode == "pre" else _full(key, G, n, C, entry="layer", **kw))
    for n in (1, 2, 3, 5, 7, 8, 9, 16):
        gpb = ROWS // n
        for G in sorted({1, gpb - 1, gpb, gpb + 1, 3 * gpb + 1} - {0}):
            cs.append(L(f"layer_rows_n{n}_G{G}", G, n, 6, "full" if n % 2 else "pre", D=5 if n % 2 else 32))
    for C in (1, 4, 5, 8, 9, 16, 17, 31, 32):
        cs.append(L(f"layer_C{C}", 7, 3, C, "pre" if C % 2 else "full", extra_nodes=max(4, C)))
    for D in (1, 3, 4, 5, 8):
        cs.append(L(f"layer_D{D}", 7, 3, 9, D=D))
    for D0 in (1, 5, 8):
        cs.append(L(f"layer_D0{D0}", 7, 3, 9, "pre", D0=D0))
    for F in (1, 15, 16, 17, 33, 64):
        cs.append(L(f"layer_F{F}", 7, 3, 9, "pre" if F % 2 else "full", F=F))
    cs += [L("layer_pad_pre", 5, 5, 9, "pre", pad=True), L("layer_pad_full", 5, 5, 9, pad=True)]
    for outs in ("Y", "cache", "qb", "attn", "xcat"):  # against the full call's bits
        cs.append(L(f"layer_outs_{outs}", 7, 3, 9, "pre", outs=outs))
        cs.append(L(f"layer_outs_{outs}_full", 7, 3, 9, outs=outs))
    cs += [L("layer_zmean_n3", 7, 3, 9, F=33, outs="zmean"), L("layer_zmean_n5_pre", 7, 5, 9, "pre", F=17, outs="zmean"),
           L("layer_zmean_Y", 7, 7, 9, F=64, outs="zmean_Y")]
    for n_out in (1, 2, 16):
        cs.append(L(f"layer_tail_{n_out}", 7, 3, 9, F=64, outs="tail", n_out=n_out))
    for name, mode in (("pre", "pre"), ("full", "full")):
        cs.append(L(f"layer_struct_{name}", 7, 3, 9, mode, seed=1, extra_nodes=9))
        cs.append(L(f"layer_free_{name}", 7, 3, 9, mode, layout="free", seed=2, extra_nodes=9))
        cs.append(L(f"layer_dup_{name}", 7, 3, 9, mode, layout="dup", seed=2, extra_nodes=9))
    assert len({c.key for c in cs}) == len(cs)
    return cs


EDGE_CASES = [(G, n, C, H, EX) for EX in (1, 2, 7, 8, 9, 16) for (G, n, C, H) in ((7, 3, 9, 3),)] + \
    [(1, 1, 1, 1, 3), (40, 8, 17, 3, 6), (5, 5, 32, 2, 16)]


def edge_inputs(G, n, C, H, EX, seed=0):
    g = make_graph(G, n, n + 4, C, seed=seed)
    rng = np.random.default_rng([11, G, n, C, H, EX])
    g["sidx"] = sender_table(g["cand"], g["receivers"], g["senders"])
    g["efx"] = _nrm(rng, (G, g["E"], EX))
    g["attn"] = _nrm(rng, (G * n, H, C))  # arbitrary weights, nonzero on masked slots too: the mask must hold
    g["dxx"] = _nrm(rng, (G * n, H * EX))
    return g
