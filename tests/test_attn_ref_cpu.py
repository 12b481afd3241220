"""tests/attn_ref.py checked without a GPU, and the host side of the direct attention tests:

  * the per-edge reference agrees with oracle.nets_t.gnn (one layer in full mode, two layers with the second in agent
    mode) at float64 round-off, and the generator keeps every index in range and builds the structure it promises;
  * the comparator of tests/test_attn_direct_gpu.py rejects a list of wrong results, each a stand-in for a kernel
    mistake, applied to the reference's own output;
  * the GPU case table, evaluated through dgppo_gnn_attn_plan, reaches every (family, direction) and instantiation
    the plan can return at default knobs, less the keys of tests/golden/attn_direct_uncovered.json, whose list of
    outputs that are not compared names only sender gradients of `free` / `dup` cases;
  * the floor term of the `close` rule stays small in every case (it cannot hide a failure);
  * dgppo_gnn_layer_supported and dgppo_gnn_attn_plan refuse exactly at their documented bounds."""
import ctypes
import json
import math
import os

import numpy as np
import pytest
import torch

import attn_ref as A
import test_attn_direct_gpu as T
from dgppo_fov_amd import _lib
from oracle import nets_t as R

HERE = os.path.dirname(os.path.abspath(__file__))
CPU = torch.device("cpu")
FAKE = 0x1000
ALL = list(T.ATTN_CASES.values()) + list(T.LAYER_CASES.values())


# ---- the generator -----------------------------------------------------------------------------------------------------
def test_every_index_is_in_range_and_the_sender_table_is_the_plain_loop():
    for c in ALL:
        d = A.inputs(c)
        E = d["E"]
        assert d["cand"].shape == (c.n, c.C) and d["cand"].min() >= -1 and d["cand"].max() < E, c.key
        assert d["senders"].shape == (c.G, E) and d["senders"].min() >= 0 and d["senders"].max() < c.N, c.key
        assert d["receivers"].min() >= 0 and d["receivers"].max() <= c.N, c.key
        assert d["sidx"].min() >= -1 and d["sidx"].max() < c.N, c.key
        if c.G * c.n * c.C <= 400:  # the vectorised table against the header's sentence, literally
            for g in range(c.G):
                for i in range(c.n):
                    for s in range(c.C):
                        e = d["cand"][i, s]
                        want = d["senders"][g, e] if e >= 0 and d["receivers"][g, e] == i else -1
                        assert d["sidx"][g, i, s] == want, (c.key, g, i, s)
        if c.layout in ("agent_first", "spread"):  # the env contract: slot c < n holds agent c, senders distinct
            s = d["sidx"]
            for slot in range(c.C):
                ok = s[:, :, slot] >= 0
                assert (s[:, :, slot][ok] == slot).all() if slot < c.n else (s[:, :, slot][ok] >= c.n).all(), c.key
        if c.layout != "dup":
            s = np.sort(d["sidx"], -1)
            assert not ((s[..., 1:] == s[..., :-1]) & (s[..., 1:] >= 0)).any(), c.key
        if c.layout == "spread" and c.otf != 0:  # at most C - 2n senders past the 2n shared rows per receiver
            assert ((d["sidx"] >= 2 * c.n).sum(-1) <= c.C - 2 * c.n).all()


def test_structure_cases_hold_every_structure_at_once():
    want = {"zero", "one", "all", "recv_mismatch", "cand_neg", "self_edge", "unnamed_edges", "sends_to_all"}
    for c in ALL:
        d = A.inputs(c)
        if "struct_" in c.key or c.key.startswith("hot_"):
            assert want <= d["flags"], (c.key, want - d["flags"])
            nv = (d["sidx"] >= 0).sum(-1)
            assert (nv == 0).any() and (nv == 1).any() and (nv == c.C).any(), c.key
            assert (d["sidx"][-1, :, 0] == 0).all(), c.key  # agent 0 sends to every receiver of the last graph
        if c.layout == "dup":
            assert {"dup_agent", "dup_other"} <= d["flags"], c.key
    # one valid candidate: weight exactly 1.0 in both precisions
    c = T.ATTN_CASES["struct_row_pre"]
    ex = A.expected(c, "fwd")["attn"]
    one = ((A.inputs(c)["sidx"] >= 0).sum(-1) == 1).reshape(-1)
    assert one.any() and (ex.ref64[one].sum(-1) == 1.0).all() and (ex.ref32[one].max(-1) == 1.0).all()
    assert any(c.N == c.n and c.agent for c in ALL)  # agent mode without never-receivers


# ---- agreement with the oracle ---------------------------------------------------------------------------------------------
def _flax_layer(rng, Din, F, H=3, edge=4):
    w = lambda *s: torch.tensor(rng.standard_normal(s) / np.sqrt(s[0]), dtype=A.T64)  # noqa: E731
    b = lambda k: torch.tensor(0.2 * rng.standard_normal(k), dtype=A.T64)  # noqa: E731
    p = {f"Dense_{j}": dict(kernel=w(Din, H * F), bias=b(H * F)) for j in range(3)}
    p["Dense_3"] = dict(kernel=w(edge, H * F))
    p["Dense_4"] = dict(kernel=w(Din, F), bias=b(F))
    return p


def _abi_weights(p, Din, F, H=3):
    """QBW, Wcat, Wu, bu of a flax layer (include/dgppo_hip.h: qt_h = Wk_h q_h, beta_h = q_h . bk_h)."""
    k = lambda j: p[f"Dense_{j}"]["kernel"].reshape(-1, H, F)  # noqa: E731
    bias = lambda j: p[f"Dense_{j}"]["bias"].reshape(H, F)  # noqa: E731
    Wq, Wk, Wv, We = k(0), k(1), k(2), k(3)
    QBW = torch.zeros(Din + 1, H * Din + H, dtype=A.T64)
    for h in range(H):
        QBW[:Din, h * Din:(h + 1) * Din] = Wq[:, h] @ Wk[:, h].T
        QBW[Din, h * Din:(h + 1) * Din] = bias(0)[h] @ Wk[:, h].T
        QBW[:Din, H * Din + h] = Wq[:, h] @ bias(1)[h]
        QBW[Din, H * Din + h] = bias(0)[h] @ bias(1)[h]
    Wcat = torch.cat([Wv[:, h] for h in range(H)] + [We[:, h] for h in range(H)] + [bias(2)])
    return dict(QBW=QBW, Wcat=Wcat, Wu=p["Dense_4"]["kernel"], bu=p["Dense_4"]["bias"])


@pytest.mark.parametrize("G,n,N,C,D0", [(3, 3, 9, 9, 5), (2, 5, 8, 6, 7), (4, 1, 4, 4, 3), (2, 4, 4, 4, 8)])
def test_reference_agrees_with_the_oracle_gnn(G, n, N, C, D0):
    rng = np.random.default_rng(G + 10 * n)
    g = A.make_graph(G, n, N, C, seed=3, named=True)
    x = rng.standard_normal((G, N, D0))
    ef = rng.standard_normal((G, g["E"], 4))
    # the oracle's graph: one more node, the pad the masked edges point at
    graph = dict(nodes=np.concatenate([x, np.zeros((G, 1, D0))], 1), edges=ef, receivers=g["receivers"],
                 senders=g["senders"])
    l1, l2 = _flax_layer(rng, D0, 32), _flax_layer(rng, 32, 64)
    base = dict(g, sidx=A.sender_table(g["cand"], g["receivers"], g["senders"]), ef=ef, scale=0.0)

    def run(c, d, p, F, monkey=A):
        d = dict(d, **{k: v.numpy() for k, v in _abi_weights(p, c.D, F).items()})
        real = monkey._scale
        monkey._scale = lambda d_, dt: torch.tensor(1.0 / math.sqrt(F), dtype=dt)  # the oracle's float64 scale
        try:
            return monkey.layer_fwd(c, d, A.T64)["Y"].reshape(G, n, F)
        finally:
            monkey._scale = real

    def close(a, b, what):
        err = (a - b).abs().max().item() / (1.0 + b.abs().max().item())
        assert err <= 1e-12, (what, err)

    # one layer, full mode: out_dim 32
    c1 = A.Case("oracle1", G, n, N, C, D0, F=32, entry="layer")
    Y1 = run(c1, dict(base, x=x), l1, 32)
    close(Y1, R.gnn([l1], graph, n, out_dim=32), "one layer")
    # two layers: the second in agent mode, its never-receivers through the first layer's Dense_4
    c2 = A.Case("oracle2", G, n, N, C, 32, F=64, D0=D0, mode="pre", entry="layer")
    d2 = dict(base, x=x, xa=Y1.numpy(), pre_W=l1["Dense_4"]["kernel"].numpy(), pre_b=l1["Dense_4"]["bias"].numpy())
    close(run(c2, d2, l2, 64), R.gnn([l1, l2], graph, n, out_dim=64, msg_dim=32), "two layers")


# ---- control inputs: the comparator must reject each -------------------------------------------------------------------------
def _rejects(got, ex, what):
    with pytest.raises(AssertionError):
        A.compare(np.asarray(got, np.float32), ex, what)


def _accepts_itself(ex):
    A.compare(ex.ref64.astype(np.float32), ex, "the reference itself")


def test_comparator_rejects_wrong_forward_results():
    c = T.ATTN_CASES["struct_row_pre"]
    d, ex = A.inputs(c), A.expected(c, "fwd")
    _accepts_itself(ex["attn"]), _accepts_itself(ex["xcat"])
    valid = (d["sidx"] >= 0).reshape(-1, 1, c.C)
    nv = valid.sum(-1, keepdims=True)
    attn = ex["attn"].ref64
    _rejects(attn * nv / c.C, ex["attn"], "softmax normalised over C instead of the valid set")
    _rejects(np.where(valid, attn, 1e-3), ex["attn"], "a masked candidate keeps a weight")
    x = ex["xcat"].ref64.copy()
    x[:, -c.H:] = 0.0
    _rejects(x, ex["xcat"], "sig dropped")
    x = ex["xcat"].ref64.copy()
    zr = (nv.reshape(-1) == 0)
    x[zr] = 1e-30
    _rejects(x, ex["xcat"], "a zero-in-degree row that is not exactly zero")
    # the layer: 1 / H of the message missing, a zero-in-degree row's Y left at a zero prefill
    c = T.LAYER_CASES["layer_struct_pre"]
    d, ex = A.inputs(c), A.expected(c, "layer")
    _accepts_itself(ex["Y"])
    t = A._tensors(c, d, A.T64)
    xi = t["xa"].reshape(-1, c.D)
    xcat = torch.tensor(ex["xcat"].ref64)
    _rejects(torch.relu(xcat @ t["Wcat"] + xi @ t["Wu"] + t["bu"]).numpy(), ex["Y"], "1 / H of the message missing")
    Y = ex["Y"].ref64.copy()
    zr = ((d["sidx"] >= 0).sum(-1) == 0).reshape(-1)
    assert zr.any() and np.abs(Y[zr]).max() > 0.1
    Y[zr] = 0.0
    _rejects(Y, ex["Y"], "a zero-in-degree row's Y left at the prefill")


def _image_sum(c, d, ed, by_slot):
    """dxa from an image indexed by (receiver, agent) with a plain store, as a kernel that assumes distinct senders
    (by_slot False: the last of two candidates with one sender wins) or that slot c holds agent c (by_slot True:
    a slot < n is credited to agent `slot`, an agent sender in a slot >= n is dropped) would compute it."""
    img = np.zeros((c.G, c.n, c.n, c.D))
    con = ed["con"].numpy()
    for g, i, slot, snd, v in zip(ed["g"].tolist(), ed["i"].tolist(), ed["slot"].tolist(), ed["snd"].tolist(), con):
        if by_slot:
            if slot < c.n and snd < c.n:
                img[g, i, slot] = v
        elif snd < c.n:
            img[g, i, snd] = v
    return d["dxa0"] + img.sum(1)


def test_comparator_rejects_wrong_backward_results():
    c = T.ATTN_CASES["struct_row_pre"]
    d, ex = A.inputs(c), A.expected(c, "bwd")
    for k in ex:
        _accepts_itself(ex[k])
    _rejects(ex["dxa"].ref64 - d["dxa0"], ex["dxa"], "dxa overwritten instead of accumulated")
    c = T.ATTN_CASES["struct_block_dx"]
    d, ex = A.inputs(c), A.expected(c, "bwd")
    _rejects(ex["dx"].ref64 - d["dx0"], ex["dx"], "dx overwritten instead of accumulated")
    # on an agent_first graph both image forms are the reference; `dup` sees the last writer, `free` the slot index
    for key, by_slot, same in (("struct_row_pre", False, True), ("struct_row_pre", True, True),
                               ("dup_row_pre", False, False), ("free_row_pre", True, False),
                               ("free_row_pre", False, True)):
        c = T.ATTN_CASES[key]
        d, ex = A.inputs(c), A.expected(c, "bwd")
        got = _image_sum(c, d, A.attn_bwd(c, d)["_edges"], by_slot)
        if same:
            A.compare(got.astype(np.float32), ex["dxa"], f"{key} image sum")
        else:
            _rejects(got, ex["dxa"], f"{key} image sum")


# ---- the floor of the close rule ------------------------------------------------------------------------------------------
def test_floor_term_is_small_in_every_case():
    """8 |ref32 - ref64| may pass 1e-3 of the scale on at most 1 % of a case's elements."""
    for c in ALL:
        for what in (("layer",) if c.entry == "layer" else ("fwd", "bwd")):
            for name, ex in A.expected(c, what).items():
                assert np.isfinite(ex.ref64).all() and np.isfinite(ex.ref32).all(), (c.key, name)
                assert ex.floor_excess() <= 0.01, (c.key, what, name, ex.floor_excess())
    for G, n, C, H, EX in A.EDGE_CASES:
        d = A.edge_inputs(G, n, C, H, EX)
        for fn, args in ((A.edge_wsum, (d["attn"],)), (A.edge_da, (d["dxx"],))):
            tail = (d["cand"], d["sidx"], d["efx"]) + ((H,) if fn is A.edge_da else ())
            r64, mag = fn(*args, *tail)
            r32, _ = fn(*args, *tail, dt=A.T32)
            assert A.Expect(r64.numpy(), r32.numpy(), mag.numpy()).floor_excess() <= 0.01


# ---- coverage through the plan ----------------------------------------------------------------------------------------------
REQUIRED = {"fwd:FWD2R:dm8", "fwd:FWD2R:dm16", "fwd:FWD2R:dm32", "bwd:BWD2R:dm8", "bwd:BWD2R:dm16", "bwd:BWD2R:dm32",
            "fwd:GRAPH_FWD:dm8", "fwd:GRAPH_FWD:dm32", "fwd:GRAPH_FWD:dm32:slots>0", "fwd:GRAPH_FWD:dm32:slots=0",
            "bwd:GRAPH_BWD:dm8", "bwd:GRAPH_BWD32:dm32", "bwd:GRAPH_BWD32:N>n", "fwd:BLOCK", "bwd:BLOCK",
            "bwd:WAVE:cp8", "bwd:WAVE:cp16", "bwd:WAVE:cp32", "bwd:WAVE:cp64", "bwd:lds>64K",
            "fwd:BLOCK:dm8", "fwd:BLOCK:dm32", "fwd:BLOCK:dm64", "bwd:BLOCK:dm8", "bwd:BLOCK:dm32", "bwd:BLOCK:dm64",
            "bwd:WAVE:dm8", "bwd:WAVE:dm32", "bwd:WAVE:dm64", "bwd:BLOCK:full_dx", "bwd:BLOCK:agent",
            # a grid below the work items: the persistent loops run more than once per workgroup
            "bwd:BWD2R:persistent", "bwd:GRAPH_BWD32:persistent", "bwd:WAVE:persistent", "bwd:BLOCK:persistent",
            "fwd:BLOCK:persistent"}


def _plans(c):
    """(forward plan, backward plan, dpre_part rows) of a case, through the structs the GPU test launches from."""
    lib = _lib.load()
    d = A.inputs(c)
    a, keep = T.attn_struct(c, d, CPU)
    o = T.bwd_outputs(c, d, CPU, a)
    pf, pb = _lib.GnnAttnPlan(), _lib.GnnAttnPlan()
    if c.otf >= 0:
        lib.dgppo_gnn_set_graph_otf(c.otf)
    try:
        assert lib.dgppo_gnn_attn_plan(ctypes.byref(a), 0, ctypes.byref(pf)) == 0, c.key
        assert lib.dgppo_gnn_attn_plan(ctypes.byref(a), 1, ctypes.byref(pb)) == 0, c.key
        rows = lib.dgppo_gnn_attn_partial_blocks(ctypes.byref(a))
    finally:
        if c.otf >= 0:
            lib.dgppo_gnn_set_graph_otf(1)
    return pf, pb, rows


def test_case_table_reaches_every_family_the_plan_can_return():
    unc = json.load(open(os.path.join(HERE, "golden", "attn_direct_uncovered.json")))
    reached, by_family = set(), {}
    for c in T.ATTN_CASES.values():
        pf, pb, rows = _plans(c)
        assert rows == pb.grid >= 1, c.key
        for dr, pl in (("fwd", pf), ("bwd", pb)):
            fam = pl.family_name
            by_family.setdefault((dr, fam, c.layout), []).append(c.key)
            reached |= {f"{dr}:{fam}", f"{dr}:{fam}:dm{pl.dm}"}
            if fam in ("BLOCK", "WAVE"):
                reached.add(f"{dr}:{fam}:cp{pl.cp}")
            if fam == "GRAPH_FWD":
                reached.add(f"{dr}:{fam}:dm{pl.dm}:slots{'>0' if pl.slots > 0 else '=0'}")
            if fam == "GRAPH_BWD32" and c.N > c.n:
                reached.add("bwd:GRAPH_BWD32:N>n")
            if dr == "bwd" and pl.lds_bytes > 64 * 1024:
                reached.add("bwd:lds>64K")
            if pl.grid < (-(-pl.nblk // 4) if fam == "WAVE" else pl.nblk):
                reached.add(f"{dr}:{fam}:persistent")
            if dr == "bwd" and fam == "BLOCK":
                reached.add("bwd:BLOCK:full_dx" if c.mode == "full_dx" else "bwd:BLOCK:agent")
    # the recorded list is exactly what the table misses, each entry with its reason
    assert all(v for v in unc["plan_keys"].values())
    assert set(unc["plan_keys"]) == REQUIRED - reached, (sorted(REQUIRED - reached - set(unc["plan_keys"])),
                                                          sorted(set(unc["plan_keys"]) - (REQUIRED - reached)))
    # every family runs the structure case, its hot variant and both other layouts, forward and backward
    fams = {(dr, fam) for dr, fam, _ in by_family}
    for dr, fam in fams:
        for layout in ("agent_first", "free", "dup"):
            assert (dr, fam, layout) in by_family, (dr, fam, layout)
        keys = by_family[(dr, fam, "agent_first")]
        assert any(k.startswith("struct_") for k in keys) and any(k.startswith("hot_") for k in keys), (dr, fam)
    # the outputs not compared: sender gradients only, of cases that break the documented precondition on purpose,
    # under the family the plan names, each with its reason
    for u in unc["cases"]:
        c = T.ATTN_CASES[u["case"]]
        assert u["reason"] and u["direction"] == "bwd" and set(u["outputs"]) <= {"dx", "dxa"} and u["outputs"], u
        assert c.layout in ("free", "dup") and u["layout"] == c.layout, u
        assert u["family"] == _plans(c)[1].family_name, u


# ---- host-only refusals ---------------------------------------------------------------------------------------------------
def _layer(n=8, N=24, C=24, D=7, F=32, agent=False, D0=7, Y=True, **kw):
    la = _lib.GnnLayerArgs()
    a = la.a
    a.G, a.N, a.E, a.n_agents, a.D, a.F, a.H, a.C, a.D0 = 4, N, n * C, n, D, F, 3, C, D0
    for f in ("cand", "receivers", "senders", "x", "ef", "sidx"):
        setattr(a, f, FAKE)
    a.x_gstride, a.ef_gstride = N * (D0 if agent else D), n * C * 4
    if agent:
        a.xa, a.pre_W, a.pre_b, a.xa_gstride = FAKE, FAKE, FAKE, n * D
    la.QBW = la.Wcat = la.Wu = la.bu = FAKE
    if Y:
        la.Y = FAKE
    for k, v in kw.items():
        if k == "tail":
            for f, _ in _lib.GnnValueTail._fields_:
                if f not in ("n_out", "on"):
                    setattr(la.tail, f, FAKE)
            la.tail.on, la.tail.n_out = 1, v
        elif hasattr(a, k):
            setattr(a, k, v)
        else:
            setattr(la, k, v)
    return la


def _ok(la):
    return bool(_lib.load().dgppo_gnn_layer_supported(ctypes.byref(la)))


def _lds_floats(n, N, agent, ytile=False, tail=False):
    """The layer kernel's LDS floats from the layout in csrc/gnn_layer.hip's comments: staged node rows, the larger
    of the raw rows and the 16-row xcat tile, 16 [qt | beta] rows, pre_W / pre_b, the Y tile, the tail's carries."""
    gpb = 16 // n
    XP, QP, XCP = (36, 100, 132) if agent else (12, 28, 44)
    r4 = lambda v: (v + 3) // 4 * 4  # noqa: E731
    o = r4(gpb * N * XP) + r4(max(gpb * N * 8 if agent else 0, 16 * XCP)) + 16 * QP + (8 * 32 + 32 if agent else 0)
    if (ytile or tail) and XCP < 68:
        o += 16 * 68
    return o + (16 * 68 + 256 if tail else 0)


def test_layer_supported_refuses_at_its_bounds():
    assert _ok(_layer()) and _ok(_layer(agent=True, D=32)) and _ok(_layer(F=64, D=7, Y=False, tail=2))
    assert _ok(_layer(n=16, N=20, C=4)) and not _ok(_layer(n=17, N=20, C=4))
    assert _ok(_layer(C=32)) and not _ok(_layer(C=33))
    assert _ok(_layer(D=8)) and not _ok(_layer(D=9))
    assert not _ok(_layer(agent=True, D=31)) and not _ok(_layer(agent=True, D=33))
    assert _ok(_layer(agent=True, D=32, D0=8)) and not _ok(_layer(agent=True, D=32, D0=9))
    assert not _ok(_layer(agent=True, D=32, D0=0))
    assert _ok(_layer(F=64)) and not _ok(_layer(F=65)) and not _ok(_layer(F=0))
    assert not _ok(_layer(H=2)) and not _ok(_layer(sidx=0)) and not _ok(_layer(Y=False))
    assert not _ok(_layer(ef_gstride=8 * 24 * 4 + 2)) and _ok(_layer(ef_gstride=8 * 24 * 4 + 4))
    assert not _ok(_layer(agent=True, D=32, xa_gstride=8 * 32 + 2)) and _ok(_layer(agent=True, D=32, xa_gstride=8 * 32 + 4))
    assert not _ok(_layer(ef=FAKE + 4)) and not _ok(_layer(agent=True, D=32, xa=FAKE + 8))
    # the tail: F = 64 only, n_out 1 .. 16, full mode, and no other output
    assert not _ok(_layer(F=32, Y=False, tail=2))
    assert _ok(_layer(F=64, Y=False, tail=16)) and not _ok(_layer(F=64, Y=False, tail=17))
    assert not _ok(_layer(F=64, Y=False, tail=0)) and not _ok(_layer(F=64, Y=False, tail=2, agent=True, D=32))
    for extra in (dict(Y=True), dict(qb=FAKE), dict(attn=FAKE), dict(xcat=FAKE), dict(zmean=FAKE)):
        kw = dict(dict(F=64, Y=False, tail=2), **extra)
        assert not _ok(_layer(**kw)), extra
    assert _ok(_layer(Y=False, zmean=FAKE)) and _ok(_layer(zmean=FAKE))
    # 64 KB of LDS: the largest N that fits and the first that does not
    for n in (1, 8, 16):
        for agent, kw in ((False, {}), (True, dict(agent=True, D=32)), (False, dict(zmean=FAKE))):
            fits = [N for N in range(n, 6000) if 4 * _lds_floats(n, N, agent, ytile="zmean" in kw) <= 64 * 1024]
            assert fits and fits[-1] - fits[0] + 1 == len(fits)
            Nmax = fits[-1]
            assert _ok(_layer(n=n, N=Nmax, C=4, **kw)), (n, agent, Nmax)
            assert not _ok(_layer(n=n, N=Nmax + 1, C=4, **kw)), (n, agent, Nmax)
    assert not _ok(_layer(n=8, N=7, C=4))  # fewer nodes than agents


def test_attn_plan_refuses_what_valid_refuses():
    lib = _lib.load()
    c = T.ATTN_CASES["struct_row_pre"]

    def rc(**kw):
        a, keep = T.attn_struct(c, A.inputs(c), CPU)
        for k, v in kw.items():
            setattr(a, k, v)
        pl = _lib.GnnAttnPlan()
        r = lib.dgppo_gnn_attn_plan(ctypes.byref(a), 0, ctypes.byref(pl))
        assert (r == 0) == (pl.family >= 0)
        return r

    assert rc() == 0
    for kw in (dict(H=0), dict(H=4), dict(D=0), dict(D=65), dict(F=0), dict(F=65), dict(C=0), dict(C=129),
               dict(n_agents=0), dict(x=None), dict(ef=None), dict(qt=None), dict(bk=None), dict(cand=None),
               dict(receivers=None), dict(senders=None), dict(beta=None), dict(beta_ld=2), dict(qt_ld=95),
               dict(dqt_ld=95), dict(dbeta_ld=2), dict(D0=0), dict(D0=9), dict(pre_b=None),
               dict(pre_W=None)):  # pre_W None with D0 != D
        assert rc(**kw) == _lib.DGPPO_EINVAL, kw
    assert rc(qt_ld=96) == 0 and rc(dqt_ld=96, dbeta_ld=3) == 0 and rc(D=64, pre_W=None, pre_b=None, D0=64) != 0
