"""The GraphTransformer kernels of csrc/attn.hip and csrc/gnn_layer.hip, called directly through the C ABI on
synthetic graphs and held to the float64 per-edge reference of tests/attn_ref.py: the sender table, the attention
forward and backward of every family the dispatch can choose, the fused layer with its zmean and value-tail
epilogues, edge_wsum and edge_da.

The env graphs of the other attention tests never vary along the axes these cases walk: receivers without in-edges,
with exactly one and with all C, candidates masked by another receiver and by cand == -1, self edges, edges no
candidate names, slot orders other than the envs' (`free`), repeated senders (`dup`), N == n, every row count around
the 16-row workgroup, every candidate and feature width around the tiles, padded strides and the shared
[qt | beta] / [dqt | dbeta] buffers.  Every output sits between guard words that must come back untouched, the row
pads of strided outputs included; accumulating outputs (dx, dxa) start from nonzero values; input pads hold NaN.

Comparison: attn_ref.compare (the `close` rule of tests/prim_ref.py, bits for the sender table, for weights that are
exactly 0 or 1 and for the rows of receivers without in-edges).  Which kernel a case runs is not asked here:
tests/test_attn_ref_cpu.py evaluates this table through dgppo_gnn_attn_plan on the CPU.  tests/golden/
attn_direct_uncovered.json lists, per (case, direction), the outputs that are not compared because the kernel family
needs a documented precondition of the candidate table (include/dgppo_hip.h) that the case breaks on purpose; the
case still runs and everything else it writes is compared."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import attn_ref as A
from dgppo_fov_amd import _lib, ops
from dgppo_fov_amd.nn import kernels as K

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
UNCOVERED = json.load(open(os.path.join(HERE, "golden", "attn_direct_uncovered.json")))
NOT_COMPARED = {(u["case"], u["direction"]): set(u["outputs"]) for u in UNCOVERED["cases"]}
ATTN_CASES = {c.key: c for c in A.attn_cases()}
LAYER_CASES = {c.key: c for c in A.layer_cases()}
GUARD, SENT = 64, 0x7FC0DEAD  # guard words on both sides of an output; the sentinel is a NaN as a float


class Buf:
    """(rows, width) float32 output with row stride ld inside guard words; the row pads are guards as well."""

    def __init__(self, dev, rows, width, ld=0, init=None, dtype=torch.float32):
        self.rows, self.width, self.ld = rows, width, ld or width
        self.flat = torch.full((2 * GUARD + rows * self.ld,), SENT, dtype=torch.int32, device=dev)
        body = self.flat[GUARD:GUARD + rows * self.ld].view(dtype).view(rows, self.ld)
        self.t = body[:, :width]
        if init is not None:
            self.t.copy_(torch.as_tensor(np.asarray(init).reshape(rows, width)))

    def read(self, what, dtype=np.float32):
        h = self.flat.cpu().numpy()
        body = h[GUARD:len(h) - GUARD].reshape(self.rows, self.ld)
        assert (h[:GUARD] == SENT).all() and (h[len(h) - GUARD:] == SENT).all(), f"{what}: guard words overwritten"
        assert (body[:, self.width:] == SENT).all(), f"{what}: row pad overwritten"
        return np.ascontiguousarray(body[:, :self.width]).view(dtype)


def _in(dev, a, ld=0):
    """A (rows, width) input on the device with row stride ld; the pad holds NaN."""
    a = np.asarray(a)
    a = a.reshape(a.shape[0], -1)
    if not ld or ld == a.shape[1]:
        return torch.as_tensor(a).to(dev).contiguous()
    t = torch.full((a.shape[0], ld), float("nan"), dtype=torch.float32, device=dev)
    t[:, :a.shape[1]] = torch.as_tensor(a)
    return t[:, :a.shape[1]]


def graph_tensors(c, d, dev, sidx=None):
    """The graph and sender-feature arguments of a case on `dev` (CPU tensors serve the plan queries)."""
    p = c.pad
    t = dict(cand=_in(dev, d["cand"]), receivers=_in(dev, d["receivers"]), senders=_in(dev, d["senders"]))
    t["sidx"] = None if not c.sidx else (_in(dev, d["sidx"].reshape(c.G * c.n, c.C)) if sidx is None else sidx)
    t["x_gstride"], t["ef_gstride"] = c.N * c.Dx + 3 * p, d["E"] * 4 + 8 * p
    t["x"], t["ef"] = _in(dev, d["x"], t["x_gstride"]), _in(dev, d["ef"], t["ef_gstride"])
    t["xa"], t["xa_gstride"], t["pre_W"], t["pre_b"] = None, 0, None, None
    if c.agent:
        t["xa_gstride"] = c.n * c.D + 4 * p
        t["xa"] = _in(dev, d["xa"], t["xa_gstride"])
    if c.mode == "pre":
        t["pre_W"], t["pre_b"] = _in(dev, d["pre_W"]), _in(dev, d["pre_b"][None])
    return t


def attn_struct(c, d, dev, sidx=None):
    """dgppo_gnn_attn_args of a case (inputs only) and the tensors it points into."""
    t = graph_tensors(c, d, dev, sidx)
    Rn, H, D = c.G * c.n, c.H, c.D
    t["bk"] = _in(dev, d["bk"][None])
    t["q"], t["beta"], t["beta_ld"], t["qt_ld"] = None, None, 0, 0
    if c.qform:
        t["q"], t["qt"] = _in(dev, d["q"]), _in(dev, d["qt"], (H * D + 2) * c.pad)
        t["qt_ld"] = (H * D + 2) * c.pad
    elif c.pad:  # [qt | beta] in one buffer
        ld = H * D + H + 2
        qb = _in(dev, np.concatenate([d["qt"], d["beta"]], 1), ld)
        t["qb"], t["qt"], t["beta"], t["qt_ld"], t["beta_ld"] = qb, qb[:, :H * D], qb[:, H * D:], ld, ld
    else:
        t["qt"], t["beta"], t["beta_ld"] = _in(dev, d["qt"]), _in(dev, d["beta"]), H
    a = ops._attn_struct([c.G, c.N, d["E"], c.n, D, c.F, H, c.C, c.D0], t["cand"], t["receivers"], t["senders"],
                         t["sidx"], t["x"], t["x_gstride"], t["ef"], t["ef_gstride"], t["q"], t["qt"], t["bk"],
                         d["scale"], t["xa"], t["xa_gstride"], t["pre_W"], t["pre_b"], t["beta"], t["beta_ld"],
                         t["qt_ld"])
    return a, t


def bwd_outputs(c, d, dev, a, rows=None):
    """Attach the backward's inputs and guarded outputs to `a`; rows: dpre_part rows (None: none attached, so that
    the struct serves dgppo_gnn_attn_plan / _partial_blocks first)."""
    Rn, H, D = c.G * c.n, c.H, c.D
    o = dict(attn_in=_in(dev, A.bwd_attn_input(c)), dxcat=_in(dev, d["dxcat"]))
    a.attn, a.dxcat = o["attn_in"].data_ptr(), o["dxcat"].data_ptr()
    if c.da_add:
        o["da_add"] = _in(dev, d["da_add"])
        a.da_add = o["da_add"].data_ptr()
    if c.pad:  # [dqt | dbeta] in one buffer
        ld = H * D + H + 2
        o["dqb"] = Buf(dev, Rn, H * D + H, ld)
        a.dqt, a.dbeta, a.dqt_ld, a.dbeta_ld = o["dqb"].t.data_ptr(), o["dqb"].t[:, H * D:].data_ptr(), ld, ld
    else:
        o["dqt"], o["dbeta"] = Buf(dev, Rn, H * D), Buf(dev, Rn, H)
        a.dqt, a.dbeta = o["dqt"].t.data_ptr(), o["dbeta"].t.data_ptr()
    if c.qform:
        o["dq"] = Buf(dev, Rn, H * c.F)
        a.dq = o["dq"].t.data_ptr()
    if c.mode == "full_dx":
        a.dx_gstride = c.N * D + 5 * c.pad
        o["dx"] = Buf(dev, c.G, c.N * D, a.dx_gstride, init=d["dx0"])
        a.dx = o["dx"].t.data_ptr()
    if c.agent:
        a.dxa_gstride = c.n * D + 4 * c.pad
        o["dxa"] = Buf(dev, c.G, c.n * D, a.dxa_gstride, init=d["dxa0"])
        a.dxa = o["dxa"].t.data_ptr()
    if c.mode == "pre" and rows is not None:
        o["dpre"] = Buf(dev, rows, c.D0 * D + D)
        a.dpre_part = o["dpre"].t.data_ptr()
    return o


def _check(rc, what):
    assert rc == 0, f"{what} returned {rc}"
    torch.cuda.synchronize()


def _sender_table(c, d, dev):
    """dgppo_gnn_sender_table into a guarded buffer, compared by bits; returns the device table."""
    sb = Buf(dev, c.G * c.n, c.C, dtype=torch.int32)
    K.sender_table(c.G, c.n, c.C, d["E"], _in(dev, d["cand"]), _in(dev, d["receivers"]), _in(dev, d["senders"]), sb.t)
    torch.cuda.synchronize()
    got = sb.read(f"{c.key} sidx", np.int32)
    assert np.array_equal(got, d["sidx"].reshape(c.G * c.n, c.C)), f"{c.key}: sender table differs"
    return sb.t


@pytest.mark.parametrize("key", list(ATTN_CASES))
def test_attn_fwd(cuda, key):
    c, lib = ATTN_CASES[key], _lib.load()
    d, ex = A.inputs(c), A.expected(c, "fwd")
    a, keep = attn_struct(c, d, cuda, sidx=_sender_table(c, d, cuda))
    Rn, W = c.G * c.n, c.H * (c.D + 5)
    if c.otf >= 0:
        assert lib.dgppo_gnn_set_graph_otf(c.otf) == 0
    try:
        attn, xcat = Buf(cuda, Rn, c.H * c.C), Buf(cuda, Rn, W)
        a.attn, a.xcat = attn.t.data_ptr(), xcat.t.data_ptr()
        _check(lib.dgppo_gnn_attn_fwd(ctypes.byref(a), _lib.stream_handle(cuda)), "dgppo_gnn_attn_fwd")
        got_x = xcat.read(f"{key} xcat")
        A.compare(attn.read(f"{key} attn").reshape(Rn, c.H, c.C), ex["attn"], f"{key} attn")
        A.compare(got_x, ex["xcat"], f"{key} xcat")
        # attn is an optional output: without it the call writes the same xcat
        xcat2 = Buf(cuda, Rn, W)
        a.attn, a.xcat = None, xcat2.t.data_ptr()
        _check(lib.dgppo_gnn_attn_fwd(ctypes.byref(a), _lib.stream_handle(cuda)), "dgppo_gnn_attn_fwd (no attn)")
        A.P.check_bits(xcat2.read(f"{key} xcat (no attn)"), got_x, f"{key} xcat without attn")
    finally:
        if c.otf >= 0:
            lib.dgppo_gnn_set_graph_otf(1)


def test_graph_forward_on_the_fly_rows_are_bit_identical(cuda):
    """The Spread-layout case with each receiver's own rows computed on the fly and with every row staged."""
    lib, outs = _lib.load(), []
    c = ATTN_CASES["graph_spread_otf1"]
    d = A.inputs(c)
    try:
        for otf in (1, 0):
            assert lib.dgppo_gnn_set_graph_otf(otf) == 0
            a, keep = attn_struct(c, d, cuda)
            attn, xcat = Buf(cuda, c.G * c.n, c.H * c.C), Buf(cuda, c.G * c.n, c.H * (c.D + 5))
            a.attn, a.xcat = attn.t.data_ptr(), xcat.t.data_ptr()
            _check(lib.dgppo_gnn_attn_fwd(ctypes.byref(a), _lib.stream_handle(cuda)), "dgppo_gnn_attn_fwd")
            outs.append((attn.read("attn"), xcat.read("xcat")))
    finally:
        lib.dgppo_gnn_set_graph_otf(1)
    A.P.check_bits(outs[0][0], outs[1][0], "attn, on the fly against staged")
    A.P.check_bits(outs[0][1], outs[1][1], "xcat, on the fly against staged")


@pytest.mark.parametrize("key", list(ATTN_CASES))
def test_attn_bwd(cuda, key):
    c, lib = ATTN_CASES[key], _lib.load()
    d, ex = A.inputs(c), A.expected(c, "bwd")
    Rn, H, D = c.G * c.n, c.H, c.D
    a, keep = attn_struct(c, d, cuda)
    o = bwd_outputs(c, d, cuda, a)
    rows = int(lib.dgppo_gnn_attn_partial_blocks(ctypes.byref(a)))
    assert rows >= 1
    if c.mode == "pre":
        o["dpre"] = Buf(cuda, rows, c.D0 * D + D)
        a.dpre_part = o["dpre"].t.data_ptr()
    _check(lib.dgppo_gnn_attn_bwd(ctypes.byref(a), _lib.stream_handle(cuda)), "dgppo_gnn_attn_bwd")
    if c.pad:
        dqb = o["dqb"].read(f"{key} [dqt | dbeta]")
        dqt, dbeta = dqb[:, :H * D], dqb[:, H * D:]
    else:
        dqt, dbeta = o["dqt"].read(f"{key} dqt"), o["dbeta"].read(f"{key} dbeta")
    A.compare(dqt, ex["dqt"], f"{key} dqt")
    A.compare(dbeta, ex["dbeta"], f"{key} dbeta")
    if c.qform:
        A.compare(o["dq"].read(f"{key} dq"), ex["dq"], f"{key} dq")
    skip = NOT_COMPARED.get((key, "bwd"), set())  # read (the guards hold in any case), not compared
    if c.mode == "full_dx":
        dx = o["dx"].read(f"{key} dx").reshape(c.G, c.N, D)
        if "dx" not in skip:
            A.compare(dx, ex["dx"], f"{key} dx")
    if c.agent:
        dxa = o["dxa"].read(f"{key} dxa").reshape(c.G, c.n, D)
        if "dxa" not in skip:
            A.compare(dxa, ex["dxa"], f"{key} dxa")
    if c.mode == "pre":  # one partial row per workgroup, summed here in float64
        part = o["dpre"].read(f"{key} dpre_part")
        assert not np.isnan(part).any(), f"{key}: a dpre_part row was not written"
        tot = part.astype(np.float64).sum(0)
        e = ex["dpre"]
        P = A.P
        P.check_close(tot, e.ref64, e.ref32, e.scale_arr(), what=f"{key} [dpre_W | dpre_b]")
    if c.agent:  # dxa and dpre_part are optional: without them the call writes the same dqt / dbeta
        a2, keep2 = attn_struct(c, d, cuda)
        o2 = bwd_outputs(c, d, cuda, a2)
        a2.dxa = None
        _check(lib.dgppo_gnn_attn_bwd(ctypes.byref(a2), _lib.stream_handle(cuda)), "dgppo_gnn_attn_bwd (no dxa)")
        got = o2["dqb"].read("dqb")[:, :H * D] if c.pad else o2["dqt"].read("dqt")
        A.P.check_bits(got, dqt, f"{key} dqt without dxa / dpre_part")
        A.P.check_bits(o2["dxa"].read("dxa"), np.asarray(d["dxa0"]).reshape(c.G, c.n * D), f"{key} dxa not passed")


# ---- the fused layer ---------------------------------------------------------------------------------------------------
def _layer_call(c, d, dev, outs, sidx=None):
    """dgppo_gnn_layer_fwd with the named outputs attached; returns {name: array read back}."""
    t = graph_tensors(c, d, dev, sidx)
    Rn, H, D, F = c.G * c.n, c.H, c.D, c.F
    w = {k: _in(dev, d[k] if d[k].ndim == 2 else d[k][None]) for k in ("QBW", "Wcat", "Wu", "bu")}
    b = {}
    shapes = dict(Y=(Rn, F), qb=(Rn, H * D + H), attn=(Rn, H * c.C), xcat=(Rn, H * (D + 5)), zmean=(c.G, F),
                  tail=(Rn, max(c.n_out, 1)))
    for name in outs:
        b[name] = Buf(dev, *shapes[name])
    tw, th = (), None
    if "tail" in outs:
        tw = [_in(dev, d["tail"][k] if d["tail"][k].ndim == 2 else d["tail"][k][None]) for k in ops.TAIL_FIELDS]
        th = _in(dev, d["tail"]["h_in"])
    g = lambda k: b[k].t if k in b else None  # noqa: E731
    kw = dict(dims=[c.G, c.N, d["E"], c.n, D, F, H, c.C, c.D0], cand=t["cand"], receivers=t["receivers"],
              senders=t["senders"], sidx=t["sidx"], x=t["x"], x_gstride=t["x_gstride"], ef=t["ef"],
              ef_gstride=t["ef_gstride"], scale=d["scale"], xa=t["xa"], xa_gstride=t["xa_gstride"], pre_W=t["pre_W"],
              pre_b=t["pre_b"], QBW=w["QBW"], Wcat=w["Wcat"], Wu=w["Wu"], bu=w["bu"], Y=g("Y"), qb=g("qb"),
              attn=g("attn"), xcat=g("xcat"), zmean=g("zmean"), tail_w=tw, tail_h=th, tail_out=g("tail"))
    assert ops.gnn_layer_supported(**kw), f"{c.key}: outside dgppo_gnn_layer_supported"
    la = ops._layer_struct(**kw)
    _check(_lib.load().dgppo_gnn_layer_fwd(ctypes.byref(la), _lib.stream_handle(dev)), "dgppo_gnn_layer_fwd")
    return {k: v.read(f"{c.key} {k}") for k, v in b.items()}


LAYER_OUTS = dict(Y=("Y",), qb=("Y", "qb"), attn=("Y", "attn"), xcat=("Y", "xcat"), zmean=("zmean",),
                  zmean_Y=("zmean", "Y"), tail=("tail",))


@pytest.mark.parametrize("key", list(LAYER_CASES))
def test_layer_fwd(cuda, key):
    c = LAYER_CASES[key]
    d, ex = A.inputs(c), A.expected(c, "layer")
    Rn = c.G * c.n
    full = _layer_call(c, d, cuda, ("Y", "qb", "attn", "xcat"), sidx=_sender_table(c, d, cuda))
    A.compare(full["qb"], ex["qb"], f"{key} [qt | beta]")
    A.compare(full["attn"].reshape(Rn, c.H, c.C), ex["attn"], f"{key} attn")
    A.compare(full["xcat"], ex["xcat"], f"{key} xcat")
    A.compare(full["Y"], ex["Y"], f"{key} Y")
    if c.outs in ("all", "cache"):
        return
    part = _layer_call(c, d, cuda, LAYER_OUTS[c.outs])
    for name, got in part.items():  # what a narrower call does write agrees with the full call bit for bit
        if name in full:
            A.P.check_bits(got, full[name], f"{key} {name} of the call with {c.outs}")
    if "zmean" in part:
        A.compare(part["zmean"], ex["zmean"], f"{key} zmean")
    if "tail" in part:
        A.compare(part["tail"], ex["tail"], f"{key} tail output")


# ---- edge columns past the first four ------------------------------------------------------------------------------------
@pytest.mark.parametrize("G,n,C,H,EX", A.EDGE_CASES)
def test_edge_wsum_and_edge_da(cuda, G, n, C, H, EX):
    d = A.edge_inputs(G, n, C, H, EX)
    Rn = G * n
    dev = dict(cand=_in(cuda, d["cand"]), sidx=_in(cuda, d["sidx"].reshape(Rn, C)), efx=_in(cuda, d["efx"]),
               attn=_in(cuda, d["attn"]), dxx=_in(cuda, d["dxx"]))
    out, da = Buf(cuda, Rn, H * EX), Buf(cuda, Rn, H * C)
    K.edge_wsum(G, n, C, H, EX, d["E"], dev["attn"], dev["cand"], dev["sidx"], dev["efx"], out.t)
    K.edge_da(G, n, C, H, EX, d["E"], dev["dxx"], dev["cand"], dev["sidx"], dev["efx"], da.t)
    torch.cuda.synchronize()
    what = f"G{G} n{n} C{C} H{H} EX{EX}"
    r64, mag = A.edge_wsum(d["attn"], d["cand"], d["sidx"], d["efx"])
    r32, _ = A.edge_wsum(d["attn"], d["cand"], d["sidx"], d["efx"], A.T32)
    A.compare(out.read("edge_wsum"), A.Expect(r64.numpy(), r32.numpy(), mag.numpy()), f"edge_wsum {what}")
    r64, mag = A.edge_da(d["dxx"], d["cand"], d["sidx"], d["efx"], H)
    r32, _ = A.edge_da(d["dxx"], d["cand"], d["sidx"], d["efx"], H, A.T32)
    masked = np.broadcast_to((d["sidx"].reshape(Rn, 1, C) < 0), (Rn, H, C))  # exactly 0, by bits
    A.compare(da.read("edge_da").reshape(Rn, H, C), A.Expect(r64.numpy(), r32.numpy(), mag.numpy(), masked),
              f"edge_da {what}")
