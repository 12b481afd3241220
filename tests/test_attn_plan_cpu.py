"""dgppo_gnn_attn_plan, the host dispatch of csrc/attn.hip, checked without a GPU: the backward's dpre_part workspace
is sized by the same plan that launches, the plan refuses exactly the shapes valid() and the 160 KB LDS limit refuse,
a handful of decisions recorded in DESIGN.md and the kernels' comments, and the coverage of the GPU case table of
test_attn_families_gpu.py (which never asks the library which kernel it ran)."""
import ctypes
import itertools
import json
import os
from types import SimpleNamespace

import pytest
import torch

from dgppo_fov_amd import _lib, ops
from dgppo_fov_amd.env import make_env
from dgppo_fov_amd.nn.layers import GNN, GraphBatch, ParamSpace
from test_attn_families_gpu import CASES

HERE = os.path.dirname(os.path.abspath(__file__))
KD0, KH, LDS_MAX = 8, 3, 160 * 1024
FAKE = 0x1000  # a non-null pointer: the plan never dereferences


def _args(G, N, n, D, F, H, C, mode, sidx=True, E=None):
    """dgppo_gnn_attn_args of the Q-free form.  mode: full | full_dx | raw (agent mode, raw rows used directly) |
    pre4 / pre8 (agent mode, relu(x_raw pre_W + pre_b) of 4- / 8-wide raw rows)."""
    a = _lib.GnnAttnArgs()
    a.G, a.N, a.E, a.n_agents, a.D, a.F, a.H, a.C = G, N, E or n * C, n, D, F, H, C
    for f in ("cand", "receivers", "senders", "x", "ef", "qt", "bk", "beta"):
        setattr(a, f, FAKE)
    a.beta_ld = a.qt_ld = H * D + H
    a.sidx = FAKE if sidx else 0
    if mode == "full_dx":
        a.dx = FAKE
    elif mode != "full":
        a.xa = a.dxa = FAKE
        a.D0 = D if mode == "raw" else int(mode[3:])
        if mode != "raw":
            a.pre_W = a.pre_b = FAKE
    return a


def _plan(a, bwd):
    pl = _lib.GnnAttnPlan()
    rc = _lib.load().dgppo_gnn_attn_plan(ctypes.byref(a), int(bwd), ctypes.byref(pl))
    return rc, pl


def _valid(a):
    """valid() of csrc/attn.hip for the arguments _args builds (pointers and row strides are in order)."""
    if not (1 <= a.H <= KH and 1 <= a.D <= 64 and 1 <= a.F <= 64 and 1 <= a.C <= 128 and a.n_agents >= 1):
        return False
    if a.xa and (not 1 <= a.D0 <= KD0 or (not a.pre_W and a.D0 != a.D)):
        return False
    return True


def _fallback_bytes(a, bwd):
    """Dynamic LDS of the block / wave fallbacks from their carves (Carve, BwdCarve, WaveCarve in csrc/attn.hip)."""
    n, N, D, C = a.n_agents, a.N, a.D, a.C
    DM = 8 if D <= 8 else (32 if D <= 32 else 64)
    CP = next(c for c in (8, 16, 32, 64, 128) if C <= c)
    CR, XP = min((C + 7) & ~7, CP), DM + 1
    full_dx = bwd and not a.xa and bool(a.dx)
    if bwd and CP <= 64 and not full_dx:
        RW = 64 // CP
        gpw = max(RW // n, 1)
        wave = (RW * (2 * KH * DM + 16) + RW * CR * (XP + KH + 4 + KD0 + 1) + gpw * n * DM + 3) & ~3
        head = (KD0 * DM + DM + 3) & ~3
        return "WAVE", 4 * (head + max(4 * wave, 32 * (32 * ((DM + 31) // 32) + 1)))
    R = 256 // CP
    fixed = KD0 * DM + DM + 16 + R * KH * DM
    if bwd:
        fixed += R * KH * (DM + 5) + R * CR * (2 * XP + KH + KD0 + 1) + R * n * DM
    else:
        fixed += R * CR * (XP + KH + 4)
    per_graph = N * D if full_dx else 0
    gpb = max(R // n, 1)
    while gpb > 1 and (fixed + gpb * per_graph) * 4 > 64 * 1024:
        gpb -= 1
    return "BLOCK", 4 * (fixed + gpb * per_graph)


def _sweep():
    for n, C, D, H, mode, sidx, G in itertools.product((1, 3, 8, 16, 17, 32, 400), (4, 9, 24, 32, 33, 64, 72, 128),
                                                       (7, 8, 10, 16, 32, 40, 64), (2, 3),
                                                       ("full", "full_dx", "raw", "pre4", "pre8"), (True, False),
                                                       (6, 20000)):
        k = C - 2 * n
        N = 2 * n + n * k + 1 if k >= 1 else n + C  # the Spread layout where the candidates allow it
        yield _args(G, N, n, D, 64 if D > 32 else 32, H, C, mode, sidx)
    yield _args(6, 10, 3, 65, 32, 3, 9, "full")   # D past 64
    yield _args(6, 10, 3, 7, 32, 4, 9, "full")    # H past 3
    yield _args(6, 10, 3, 7, 32, 3, 129, "full")  # C past 128
    yield _args(6, 10, 0, 7, 32, 3, 9, "full")    # no agents
    yield _args(6, 10, 3, 32, 32, 3, 9, "pre9")   # raw rows past 8 columns


def test_plan_sizes_the_workspace_refuses_what_the_launch_refuses_and_fits_the_lds():
    lib = _lib.load()
    seen, refused_lds, refused_shape = set(), 0, 0
    for a in _sweep():
        rcb, plb = _plan(a, True)
        assert lib.dgppo_gnn_attn_partial_blocks(ctypes.byref(a)) == plb.grid
        for bwd, (rc, pl) in ((False, _plan(a, False)), (True, (rcb, plb))):
            what = (bwd, a.G, a.N, a.n_agents, a.D, a.H, a.C, a.D0, bool(a.xa), bool(a.pre_W), bool(a.dx), bool(a.sidx))
            if not _valid(a):
                assert rc == _lib.DGPPO_EINVAL and pl.family == -1, what
                refused_shape += 1
                continue
            fam, fb = _fallback_bytes(a, bwd)
            if rc != 0:  # the only refusal of a valid call: no tuned kernel takes it and the fallback's LDS is too large
                assert rc == _lib.DGPPO_EINVAL and pl.family == -1 and pl.grid == 0 and fb > LDS_MAX, what
                refused_lds += 1
                continue
            assert 0 < pl.lds_bytes <= LDS_MAX and pl.grid >= 1 and pl.threads in (256, 512), what
            if pl.family_name in ("BLOCK", "WAVE"):
                assert (pl.family_name, pl.lds_bytes) == (fam, fb), what
                assert pl.grid == min(-(-pl.nblk // (4 if fam == "WAVE" else 1)), 2048), what
            seen.add((bwd, pl.family_name))
    assert refused_shape >= 10 and refused_lds > 0
    assert seen == {(False, "FWD2R"), (False, "GRAPH_FWD"), (False, "BLOCK"), (True, "BWD2R"), (True, "GRAPH_BWD"),
                    (True, "GRAPH_BWD32"), (True, "WAVE"), (True, "BLOCK")}


def test_plan_requires_an_output_struct_and_arguments():
    lib = _lib.load()
    pl = _lib.GnnAttnPlan()
    assert lib.dgppo_gnn_attn_plan(None, 0, ctypes.byref(pl)) == _lib.DGPPO_EINVAL and pl.family == -1
    assert lib.dgppo_gnn_attn_plan(ctypes.byref(_args(6, 81, 8, 7, 32, 3, 24, "full")), 0, None) == _lib.DGPPO_EINVAL
    assert lib.dgppo_gnn_attn_partial_blocks(None) == 0


def _fam(a, bwd):
    rc, pl = _plan(a, bwd)
    assert rc == 0
    return pl


def test_recorded_decisions():
    """Decisions the kernels' comments and DESIGN.md record (not read off the dispatch code)."""
    G = 16384
    # LidarSpread n = 8 (N = 81, C = 24): the 7-wide first layer runs the row-block pair at DM = 8
    for D in (7, 8):
        a = _args(G, 81, 8, D, 32, 3, 24, "full")
        f, b = _fam(a, False), _fam(a, True)
        assert (f.family_name, f.dm, f.grid) == ("FWD2R", 8, G * 8 // 16)
        assert (b.family_name, b.dm, b.gpb, b.grid) == ("BWD2R", 8, 2, 1536)
    # its second layer (agent mode through pre_W, D = 32): DM = 32, the backward's persistent grid capped at 768
    a = _args(G, 81, 8, 32, 64, 3, 24, "pre7")
    f, b = _fam(a, False), _fam(a, True)
    assert (f.family_name, f.dm) == ("FWD2R", 32)
    assert (b.family_name, b.dm, b.nblk, b.grid) == ("BWD2R", 32, G // 2, 768)
    # LidarOmniTarget's 10-wide first layer (n = 8: N = 81, C = 17): DM = 16
    a = _args(G, 81, 8, 10, 32, 3, 17, "full")
    assert [(p.family_name, p.dm) for p in (_fam(a, False), _fam(a, True))] == [("FWD2R", 16), ("BWD2R", 16)]
    # LidarSpread n = 32 (N = 321, C = 72), second layer: graph forward with the 64 agent / goal rows staged and the
    # receiver's 8 own hit rows on the fly; the D = 32 graph backward on min(G, 256) workgroups of 512 threads
    for G2 in (100, 4096):
        a = _args(G2, 321, 32, 32, 64, 3, 72, "pre7")
        f, b = _fam(a, False), _fam(a, True)
        assert (f.family_name, f.dm, f.ns, f.slots, f.cp, f.grid) == ("GRAPH_FWD", 32, 64, 8, 72, G2)
        assert (b.family_name, b.grid, b.threads) == ("GRAPH_BWD32", min(G2, 256), 512)
    # ... and its 7-wide first layer: every row staged; the D <= 8 graph backward, one workgroup per graph
    a = _args(4096, 321, 32, 7, 32, 3, 72, "full")
    f, b = _fam(a, False), _fam(a, True)
    assert (f.family_name, f.dm, f.ns, f.slots, f.grid) == ("GRAPH_FWD", 8, 321, 0, 4096)
    assert (b.family_name, b.dm, b.cp, b.grid) == ("GRAPH_BWD", 8, 72, 4096)
    # every sender's gradient asked for (layers past the second): the block backward
    for N, n, C in ((81, 8, 24), (321, 32, 72)):
        assert _fam(_args(G, N, n, 32, 32, 3, C, "full_dx"), True).family_name == "BLOCK"
    # the wave backward takes CP <= 64 without dx, the block backward CP = 128
    assert _fam(_args(G, 81, 8, 40, 64, 3, 24, "pre7"), True).family_name == "WAVE"
    assert _fam(_args(G, 321, 32, 40, 64, 3, 72, "pre7"), True).family_name == "BLOCK"


# ---- coverage of the GPU case table ---------------------------------------------------------------------------
def _case_calls(eid, n, obs, kw, G=6):
    """(layer, plan of the forward or None where the fused layer kernel takes it, plan of the backward) of a case
    of test_attn_families_gpu, through the real GraphTransformer._attn_args on a CPU GraphBatch of zeros."""
    env = make_env(eid, n, num_obs=obs)
    cpu = torch.device("cpu")
    N, E = env.n_nodes, env.n_edges
    idx = torch.zeros((G, E), dtype=torch.int32)
    gb = GraphBatch(torch.zeros(G, N, env.node_dim), torch.zeros(G, E, env.edge_dim), idx, idx, n,
                    env.agent_candidates(cpu), raw_cols=env.nonagent_feature_cols)
    gb._sidx = torch.zeros((G * n, gb.C), dtype=torch.int32)  # the sender table is a kernel's output
    ps = ParamSpace()
    net = GNN(ps, "gnn", env.node_dim, 2, edge_dim=env.edge_dim, **kw)
    ps.build(cpu)
    out = []
    for i, layer in enumerate(net.layers):
        z = torch.zeros(G * n, max(layer.D, layer.H * layer.D + layer.H))
        xa, pre = (z[:, :layer.D].contiguous(), net.layers[0]) if i else (None, None)
        args = layer._attn_args(gb, z[:, :layer.H * layer.D + layer.H].contiguous(), xa, pre)
        fused = False
        if not layer.EX and (xa is None or gb.sender_raw[1] is None):  # GraphTransformer._fused_fwd's own gates
            kw_l = {k: args[k] for k in ("dims", "cand", "receivers", "senders", "sidx", "x", "x_gstride", "ef",
                                         "ef_gstride", "scale", "xa", "xa_gstride", "pre_W", "pre_b")}
            fused = ops.gnn_layer_supported(**kw_l, QBW=z, Wcat=z, Wu=z, bu=z, Y=z)
        out.append(SimpleNamespace(fused=fused, fwd=None if fused else ops.gnn_attn_plan(False, **args),
                                   bwd=ops.gnn_attn_plan(True, dxa=xa, **args),
                                   rows=ops.gnn_attn_partial_blocks(**args)))  # as GraphTransformer.bwd sizes dpre_part
    return out


REQUIRED = {"fwd:FWD2R", "fwd:GRAPH_FWD", "fwd:BLOCK", "bwd:BWD2R", "bwd:GRAPH_BWD", "bwd:GRAPH_BWD32", "bwd:WAVE",
            "bwd:BLOCK",  # every (direction, family) pair the kernels support at default knobs
            "fwd:BLOCK:cp8", "fwd:BLOCK:cp32", "fwd:BLOCK:cp128", "fwd:BLOCK:dm8", "fwd:BLOCK:dm32", "fwd:BLOCK:dm64",
            "bwd:WAVE:cp8", "bwd:WAVE:cp32", "bwd:WAVE:cp64", "bwd:WAVE:dm8", "bwd:WAVE:dm32", "bwd:WAVE:dm64",
            "bwd:BLOCK:cp128", "bwd:BLOCK:dm64", "bwd:BLOCK:lds>64K"}


def test_gpu_case_table_reaches_every_family():
    reached = set()
    for key, (eid, n, obs, kw, fused) in CASES.items():
        calls = _case_calls(eid, n, obs, kw)
        assert tuple(c.fused for c in calls) == fused, key
        for c in calls:
            assert c.rows == c.bwd.grid, key
            for d, pl in (("fwd", c.fwd), ("bwd", c.bwd)):
                if pl is None:
                    continue
                reached.add(f"{d}:{pl.family_name}")
                if pl.family_name in ("BLOCK", "WAVE"):
                    reached |= {f"{d}:{pl.family_name}:cp{pl.cp}", f"{d}:{pl.family_name}:dm{pl.dm}"}
                    if pl.lds_bytes > 64 * 1024:
                        reached.add(f"{d}:{pl.family_name}:lds>64K")
    # tests/golden/attn_uncovered.json: coverage keys whose GPU case was taken out because it fails on the parent
    # commit too (named in DESIGN.md); never a family the bench configurations run
    uncovered = set(json.load(open(os.path.join(HERE, "golden", "attn_uncovered.json"))))
    assert uncovered <= REQUIRED and not any(k.split(":")[1] in ("FWD2R", "BWD2R", "GRAPH_FWD", "GRAPH_BWD",
                                                                 "GRAPH_BWD32") for k in uncovered)
    assert REQUIRED - uncovered <= reached, sorted(REQUIRED - uncovered - reached)
