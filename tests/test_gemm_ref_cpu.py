"""tests/gemm_ref.py checked without a GPU: the reference against torch float64 on dense views, each comparison class
against its mutation, the coverage of the GPU case table (the kernel keys of dgppo_gemm_plan it reaches are the keys
the sweep reaches, at default knobs and per knob set), the DGPPO_EINVAL returns of dgppo_gemm /
dgppo_gemm_wgrad_grouped, the two workspace-size functions, and the float-reciprocal index split of the B staging."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gemm_ref as R
import prim_ref as P
from dgppo_fov_amd import _lib

F32, F64 = np.float32, np.float64
HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL = _lib.DGPPO_EINVAL


# ---- the reference against torch on dense views --------------------------------------------------------------------------
def _dense(buf, off, rows, cols, ld, grp, gs):
    """(rows, cols) float64 matrix of a flat buffer by torch.as_strided (no index arithmetic shared with gemm_ref)."""
    t = torch.from_numpy(np.concatenate([buf, np.zeros(max(grp, 1) * max(ld, gs, 1) + cols, buf.dtype)]))
    if grp <= 0:
        return torch.as_strided(t, (rows, cols), (ld, 1), off).double()
    groups = -(-rows // grp)
    return torch.as_strided(t, (groups, grp, cols), (gs, ld, 1), off).reshape(groups * grp, cols)[:rows].double()


def _torch_ref(s, bufs):
    out = torch.from_numpy(bufs["C"].astype(F64))
    for b in range(s.batch):
        A = _dense(bufs["A"], s.a_off + b * s.sa, *((s.K, s.M) if s.ta else (s.M, s.K)), s.lda, s.a_grp, s.a_gs)
        B = _dense(bufs["B"], s.b_off + b * s.sb, *((s.N, s.K) if s.tb else (s.K, s.N)), s.ldb, s.b_grp, s.b_gs)
        v = s.alpha * ((A.T if s.ta else A) @ (B.T if s.tb else B))
        if s.bias:
            v = v + torch.from_numpy(bufs["bias"]).double()
        x = None
        if s.beta != 0:
            x = s.beta * _dense(bufs["C"], s.c_off + b * s.sc, s.M, s.N, s.ldc, s.c_grp, s.c_gs)
        if s.addend:
            d = _dense(bufs["addend"], s.add_off + b * s.s_add, s.M, s.N, s.ld_add, s.add_grp, s.add_gs)
            x = d if x is None else x + d
        if x is not None:
            v = v + x
        if s.relu:
            v = v.clamp(min=0)
        if s.epi == 1:
            v = torch.where(_dense(bufs["mask"], s.mask_off, s.M, s.N, s.ld_mask, s.c_grp, s.c_gs) > 0, v, 0.0)
        for m in range(s.M):  # the C rows, written one by one at their own address
            q = m // s.c_grp * s.c_gs + m % s.c_grp * s.ldc if s.c_grp > 0 else m * s.ldc
            out[s.c_off + b * s.sc + q:s.c_off + b * s.sc + q + s.N] = v[m]
    return out.numpy()


@pytest.mark.parametrize("form", ["prefetch", "breg", "plain", "scalar", "tile", "wgrad"])
def test_reference_matches_torch_float64(form):
    n = 0
    for s in R.address_specs(form):
        bufs = R.make_inputs(s, 5, "close")
        outs, touched, _ = R.reference(s, bufs)
        ref = _torch_ref(s, bufs)
        t = touched["C"]
        assert np.abs(outs["C"][t] - ref[t]).max() <= 1e-12 * max(1.0, np.abs(ref[t]).max()), s
        rest = np.ones(ref.size, bool)
        rest[t] = False
        assert np.array_equal(outs["C"][rest], ref[rest], equal_nan=True), s
        n += 1
    assert n >= 5


# ---- each comparison fails on its mutation ----------------------------------------------------------------------------------
MUTANTS = [
    ("wgrad_row_dropped", R.Spec(40, 70, 300, ta=1, beta=1.0, bias_grad=1)),
    ("epilogue_order", R.Spec(33, 40, 24, bias=1, beta=0.5, addend=1, alpha=0.5)),
    ("addend_gstride", R.Spec(33, 40, 24, addend=1, ld_add=40, add_grp=5, add_gs=7 * 40)),
    ("mask_next_row", R.Spec(33, 40, 24, epi=1, ld_mask=45)),
    ("batch_c_stride", R.Spec(33, 40, 24, batch=3, ldc=43)),
]


@pytest.mark.parametrize("mutate,s", MUTANTS, ids=[m for m, _ in MUTANTS])
def test_comparisons_catch_mutations(mutate, s):
    if mutate == "epilogue_order":
        # The order is a rounding property: integers make both orders exact and the close bound admits either, so the
        # comparison that owns it is check_bits against the float32 restatement on gemm_ref.epilogue_inputs (the GPU
        # file's test_epilogue_bits_do_not_depend_on_the_path holds every path to exactly that).
        bufs = R.epilogue_inputs(s, 11)
        good, touched, _ = R.reference(s, bufs)
        t = touched["C"]
        same = R.reference(s, bufs, dt=F32)[0]["C"][t]
        bad = R.reference(s, bufs, dt=F32, mutate=mutate)[0]["C"][t]
        assert same.dtype == F32 and bad.dtype == F32
        P.check_bits(same, R.reference(s, bufs, dt=F32)[0]["C"][t], "restatement is deterministic")
        assert np.abs(same.astype(F64) - good["C"][t]).max() < 1e-4  # and it is the contract's result, rounded
        with pytest.raises(AssertionError):
            P.check_bits(bad, same, "swapped epilogue order")
        return
    for cls in ("exact", "close"):
        bufs = R.make_inputs(s, 11, cls)
        good, touched, mag = R.reference(s, bufs)
        dt = F64 if cls == "exact" else F32
        bad = R.reference(s, bufs, dt=dt, mutate=mutate)[0]["C"].astype(F32)
        same = R.reference(s, bufs, dt=dt)[0]["C"].astype(F32)
        t = touched["C"]
        if cls == "exact":
            P.check_exact(same[t], good["C"][t])
            with pytest.raises(AssertionError):
                P.check_exact(np.nan_to_num(bad[t], nan=1e9), good["C"][t])
        else:
            P._ratio(np.abs(same[t].astype(F64) - good["C"][t]), R.close_bound(s, mag[t]), "close")
            with pytest.raises(AssertionError):
                P._ratio(np.abs(np.nan_to_num(bad[t], nan=1e9).astype(F64) - good["C"][t]), R.close_bound(s, mag[t]),
                         "close")


def test_layernorm_epilogue_gates_meet_the_ambiguity_cap():
    """The cap on ambiguous gates is a condition on the inputs: the reference alone meets it for the GPU cases' seeds."""
    for s, seed in R.ln_specs():
        bufs = R.make_inputs(s, seed, "close")
        fwd = R.reference(s, bufs)[0]
        s3 = s.but(epi=3)
        b3 = dict(R.make_inputs(s3, seed + 1, "close"), ln_scale=bufs["ln_scale"], ln_bias=bufs["ln_bias"],
                  ln_h=fwd["ln_h"].astype(F32), ln_mean=fwd["ln_mean"].astype(F32), ln_rstd=fwd["ln_rstd"].astype(F32))
        bwd = R.reference(s3, b3)[0]
        assert P.amb_ok(bwd["amb"]), (s, int(bwd["amb"].sum()))
        assert P.amb_ok(np.abs(fwd["pre"]) < P.AMB * fwd["y_scale"]), s


# ---- coverage ----------------------------------------------------------------------------------------------------------
def test_case_table_reaches_every_kernel_key_at_default_knobs():
    reach, table, calls = R.coverage()
    print(f"[gemm coverage] default knobs: {calls} plans swept, {len(reach)} kernel keys reachable, "
          f"{len(table)} reached by the GPU case table")
    assert reach == table, (sorted(reach - table), sorted(table - reach))
    assert {k[0] for k in reach} == {"rows", "wgrad", "tile"}
    forms = {(k[1], k[2], k[3]) for k in reach if k[0] == "rows"}
    for ntw, ncg in ((1, 1), (2, 1), (1, 3), (2, 2), (2, 3)):
        assert ("prefetch", ntw, ncg) in forms and ("plain", ntw, ncg) in forms
    assert {(k[1], k[2]) for k in reach if k[0] == "wgrad"} >= {(1, 1), (1, 2), (1, 3), (1, 4), (2, 1), (2, 2), (3, 1),
                                                                (4, 1)}


def test_case_table_reaches_every_kernel_key_per_knob_set():
    """The knobs are read once per process: one child per set (no GPU needed), started together."""
    code = (f"import sys, json; sys.path.insert(0, {os.path.dirname(HERE)!r}); sys.path.insert(0, {HERE!r}); "
            "import gemm_ref as R; a, b, n = R.coverage(); print(json.dumps([sorted(a), sorted(b), n]))")
    procs = [subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, **knobs), stdout=subprocess.PIPE)
             for knobs in R.KNOB_SETS]
    default = R.coverage()[0]
    union = set(default)
    for knobs, p in zip(R.KNOB_SETS, procs):
        out, _ = p.communicate(timeout=300)
        assert p.returncode == 0, knobs
        reach, table, calls = json.loads(out.decode().strip().splitlines()[-1])
        reach, table = {tuple(k) for k in reach}, {tuple(k) for k in table}
        print(f"[gemm coverage] {knobs}: {calls} plans swept, {len(reach)} keys reachable ({len(reach - default)} "
              f"new), {len(table)} reached by the case table")
        assert reach == table, knobs
        assert reach - default, knobs
        union |= reach
    missing = sorted(R.instantiations() - {R.template_of(k) for k in union})
    print(f"[gemm coverage] instantiations of gemm.hip no knob set reaches: {len(missing)}")
    for m in missing:
        print("   ", m)
    assert set(missing) == R.UNREACHABLE, (sorted(set(missing) - R.UNREACHABLE), sorted(R.UNREACHABLE - set(missing)))


# ---- argument checks ---------------------------------------------------------------------------------------------------------
def _rc(s, drop=(), **fields):
    """dgppo_gemm's and dgppo_gemm_plan's return for a Spec with fake (never dereferenced when refused) pointers."""
    ptr = {k: v for k, v in R._FAKE.items() if k not in drop}
    g = R.fill_args(s, ptr)
    for k, v in fields.items():
        setattr(g, k, v)
    pl = _lib.GemmPlan()
    rc = _lib.load().dgppo_gemm_plan(ctypes.byref(g), ctypes.byref(pl))
    if rc != 0 or pl.path == -1:  # nothing would be launched: the launch entry point itself is safe to call
        assert _lib.load().dgppo_gemm(ctypes.byref(g), None) == rc
    return rc, g


ROWS_S, TILE_S, WG_S = R.Spec(40, 64, 32), R.Spec(40, 64, 300, ta=1, tb=1), R.Spec(40, 64, 300, ta=1)
LN_S = R.Spec(40, 64, 32, epi=2)
REFUSED = [
    ("null A", ROWS_S, ("A",), {}), ("null B", ROWS_S, ("B",), {}), ("null C", ROWS_S, ("C",), {}),
    ("M < 0", ROWS_S, (), dict(M=-1)), ("N < 0", ROWS_S, (), dict(N=-1)), ("K < 0", ROWS_S, (), dict(K=-1)),
    ("batch 0", ROWS_S, (), dict(batch=0)), ("split_k 0", TILE_S, (), dict(split_k=0)),
    ("split_k 4097", TILE_S, (), dict(split_k=4097)),
    ("bias_grad on rows", R.Spec(40, 64, 32, bias_grad=1), (), {}),
    ("bias_grad on tile", R.Spec(40, 64, 300, ta=1, tb=1, bias_grad=1), (), {}),
    ("epi on tile", R.Spec(40, 64, 300, epi=1), (), {}), ("epi on wgrad", R.Spec(40, 64, 300, ta=1, epi=1), (), {}),
    ("epi 4", ROWS_S, (), dict(epi=4)),
    ("epi 1 no mask", R.Spec(40, 64, 32, epi=1), ("mask",), {}),
    ("epi 1 addend", R.Spec(40, 64, 32, epi=1, addend=1), (), {}),
    ("epi 1 relu", R.Spec(40, 64, 32, epi=1, relu=1), (), {}),
    ("epi 2 N 63", R.Spec(40, 63, 32, epi=2), (), {}), ("epi 3 N 65", R.Spec(40, 65, 32, epi=3), (), {}),
    ("epi 2 batch 2", R.Spec(40, 64, 32, epi=2, batch=2), (), {}),
    ("epi 2 beta", R.Spec(40, 64, 32, epi=2, beta=1.0), (), {}),
    ("epi 3 addend", R.Spec(40, 64, 32, epi=3, addend=1), (), {}),
    ("epi 2 relu", R.Spec(40, 64, 32, epi=2, relu=1), (), {}),
] + [(f"epi 2 no {k}", LN_S, (k,), {}) for k in ("ln_scale", "ln_bias", "ln_h", "ln_mean", "ln_rstd")] + [
    ("epi 3 no ln_part", R.Spec(40, 64, 32, epi=3), ("ln_part",), {}),
    ("split_k 2 no workspace", R.Spec(40, 64, 300, ta=1, tb=1, split_k=2), ("workspace",), {}),
    ("wgrad chunks 3 no workspace", WG_S, ("workspace",), {}),
]


@pytest.mark.parametrize("what,s,drop,fields", REFUSED, ids=[r[0] for r in REFUSED])
def test_gemm_refuses(what, s, drop, fields):
    assert _rc(s, drop, **fields)[0] == EINVAL
    ok = {k: v for k, v in fields.items() if k not in ("M", "N", "K", "batch", "split_k", "epi")}
    if not drop and not fields:
        return
    rc, _ = _rc(s, (), **ok)  # the same call without the defect is accepted: the refusal is about the defect
    assert rc == 0, what


def test_gemm_empty_output_returns_zero():
    for f in (dict(M=0), dict(N=0)):
        rc, g = _rc(ROWS_S, ("A", "B", "C"), **f)  # nothing to do: not even the pointers are looked at
        assert rc == 0
    # K = 0 with 16-byte aligned rows plans the prefetch form, which has no kernel without a k-chunk: refused before
    # any launch (no caller passes K = 0)
    assert _rc(ROWS_S, (), K=0)[0] == EINVAL


def test_grouped_wgrad_refuses():
    lib = _lib.load()
    good = [R.fill_args(R.Spec(40, 64, 100, ta=1)), R.fill_args(R.Spec(8, 27, 50, ta=1, bias_grad=1))]
    bad = {"rows problem": R.Spec(40, 64, 32), "trans_b": R.Spec(40, 64, 100, ta=1, tb=1),
           "N 193": R.Spec(40, 193, 100, ta=1), "M 4097": R.Spec(4097, 64, 100, ta=1),
           "relu": R.Spec(40, 64, 100, ta=1, relu=1), "bias": R.Spec(40, 64, 100, ta=1, bias=1),
           "addend": R.Spec(40, 64, 100, ta=1, addend=1), "epi": R.Spec(40, 64, 100, ta=1, epi=1),
           "M 0": R.Spec(0, 64, 100, ta=1), "batch 0": R.Spec(40, 64, 100, ta=1, batch=0)}
    for what, s in bad.items():
        arr = (_lib.GemmArgs * 3)(good[0], R.fill_args(s), good[1])
        assert lib.dgppo_gemm_wgrad_grouped(arr, 3, R._FAKE["workspace"], None) == EINVAL, what
    nul = R.fill_args(R.Spec(40, 64, 100, ta=1), {k: v for k, v in R._FAKE.items() if k != "B"})
    assert lib.dgppo_gemm_wgrad_grouped((_lib.GemmArgs * 1)(nul), 1, R._FAKE["workspace"], None) == EINVAL
    assert lib.dgppo_gemm_wgrad_grouped(None, 1, None, None) == EINVAL
    assert lib.dgppo_gemm_wgrad_grouped((_lib.GemmArgs * 1)(good[0]), -1, None, None) == EINVAL
    big = (_lib.GemmArgs * 1)(R.fill_args(R.Spec(40, 64, 300, ta=1)))  # three chunks: needs the workspace
    assert lib.dgppo_gemm_wgrad_grouped(big, 1, None, None) == EINVAL


# ---- workspace sizes ---------------------------------------------------------------------------------------------------------
def _chunks(K):
    c = min(max(-(-K // 128), 1), 256)
    return c & ~7 if c > 8 else c


def test_workspace_floats_follow_their_formulas():
    lib = _lib.load()
    assert [_chunks(K) for K in (1, 128, 129, 1024, 1025, 1152, 1153, 2047, 2048, 10 ** 6)] == \
        [1, 1, 2, 8, 8, 8, 8, 16, 16, 256]
    probs = []
    for K in (0, 1, 128, 129, 1024, 1025, 1152, 1153, 2048, 32768, 32769, 70001):
        for M, N, batch, bg in ((40, 64, 1, 0), (3, 5, 3, 1), (128, 192, 2, 1)):
            s = R.Spec(M, N, K, ta=1, batch=batch, bias_grad=bg)
            g = R.fill_args(s)
            c = _chunks(K)
            want = c * batch * (M * N + N) if c > 1 else 0
            assert lib.dgppo_gemm_workspace_floats(ctypes.byref(g)) == want, (K, M, N, batch)
            rc, pl = R.plan(s)
            assert rc == 0 and pl.chunks == c and pl.path == R.WGRAD
            probs.append((g, want))
    arr = (_lib.GemmArgs * len(probs))(*[g for g, _ in probs])
    for n in (0, 1, 12, 13, len(probs)):
        assert lib.dgppo_gemm_wgrad_grouped_workspace_floats(arr, n) == sum(w for _, w in probs[:n])
    assert lib.dgppo_gemm_wgrad_grouped_workspace_floats(None, 3) == 0
    for split_k in (1, 2, 7):  # tiled: split_k slabs of (batch, M, N); rows: none
        g = R.fill_args(R.Spec(65, 193, 300, batch=2, split_k=split_k))
        assert lib.dgppo_gemm_workspace_floats(ctypes.byref(g)) == (split_k * 2 * 65 * 193 if split_k > 1 else 0)
    assert lib.dgppo_gemm_workspace_floats(ctypes.byref(R.fill_args(R.Spec(65, 64, 32, split_k=4)))) == 0
    assert lib.dgppo_gemm_workspace_floats(None) == 0


def test_partial_rows_reads_the_plan():
    lib = _lib.load()
    for M in (1, 77, 4096, 200000):
        s = R.Spec(M, 64, 64, epi=3)
        rc, pl = R.plan(s)
        assert rc == 0 and lib.dgppo_gemm_partial_rows(ctypes.byref(R.fill_args(s))) == pl.grid
        assert pl.units == -(-M // 32) and pl.grid == min(-(-pl.units // 4), 512)
    assert lib.dgppo_gemm_partial_rows(ctypes.byref(R.fill_args(R.Spec(77, 64, 300)))) == 0


# ---- the B staging loop's index split ------------------------------------------------------------------------------------------
def test_float_reciprocal_index_split_is_exact():
    """csrc/gemm.hip stages op(B) with e -> (e / dv, e % dv) computed as int((e + 0.5f) * (1.0f / dv)) in float32, for
    every minor extent dv the three row kernels use and every e the loop forms (the LDS limit plus one pass)."""
    e = np.arange(12800 + 4096, dtype=np.int64)
    ef = e.astype(F32) + F32(0.5)
    for dv in sorted({32 * j for j in range(1, 7)} | {16 * j for j in range(1, 17)}):
        inv = F32(1.0) / F32(dv)
        q = (ef * inv).astype(np.int32)
        assert (ef * inv).dtype == F32
        assert np.array_equal(q, e // dv), dv
