"""Every kernel of csrc/gemm.hip that dgppo_gemm can reach, called through ctypes (so stride_add, ld_mask ... are
reachable) and compared with the float64 restatement of tests/gemm_ref.py.  dgppo_gemm_plan names the kernel each case
runs; the case table of the first test is generated from the plan sweep (tests/test_gemm_ref_cpu.py proves that it
reaches every reachable kernel key).

Conventions of every case (Case of tests/test_primitives_gpu.py): 64 guard floats on both sides of every buffer;
outputs NaN-filled, or integer / random non-zero values when beta != 0; every element of A, B, addend and mask outside
op(A) / op(B) / the (M, N) view is NaN, so any read outside them poisons the result; every output element outside the
reference's touched set must come back bit-identical; one synchronize per case; time and worst error / bound printed.
Classes (gemm_ref): exact (integers: any summation order is exact), close ((K + 8) 2^-24 S, derived), and for the
LayerNorm epilogues prim_ref.check_close / check_sums with the ambiguous gates left out."""
import ctypes

import numpy as np
import pytest
import torch

import gemm_ref as R
import prim_ref as P
from dgppo_fov_amd import _lib
from test_primitives_gpu import Case

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
_INPUTS = ("A", "B", "addend", "mask", "bias", "ln_scale", "ln_bias")
_OUTPUTS = ("C", "bias_grad", "ln_h", "ln_mean", "ln_rstd")


def launch(c, s, bufs, cls="exact", want_key=None, shared=None):
    """Upload, plan, call dgppo_gemm; returns the function that compares after the case's synchronize (it returns the
    outputs as numpy arrays).  shared: device tensors to use instead of fresh uploads (name -> tensor)."""
    lib = _lib.load()
    dev = dict(shared or {})
    for k in _INPUTS:
        if k in bufs and k not in dev:
            dev[k] = c.inp(bufs[k])
    for k in _OUTPUTS:
        if k in bufs and k not in dev:
            dev[k] = c.out(bufs[k].size, init=bufs[k])
    ptr = {k: v.data_ptr() for k, v in dev.items()}
    if s.epi == 3:  # sized from the plan's grid before the buffer exists, as nn.kernels.gemm does
        rows = lib.dgppo_gemm_partial_rows(ctypes.byref(R.fill_args(s, dict(ptr, ln_part=1 << 40))))
        dev["ln_part"] = c.out(rows * 128)
        ptr["ln_part"] = dev["ln_part"].data_ptr()
    nws = lib.dgppo_gemm_workspace_floats(ctypes.byref(R.fill_args(s, ptr)))
    if nws:
        dev["workspace"] = c.out(nws)
        ptr["workspace"] = dev["workspace"].data_ptr()
    g = R.fill_args(s, ptr)
    pl = _lib.GemmPlan()
    assert lib.dgppo_gemm_plan(ctypes.byref(g), ctypes.byref(pl)) == 0, s
    k = R.key(pl, s.K)
    assert want_key is None or k == want_key, (s, k, want_key)
    assert not hasattr(s, "expect") or R.expect_of(pl) == s.expect, (s, R.expect_of(pl), s.expect)
    assert lib.dgppo_gemm(ctypes.byref(g), _lib.stream_handle(c.dev)) == 0, s
    part_rows = pl.grid if s.epi == 3 else 0

    def finish():
        outs, touched, mag = R.reference(s, bufs, part_rows=part_rows)
        got = {}
        for name in [n for n in _OUTPUTS if n in bufs and (n == "C" or n in touched)]:
            a = c.get(dev[name], nan_ok=True).reshape(-1)
            got[name] = a
            t = touched[name]
            assert t.size and a.size == bufs[name].size, s
            rest = np.ones(a.size, bool)
            rest[t] = False
            P.check_bits(a[rest], bufs[name][rest], f"{s}: {name} outside the call's extent")
            assert not np.isnan(a[t]).any(), f"{s}: NaN in {name}"
            if s.epi in (2, 3):
                continue  # the LayerNorm classes: check_ln below
            if cls == "exact":
                c.add(P.check_exact(a[t], outs[name][t], f"{s}: {name}"))
            else:
                m = mag[t] if name == "C" else outs["bias_grad_mag"]
                c.add(P._ratio(np.abs(a[t].astype(F64) - outs[name][t]), R.close_bound(s, m), f"{s}: {name}"))
        if s.epi == 3:  # the forward's h / mean / rstd are inputs here: the backward must leave them as they were
            for name in ("ln_h", "ln_mean", "ln_rstd"):
                P.check_bits(c.get(dev[name]).reshape(-1), bufs[name], f"{s}: {name} is read-only for epi 3")
        if "ln_part" in dev:
            got["ln_part"] = c.get(dev["ln_part"]).reshape(-1, 128)
            assert got["ln_part"].shape[0] == pl.grid
        got["plan"], got["ref"], got["dev"] = pl, outs, dev
        if s.epi in (2, 3):
            check_ln(c, s, bufs, got, outs, R.reference(s, bufs, dt=F32, part_rows=part_rows)[0])
        return got

    return finish


def check_ln(c, s, bufs, got, r64, r32):
    """The LayerNorm epilogues under prim_ref's classes (float32 restatement as floor, ambiguous gates left out)."""
    mat = lambda a: np.asarray(a)[:s.M * 64].reshape(s.M, 64)  # noqa: E731
    if s.epi == 2:
        c.add(P.check_close(got["ln_h"], r64["ln_h"], r32["ln_h"], what=f"{s}: ln_h"))
        c.add(P.check_close(got["ln_mean"], r64["ln_mean"], r32["ln_mean"], what=f"{s}: mean"))
        c.add(P.check_close(got["ln_rstd"], r64["ln_rstd"], r32["ln_rstd"], scale=r64["rstd_scale"], what=f"{s}: rstd"))
        keep = np.abs(r64["pre"]) >= P.AMB * r64["y_scale"]
        c.add(P.check_close(mat(got["C"]), mat(r64["C"]), mat(r32["C"]), scale=r64["y_scale"], keep=keep,
                            what=f"{s}: y"))
        return
    amb = r64["amb"]
    assert P.amb_ok(amb), s
    c.add(P.check_close(mat(got["C"]), mat(r64["C"]), mat(r32["C"]), scale=1 + r64["dx_scale"],
                        keep=~amb.any(-1, keepdims=True), what=f"{s}: dx"))
    xh = np.abs((mat(bufs["ln_h"]).astype(F64) - bufs["ln_mean"][:, None]) * bufs["ln_rstd"][:, None])
    dy = np.abs(r64["dy"])
    part = got["ln_part"].astype(F64).sum(0)
    c.add(P.check_sums(part[:64], r64["ln_dscale"], r64["ds_mag"], slack=(amb * dy * xh).sum(0), what=f"{s}: dscale"))
    c.add(P.check_sums(part[64:], r64["ln_dbias"], r64["db_mag"], slack=(amb * dy).sum(0), what=f"{s}: dbias"))


def run_all(c, jobs):
    """jobs: (Spec, seed, class[, key]) -> launch everything, synchronize once, compare."""
    fins = [launch(c, s, R.make_inputs(s, seed, cls), cls, *rest) for s, seed, cls, *rest in jobs]
    c.sync()
    return [f() for f in fins]


# ---- every kernel key ----------------------------------------------------------------------------------------------------
GROUPS = [("rows", "prefetch"), ("rows", "breg"), ("rows", "plain"), ("wgrad",), ("tile",)]


@pytest.mark.parametrize("group", GROUPS, ids=["-".join(g) for g in GROUPS])
def test_every_kernel_key(cuda, group):
    """One exact case per kernel key of the sweep (M = 77: three panels, the last with 13 rows), M = 1 for one key per
    form, one close case per (form, k-chunk count)."""
    c = Case(cuda, f"gemm keys {' '.join(group)}")
    table = [(k, cfg) for k, cfg in R.case_table(R.sweep()[0]) if k[:len(group)] == group]
    assert table
    jobs = [(R._spec_for(*cfg), 100 + i, "exact", k) for i, (k, cfg) in enumerate(table)]
    k0, cfg0 = table[0]
    if group[0] == "rows":
        jobs.append((R._spec_for(1, *cfg0[1:]), 7, "exact", k0))
        seen = set()
        for k, cfg in table:  # close: one per (form, nch); K <= 256 on the row paths
            if (k[4], k[5]) not in seen and k[6] == 3 and k[7] == 0:
                seen.add((k[4], k[5]))
                jobs.append((R._spec_for(*cfg), 9, "close", k))
    else:
        jobs.append((R._spec_for(*cfg0), 9, "close", k0))
    run_all(c, jobs)
    print(f"[gemm] {len(table)} keys, {len(jobs)} calls")
    c.done()


# ---- a second work unit per wave ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,ncg", sorted(R.SECOND_UNIT))
def test_second_unit_per_wave(cuda, form, ncg):
    """M from the plan: the smallest panel count with units > 4 grid, plus three panels and five rows, so every wave
    prefetches and hands over a next unit (and the LayerNorm backward accumulates its column partials across units)."""
    c = Case(cuda, f"gemm second unit {form} ncg={ncg}")
    N, K = R.SECOND_UNIT[(form, ncg)]
    base = R.Spec(64, N, K, name=f"second unit {form}")
    M = R.second_unit_M(base)
    jobs = [(base.but(M=M, bias=1, alpha=0.5), 1, "exact")]
    if ncg == 1:
        jobs += [(base.but(M=M, addend=1, beta=-2.0, relu=1), 2, "exact"),
                 (base.but(M=M, epi=1, beta=0.5), 3, "exact")]
    for r in run_all(c, jobs):
        pl = r["plan"]
        print(f"[gemm] {form} ncg={pl.ncg}: M={M} units={pl.units} grid={pl.grid} (units > 4 grid: {pl.units > 4 * pl.grid})")
        assert pl.units > 4 * pl.grid and pl.ncg == ncg
        assert R.FORM_NAMES[pl.form] == ("plain" if form == "scalar" else form) and pl.vec == (form != "scalar")
    c.done()


@pytest.mark.parametrize("k", range(len(R.LN_K)), ids=list(R.LN_K))
def test_second_unit_layernorm_epilogues(cuda, k):
    """epi 2, then epi 3 on the forward's own ln_h / mean / rstd (the device buffers are shared), M from the plan so
    that every wave takes a second unit and the backward accumulates its column partials across units: forward
    statistics and y close; dx close; dscale / dbias under check_sums with the slack of the ambiguous gates; the
    backward's gates equal to the forward's by the integer count (a call with dy = 1: its dbias partials sum to the
    number of open gates per column, exact in any order, and must equal the count of y > 0 of the forward)."""
    s, seed = R.ln_specs()[k]
    c = Case(cuda, f"gemm {s.name} M={s.M} K={s.K}")
    bufs = R.make_inputs(s, seed, "close")
    fwd = launch(c, s, bufs, "close")
    c.sync()
    f = fwd()
    pl = f["plan"]
    print(f"[gemm] {s.name}: units={pl.units} grid={pl.grid} form={R.FORM_NAMES[pl.form]} vec={pl.vec}")
    assert pl.units > 4 * pl.grid
    # backward on what the forward stored (device buffers shared: the same bits)
    s3 = s.but(epi=3, name=s.name + " bwd")
    b3 = R.make_inputs(s3, seed + 1, "close")
    b3.update(ln_scale=bufs["ln_scale"], ln_bias=bufs["ln_bias"], ln_h=f["ln_h"], ln_mean=f["ln_mean"],
              ln_rstd=f["ln_rstd"])
    shared = {n: f["dev"][n] for n in ("ln_scale", "ln_bias", "ln_h", "ln_mean", "ln_rstd")}
    bwd = launch(c, s3, b3, "close", shared=shared)
    # gate count: B = 0, bias = 1 -> dy = 1 everywhere: dbias[col] = number of rows whose gate is open, an integer
    # below 2^24, exact in any order; the forward's gates are y > 0
    s1 = s3.but(name=s.name + " gate count")
    b1 = dict(b3, B=np.where(np.isnan(b3["B"]), b3["B"], F32(0)), bias=np.ones(64, F32))
    cnt = launch(c, s1, b1, "close", shared=shared)
    c.sync()
    bwd()
    gc = cnt()
    y = f["C"][:s.M * 64].reshape(s.M, 64)
    P.check_exact(gc["ln_part"][:, 64:].astype(F64).sum(0), (y > 0).sum(0), "open gates per column: backward == forward")
    c.done()


# ---- address modes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["prefetch", "breg", "plain", "scalar", "tile", "wgrad"])
def test_address_modes(cuda, form):
    """Every address mode production uses (gemm_ref.address_specs), exact class, plus one close run of each; every
    call is held to the kernel its Spec names (the two LDS-limit fall-throughs to the tiled kernel among them)."""
    c = Case(cuda, f"gemm address modes {form}")
    specs = R.address_specs(form)
    jobs = [(s, 200 + i, "exact") for i, s in enumerate(specs)]
    jobs += [(s, 300 + i, "close") for i, s in enumerate(specs) if s.K <= 300]
    res = run_all(c, jobs)
    # launch() held every call to its Spec's `expect` (path, row form and load width, or flat rows on wgrad)
    assert all(R.expect_of(r["plan"]) == sp.expect for r, (sp, _, _) in zip(res, jobs))
    want = {"tile": (R.TILE,), "wgrad": (R.WGRAD, 1), "prefetch": (R.ROWS, R.PREFETCH, 1), "breg": (R.ROWS, R.BREG, 1),
            "plain": (R.ROWS, R.PLAIN, 1), "scalar": (R.ROWS, R.PLAIN, 0)}[form]
    assert sum(sp.expect == want for sp in specs) >= 10, form
    if form == "wgrad":  # repeated calls: bit-identical (fixed-order chunk and wave sums)
        again = run_all(c, jobs[len(specs):])
        for a, b in zip(res[len(specs):], again):
            P.check_bits(a["C"], b["C"], "repeated wgrad call")
            if "bias_grad" in a:
                P.check_bits(a["bias_grad"], b["bias_grad"], "repeated wgrad call, bias_grad")
    c.done()


def test_epilogue_bits_do_not_depend_on_the_path(cuda):
    """The claim above epi_combine: rows / prefetch / B-in-registers / tiled / split-K reduce round the epilogue alike,
    as (alpha acc + bias) + (beta C + addend).  gemm_ref.epilogue_inputs: A, B integers (the accumulator is exact on
    every path), bias / C / addend random floats, alpha = 0.5, beta = 0.3.  Every path must give the bits of the
    float32 restatement of that order (a kernel set that swapped the order on every path would still agree with
    itself); the tiled kernel runs the same problem from the transposed storage of A and B."""
    c = Case(cuda, "gemm epilogue bits rows == tile == float32 restatement")
    fins = []
    for (N, K) in R.FORM_SHAPE.values():
        for relu, addend in ((1, 1), (0, 0)):
            s = R.Spec(77, N, K, bias=1, addend=addend, beta=0.3, alpha=0.5, relu=relu)
            bufs = R.epilogue_inputs(s, 17 + K)
            st = s.but(ta=1, tb=1, lda=77, ldb=K)
            bt = dict(bufs, A=np.concatenate([bufs["A"][:77 * K].reshape(77, K).T.reshape(-1), np.full(3, np.nan, F32)]),
                      B=np.concatenate([bufs["B"][:K * N].reshape(K, N).T.reshape(-1), np.full(3, np.nan, F32)]))
            ss = st.but(split_k=3)
            ref32, touched, _ = R.reference(s, bufs, dt=F32)
            fins.append(([launch(c, x, b, "close") for x, b in ((s, bufs), (st, bt), (ss, bt))], ref32["C"], touched["C"]))
    c.sync()
    forms = set()
    for trio, ref32, t in fins:
        a, b, d = [f() for f in trio]
        assert a["plan"].path == R.ROWS and b["plan"].path == R.TILE and d["plan"].split_k == 3
        forms.add((a["plan"].form, a["plan"].vec))
        assert ref32.dtype == F32
        P.check_bits(a["C"][t], ref32[t], "rows vs the float32 restatement of the contract's order")
        P.check_bits(b["C"][t], ref32[t], "tile vs the float32 restatement")
        P.check_bits(d["C"][t], ref32[t], "split-K vs the float32 restatement")
    assert forms == {(R.PREFETCH, 1), (R.BREG, 1), (R.PLAIN, 1), (R.PLAIN, 0)}
    c.done()


# ---- grouped weight gradients ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [13, 25])
def test_grouped_wgrad_many_problems(cuda, n):
    """More than 12 problems: two / three launch pairs with the workspace offsets carried across; mixed shapes, some
    with one chunk (written directly, no workspace); every output bit-identical to its own dgppo_gemm call; the
    workspace and every buffer guarded."""
    c = Case(cuda, f"gemm grouped wgrad n={n}")
    lib = _lib.load()
    shapes = [(40, 70, 300), (8, 27, 50), (64, 64, 1025), (3, 5, 2), (111, 64, 129), (32, 99, 128), (128, 128, 700)]
    specs = []
    for i in range(n):
        M, N, K = shapes[i % len(shapes)]
        kw = [dict(), dict(bias_grad=1, beta=1.0), dict(batch=2, bias_grad=1), dict(lda=M + 3, a_grp=7, a_gs=9 * (M + 3)),
              dict(ldc=N + 3, c_grp=5, c_gs=5 * (N + 3) + 2, beta=1.0)][i % 5]
        specs.append(R.Spec(M, N, K + i, ta=1, alpha=0.5, name=f"grouped {i}", **kw))
    single = run_all(c, [(s, 400 + i, "close") for i, s in enumerate(specs)])
    args, outs = [], []
    for i, s in enumerate(specs):
        bufs = R.make_inputs(s, 400 + i, "close")
        dev = {k: single[i]["dev"][k] for k in ("A", "B")}  # the same inputs
        for k in ("C", "bias_grad"):
            if k in bufs:
                dev[k] = c.out(bufs[k].size, init=bufs[k])
        args.append(R.fill_args(s, {k: v.data_ptr() for k, v in dev.items()}))
        outs.append(dev)
    arr = (_lib.GemmArgs * n)(*args)
    nws = lib.dgppo_gemm_wgrad_grouped_workspace_floats(arr, n)
    assert nws > 0 and any(R.plan(s)[1].chunks == 1 for s in specs) and any(R.plan(s)[1].chunks > 1 for s in specs)
    ws = c.out(nws)
    assert lib.dgppo_gemm_wgrad_grouped(arr, n, ws.data_ptr(), _lib.stream_handle(cuda)) == 0
    c.sync()
    for i, s in enumerate(specs):
        for k in ("C", "bias_grad"):
            if k in outs[i]:
                P.check_bits(c.get(outs[i][k], nan_ok=True).reshape(-1), single[i][k], f"{s}: {k}")
    c.done()


# ---- kernels only the environment knobs select ------------------------------------------------------------------------------
def _knob_table(default_keys):
    """The case table of this process's knobs, cut down to the keys the default knobs do not reach."""
    return [(k, cfg) for k, cfg in R.case_table(R.sweep()[0]) if k not in default_keys]


def _knob_child(keys_path, out_path):
    """Runs in a child process under one knob set: the exact-class table of the keys the set adds; saves the outputs."""
    import json

    default_keys = {tuple(k) for k in json.load(open(keys_path))}
    dev = torch.device("cuda", 0)
    c = Case(dev, "gemm knob child")
    table = _knob_table(default_keys)
    res = run_all(c, [(R._spec_for(*cfg), 500 + i, "exact", k) for i, (k, cfg) in enumerate(table)])
    c.done()
    out = {"cfgs": np.array(json.dumps([list(cfg) for _, cfg in table]))}
    for i, r in enumerate(res):
        for name in _OUTPUTS + ("ln_part",):
            if name in r:
                out[f"{name}:{i}"] = r[name]
    np.savez(out_path, **out)


_CHILD_FAULTED = []


@pytest.mark.parametrize("k", range(len(R.KNOB_SETS)), ids=["+".join(f"{a[6:]}={b}" for a, b in ks.items())
                                                            for ks in R.KNOB_SETS])
def test_knob_selected_kernels(cuda, tmp_path, k):
    """One GPU child process per knob set (the knobs are read once per process), one after another: the child runs the
    exact-class cases of the kernel keys its set adds; here they are held equal to the float64 reference and, bit for
    bit, to the default-knob kernels' results on the same inputs.  After a child that did not end with status 0 (a
    fault, an abort, a hang killed at its time limit, any error) no further child is started."""
    import json
    import os
    import subprocess
    import sys

    if _CHILD_FAULTED:
        pytest.fail(f"not started: the child of {_CHILD_FAULTED[0]} did not end with status 0")
    here = os.path.dirname(os.path.abspath(__file__))
    knobs = R.KNOB_SETS[k]
    keys_path, out_path = tmp_path / "default_keys.json", tmp_path / "child.npz"
    keys_path.write_text(json.dumps(sorted(R.sweep()[0])))
    code = (f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); "
            f"import test_gemm_paths_gpu as T; T._knob_child({str(keys_path)!r}, {str(out_path)!r})")
    try:
        rc = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **knobs), timeout=120).returncode
    except subprocess.TimeoutExpired:
        rc = "a hang (killed at its time limit)"
    if rc != 0:  # a fault, an abort, a hang or any other failure on the GPU: nothing further is started on it
        _CHILD_FAULTED.append(knobs)
        pytest.fail(f"child of {knobs} ended with {rc}")
    z = np.load(out_path)
    cfgs = [tuple(cfg) for cfg in json.loads(str(z["cfgs"]))]
    assert cfgs, knobs
    c = Case(cuda, f"gemm knobs {knobs}")
    mine = run_all(c, [(R._spec_for(*cfg), 500 + i, "exact") for i, cfg in enumerate(cfgs)])  # default-knob kernels
    for i, (cfg, r) in enumerate(zip(cfgs, mine)):
        s = R._spec_for(*cfg)
        bufs = R.make_inputs(s, 500 + i, "exact")
        child = {name: z[f"{name}:{i}"] for name in _OUTPUTS + ("ln_part",) if f"{name}:{i}" in z}
        rows = child["ln_part"].shape[0] if "ln_part" in child else 0
        outs, touched, _ = R.reference(s, bufs, part_rows=rows)
        if s.epi in (2, 3):  # the LayerNorm classes against float64, on the child's own outputs
            check_ln(c, s, bufs, child, outs, R.reference(s, bufs, dt=F32, part_rows=rows)[0])
        else:
            c.add(P.check_exact(child["C"][touched["C"]], outs["C"][touched["C"]], f"{knobs} {s}"))
        for name in [n for n in _OUTPUTS if n in child]:
            P.check_bits(child[name], r[name], f"{knobs} {s}: {name}, child vs default knobs")
        if "bias_grad" in child:
            c.add(P.check_exact(child["bias_grad"], outs["bias_grad"], f"{knobs} {s}: bias_grad"))
    print(f"[gemm] {knobs}: {len(cfgs)} added kernel keys")
    c.done()
