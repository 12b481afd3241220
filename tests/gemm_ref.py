"""NumPy restatement of dgppo_gemm (include/dgppo_hip.h) and the tables the GEMM tests share (helper, not a test;
tests/test_gemm_ref_cpu.py checks it, tests/test_gemm_paths_gpu.py compares the kernels of csrc/gemm.hip with it).

The reference is written from the header's contract, never from a kernel: every operand is a flat float buffer plus an
element offset, every element is addressed as (r // grp) * gstride + (r % grp) * ld (+ batch stride), and the result is
(alpha acc + bias) + (beta C + addend), ReLU last, then the fused epilogue (epi 1 mask, epi 2 / 3 the LayerNorm(64)
restatements of prim_ref).  `reference` also returns, per output buffer, the flat indices the call may write.

Comparison classes (prim_ref's):
  exact   A, B integers in [-3, 3], alpha / beta powers of two, integer bias / C / addend: every partial sum is a
          multiple of 1/4 far below 2^24, so any fp32 summation order gives the float64 result exactly
  close   random normal inputs: |got - ref64| <= (K + 8) 2^-24 S elementwise, S = sum_k |alpha a b| + |bias| +
          |beta c| + |addend| -- the first-order worst case of ANY fp32 summation order of K products (each partial
          sum is bounded by S and rounded once per addition: at most K - 1 additions, K product roundings folded into
          the fma, and the epilogue's four operations)
  LayerNorm epilogues: prim_ref.check_close with the float32 restatement as floor and the ambiguous gates left out

The kernel key (`key`) is the template instantiation of csrc/gemm.hip a call reaches, read from dgppo_gemm_plan.
"""
import ctypes
import functools
import itertools

import numpy as np

import prim_ref as P
from dgppo_fov_amd import _lib

F32, F64 = np.float32, np.float64
TILE, ROWS, WGRAD = 0, 1, 2
PLAIN, PREFETCH, BREG = 0, 1, 2
FORM_NAMES = {PLAIN: "plain", PREFETCH: "prefetch", BREG: "breg"}

_DEFAULTS = dict(batch=1, ta=0, tb=0, lda=None, ldb=None, ldc=None, sa=None, sb=None, sc=None, a_off=0, b_off=0,
                 c_off=0, a_grp=0, b_grp=0, c_grp=0, a_gs=0, b_gs=0, c_gs=0, bias=0, addend=0, ld_add=None, s_add=0,
                 add_off=0, add_grp=0, add_gs=0, alpha=1.0, beta=0.0, relu=0, split_k=1, bias_grad=0, epi=0,
                 ld_mask=None, mask_off=0, name="")


def _rowoff(r, ld, grp, gs):
    return r * ld if grp <= 0 else (r // grp) * gs + (r % grp) * ld


class Spec:
    """The fields of dgppo_gemm_args with element offsets in place of pointers.  Leading dimensions default to the
    dense ones, batch strides to the extent of one entry (addend: 0, as nn.kernels.gemm passes it)."""

    def __init__(self, M, N, K, **kw):
        bad = set(kw) - set(_DEFAULTS)
        assert not bad, bad
        self.__dict__.update(_DEFAULTS, M=M, N=N, K=K, **kw)
        s = self
        s.lda = (M if s.ta else K) if s.lda is None else s.lda
        s.ldb = (K if s.tb else N) if s.ldb is None else s.ldb
        s.ldc = N if s.ldc is None else s.ldc
        s.ld_add = N if s.ld_add is None else s.ld_add
        s.ld_mask = N if s.ld_mask is None else s.ld_mask
        for st, which in (("sa", "A"), ("sb", "B"), ("sc", "C")):
            if getattr(s, st) is None:
                setattr(s, st, 0)
                setattr(s, st, s._extent(which) + 3 if s.batch > 1 and min(M, N, K) > 0 else 0)

    def _extent(self, which):
        """One past the largest index of batch entry 0 (positive strides: the last row, or the last row of the last
        whole group)."""
        s = self
        off, R, Cn, ld, grp, gs = {"A": (s.a_off,) + ((s.K, s.M) if s.ta else (s.M, s.K)) + (s.lda, s.a_grp, s.a_gs),
                                   "B": (s.b_off,) + ((s.N, s.K) if s.tb else (s.K, s.N)) + (s.ldb, s.b_grp, s.b_gs),
                                   "C": (s.c_off, s.M, s.N, s.ldc, s.c_grp, s.c_gs)}[which]
        rows = {R - 1} | ({(R - 1) // grp * grp - 1} if grp > 0 and R > grp else set())
        return off + max(_rowoff(r, ld, grp, gs) for r in rows) + Cn

    def but(self, **kw):
        d = {k: v for k, v in self.__dict__.items() if k in _DEFAULTS}
        d.update(kw)
        return Spec(kw.pop("M", self.M), kw.pop("N", self.N), kw.pop("K", self.K),
                    **{k: v for k, v in d.items() if k not in ("M", "N", "K")})

    def idx(self, which, b):
        """Flat index of every element of op(A) (M, K), op(B) (K, N), C / addend / mask (M, N) of batch entry b."""
        s = self
        ar = np.arange
        if which == "A":
            R, Cn = (s.K, s.M) if s.ta else (s.M, s.K)
            i = s.a_off + b * s.sa + _rowoff(ar(R), s.lda, s.a_grp, s.a_gs)[:, None] + ar(Cn)[None]
            return i.T if s.ta else i
        if which == "B":
            R, Cn = (s.N, s.K) if s.tb else (s.K, s.N)
            i = s.b_off + b * s.sb + _rowoff(ar(R), s.ldb, s.b_grp, s.b_gs)[:, None] + ar(Cn)[None]
            return i.T if s.tb else i
        if which == "C":
            return s.c_off + b * s.sc + _rowoff(ar(s.M), s.ldc, s.c_grp, s.c_gs)[:, None] + ar(s.N)[None]
        if which == "addend":
            return s.add_off + b * s.s_add + _rowoff(ar(s.M), s.ld_add, s.add_grp, s.add_gs)[:, None] + ar(s.N)[None]
        if which == "mask":  # addressed with C's grouping; no batch stride: every entry reads the same mask
            return s.mask_off + _rowoff(ar(s.M), s.ld_mask, s.c_grp, s.c_gs)[:, None] + ar(s.N)[None]
        raise KeyError(which)

    def size(self, which):
        if min(self.M, self.N) == 0 or (which in "AB" and self.K == 0):
            return 4
        return max(int(self.idx(which, b).max()) for b in range(self.batch)) + 1 + 3  # three floats of tail padding

    def __repr__(self):
        d = {k: v for k, v in self.__dict__.items() if k in _DEFAULTS and v != _DEFAULTS[k] and k != "name"}
        return f"{self.name} M={self.M} N={self.N} K={self.K} " + " ".join(f"{k}={v}" for k, v in d.items())


def make_inputs(s, seed, cls="exact"):
    """Buffers of a case: every element a call may read holds a value, every other element of A, B, addend and mask is
    NaN (a read outside op(A) / op(B) poisons the result).  C is NaN everywhere, or values everywhere when beta != 0."""
    rng = np.random.default_rng(seed)
    ints = cls == "exact"
    val = (lambda n, lim=3: rng.integers(-lim, lim + 1, n).astype(F32)) if ints else \
        (lambda n, lim=3: rng.standard_normal(n).astype(F32))
    bufs = {}
    for which in ("A", "B") + (("addend",) if s.addend else ()) + (("mask",) if s.epi == 1 else ()):
        buf = np.full(s.size(which), np.nan, F32)
        for b in range(s.batch):
            i = s.idx(which, b)
            buf[i] = rng.integers(-1, 3, i.shape).astype(F32) if which == "mask" else val(i.size, 8 if which == "addend" else 3).reshape(i.shape)
        bufs[which] = buf
    n = s.size("C")
    if s.beta != 0:
        c = val(n, 8)
        bufs["C"] = np.where(c == 0, F32(1), c)
    else:
        bufs["C"] = np.full(n, np.nan, F32)
    if s.bias:
        bufs["bias"] = val(s.N, 8)
    if s.bias_grad:
        bufs["bias_grad"] = val(s.batch * s.N, 8) if s.beta != 0 else np.full(s.batch * s.N, np.nan, F32)
    if s.epi in (2, 3):
        bufs["ln_scale"] = (1 + 0.3 * rng.standard_normal(64)).astype(F32)
        bufs["ln_bias"] = (0.2 * rng.standard_normal(64)).astype(F32)
        for k, n in (("ln_h", s.M * 64), ("ln_mean", s.M), ("ln_rstd", s.M)):
            bufs[k] = np.full(n, np.nan, F32)
        if s.epi == 3:  # a forward's outputs (a caller with a real forward puts its own in their place)
            h = (rng.standard_normal((s.M, 64)) * 2 + 0.5).astype(F32)
            _, _, mean, rstd, _, _ = P.layernorm_fwd(h, bufs["ln_scale"], bufs["ln_bias"], True)
            bufs.update(ln_h=h.reshape(-1), ln_mean=mean.astype(F32), ln_rstd=rstd.astype(F32))
    return bufs


def reference(s, bufs, dt=F64, part_rows=0, mutate=None):
    """(outs, touched, mag): outs[name] the whole output buffer after the call (in dt), touched[name] the sorted flat
    indices the call may write, mag the summand magnitudes S of C's elements (flat, 0 where untouched).  epi 2 / 3 also
    return ln_* outputs; epi 3's ln_part is returned as its column sums `ln_dscale` / `ln_dbias` (the host sums the
    partial rows) with touched["ln_part"] = part_rows * 128 floats.  mutate: a negative control (see the CPU file)."""
    f = lambda name: bufs[name].astype(dt)  # noqa: E731
    A, B = f("A"), f("B")
    outs = {"C": f("C")}
    mag = np.zeros(outs["C"].size, F64)
    touched = {"C": []}
    alpha, beta = dt(s.alpha), dt(s.beta)
    wgrad = bool(s.bias_grad)
    if wgrad:
        outs["bias_grad"] = f("bias_grad")
        touched["bias_grad"] = np.arange(s.batch * s.N)
    bias = f("bias") if s.bias else np.zeros(s.N, dt)
    for b in range(s.batch):
        a, bm = A[s.idx("A", b)], B[s.idx("B", b)]
        if mutate == "wgrad_row_dropped" and s.ta:
            a = a.copy()
            a[:, s.K // 2] = 0
        acc = a @ bm if s.K else np.zeros((s.M, s.N), dt)
        S = abs(s.alpha) * (np.abs(a).astype(F64) @ np.abs(bm).astype(F64)) + np.abs(bias)
        ic = s.idx("C", b - 1 if mutate == "batch_c_stride" and b == s.batch - 1 and b > 0 else b)
        if mutate == "batch_c_stride" and b == s.batch - 1 and b > 0:
            ic = ic + s.sc - 1
        v = alpha * acc + bias
        x = None
        if s.beta != 0:
            x = beta * outs["C"][ic]
            S = S + np.abs(x)
        if s.addend:
            ia = s.idx("addend", b)
            if mutate == "addend_gstride" and s.add_grp > 0:
                ia = s.but(add_gs=s.add_gs + s.ld_add if s.ld_add else s.add_gs + s.N).idx("addend", b)
            d = f("addend")[np.minimum(ia, bufs["addend"].size - 1)]
            x = d if x is None else x + d
            S = S + np.abs(d)
        if mutate == "epilogue_order" and x is not None:
            v = alpha * acc + (bias + x)
        elif x is not None:
            v = v + x
        if s.relu:
            v = np.maximum(v, 0)
        if s.epi == 1:
            im = s.idx("mask", b)
            if mutate == "mask_next_row":
                im = np.minimum(im + s.ld_mask, bufs["mask"].size - 1)
            v = np.where(bufs["mask"][im] > 0, v, dt(0))
        if s.epi == 2:
            y, pre, mean, rstd, y_scale, rstd_scale = P.layernorm_fwd(v, bufs["ln_scale"], bufs["ln_bias"], True, dt=dt)
            outs.update(ln_h=v.reshape(-1), ln_mean=mean, ln_rstd=rstd, y_scale=y_scale, rstd_scale=rstd_scale,
                        pre=pre)
            for k, n in (("ln_h", s.M * 64), ("ln_mean", s.M), ("ln_rstd", s.M)):
                touched[k] = np.arange(n)
            v = y
        if s.epi == 3:
            h, mean, rstd = f("ln_h").reshape(s.M, 64), f("ln_mean"), f("ln_rstd")
            sc, bi = f("ln_scale"), f("ln_bias")
            pre = ((h - mean[:, None]) * rstd[:, None]) * sc + bi
            dx, ds, db, ds_mag, db_mag, dx_scale = P.layernorm_bwd(h, v, sc, mean, rstd, pre > 0, dt=dt)
            pre_scale = np.abs(sc) * (np.abs(h) + np.abs(mean)[:, None]) * np.abs(rstd)[:, None] + np.abs(bi)
            outs.update(ln_dscale=ds, ln_dbias=db, ds_mag=ds_mag, db_mag=db_mag, dx_scale=dx_scale, pre=pre,
                        amb=np.abs(pre) < P.AMB * pre_scale, dy=v)
            touched["ln_part"] = np.arange(part_rows * 128)
            v = dx
        outs["C"][ic] = v
        mag[ic] = S
        touched["C"].append(ic.reshape(-1))
        if wgrad:
            col = alpha * bm.sum(0)
            prev = beta * outs["bias_grad"][b * s.N:(b + 1) * s.N] if s.beta != 0 else 0
            outs["bias_grad"][b * s.N:(b + 1) * s.N] = col + prev
            outs.setdefault("bias_grad_mag", np.zeros(s.batch * s.N, F64))[b * s.N:(b + 1) * s.N] = \
                abs(s.alpha) * np.abs(bm).astype(F64).sum(0) + np.abs(prev)
    touched["C"] = np.unique(np.concatenate(touched["C"])) if touched["C"] else np.zeros(0, np.int64)
    return outs, touched, mag


def close_bound(s, mag):
    return (s.K + 8) * 2.0 ** -24 * mag + 1e-30


# ---- ctypes ----------------------------------------------------------------------------------------------------------
_FAKE = {k: (i + 1) << 32 for i, k in enumerate(("A", "B", "C", "bias", "addend", "mask", "bias_grad", "workspace",
                                                  "ln_scale", "ln_bias", "ln_h", "ln_mean", "ln_rstd", "ln_part"))}


def fill_args(s, ptr=None, g=None):
    """dgppo_gemm_args of a Spec; ptr: name -> base address of the buffer (default: fake, 16-byte aligned, non-null
    addresses for the host-only queries)."""
    ptr = _FAKE if ptr is None else ptr
    g = _lib.GemmArgs() if g is None else g
    p = lambda name, off=0: ptr[name] + 4 * off if ptr.get(name) else None  # noqa: E731
    g.M, g.N, g.K, g.batch, g.trans_a, g.trans_b = s.M, s.N, s.K, s.batch, s.ta, s.tb
    g.A, g.lda, g.stride_a = p("A", s.a_off), s.lda, s.sa
    g.B, g.ldb, g.stride_b = p("B", s.b_off), s.ldb, s.sb
    g.C, g.ldc, g.stride_c = p("C", s.c_off), s.ldc, s.sc
    g.a_grp, g.b_grp, g.c_grp, g.a_gstride, g.b_gstride, g.c_gstride = s.a_grp, s.b_grp, s.c_grp, s.a_gs, s.b_gs, s.c_gs
    g.bias = p("bias") if s.bias else None
    g.addend = p("addend", s.add_off) if s.addend else None
    g.ld_add, g.stride_add, g.add_grp, g.add_gstride = s.ld_add, s.s_add, s.add_grp, s.add_gs
    g.alpha, g.beta, g.relu, g.split_k = s.alpha, s.beta, s.relu, s.split_k
    g.workspace = p("workspace")
    g.bias_grad = p("bias_grad") if s.bias_grad else None
    g.epi = s.epi
    g.mask, g.ld_mask = (p("mask", s.mask_off) if s.epi == 1 else None), s.ld_mask
    for k in ("ln_scale", "ln_bias", "ln_h", "ln_mean", "ln_rstd"):
        setattr(g, k, p(k) if s.epi in (2, 3) else None)
    g.ln_part = p("ln_part") if s.epi == 3 else None
    return g


def plan(s, ptr=None):
    """(rc, GemmPlan) of dgppo_gemm_plan."""
    pl = _lib.GemmPlan()
    rc = _lib.load().dgppo_gemm_plan(ctypes.byref(fill_args(s, ptr)), ctypes.byref(pl))
    return rc, pl


def key(pl, K):
    """The kernel instantiation a plan names (plus, on the 16-byte-load forms, whether the last k-chunk is half
    filled, and on wgrad whether a reduce launch follows).  The plain row kernel loops over its k-chunks at run time:
    nch is no template parameter there."""
    if pl.path == ROWS:
        return ("rows", FORM_NAMES[pl.form], pl.ntw, pl.ncg, pl.nch if pl.form != PLAIN else 0, pl.vec, pl.extra,
                pl.epi, int(bool(pl.vec) and K % 16 == 8))
    if pl.path == WGRAD:
        return ("wgrad", pl.mt, pl.nt, pl.unroll, pl.flat, pl.pipe, int(pl.chunks > 1))
    return ("tile", int(pl.split_k > 1))


# ---- the coverage sweep and the case table generated from it ------------------------------------------------------------
N_EDGES = (1,) + tuple(n for e in (32, 64, 96, 128, 160, 192) for n in (e - 1, e, e + 1))
K_ALL = tuple(range(1, 265))
K_SOME = (1, 7, 8, 9, 16, 17, 24, 32, 33, 40, 48, 49, 56, 64, 65, 72, 80, 128, 129, 200, 256, 257, 264)
# everything that turns the 16-byte A loads off (name -> Spec fields given K), and "none"
BREAKERS = {"none": lambda K: {}, "lda%4": lambda K: dict(lda=K + 1), "A+4B": lambda K: dict(a_off=1),
            "a_gs%4": lambda K: dict(a_grp=5, a_gs=5 * K + 1), "sa%4": lambda K: dict(batch=2, sa=None)}
EXTRAS = {0: {}, 1: dict(addend=1), 2: dict(beta=0.5), 3: dict(addend=1, beta=-2.0)}


def _spec_for(M, N, K, ta, tb, brk, extra, epi, batch):
    kw = dict(ta=ta, tb=tb, batch=batch, epi=epi, name=f"{brk}")
    kw.update(EXTRAS[extra])
    if not ta or brk == "a_gs%4":
        kw.update(BREAKERS[brk](M if ta else K))  # the stored row length of A
    if brk == "sa%4":
        kw["sa"] = M * K + 5 if not ta else None
    if ta and not tb and N <= 192 and M <= 4096 and not (extra & 1):
        kw["bias_grad"] = 1 if (N + K) % 2 else 0
    else:
        kw.update(bias=1, alpha=0.5)
    return Spec(M, N, K, **kw)


def sweep_configs():
    """The configurations of the coverage sweep: every K with every N edge and transpose; then every VEC breaker,
    extra, epi, M and batch on a K grid that holds every value at which the host code takes another branch."""
    for N, K, ta, tb in itertools.product(N_EDGES, K_ALL, (0, 1), (0, 1)):
        for M in ((1, 33, 77, 4096, 4097) if ta and not tb else (4096,)):
            yield (M, N, K, ta, tb, "none", 0, 0, 1)
            if ta and not tb and K in K_SOME:  # grouped A rows: the weight-gradient kernel's 32-bit row arithmetic
                yield (M, N, K, ta, tb, "a_gs%4", 0, 0, 1)
    for N, K, tb, brk, extra, epi in itertools.product(N_EDGES, K_SOME, (0, 1), BREAKERS, EXTRAS, (0, 1, 2, 3)):
        for M, batch in ((4096, 1), (4096, 2)) + (((1, 1), (4097, 1)) if extra == 0 and epi == 0 else ()):
            if brk == "sa%4" and batch == 1:
                continue
            yield (M, N, K, 0, tb, brk, extra, epi, batch)
    for N, K, extra in itertools.product(N_EDGES, K_SOME, EXTRAS):  # the wgrad path refuses an addend: tile
        yield (4096, N, K, 1, 0, "none", extra, 0, 2)


@functools.lru_cache(None)
def sweep():
    """key -> the first configuration of the sweep that reaches it (accepted calls only), and the number of calls."""
    lib = _lib.load()
    reps, n = {}, 0
    pl, g = _lib.GemmPlan(), _lib.GemmArgs()
    for cfg in sweep_configs():
        M, N, K = cfg[:3]
        s = _spec_for(*cfg)
        fill_args(s, g=g)
        n += 1
        if lib.dgppo_gemm_plan(ctypes.byref(g), ctypes.byref(pl)) == 0:
            reps.setdefault(key(pl, K), cfg)
    return reps, n


def case_table(reps):
    """One GPU case per reachable key: its sweep representative at M = 77 (three panels, the last with 13 rows); the
    weight-gradient and tiled paths keep their M (the path depends on it)."""
    table = []
    for k, cfg in sorted(reps.items(), key=lambda kv: str(kv[0])):
        M = 77 if k[0] == "rows" else cfg[0]
        table.append((k, (M,) + tuple(cfg[1:])))
    return table


def replan_key(cfg, ptr=None):
    s = _spec_for(*cfg)
    rc, pl = plan(s, ptr)
    return key(pl, s.K) if rc == 0 else None


def coverage():
    """(keys the sweep reaches, keys the case table reaches, plans swept) under this process's knobs."""
    reps, n = sweep()
    return set(reps), {replan_key(cfg) for _, cfg in case_table(reps)}, n


# at most four knob sets (read once per process); together with the defaults they reach every instantiation of
# csrc/gemm.hip but those listed in tests/golden/gemm_unreachable.json ("GEMM tests")
KNOB_SETS = (
    dict(DGPPO_WGRAD_MAXACC="12", DGPPO_ROWS_NTW="3"),
    dict(DGPPO_WGRAD_U="8", DGPPO_ROWS_NTW="6"),
    dict(DGPPO_WGRAD_U="2", DGPPO_WGRAD_PIPE="0", DGPPO_ROWS_BREG="0"),
    dict(DGPPO_WGRAD_MAXACC="12", DGPPO_WGRAD_PIPE="0", DGPPO_ROWS_PF="0"),
)


def template_of(k):
    """The template arguments of a kernel key."""
    if k[0] == "rows":
        _, form, ntw, ncg, nch, vec, extra, epi, half = k
        return ("rows", form, ntw, vec, extra, epi) if form == "plain" else ("rows", form, ntw, nch, extra, epi)
    if k[0] == "wgrad":
        return tuple(k[:6])
    return ("tile",)


def instantiations():
    """Every kernel template instantiation csrc/gemm.hip names, read from its launch macros (the DG_WGRAD_SHAPES list,
    the DG_PF / DG_RB / DG_R expansions and the launch_rows_t<NTW, EPI> calls); only epi_combo's rule is restated."""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dgppo_fov_amd", "csrc",
                            "gemm.hip")).read()
    shapes = re.findall(r"X\((\d), (\d)\)", src[src.index("#define DG_WGRAD_SHAPES"):src.index("// the wgrad fields")])
    shapes = [(int(a), int(b)) for a, b in shapes]
    pf = {(int(c), int(x)) for c, x in re.findall(r"DG_PF\((\d), (\d)\)", src)}
    rb = {(int(c), int(x)) for c, x in re.findall(r"DG_RB\((\d), (\d)\)", src)}
    pl = {(int(v == "true"), int(x)) for v, x in re.findall(r"DG_R\((true|false), (\d)\)", src)}
    epi_id = {"0": 0, "dgppo::kEpiMask": 1, "dgppo::kEpiLnFwd": 2, "dgppo::kEpiLnBwd": 3}
    rows_t = {(int(n), epi_id[e]) for n, e in re.findall(r"launch_rows_t<(\d), ([\w:]+)>\(p, r, s\)", src)}
    assert len(shapes) == 15 and len(pf) == 16 and len(rb) == 16 and len(pl) == 8 and len(rows_t) == 8, "launch macros"
    combo = lambda epi, ntw, x: epi == 0 or (epi == 1 and x in (0, 2)) or (ntw == 2 and x == 0)  # noqa: E731 epi_combo
    out = {("tile",)}
    for ntw, epi in rows_t:
        out |= {("rows", "plain", ntw, v, x, epi) for v, x in pl if combo(epi, ntw, x)}
        out |= {("rows", "prefetch", ntw, c, x, epi) for c, x in pf if combo(epi, ntw, x)}
        out |= {("rows", "breg", ntw, c, x, epi) for c, x in rb if combo(epi, ntw, x)}
    u_forms = re.findall(r"DG_WL\((\d), (true|false), (true|false)\);", src)
    forms = {(int(u), int(f == "true"), int(pp == "true")) for u, f, pp in u_forms}
    assert len(forms) == 9, forms
    for mt, nt in shapes:
        out |= {("wgrad", mt, nt, u, fl, pp) for u, fl, pp in forms}
    return out


# ---- the GPU case lists (also walked by the CPU file) ---------------------------------------------------------------------
FORM_SHAPE = {"prefetch": (40, 32), "breg": (64, 64), "plain": (40, 80), "scalar": (40, 6)}  # form -> (N, K)


def address_specs(form):
    """Every address mode production uses, on one row form, the tiled kernel or the weight-gradient kernel.  Each Spec
    carries `expect`, the kernel it must reach: (TILE,), (WGRAD, flat) or (ROWS, row form, vec)."""
    out = _address_specs(form)
    for s in out:
        if form == "wgrad":
            s.expect = (WGRAD, int(s.a_grp == 0 and s.b_grp == 0))
        elif form == "tile":  # the small untransposed shapes (K = 1, 33) stay on the scalar-load row kernel
            small = not s.ta and s.K <= 33
            s.expect = (ROWS, PLAIN, 0) if small else (TILE,)
        else:
            broken = form == "scalar" or s.lda % 4 or s.a_off % 4 or (s.a_grp > 0 and s.a_gs % 4) or s.K % 8
            f = {"prefetch": PREFETCH, "breg": BREG}.get(form, PLAIN)
            s.expect = (ROWS, PLAIN, 0) if broken else (ROWS, f, 1)
    return out


def expect_of(pl):
    return (TILE,) if pl.path == TILE else (WGRAD, pl.flat) if pl.path == WGRAD else (ROWS, pl.form, pl.vec)


def epilogue_inputs(s, seed):
    """Inputs on which the epilogue's roundings decide the bits: A, B integers (the accumulator is exact on every
    path and in float32), bias / C / addend random floats.  With a power-of-two alpha, alpha acc is exact, so
    fma(alpha, acc, bias) is alpha acc + bias rounded once and reference(dt=float32) -- (alpha acc + bias), then
    beta C, + addend, + -- reproduces epi_combine bit for bit."""
    bufs = make_inputs(s, seed, "exact")
    rng = np.random.default_rng(seed + 1)
    for k in ("bias", "C", "addend"):
        if k in bufs:
            bufs[k] = np.where(np.isnan(bufs[k]), bufs[k], rng.standard_normal(bufs[k].size).astype(F32))
    return bufs


def _address_specs(form):
    M = 77
    if form == "tile":
        out = [Spec(M, N, K, ta=ta, tb=tb, bias=1, name=f"tile {ta}{tb}") for ta in (0, 1) for tb in (0, 1)
               for M, N, K in ((1, 1, 1), (63, 65, 33), (65, 193, 300)) if not (ta and not tb)]
        out += [Spec(M, N, K, ta=1, tb=0, bias=1, name="tile 10 (bias: off the wgrad path)")
                for M, N, K in ((1, 1, 1), (63, 65, 33), (65, 193, 300))]
        out += [Spec(77, 64, 200, name="tile LDS limit K"), Spec(77, 150, 80, name="tile LDS limit N")]
        out += [Spec(65, 70, 300, split_k=k, name=f"tile split_k {k}") for k in (1, 2, 7)]
        out += [Spec(65, 70, 40, ta=1, tb=1, split_k=4, name="tile split_k 4 of K 40: two empty splits"),
                Spec(65, 70, 300, batch=2, split_k=2, bias=1, name="tile batch 2"),
                Spec(65, 70, 300, lda=303, a_grp=5, a_gs=5 * 303 + 2, tb=1, ldb=301, b_grp=3, b_gs=3 * 301 + 1,
                     ldc=73, c_grp=7, c_gs=7 * 73 + 3, addend=1, ld_add=72, add_grp=4, add_gs=4 * 72 + 5, beta=0.5,
                     name="tile a/b/c/add grouping"),
                Spec(65, 70, 300, bias=1, beta=-2.0, addend=1, relu=1, alpha=0.5, name="tile bias beta addend relu")]
        return out
    if form == "wgrad":
        H = 16
        out = [Spec(m, n, 300, ta=1, beta=1.0, bias_grad=1, name=f"wgrad shape M{m} N{n}")
               for m, n in ((8, 27), (20, 40), (20, 70), (20, 99), (33, 20), (40, 40), (77, 20), (128, 20), (20, 192),
                            (20, 130))]
        out += [Spec(40, 70, R, ta=1, alpha=0.5, beta=(R % 2) * 1.0, bias_grad=1, name=f"wgrad rows {R}")
                for R in (1, 2, 3, 127, 128, 129, 1025, 255, 257, 70001)]
        out += [Spec(200, 20, 300, ta=1, bias_grad=1, beta=1.0, name="wgrad gm > 1 with bias_grad"),
                Spec(4096, 5, 130, ta=1, name="wgrad M 4096"),
                Spec(40, 70, 300, ta=1, batch=3, bias_grad=1, beta=1.0, name="wgrad batch 3 bias_grad"),
                Spec(40, H, 300, ta=1, ldb=4 * H, b_off=2 * H, ldc=4 * H, c_off=2 * H, beta=1.0, bias_grad=1,
                     name="wgrad gate block of (R, 4H) / (M, 4H)"),
                Spec(40, 70, 300, ta=1, lda=45, a_grp=7, a_gs=9 * 45, b_grp=5, b_gs=6 * 75, ldb=75, b_off=3,
                     name="wgrad a_grp != b_grp, b_off"),
                Spec(40, 70, 300, ta=1, b_grp=5, b_gs=6 * 70 + 1, name="wgrad b_grp alone"),
                Spec(40, 70, 300, ta=1, ldc=73, c_grp=7, c_gs=7 * 73 + 3, beta=1.0, name="wgrad c_grp"),
                Spec(40, 70, 300, ta=1, lda=43, bias_grad=1, name="wgrad lda M + 3")]
        return out
    N, K = FORM_SHAPE[form]
    r4 = lambda x: (x + 3) // 4 * 4  # noqa: E731
    base = dict(bias=1, alpha=0.5)
    sA = r4(M * K) + 8
    out = [
        Spec(M, N, K, lda=K + 4, name="lda K + 4", **base), Spec(M, N, K, lda=K + 3, name="lda K + 3", **base),
        Spec(M, N, K, a_off=1, name="a_off 1", **base),
        Spec(M, N, K, a_grp=5, a_gs=5 * K + 4, name="a_grp 5, a_gs % 4 = 0", **base),
        Spec(M, N, K, a_grp=5, a_gs=5 * K + 5, name="a_grp 5, a_gs % 4 = 1", **base),
        Spec(M, N, K, c_grp=5, c_gs=5 * N + 7, beta=1.0, name="c_grp + beta 1", **base),
        Spec(M, N, K, addend=1, ld_add=0, add_grp=7, add_gs=64, name="broadcast addend", **base),
        Spec(M, N, K, addend=1, add_grp=5, add_gs=5 * N + 3, c_grp=7, c_gs=7 * N + 1, name="add_grp != c_grp", **base),
        Spec(M, N, K, ldc=N + 3, name="ldc N + 3", **base),
        Spec(M, N, K, epi=1, ld_mask=N + 5, name="ld_mask N + 5", **base),
        Spec(M, N, K, epi=1, ld_mask=N + 5, c_grp=5, c_gs=5 * (N + 5) + 2, beta=0.5, name="mask with c_grp", **base),
        Spec(M, N, K, tb=1, ldb=K + 1, b_grp=3, b_gs=3 * (K + 1) + 2, name="tb ldb K + 1 b_grp", **base),
        Spec(M, N, K, batch=3, sa=sA, sb=K * N + 5, sc=M * N + 7, name="batch 3 padded", **base),
        Spec(M, N, K, batch=3, sa=sA, sb=K * N + 5, sc=M * N + 7, addend=1, s_add=M * N + 5, beta=1.0,
             name="batch 3 stride_add", **base),
        Spec(M, N, K, batch=2, sa=sA, epi=1, beta=0.5, name="epi 1 batch 2: one mask for both entries"),
        Spec(M, 1, K, batch=3, lda=3 * K, sa=K, ldb=1, sb=K, ldc=3 * 9 + 3, sc=1, c_off=3 * 9, beta=0.0,
             name="interleaved N 1 outputs"),
    ]
    if form == "scalar":
        out.append(Spec(M, N, 1, batch=3, lda=3 * 9 + 3, a_off=3 * 9, sa=1, ldb=N, sb=N, ldc=3 * N, sc=N, beta=1.0,
                        name="K 1 outer product"))
    return out


def second_unit_M(s):
    """Smallest M = 32 (P + 3) + 5 whose plan gives a wave a second work unit (units > 4 grid), from the plan."""
    rc, big = plan(s.but(M=1 << 22))
    assert rc == 0
    P = 4 * big.grid // big.ncg + 1
    while True:
        rc, pl = plan(s.but(M=32 * P))
        assert rc == 0
        if pl.units > 4 * pl.grid:
            break
        P += 1
    return 32 * (P + 3) + 5


# (form, ncg) -> the smallest (N, K) that reaches it
SECOND_UNIT = {("prefetch", 1): (1, 8), ("prefetch", 2): (97, 8), ("prefetch", 3): (65, 8), ("breg", 1): (1, 40),
               ("plain", 1): (1, 72), ("plain", 2): (97, 72), ("plain", 3): (65, 72),
               ("scalar", 1): (1, 1), ("scalar", 2): (97, 1), ("scalar", 3): (65, 1)}
LN_K = {"prefetch": 16, "breg": 48, "plain": 72, "scalar": 6}


def ln_specs():
    """The LayerNorm-epilogue forward cases (second unit per wave), with their seeds."""
    return [(Spec(second_unit_M(Spec(64, 64, K, epi=2)), 64, K, epi=2, bias=1, name=f"LayerNorm {form}"), 40 + i)
            for i, (form, K) in enumerate(LN_K.items())]


def _unreachable():
    import json
    import os

    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gemm_unreachable.json")
    return {tuple(t) for t in json.load(open(path))}


UNREACHABLE = _unreachable()  # instantiations no knob set of KNOB_SETS reaches (recorded list, checked by the CPU file)
