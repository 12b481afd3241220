"""tests/policy_ref.py held to the oracle, the coverage of the GPU case table of tests/test_policy_direct_gpu.py (through
policy_ref.instantiation: the library does not report which policy_step_kernel it launched), and the host-side
contract of dgppo_policy_step_supported / dgppo_policy_step, which return before any launch (the library loads
without a GPU)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import policy_ref as PR
import prim_ref as P
from dgppo_fov_amd import _lib
from oracle import nets_t as R

CASES = PR.cases()
FAKE = 0x1000  # a non-null pointer: the calls under test never dereference


def _rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape
    return float((np.abs(got - ref) / (1.0 + np.abs(ref))).max())


# ---- the reference against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("L,ED", [(1, 4), (2, 4), (1, 10), (2, 10)])
def test_reference_agrees_with_the_oracle(monkeypatch, L, ED):
    """On graphs whose candidate table names every edge (masked edges target a pad node), the float64 reference is
    oracle.nets_t's actor: carry, mean / std and the clipped log-prob, the clip branches included."""
    monkeypatch.setattr(R, "THRESH", P.THRESH)  # the float32 constant of the reference program (prim_ref.THRESH)
    c = PR.Case("oracle", 3, 8, 7, 10 if ED > 4 else 5, 2, ED=ED, L=L, G=4, layout="free", seed=3)
    d = PR.make_inputs(c, named=True)
    G, n = c.Gn, c.n
    assert d["E"] == n * c.C and (d["sidx"] >= 0).any() and (d["sidx"][0, n - 1] < 0).all()
    r = PR.step(c, d)
    graph = dict(nodes=np.concatenate([d["x"], np.zeros((G, 1, c.D0), np.float32)], 1), edges=d["ef"],
                 receivers=d["receivers"], senders=d["senders"])
    p = R.to_t(PR.to_flax(d["params"], ED))
    h2 = R.actor_carry(p, graph, d["h_in"].reshape(G, n, 64), n)
    mu, sd = R.policy_dist(p, h2)
    assert _rel(r["h_out"], h2.numpy().reshape(G * n, 64)) <= 1e-12
    assert _rel(r["mean"], mu.numpy().reshape(G * n, c.A)) <= 1e-12
    rng = np.random.default_rng(5)
    act = rng.uniform(-0.99, 0.99, (G * n, c.A)).astype(np.float32)
    act[0], act[1], act[2, 0], act[3, 1] = 1.0, -1.0, np.float32(0.999), np.float32(-0.999)
    lp = PR.log_pi(r, act, std_shift=R.STD_INIT_INV, std_min=1e-5)
    assert lp["clip"].sum() == 6
    assert _rel(lp["std"], sd.numpy().reshape(G * n, c.A)) <= 1e-12
    want = R.tanh_normal_log_prob(torch.as_tensor(act.reshape(G, n, c.A)), mu, sd).numpy().reshape(G * n)
    assert _rel(lp["log_pi"], want) <= 1e-12
    for noise in (None, d["noise"]):
        pre = mu if noise is None else mu + sd * torch.as_tensor(noise, dtype=torch.float64).reshape(G, n, c.A)
        got = PR.action(r, noise, std_shift=R.STD_INIT_INV, std_min=1e-5)
        assert _rel(got, torch.tanh(pre).numpy().reshape(G * n, c.A)) <= 1e-12


def test_dead_receivers_get_a_zero_attention_sum():
    for c in CASES:
        d = PR.inputs(c)
        r64, _ = PR.expected(c)
        dead = np.array([g * c.n + i for g, i in c.dead])
        assert (d["sidx"].reshape(c.Gn * c.n, c.C)[dead] < 0).all(), c.key
        none = (d["sidx"] < 0).all(-1).reshape(-1)
        assert none[dead].all() and not none.all(), c.key
        for tot in r64["tot"]:
            assert (tot[none] == 0.0).all() and np.abs(tot[~none] - 1.0).max() <= 1e-12, c.key
    # such a receiver's layer output is its own update term alone
    c = next(c for c in CASES if c.L == 1 and c.n > 1)
    d, ly = PR.inputs(c), PR.inputs(c)["params"]["layers"][0]
    x = torch.as_tensor(d["x"], dtype=torch.float64)
    y, _, _ = PR.gt_layer(ly, x, torch.as_tensor(d["ef"], dtype=torch.float64), torch.as_tensor(d["cand"]).long(),
                          torch.as_tensor(d["sidx"]).long(), c.n, torch.float64)
    g, i = c.dead[0]
    own = np.maximum(d["x"][g, i].astype(np.float64) @ ly["Wu"].astype(np.float64) + ly["bu"], 0.0)
    assert np.array_equal(y[g, i].numpy(), own)


def test_float32_reference_stays_near_the_float64_one():
    """The floor 8 |ref32 - ref64| of the `close` rule stays below 1e-3 of the scale on every element of every case:
    the inputs are tame enough that the rule does not excuse a wrong kernel."""
    worst = 0.0
    for c in CASES:
        r64, r32 = PR.expected(c)
        for name in ("h_out", "mean", "std_raw"):
            assert PR.floor_excess(r64, r32, name) == 0.0, (c.key, name)
        worst = max(worst, r64["max_logit"])
    assert 1.0 <= worst <= 60.0, worst  # the softmax is neither uniform nor saturated everywhere


def test_first_layer_inputs_are_exact():
    for c in CASES:
        d = PR.inputs(c)
        ly = d["params"]["layers"][0]
        for a in (d["x"], ly["Wu"], ly["bu"]):
            assert np.array_equal(a * 8, np.round(a * 8)) and np.abs(a).max() <= 2.0, c.key


# ---- coverage of the GPU case table --------------------------------------------------------------------------------------
def test_case_table_covers_the_supported_domain():
    assert {c.n for c in CASES} == set(range(1, 17))
    assert {c.A for c in CASES} == {1, 2, 3, 4}
    assert {c.inst for c in CASES} == {"narrow", "node_table", "wide"}
    assert {c.L for c in CASES} == {1, 2} and {c.layout for c in CASES} == set(PR.LAYOUTS)
    for c in CASES:
        assert PR.supported(c.n, c.C, c.D0, c.A, c.ED, c.N, c.L, c.dims), c.key
    # both sides of gpg (N - n) <= 160 at 1, 2 and 5 graphs per group
    for gpg in (1, 2, 5):
        at = {c.inst for c in CASES if c.gpg == gpg and c.L == 2 and c.gpg * (c.N - c.n) == PR.PRE_MAX}
        past = {c.inst for c in CASES if c.gpg == gpg and c.L == 2 and PR.PRE_MAX < c.gpg * (c.N - c.n) <= PR.PRE_MAX + gpg}
        assert at == {"node_table"} and past == {"narrow"}, gpg
    # a node table whose last 16-row tile is partial, and one filled to the last row
    tables = [c.gpg * (c.N - c.n) for c in CASES if c.inst == "node_table"]
    assert any(t % 16 for t in tables) and PR.PRE_MAX in tables
    # both reasons for the wide kernel, apart and together; every wide edge width; ED == 4 leaves Wex NULL
    wide = {(c.D0 > PR.NARROW_D0, c.ED > 4) for c in CASES if c.inst == "wide"}
    assert wide == {(True, False), (False, True), (True, True)}
    assert {c.D0 for c in CASES if c.ED == 4 and c.inst == "wide"} == {9, 10, 11, 12}
    assert {c.ED for c in CASES if c.D0 <= PR.NARROW_D0} >= {4, 5, 6, 7, 9, 10}
    assert {c.D0 for c in CASES} >= {1, 2, 3}
    # an all-agent graph with two layers: the narrow kernel (the node table would divide by N - n)
    assert any(c.N == c.n and c.L == 2 and c.inst == "narrow" for c in CASES)
    # a partial last group everywhere but the single-group cases; fewer graphs than a group; dead rows in the group
    assert all(c.Gn % c.gpg or c.gpg == 1 for c in CASES if not c.G)
    assert any(c.Gn < c.gpg for c in CASES) and any(c.Gn == 1 and c.n == 3 for c in CASES)
    assert {c.n for c in CASES if PR.ROWS % c.n} >= {5, 6, 7}
    # every case holds receivers without candidates in its first and last graph, cand == -1 and mismatched edges
    flags = set()
    for c in CASES:
        assert c.dead[0][0] == 0 and c.dead[-1][0] == c.Gn - 1, c.key
        flags |= PR.inputs(c)["flags"]
    assert flags >= {"cand_neg", "recv_mismatch", "free", "dup_agent", "dup_other", "unnamed_edges", "self_edge"}


def test_instantiation_boundaries():
    assert PR.instantiation(8, 88, 7, 4, 2) == "node_table" and PR.instantiation(8, 89, 7, 4, 2) == "narrow"
    assert PR.instantiation(8, 88, 7, 4, 1) == "narrow" and PR.instantiation(8, 8, 7, 4, 2) == "narrow"
    assert PR.instantiation(8, 88, 9, 4, 2) == "wide" and PR.instantiation(8, 88, 8, 5, 2) == "wide"
    assert PR.instantiation(16, 176, 8, 4, 2) == "node_table" and PR.instantiation(3, 36, 8, 4, 2) == "narrow"


# ---- prepare's reference ---------------------------------------------------------------------------------------------------
def test_expected_work_is_the_query_key_product():
    c = next(c for c in CASES if c.L == 2 and c.D0 == 5)
    p = PR.inputs(c)["params"]
    w, mag = PR.expected_work(p)
    assert w.shape == mag.shape == (2, PR.QK_ROWS, PR.QK_COLS)
    rng = np.random.default_rng(0)
    for l, ly in enumerate(p["layers"]):
        D, F = ly["D"], ly["F"]
        x = rng.standard_normal((4, D))
        q = (x @ ly["Wq"].astype(np.float64) + ly["bq"]).reshape(4, PR.H, F)
        qb = np.concatenate([x, np.zeros((4, 32 - D)), np.ones((4, 1))], 1) @ w[l]
        for h in range(PR.H):  # [x 1] work = [q_h Wkt_h | q_h . bk_h]
            assert np.allclose(qb[:, 32 * h:32 * h + D], q[:, h] @ ly["Wkt"][h].astype(np.float64), rtol=0, atol=1e-12)
            assert np.allclose(qb[:, 96 + h], q[:, h] @ ly["bk"].reshape(PR.H, F)[h].astype(np.float64), rtol=0, atol=1e-12)
        used = np.zeros((PR.QK_ROWS, PR.QK_COLS), bool)
        rows = np.r_[np.arange(D), 32]
        for h in range(PR.H):
            used[np.ix_(rows, np.r_[np.arange(32 * h, 32 * h + D), 96 + h])] = True
        assert (w[l][~used] == 0).all() and (mag[l][~used] == 0).all() and (mag[l][used] > 0).all()
        assert (np.abs(w[l]) <= mag[l]).all()


# ---- the host-side contract ------------------------------------------------------------------------------------------------
PTRS = ("cand", "nodes", "edges", "receivers", "senders", "h_in", "h_out", "action", "work")


def _args(n=3, N=8, C=7, D0=5, A=2, ED=4, L=2, G=4, mode=0, Hh=3, dims=None, wex=None):
    a = _lib.PolicyStepArgs()
    a.G, a.N, a.E, a.n_agents, a.C, a.D0, a.A, a.n_layers, a.H, a.mode, a.ED = G, N, n * C, n, C, D0, A, L, Hh, mode, ED
    dims = dims or (((D0, 32), (32, 64)) if L == 2 else ((D0, 64), (0, 0)))
    wex = (ED > 4, ED > 4) if wex is None else wex
    for l in (0, 1):
        ly = a.layer[l]
        for f in ("Wq", "bq", "Wkt", "bk", "Wcat", "Wu", "bu"):
            setattr(ly, f, FAKE)
        ly.D, ly.F = dims[l]
        ly.Wex = FAKE if wex[l] else None
    for f, _ in _lib.PolicyStepArgs._fields_:
        if f in PTRS or f in ("head_W0", "head_b0", "ln0_s", "ln0_b", "head_W1", "head_b1", "ln1_s", "ln1_b", "gru_Wi",
                              "gru_bi", "gru_Wh", "gru_bhn", "Ws", "bs", "Wm", "bm", "Wsd", "bsd", "log_pi"):
            setattr(a, f, FAKE)
    a.nodes_gstride, a.edges_gstride, a.idx_gstride = N * D0, n * C * ED, n * C
    return a


def test_supported_equals_its_rule():
    lib = _lib.load()
    assert lib.dgppo_policy_step_supported(None) == 0
    yes = no = 0
    for n, C, D0, A, ED, dN, L in itertools.product((0, 1, 7, 16, 17), (0, 1, 32, 33), (0, 1, 8, 9, 12, 13),
                                                     (0, 1, 4, 5), (3, 4, 5, 10, 11), (-1, 0, 1, 200), (0, 1, 2, 3)):
        for dims, wex, Hh in ((None, None, 3), (((D0, 32), (32, 32)), None, 3), (((D0 + 1, 64), (32, 64)), None, 3),
                              (None, (True, False), 3), (None, (False, True), 3), (None, None, 2)):
            a = _args(n, n + dN, C, D0, A, ED, L, dims=dims, wex=wex, Hh=Hh)
            d = [(a.layer[l].D, a.layer[l].F) for l in (0, 1)]
            want = PR.supported(n, C, D0, A, ED, n + dN, L, d, [bool(a.layer[l].Wex) for l in (0, 1)], Hh)
            assert bool(lib.dgppo_policy_step_supported(ctypes.byref(a))) == want, (n, C, D0, A, ED, dN, L, dims, wex, Hh)
            yes, no = yes + want, no + (not want)
    assert yes > 1000 and no > 1000


def test_step_refuses_bad_arguments_before_any_launch():
    lib = _lib.load()
    E = _lib.DGPPO_EINVAL
    assert lib.dgppo_policy_step(None, None) == E and lib.dgppo_policy_prepare(None, None) == E
    for f in PTRS:
        a = _args(G=0)
        setattr(a, f, None)
        assert lib.dgppo_policy_step(ctypes.byref(a), None) == E, f
    a = _args(G=0)
    a.work = None
    assert lib.dgppo_policy_prepare(ctypes.byref(a), None) == E
    a = _args(G=0, mode=1)
    a.noise, a.noise_seed = None, None
    assert lib.dgppo_policy_step(ctypes.byref(a), None) == E
    assert lib.dgppo_policy_step(ctypes.byref(_args(G=-1)), None) == E
    for N in (2, 0, -5):  # fewer nodes than agents
        a = _args(n=3, N=N, G=0)
        assert lib.dgppo_policy_step_supported(ctypes.byref(a)) == 0
        assert lib.dgppo_policy_step(ctypes.byref(a), None) == E and lib.dgppo_policy_prepare(ctypes.byref(a), None) == E
    # no graphs: nothing to do, for every noise form and without log_pi
    for mode, noise, seed in ((0, None, None), (1, FAKE, None), (1, None, FAKE)):
        a = _args(G=0, mode=mode)
        a.noise, a.noise_seed, a.log_pi = noise, seed, None
        assert lib.dgppo_policy_step(ctypes.byref(a), None) == 0
    assert lib.dgppo_policy_step(ctypes.byref(_args(n=3, N=3, C=3, G=0)), None) == 0  # N == n_agents is in the domain
    assert lib.dgppo_policy_work_floats() == 2 * PR.QK_ROWS * PR.QK_COLS
