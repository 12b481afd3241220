"""The Philox normal stream and its consumers on the GPU against the host definition (tests/noise_ref.py, checked on
its own in tests/test_noise_ref_cpu.py): dgppo_normal (K.normal_) element by element, its launch edges, the tail of
the first uniform, the separation of streams that differ in one 32-bit word, LidarNoise against the float64 sensor
model, and env.observe against the chain fed the sensed alpha this file has just held to the model.

Bars: |gpu - ref| <= normal_bound = 1e-6 r + 1e-7 per element (derived in noise_ref.normal_bound); BIT-EXACT between
launches and between observe and the chain; the sensor model within lidar_noise_ref's per-beam tolerance.
Host work: one 2^21-element reference (about 1.3 s), shared by the launch-edge and tail tests."""
import functools
import itertools

import numpy as np
import pytest
import torch

from dgppo_fov_amd import _lib
from dgppo_fov_amd.nn import kernels as K
from dgppo_fov_amd.utils.sensor import LidarNoise

import noise_ref as NR
from test_observe_gpu import MODELS, hit_rows, scene_of
from test_sensor_gpu import lidar_env

pytestmark = pytest.mark.gpu

SEEDS, STREAMS, N_EL = NR.SEEDS, NR.STREAMS, NR.N_EL  # 5 x 6 (seed, stream) pairs, 4099 elements each
SENT = -12345.0  # no normal of this generator reaches it (|z| <= sqrt(48 ln 2) = 5.77)
LEAD, TRAIL = 5, 64  # floats of guard; LEAD = 5 puts the output one float past a 16-byte boundary
BIG_SEED, BIG_STREAM, BIG_N = 123, 5, (1 << 21) + 257  # the grid is capped at 8192 x 256 = 2^21 threads


def as_i64(seed: int) -> int:
    """A 64-bit seed as the int64 with the same bits (what a key tensor holds)."""
    seed &= NR.M64
    return seed - (1 << 64) if seed >> 63 else seed


def guarded(n: int, cuda):
    buf = torch.full((LEAD + n + TRAIL,), SENT, dtype=torch.float32, device=cuda)
    assert (buf.data_ptr() + 4 * LEAD) % 16 == 4
    return buf, buf[LEAD:LEAD + n]


def guards_intact(buf, n: int) -> bool:
    return bool((buf[:LEAD] == SENT).all()) and bool((buf[LEAD + n:] == SENT).all())


def draw(cuda, n: int, seed: int, stream: int, by_tensor: bool = False) -> np.ndarray:
    """n elements of (seed, stream) through K.normal_ into a guarded, 4-byte-aligned output; the seed by value or
    through a device int64 tensor."""
    buf, out = guarded(n, cuda)
    if by_tensor:
        key = torch.tensor([as_i64(seed)], dtype=torch.int64, device=cuda)
        K.normal_(out, seed=0, stream_id=stream, seed_tensor=key)
    else:
        K.normal_(out, seed=seed, stream_id=stream)
    torch.cuda.synchronize(cuda)
    assert guards_intact(buf, n), f"guard overwritten at n = {n}"
    got = out.cpu().numpy()
    assert not (got == np.float32(SENT)).any(), f"element not written at n = {n}"
    return got


_TABLE = {}


def table_draw(cuda, seed, stream):
    if (seed, stream) not in _TABLE:
        _TABLE[seed, stream] = draw(cuda, N_EL, seed, stream)
    return _TABLE[seed, stream]


@functools.lru_cache(maxsize=None)
def table_ref(seed, stream):
    return NR.normal_ref(np.arange(N_EL, dtype=np.int64), seed, stream)


@functools.lru_cache(maxsize=None)
def big_ints():
    return NR.uniform_ints(np.arange(BIG_N, dtype=np.int64), BIG_SEED, BIG_STREAM)


def worst(got, z, r):
    """(max of |got - z| / bound, its element)."""
    ratio = np.abs(got.astype(np.float64) - z) / NR.normal_bound(z, r)
    k = int(np.argmax(ratio))
    return float(ratio[k]), k


def assert_within_bound(got, z, r, what):
    assert got.dtype == np.float32 and got.shape == z.shape and np.isfinite(got).all(), what
    ratio, k = worst(got, z, r)
    print(f"{what}: worst |gpu - ref| / bound = {ratio:.3f} at element {k} (gpu {float(got[k])!r}, "
          f"ref {float(z[k])!r}, r {r[k]:.4f})")
    assert ratio <= 1.0, (what, ratio, k, float(got[k]), float(z[k]))


# ---- 1. dgppo_normal against the reference ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS, ids=[f"seed{s:#x}" for s in SEEDS])
def test_normal_matches_reference(cuda, seed):
    """Every (seed, stream) of the table, each 32-bit word of both alone and all together: within normal_bound of the
    float64 reference element by element, and the same bits whether the seed comes by value or from a device tensor."""
    for stream in STREAMS:
        got = table_draw(cuda, seed, stream)
        z, r = table_ref(seed, stream)
        assert_within_bound(got, z, r, f"seed {seed:#x} stream {stream:#x}")
        assert np.array_equal(draw(cuda, N_EL, seed, stream, by_tensor=True), got), (hex(seed), hex(stream))
    # bit 63 of a stream id is the domain bit's: the same stream
    assert np.array_equal(draw(cuda, N_EL, seed, (1 << 63) | 7), table_draw(cuda, seed, 7))


def words(seed, stream):
    return seed & NR.M32, seed >> 32, stream & NR.M32, stream >> 32


ONE_WORD_PAIRS = [(a, b) for a, b in itertools.combinations(itertools.product(SEEDS, STREAMS), 2)
                  if sum(x != y for x, y in zip(words(*a), words(*b))) == 1]


def test_streams_one_word_apart_share_no_element(cuda):
    """Pairs of the table that differ in exactly one of the four 32-bit words (seed lo / hi, stream lo / hi): no
    element of the first 4099 is equal.  Shown on the reference first -- the integer pairs differ everywhere and so do
    the float32 roundings of the float64 normals -- so the GPU condition is one the definition meets."""
    assert len(ONE_WORD_PAIRS) == 42 and {k for a, b in ONE_WORD_PAIRS for k in range(4)
                                          if words(*a)[k] != words(*b)[k]} == {0, 1, 2, 3}
    idx = np.arange(N_EL, dtype=np.int64)
    for a, b in ONE_WORD_PAIRS:
        (ia, ib), (ja, jb) = NR.uniform_ints(idx, *a), NR.uniform_ints(idx, *b)
        assert ((ia != ja) | (ib != jb)).all(), (a, b)
        assert (table_ref(*a)[0].astype(np.float32) != table_ref(*b)[0].astype(np.float32)).all(), (a, b)
        same = table_draw(cuda, *a) == table_draw(cuda, *b)
        assert not same.any(), (a, b, np.flatnonzero(same)[:4])


# ---- 2. launch edges -------------------------------------------------------------------------------------------------
def test_launch_edges_prefix_and_guards(cuda):
    """n across a block (255, 256, 257) and across the grid cap (2^21 - 1, 2^21, 2^21 + 257: the grid-stride loop's
    second pass), every output one float past a 16-byte boundary between sentinel guards.  The longest draw is held
    to the reference; every other n must be its prefix, bit for bit; n = 0 writes nothing."""
    big = draw(cuda, BIG_N, BIG_SEED, BIG_STREAM)
    z, r = NR.box_muller(*big_ints())
    assert_within_bound(big, z, r, f"n = {BIG_N}")
    for n in (1, 255, 256, 257, (1 << 21) - 1, 1 << 21):
        assert np.array_equal(draw(cuda, n, BIG_SEED, BIG_STREAM), big[:n]), n
    assert draw(cuda, 0, BIG_SEED, BIG_STREAM).shape == (0,)
    # n = 0 at the entry point itself, with a live output pointer
    buf, _ = guarded(8, cuda)
    rc = _lib.load().dgppo_normal(buf.data_ptr() + 4 * LEAD, 0, None, BIG_SEED, BIG_STREAM, _lib.stream_handle(cuda))
    torch.cuda.synchronize(cuda)
    assert rc == 0 and bool((buf == SENT).all())


def test_tail_of_the_first_uniform(cuda):
    """The 1024 elements of the first 2^21 with the smallest ia (found on the host), where an off-by-one in ia moves
    most elements by more than twice their bound (tests/test_noise_ref_cpu.py): within bound on the GPU."""
    ia, ib = (v[:1 << 21] for v in big_ints())
    tail = np.sort(np.argsort(ia, kind="stable")[:1024])
    z, r = NR.box_muller(ia[tail], ib[tail])
    assert r.min() > 3.8  # ia <= 2^13.1 of 2^24: the tail indeed
    buf, out = guarded(1 << 21, cuda)
    K.normal_(out, seed=BIG_SEED, stream_id=BIG_STREAM)
    got = out[torch.from_numpy(tail).to(cuda)].cpu().numpy()
    assert_within_bound(got, z, r, "tail")


# ---- 3. the sensor model ---------------------------------------------------------------------------------------------
SENSE_RANGE = 0.5


@pytest.mark.parametrize("n,R", NR.SENSOR_SHAPES, ids=[f"n{n}-R{r}" for n, r in NR.SENSOR_SHAPES])
def test_lidar_noise_matches_the_model(cuda, n, R):
    """LidarNoise on hand-made scans (negative, -0, NaN, +-inf, ties, 1e6) with 0, 1, nextafter(1, 2), 1e6, NaN and
    1e-8 written over some beams: every decidable beam within the float64 model's tolerance, exact where the model
    is (dropped beams, non-returns, NaN), at most 1 beam in 1000 undecidable."""
    alpha = NR.sensor_alpha(n, R)
    dev = torch.from_numpy(alpha).to(cuda)
    seed = NR.sensor_seed(R)
    for sigma, dropout in MODELS:
        for t in NR.SENSOR_T:
            seen = LidarNoise(sigma, dropout, seed, sense_range=SENSE_RANGE)(dev, t)
            assert seen.shape == dev.shape and seen.dtype == torch.float32
            ref = NR.lidar_noise_ref(alpha, t, sigma, dropout, seed, SENSE_RANGE)
            bad, und = NR.sensed_mismatches(seen.cpu().numpy(), ref)
            assert not bad.any(), (sigma, dropout, t, int(bad.sum()), np.argwhere(bad)[:4].tolist())
            assert und.sum() <= alpha.size / 1000, (sigma, dropout, t, int(und.sum()))
    assert np.array_equal(dev.cpu().numpy(), alpha, equal_nan=True)  # the input is never written


# ---- 4. observe: the in-kernel draws ---------------------------------------------------------------------------------
OBSERVE_CASES = [("LidarSpread", 8, 3, 32, 0), ("LidarTarget", 3, 2, 8, 0), ("LidarBicycleTarget", 2, 3, 128, 0),
                 ("LidarOmniTarget", 3, 2, 32, 4)]  # (env, n, obstacles, R, env_offset)


def same(x, y):
    """Equal bit for bit up to NaN payloads (NaN equal to NaN), tensors or arrays."""
    return bool(((x == y) | ((x != x) & (y != y))).all())


@pytest.mark.parametrize("eid,n,obs,R,off", OBSERVE_CASES, ids=[f"{c[0]}-off{c[4]}" for c in OBSERVE_CASES])
def test_observe_draws_the_reference_streams(cuda, eid, n, obs, R, off):
    """env.observe (the fused kernel's own draws at element ((env_offset + b) n + i) R + r) against
    get_graph(lidar_hits(sensed alpha)), the sensed alpha being LidarNoise's on the GPU, held to the float64 model
    right here: the hit rows, nodes and edges of every agent without an undecidable beam are equal bit for bit."""
    sigma, dropout, t, seed = 0.05, 0.3, 5, NR.sensor_seed(R)
    env, _ = lidar_env(eid, n, obs, R, cuda)
    sense_range = float(env.params["comm_radius"])
    state = scene_of(env, 40 + R)
    agent, goal, ob = state
    B, k = agent.shape[0], env.params["top_k_rays"]
    alpha = env.lidar_scan(agent, ob)
    # LidarNoise draws by flat index: rows off.. of a taller scan are env_offset = off
    wide = torch.cat([torch.full((off, n, R), 0.5, device=cuda), alpha])
    seen = LidarNoise(sigma, dropout, seed, sense_range=sense_range)(wide, t)[off:].contiguous()
    ref = NR.lidar_noise_ref(alpha.cpu().numpy(), t, sigma, dropout, seed, sense_range, env_offset=off)
    bad, und = NR.sensed_mismatches(seen.cpu().numpy(), ref)
    assert not bad.any() and und.sum() <= alpha.numel() / 1000
    ret = alpha <= 1.0  # the model bites: returns dropped, returns kept and moved
    assert bool((ret & (seen == 1e6)).any()) and bool((ret & (seen != 1e6) & (seen != alpha)).any())
    want = env.get_graph(state, lidar_data=env.lidar_hits(agent, seen))
    got = env.observe(state, t, sigma=sigma, dropout=dropout, seed=seed, env_offset=off)
    clear = ~und.any(-1)  # (B, n): agents whose top-k is decided
    assert clear.sum() >= B * n - 1
    first_row, first_edge = hit_rows(env).start, env.n_edges - n * k
    assert same(got.states[:, :first_row], want.states[:, :first_row])
    host = {f: (getattr(got, f).cpu().numpy(), getattr(want, f).cpu().numpy())
            for f in ("states", "nodes", "edges", "receivers", "senders")}
    for b, i in zip(*np.nonzero(clear)):
        rows = slice(first_row + i * k, first_row + (i + 1) * k)
        edges = slice(first_edge + i * k, first_edge + (i + 1) * k)
        for f, (x, y) in host.items():
            sl = rows if f in ("states", "nodes") else edges
            assert same(x[b, sl], y[b, sl]), (eid, int(b), int(i), f)
    if off:  # and the offset is what selected those draws
        zero = env.observe(state, t, sigma=sigma, dropout=dropout, seed=seed)
        assert not same(zero.states, got.states)
