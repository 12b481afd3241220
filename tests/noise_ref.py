"""The host definition of the project's standard-normal stream (csrc/noise.h, dgppo_normal) and of the LidarNoise
sensor model (utils/sensor.py) on top of it: plain NumPy over oracle.math32.philox4x32, which tests/test_oracle_kat.py
holds to Random123's known-answer vectors.  Nothing here touches the package under test.

Element `idx` of the stream (seed, stream), all three 64-bit:
    counter = (idx lo, idx hi, stream lo, stream hi | 0x80000000)      key = (seed lo, seed hi)
    ia = (word0 >> 8) + 1 in [1, 2^24]        ib = word1 >> 8 in [0, 2^24)
    z  = sqrt(-2 ln(ia / 2^24)) cos(2 pi ib / 2^24)
The domain bit 0x80000000 absorbs bit 63 of the stream id: streams s and s | 2^63 are the same stream."""
import statistics

import numpy as np

from oracle.math32 import philox4x32

F32, F64 = np.float32, np.float64
M32, M64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
DOMAIN = 0x80000000
TWO24 = 16777216.0
NO_RETURN = 1e6               # utils/sensor.py: the alpha of a beam without a return
SENSOR_STREAM_BASE = 1 << 62  # LidarNoise: streams 2^62 + 2t (range noise) and 2^62 + 2t + 1 (dropout)


def counter_of(idx: int, stream: int):
    """The four counter words of one element."""
    idx, stream = int(idx) & M64, int(stream) & M64
    return idx & M32, idx >> 32, stream & M32, (stream >> 32) | DOMAIN


def uniform_ints(idx, seed, stream):
    """(ia, ib) int64 arrays of the shape of `idx` (element indices >= 0): exact integers."""
    idx = np.asarray(idx)
    assert idx.dtype.kind in "iu" and (idx.size == 0 or int(idx.min()) >= 0)
    i = idx.astype(np.uint64)
    seed, stream = int(seed) & M64, int(stream) & M64
    w = philox4x32(i & np.uint64(M32), i >> np.uint64(32), stream & M32, (stream >> 32) | DOMAIN, seed & M32,
                   seed >> 32)
    return (w[0] >> np.uint32(8)).astype(np.int64) + 1, (w[1] >> np.uint32(8)).astype(np.int64)


def box_muller(ia, ib):
    """(z, r) in float64 from the two integers."""
    r = np.sqrt(-2.0 * np.log(np.asarray(ia, F64) / TWO24))
    return r * np.cos(2.0 * np.pi * (np.asarray(ib, F64) / TWO24)), r


def normal_ref(idx, seed, stream):
    """(z, r) in float64: the stream's elements `idx` and their Box-Muller radii."""
    return box_muller(*uniform_ints(idx, seed, stream))


def normal_f32(ia, ib):
    """The kernel's own formula evaluated in NumPy float32 (every operation rounded to float32)."""
    u1 = np.asarray(ia).astype(F32) * F32(1.0 / TWO24)
    u2 = np.asarray(ib).astype(F32) * F32(1.0 / TWO24)
    with np.errstate(divide="ignore"):
        return np.sqrt(F32(-2.0) * np.log(u1)) * np.cos(F32(6.28318530717958648) * u2)


def normal_bound(z, r):
    """The float32 evaluation error allowed to the kernel on an element of radius r: 1e-6 r + 1e-7.

    The kernel evaluates sqrtf(-2 logf(u1)) cosf(2pi_f32 * u2) with u1 = ia 2^-24 and u2 = ib 2^-24, both exact in
    float32 (24-bit integers times a power of two).  With eps = 2^-24 = 6.0e-8 (half an ulp, relative):
      angle   float32(2 pi) differs from 2 pi by 1.75e-7, times u2 < 1; the product 2pi_f32 * u2 < 2 pi is rounded once,
              half an ulp of [4, 8) = 2.4e-7: the angle is off by at most 4.2e-7, and |d cos| <= |d angle|;
      cosf    a few ulp of a result <= 1: 2 ulp = 2.4e-7 absolute;
      radius  logf within 2 ulp relative (2.4e-7), halved by the square root, sqrtf within 1 ulp: 2.4e-7 r at most,
              entering z through |cos| <= 1;
      product one rounding, eps |z| <= 0.6e-7 r.
    Sum: |z32 - z| <= r (4.2e-7 + 2.4e-7 + 2.4e-7 + 0.6e-7) = 9.6e-7 r <= 1e-6 r.  The absolute 1e-7 covers r -> 0
    (u1 -> 1), where relative statements about logf stop being meaningful.  The bound is relative to the radius r,
    never to |z|: near the zeros of the cosine the error stays of size 1e-6 r while z vanishes.
    A NumPy float32 evaluation of the same formula (normal_f32) over 2^22 elements of (seed 123, stream 5) reaches
    0.38 of this bound (tests/test_noise_ref_cpu.py); dgppo_normal on an MI355X reaches 0.385 over 2^21 + 257
    elements of that stream and 0.34 to 0.37 on each row of the (seed, stream) table below."""
    return 1e-6 * np.asarray(r, F64) + 1e-7


def drop_threshold(dropout: float) -> float:
    """float32(Phi^-1(dropout)) as a float: what a dropout draw is compared against; -inf / +inf at 0 / 1."""
    if dropout <= 0.0:
        return -np.inf
    if dropout >= 1.0:
        return np.inf
    return float(F32(statistics.NormalDist().inv_cdf(dropout)))


def beam_index(shape, env_offset=0):
    """Element index of beam (b, i, r) of a (B, n, R) scan: ((env_offset + b) n + i) R + r (ops.lidar_observe)."""
    B, n, R = shape
    b, i, r = np.meshgrid(np.arange(B, dtype=np.int64), np.arange(n, dtype=np.int64), np.arange(R, dtype=np.int64),
                          indexing="ij")
    return ((env_offset + b) * n + i) * R + r


def lidar_noise_ref(alpha, t, sigma, dropout, seed, sense_range, env_offset=0):
    """The float64 model of LidarNoise(sigma, dropout, seed, sense_range)(alpha, t), per beam of a (B, n, R) float32
    scan whose env b sits at row env_offset + b of the noise streams.  Returns (value, tol, undecidable):
      value        float64, what the sensed alpha must equal (NaN: must be NaN);
      tol          float64, the allowed |sensed - value| (0: exact);
      undecidable  bool, the beam's dropout draw is within normal_bound of the threshold: either outcome is right.
    Range noise, where alpha <= 1 (decided on the exact input): max(alpha + z scale, 0) with z element e of stream
    2^62 + 2t and scale = float32(sigma / sense_range), the model's constant (dgppo_hip.h: noise_scale).  max is
    continuous (1-Lipschitz), so the float32 result is within normal_bound scale (the draw) + 2^-24 |z| scale (the
    product) + 2^-24 (|alpha| + |z| scale) (the sum) <= normal_bound scale + 2^-23 (|alpha| + |z| scale).
    Dropout, where alpha is not NaN: NO_RETURN where z2 < float32(Phi^-1(dropout)), z2 element e of stream
    2^62 + 2t + 1.  Everything else (non-returns, NaN, kept beams without range noise) passes through exactly."""
    alpha = np.asarray(alpha)
    assert alpha.dtype == F32 and alpha.ndim == 3
    a = alpha.astype(F64)
    e = beam_index(alpha.shape, env_offset)
    value, tol = a.copy(), np.zeros(a.shape, F64)
    with np.errstate(invalid="ignore"):
        if sigma > 0.0:
            z, r = normal_ref(e, seed, SENSOR_STREAM_BASE + 2 * int(t))
            scale = float(F32(sigma / sense_range))
            ret = a <= 1.0  # False for NaN
            value = np.where(ret, np.maximum(a + z * scale, 0.0), a)
            tol = np.where(ret & np.isfinite(a),  # alpha = -inf is floored to exactly 0
                           normal_bound(z, r) * scale + 2.0 ** -23 * (np.abs(a) + np.abs(z) * scale), 0.0)
        undecidable = np.zeros(a.shape, bool)
        if dropout > 0.0:
            z2, r2 = normal_ref(e, seed, SENSOR_STREAM_BASE + 2 * int(t) + 1)
            thr = drop_threshold(dropout)
            live = ~np.isnan(a)
            drop = (z2 < thr) & live
            undecidable = (np.abs(z2 - thr) <= normal_bound(z2, r2)) & live
            value = np.where(drop, NO_RETURN, value)
            tol = np.where(drop, 0.0, tol)
    return value, tol, undecidable


def sensed_mismatches(seen, ref):
    """(bad, undecidable): bool arrays over the beams of a sensed float32 scan `seen` against lidar_noise_ref's
    triple.  A decidable beam is bad when it is not within tol of the value (NaN where NaN is due); undecidable beams
    are not compared."""
    value, tol, und = ref
    s = np.asarray(seen).astype(F64)
    with np.errstate(invalid="ignore"):
        ok = np.where(np.isnan(value), np.isnan(s), np.abs(s - value) <= tol)
        ok |= (s == value)  # infinities
    return ~ok & ~und, und


# ---- the (seed, stream) table of tests/test_normal_stream_gpu.py: each 32-bit word alone, all together ----
SEEDS = [0, 1, 1 << 32, 0xFFFFFFFFFFFFFFFF, 0x123456789ABC]
STREAMS = [0, 7, (5 << 32) | 7, ((1 << 30) - 1) << 32, 1 << 62, (1 << 62) + 11]
N_EL = 4099  # 16 full blocks of 256 and 3 elements


# ---- the inputs of the sensor comparison (tests/test_normal_stream_gpu.py; decidability in test_noise_ref_cpu.py) ----
SENSOR_SHAPES = [(1, 1), (3, 8), (8, 32), (2, 128)]  # (n, R), B = 5
SENSOR_ENVS = (1, 2, 3, 5, 6)  # of sensor_ref.hand_made_alpha's 7 rows, the five that differ beam to beam
SENSOR_T = (0, 5)
EDGE_ALPHAS = (0.0, 1.0, float(np.nextafter(F32(1), F32(2))), 1e6, float("nan"), 1e-8)


def sensor_seed(R: int) -> int:
    return 0x9E3779B97F4A7C15 + R  # both key words in use


def sensor_alpha(n: int, R: int):
    """(5, n, R) float32: hand_made_alpha's rows SENSOR_ENVS with EDGE_ALPHAS written over the first beams (as many
    as fit) of env b, agent b mod n -- both sides of the return test alpha <= 1, a NaN and a value the noise floors."""
    from sensor_ref import hand_made_alpha

    a = hand_made_alpha(R, n, seed=R)[list(SENSOR_ENVS)].copy()
    flat = a.reshape(a.shape[0], -1)
    for b in range(a.shape[0]):
        k = min(len(EDGE_ALPHAS), flat.shape[1])
        at = (b % n) * R
        k = min(k, flat.shape[1] - at)
        flat[b, at:at + k] = np.roll(np.array(EDGE_ALPHAS, F32), b)[:k]
    return a
