"""Sensor models for the LiDAR envs: what sits between `env.lidar_scan` and `env.lidar_hits`.

The scan is `alpha` (B, n, R): per beam the hit distance as a fraction of the sensing range (the env's
comm_radius), NO_RETURN = 1e6 where nothing is hit (the reference's env/utils.py:115-130).  A sensor is any callable
`sensor(alpha, t) -> alpha_obs` of the same shape and device; trainer/rollout.py SensorRolloutEngine runs one in the
loop, `env.get_graph(state, lidar_data=env.lidar_hits(agent, alpha_obs))` builds a graph from its output.

The other half of an observed graph, who sees whom: `mask_unseen(graph, env.line_of_sight(agent, obstacles))` drops the
agent-agent edges that an obstacle cuts (`env.observe(..., occlusion=True)` is the fused form), and
`mask_unseen(graph, env.field_of_view(agent, deg))` those whose sender is outside the receiver's camera cone
(`env.observe(..., fov=deg)`; both at once: `field_of_view(...) & line_of_sight(...)`).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import torch

from .. import _lib

NO_RETURN = 1e6  # the reference's alpha of a beam that hits nothing


def ranges_to_alpha(ranges: torch.Tensor, sense_range: float) -> torch.Tensor:
    """Range readings in metres (any shape; a real sensor's or a recorded scan's) -> alpha for `env.lidar_hits`:
    ranges / sense_range, with non-finite readings and readings outside [0, sense_range] as NO_RETURN."""
    if not isinstance(ranges, torch.Tensor) or not ranges.is_floating_point():
        raise ValueError("ranges_to_alpha: ranges must be a floating-point tensor")
    if not (math.isfinite(sense_range) and sense_range > 0):
        raise ValueError(f"ranges_to_alpha: sense_range must be positive and finite, got {sense_range}")
    r = ranges.to(torch.float32)
    ok = torch.isfinite(r) & (r >= 0) & (r <= sense_range)
    return torch.where(ok, r / sense_range, torch.full_like(r, NO_RETURN))


def mask_unseen(graph, visible: torch.Tensor):
    """Hide the neighbours a receiver cannot see: for every pair with `~visible[..., i, j]` (bool, the graph's batch
    shape + (n, n): `env.line_of_sight`, `env.field_of_view` or their conjunction), edge i * n + j of the leading
    agent-agent block gets receivers = senders = the pad node (the last node), as out-of-range pairs are stored.  In
    place on the graph's index tensors; edge features, nodes, states and all other edges are untouched.  Returns the
    graph."""
    if not isinstance(visible, torch.Tensor) or visible.dtype != torch.bool:
        raise ValueError("mask_unseen: visible must be a bool tensor")
    recv, send = graph.receivers, graph.senders
    if visible.dim() < 2 or visible.shape[-1] != visible.shape[-2] or tuple(visible.shape[:-2]) != tuple(recv.shape[:-1]):
        raise ValueError(f"mask_unseen: visible must be {tuple(recv.shape[:-1])} + (n, n), got {tuple(visible.shape)}")
    n = int(visible.shape[-1])
    if n * n > recv.shape[-1] or visible.device != recv.device:
        raise ValueError("mask_unseen: visible does not fit the graph's agent-agent edges or is on another device")
    pad = int(graph.states.shape[-2]) - 1
    hide = ~visible.reshape(tuple(visible.shape[:-2]) + (n * n,))
    recv[..., :n * n].masked_fill_(hide, pad)
    send[..., :n * n].masked_fill_(hide, pad)
    return graph


def noise_domain(sigma, dropout) -> None:
    """LidarNoise's domain: sigma finite and >= 0, dropout in [0, 1], else ValueError."""
    if not (math.isfinite(sigma) and sigma >= 0):
        raise ValueError(f"LidarNoise: sigma must be >= 0, got {sigma}")
    if not 0.0 <= dropout <= 1.0:
        raise ValueError(f"LidarNoise: dropout must be in [0, 1], got {dropout}")


def drop_below(dropout: float) -> float:
    """Phi^-1(dropout) = sqrt(2) erfinv(2 dropout - 1): a beam is dropped where its standard normal draw is below it."""
    if dropout <= 0.0:
        return -math.inf
    if dropout >= 1.0:
        return math.inf
    return math.sqrt(2.0) * float(torch.erfinv(torch.tensor(2.0 * dropout - 1.0, dtype=torch.float64)))


def cone_angle(env, what: str, fov) -> Optional[float]:
    """The half angle of a sensing cone in degrees, or None for no cone (`fov` None or exactly 180).  A cone needs an
    env whose state carries a heading (LidarBicycleTarget, LidarOmniTarget) and 0 < fov <= 180: ValueError otherwise
    (NotImplementedError for the VMAS envs), before the GPU is touched."""
    if fov is None:
        return None
    if env.ENGINE in env._VMAS_ENGINES:
        raise NotImplementedError(f"{what}: the VMAS envs have no field-of-view sensor model")
    if env.ENGINE not in (_lib.DGPPO_ENGINE_BICYCLE, _lib.DGPPO_ENGINE_OMNI):
        raise ValueError(f"{what}: a field of view needs a heading in the state (LidarBicycleTarget, "
                         f"LidarOmniTarget); {type(env).__name__} has no heading")
    deg = float(fov)
    if not 0.0 < deg <= 180.0:
        raise ValueError(f"{what}: the half angle must be in (0, 180] degrees, got {fov}")
    return None if deg == 180.0 else deg


def bodies_option(env, what: str, bodies, algo_cls=None) -> bool:
    """The `bodies` option (the LiDAR's beams also return off the other agents' bodies), validated: False for a false
    value; a true one needs an algorithm that does not read the true state off the rollout's graphs (`algo_cls` with
    SENSOR_OK) and a LiDAR env with obstacles, because the hit rows exist only there.  ValueError, or
    NotImplementedError for the VMAS envs, before the GPU is touched.  It travels beside the Sensing record."""
    if not bodies:
        return False
    if algo_cls is not None and not algo_cls.SENSOR_OK:
        raise ValueError(f"{algo_cls.__name__} evaluates env.get_cost on the rollout's graphs, which must be the true "
                         "ones: lidar_bodies is not supported (dgppo, informarl, informarl_lagr are)")
    env._require_lidar(what)
    return True


@dataclass(frozen=True)
class Sensing:
    """What stands between the world and the policy, validated once: range noise `sigma` (world units) and beam
    `dropout` (LidarNoise; both None when no noise value was given, which is not the same as 0: the algorithms report
    it as `sensor is None`), `occlusion` (obstacles hide agents from each other) and `fov` (the half angle in degrees
    of the camera cone, None for no cone).  make_algo, Trainer.evaluate, both sensor rollout engines, env.observe and
    test.py all get theirs from `Sensing.of`."""

    sigma: Optional[float]
    dropout: Optional[float]
    occlusion: bool
    fov: Optional[float]

    @classmethod
    def of(cls, env, what: str, noise=None, dropout=None, occlusion=False, fov=None, algo_cls=None) -> Optional["Sensing"]:
        """The record for these options on `env`, or None when nothing is sensed (no noise value given, no occlusion,
        `fov` None or exactly 180).  `what` prefixes the messages.  The checks, in order: an algorithm (`algo_cls`)
        that reads the true state off the rollout's graphs (SENSOR_OK False) takes no option at all, and one that can
        needs a LiDAR env (its own wording); noise values are checked where they are given, first that the env has a
        LiDAR, then LidarNoise's domain; then the cone (cone_angle); then, if not yet done, that the env has a LiDAR.
        ValueError, or NotImplementedError for the VMAS envs, before the GPU is touched."""
        if noise is None and dropout is None and not occlusion and fov is None:
            return None
        no_lidar = env._obstacle_fields() == 0 or env.n_obs == 0
        if algo_cls is not None:
            flags = "lidar_noise / lidar_dropout / lidar_occlusion / lidar_fov"
            if not algo_cls.SENSOR_OK:
                raise ValueError(f"{algo_cls.__name__} evaluates env.get_cost on the rollout's graphs, which must be "
                                 f"the true ones: {flags} are not supported (dgppo, informarl, informarl_lagr are)")
            if env.ENGINE in env._VMAS_ENGINES or no_lidar:
                raise ValueError(f"{flags} need a LiDAR env with obstacles; {type(env).__name__} with {env.n_obs} "
                                 "obstacles has no LiDAR")
        sigma = drop = None
        if noise is not None or dropout is not None:
            env._require_lidar(what)
            noise_domain(noise or 0.0, dropout or 0.0)
            sigma, drop = float(noise or 0.0), float(dropout or 0.0)
        fov = cone_angle(env, what, fov)
        if sigma is None and not occlusion and fov is None:
            return None
        if sigma is None:
            env._require_lidar(what)
        return cls(sigma, drop, bool(occlusion), fov)

    def model(self, sense_range: float, seed: int = 0) -> "LidarNoise":
        """The record's LidarNoise (sigma = dropout = 0, the identity, when no noise value was given)."""
        return LidarNoise(self.sigma or 0.0, self.dropout or 0.0, seed, sense_range=sense_range)


class LidarNoise:
    """Range noise and beam dropout: `LidarNoise(sigma, dropout, seed)(alpha, t)`.

    Beams with a return (alpha <= 1) get additive Gaussian range noise of std `sigma` world units (sigma /
    sense_range in alpha), floored at 0; then each beam is independently replaced by NO_RETURN with probability
    `dropout`.  Non-returns and NaN pass through.  The draws come from the project's Philox generator
    (dgppo_normal) keyed (seed, stream id), the stream ids 2^62 + 2t and 2^62 + 2t + 1: reproducible for a seed,
    independent across t, and disjoint from the policy's sampling streams ((env_offset << 32) | t, env_offset <
    2^30, which RolloutEngine enforces; bit 63 is the generator's own domain bit, so it cannot tell streams
    apart).  A dropout decision is `z < Phi^-1(dropout)` on a standard normal z, the threshold rounded to float32.
    sigma = 0 and dropout = 0 returns the input tensor itself.  tests/noise_ref.py restates the stream and this
    model in float64."""

    STREAM_BASE = 1 << 62

    def __init__(self, sigma: float = 0.0, dropout: float = 0.0, seed: int = 0, sense_range: float = 0.5):
        noise_domain(sigma, dropout)
        if not (math.isfinite(sense_range) and sense_range > 0):
            raise ValueError(f"LidarNoise: sense_range must be positive, got {sense_range}")
        self.sigma, self.dropout, self.seed, self.sense_range = float(sigma), float(dropout), int(seed), float(sense_range)
        self._drop_below = drop_below(self.dropout)

    def __call__(self, alpha: torch.Tensor, t: int) -> torch.Tensor:
        if self.sigma == 0.0 and self.dropout == 0.0:
            return alpha
        from ..nn import kernels as K

        _lib.require_gpu(alpha.device, "LidarNoise")
        if alpha.dtype != torch.float32:
            raise ValueError(f"LidarNoise: alpha must be float32, got {alpha.dtype}")
        out = alpha
        z = torch.empty(alpha.shape, dtype=torch.float32, device=alpha.device)
        if self.sigma > 0.0:
            K.normal_(z, seed=self.seed, stream_id=self.STREAM_BASE + 2 * int(t))
            noisy = torch.clamp_min(alpha + z * (self.sigma / self.sense_range), 0.0)
            out = torch.where(alpha <= 1.0, noisy, alpha)
        if self.dropout > 0.0:
            K.normal_(z, seed=self.seed, stream_id=self.STREAM_BASE + 2 * int(t) + 1)
            drop = (z < self._drop_below) & ~torch.isnan(alpha)
            out = torch.where(drop, torch.full_like(alpha, NO_RETURN), out)
        return out
