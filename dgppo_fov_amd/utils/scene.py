"""Scenes on disk: the initial states of a batch of episodes as one `.npz`, so a checkpoint can be evaluated on
a fixed or hand-built set of scenes (test.py --scene / --dump-scene) and an episode restarted from a saved state.

Arrays (float32): `agent` (E, n, sd), `goal` (E, n_goal_rows, sd) and the obstacles -- `obstacle` (E, O, 16)
packed Rectangle records for the Lidar envs, `obs` (E, O, 4) obstacle states for the MPE envs -- plus `env_id`, the
env's class name.  A loaded scene is the state tuple `env.get_graph` and `RolloutEngine(init_state=...)` take.
"""
from __future__ import annotations

import numpy as np
import torch


def _layout(env):
    """name -> per-episode shape of the arrays a scene of `env` holds."""
    from .. import _lib

    sd = env.state_dim
    shapes = {"agent": (env.num_agents, sd), "goal": (env.num_goals, sd)}
    if env.ENGINE == _lib.DGPPO_ENGINE_MPE:
        shapes["obs"] = (env.n_obs, sd)
    else:
        shapes["obstacle"] = (env.n_obs, 16)
    return shapes


def save_scene(path, env, state) -> None:
    """Write the env state tuple `state` (agent, goal, obstacle), one leading episode axis, to `path` (.npz)."""
    shapes = _layout(env)
    arrays = {"env_id": np.array(type(env).__name__)}
    E = None
    for (name, shape), part in zip(shapes.items(), tuple(state) + (None,) * (3 - len(tuple(state)))):
        part = getattr(part, "packed", part)
        if part is None:
            if shape[0] != 0:
                raise ValueError(f"save_scene: state.{name} is None but the env has {shape[0]} obstacles")
            part = np.zeros((E or 0, 0, shape[1]), np.float32)
        a = part.detach().cpu().numpy() if isinstance(part, torch.Tensor) else np.asarray(part)
        a = np.ascontiguousarray(a, dtype=np.float32)
        E = a.shape[0] if E is None else E
        if a.ndim != 3 or a.shape != (E,) + shape:
            raise ValueError(f"save_scene: {name} must be ({E}, {shape[0]}, {shape[1]}), got {a.shape}")
        arrays[name] = a
    with open(path, "wb") as f:  # (a file object: np.savez would append .npz to a bare name)
        np.savez(f, **arrays)


def load_scene(path, env, device=None):
    """Read a scene written by save_scene as `env`'s state tuple on `device` (default: the env's).  Every array
    must match `env`'s sizes; a mismatch raises a ValueError naming the array."""
    device = torch.device(device) if device is not None else env.device
    with np.load(path, allow_pickle=False) as z:
        data = {k: z[k] for k in z.files}
    shapes = _layout(env)
    E = None
    parts = []
    for name, shape in shapes.items():
        if name not in data:
            raise ValueError(f"load_scene: {path} has no array '{name}' (a scene of {data.get('env_id', '?')}?)")
        a = data[name]
        E = a.shape[0] if E is None and a.ndim == 3 else E
        if a.ndim != 3 or a.shape != (E,) + shape or a.dtype != np.float32:
            raise ValueError(f"load_scene: array '{name}' must be float32 ({E}, {shape[0]}, {shape[1]}) for "
                             f"{type(env).__name__} n={env.num_agents} obs={env.n_obs}, got {a.dtype} {a.shape}")
        parts.append(torch.from_numpy(np.ascontiguousarray(a)).to(device))
    agent, goal, third = parts
    if env.n_obs == 0 and "obstacle" in shapes:
        third = None
    return _as_state(env, agent, goal, third)


def _as_state(env, agent, goal, third):
    from .. import _lib
    from ..env.obstacle import Rectangle

    if env.ENGINE == _lib.DGPPO_ENGINE_MPE:
        from ..env.mpe.base import MPEEnvState

        return MPEEnvState(agent, goal, third)
    from ..env.lidar_env.base import LidarEnvState

    return LidarEnvState(agent, goal, Rectangle(third) if third is not None else None)
