"""PyTorch-ROCm custom ops over libdgppo_hip.so: `torch.ops.dgppo.*`.

The hot-path kernels are registered with `torch.library` so the torch dispatcher, FakeTensor /
meta tracing (torch.compile, export) and CUDA-graph capture all see them as ordinary ops.  Each op
is a thin shim over the C-ABI entry point declared in include/dgppo_hip.h (the same function a
cgo / JNI / ctypes binding would call); outputs are caller-allocated and written
in place (`mutates_args`), launches go on torch's current stream, and there is no CPU kernel: a
non-CUDA tensor raises NativeLibraryError (`_lib.require_gpu`).

  dgppo::env_reset      dgppo_env_reset      vmap(env.reset)      lidar_env/base.py:89-124, mpe/base.py:81-127
  dgppo::env_step       dgppo_env_step       vmap(env.step)       lidar_env/base.py:151-174, mpe/base.py:137-158
  dgppo::env_reset_states dgppo_env_reset_states  the sampling half of env_reset (no graph)
  dgppo::env_rollout    dgppo_env_rollout    lax.scan of env.step over T given actions, trainer/utils.py:45-55
  dgppo::env_get_graph  dgppo_env_get_graph  vmap(env.get_graph)  lidar_env/base.py:126-140, 227-271, mpe/base.py:211-241
  dgppo::lidar_scan     dgppo_lidar_scan     the per-beam alphas of get_lidar, env/utils.py:115-130
  dgppo::lidar_hits     dgppo_lidar_hits     alphas -> top-k hit points, env/utils.py:66-79
  dgppo::env_get_graph_hits dgppo_env_get_graph_hits  get_graph(state, lidar_data), lidar_env/base.py:227-271
  dgppo::lidar_observe  dgppo_lidar_observe  scan, LidarNoise, hits and graph fused: the observed graph of a true state
  dgppo::lidar_sight    dgppo_lidar_sight    which agents see each other past the obstacles (not in the reference)
  dgppo::lidar_observe_los dgppo_lidar_observe_los  lidar_observe with the unseen agent-agent edges sent to the pad node
  dgppo::agent_fov      dgppo_agent_fov      which agents lie in each other's forward cone, the FoV cost's arithmetic
  dgppo::lidar_observe_fov dgppo_lidar_observe_fov  lidar_observe_los with the senders outside the receiver's cone masked too
  dgppo::lidar_scan_bodies dgppo_lidar_scan_bodies  lidar_scan whose beams also return off the other agents' bodies
  dgppo::lidar_observe_bodies dgppo_lidar_observe_bodies  lidar_observe_fov on lidar_scan_bodies' alphas
  dgppo::render_frames  dgppo_render_frames  the drawing half of env.render_video, env/plot.py render_lidar / render_mpe
  dgppo::render_frames_field  dgppo_render_frames_field  the same under a banded scalar field, plot.py viz_opts["cbf"]
  dgppo::render_frames_vmas  dgppo_render_frames_vmas  the drawings of vmas_wheel.py / vmas_reverse_transport.py render_video
  dgppo::gnn_attn_fwd   dgppo_gnn_attn_fwd   GraphTransformer attention core, gnn.py:83-117
  dgppo::gnn_attn_bwd   dgppo_gnn_attn_bwd   its gradient (the jax.grad of update_Vl / update_policy)
  dgppo::gae            dgppo_gae            compute_dec_ocp_gae, algo/utils.py:11-79
  dgppo::grad_norm      dgppo_grad_norm      compute_norm + has_any_nan_or_inf, trainer/utils.py:105-118
  dgppo::adam           dgppo_adam           clip + optax.apply_if_finite(optax.adam), informarl.py:131-137
  dgppo::gather_env_steps dgppo_gather_env_steps  tree_map(lambda x: x[idx], rollout), dgppo.py:275-289

An env's static configuration (dgppo_env_cfg: engine, sizes, radii, limits) is not a tensor; it is
registered once per env instance and the ops take its integer handle.
"""
from __future__ import annotations

import ctypes
import itertools
import weakref
from typing import List, Optional

import torch
from torch import Tensor

from . import _lib

_CFGS: dict = {}
_NEXT_HANDLE = itertools.count(1)


def register_env_cfg(cfg: _lib.EnvCfg, owner=None) -> int:
    """Keep `cfg` alive and return the handle the env ops take (handles are never reused).  With an
    `owner` the entry is released when the owner is garbage-collected, so per-test / per-config envs
    do not accumulate for the life of the process."""
    h = next(_NEXT_HANDLE)
    _CFGS[h] = cfg
    if owner is not None:
        weakref.finalize(owner, _CFGS.pop, h, None)
    return h


def env_cfg(handle: int) -> _lib.EnvCfg:
    try:
        return _CFGS[int(handle)]
    except KeyError:
        raise ValueError(f"unknown env cfg handle {handle}") from None


def _stride(t: Tensor, inner: int) -> int:
    """Per-env element stride of t, requiring the trailing `inner` dims to be contiguous."""
    tail = 1
    for d in range(t.dim() - 1, t.dim() - 1 - inner, -1):
        if t.stride(d) != tail:
            raise ValueError("trailing dims must be contiguous")
        tail *= t.shape[d]
    return t.stride(t.dim() - 1 - inner) if t.dim() > inner else tail


def _p(t: Optional[Tensor]) -> int:
    return 0 if t is None else int(t.data_ptr())


def _stream(t: Tensor) -> int:
    return _lib.stream_handle(t.device)


def _returns_none(*args, **kwargs) -> None:
    """The fake of every op here that only writes into its arguments."""
    return None


# ---- env -------------------------------------------------------------------------------------------
@torch.library.custom_op("dgppo::env_step", mutates_args=("nodes", "edges", "out_states", "receivers", "senders",
                                                           "reward", "cost"))
def env_step(cfg: int, states: Tensor, obstacles: Optional[Tensor], action: Tensor, ray_dirs: Tensor, nodes: Tensor,
             edges: Tensor, out_states: Tensor, receivers: Tensor, senders: Tensor, reward: Tensor,
             cost: Tensor) -> None:
    """One fused env step for B envs: states (B, N, sd) [+ obstacles (B, O, 16)] and actions (B, n, A)
    -> next graph rows, reward (B,), cost (B, n, n_cost).  Per-env strides are free (views into a
    time-major rollout buffer); the trailing dims must be contiguous."""
    _lib.require_gpu(states.device, "dgppo::env_step")
    io = _lib.EnvStepIO()
    io.states, io.states_stride = _p(states), _stride(states, 2)
    io.obstacles = _p(obstacles)
    io.obstacles_stride = obstacles.stride(-3) if obstacles is not None else 0
    io.action, io.action_stride = _p(action), _stride(action, 2)
    io.ray_dirs = _p(ray_dirs)
    io.nodes, io.nodes_stride = _p(nodes), _stride(nodes, 2)
    io.edges, io.edges_stride = _p(edges), _stride(edges, 2)
    io.out_states, io.out_states_stride = _p(out_states), _stride(out_states, 2)
    io.receivers, io.senders = _p(receivers), _p(senders)
    io.edge_index_stride = _stride(receivers, 1)
    io.reward, io.reward_stride = _p(reward), (reward.stride(0) if reward.dim() > 0 else 1)
    io.cost, io.cost_stride = _p(cost), _stride(cost, 2)
    io.n_env = int(states.shape[0])
    _lib.check(_lib.load().dgppo_env_step(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(states)),
               "dgppo_env_step")


env_step.register_fake(_returns_none)


@torch.library.custom_op("dgppo::env_reset", mutates_args=("obstacles", "nodes", "edges", "out_states", "receivers",
                                                            "senders"))
def env_reset(cfg: int, key: Optional[Tensor], seed: int, env_offset: int, n_env: int, obstacles: Optional[Tensor],
              ray_dirs: Tensor, nodes: Tensor, edges: Tensor, out_states: Tensor, receivers: Tensor,
              senders: Tensor) -> None:
    """Reset n_env envs (env b draws from Philox keyed (seed or *key, env_offset + b)) and write the
    initial graph.  `key`: optional 1-element int64 device tensor read at run time (hipGraph replays)."""
    _lib.require_gpu(nodes.device, "dgppo::env_reset")
    io = _reset_io(key, seed, env_offset, n_env, obstacles, ray_dirs, nodes, edges, out_states, receivers, senders)
    _lib.check(_lib.load().dgppo_env_reset(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(nodes)),
               "dgppo_env_reset")


env_reset.register_fake(_returns_none)


def _reset_io(key, seed, env_offset, n_env, obstacles, ray_dirs, nodes, edges, out_states, receivers, senders):
    io = _lib.EnvResetIO()
    if key is not None:
        if key.device != out_states.device or key.numel() != 1 or key.dtype not in (torch.int64, torch.uint64):
            raise ValueError("tensor key must be a 1-element int64 tensor on the env's device")
        io.seed, io.seed_ptr = 0, key.data_ptr()
    else:
        io.seed, io.seed_ptr = int(seed) & 0xFFFFFFFFFFFFFFFF, None
    io.env_offset = int(env_offset)
    io.obstacles = _p(obstacles)
    io.obstacles_stride = obstacles.stride(0) if obstacles is not None else 0
    io.ray_dirs = _p(ray_dirs)
    io.nodes, io.nodes_stride = _p(nodes), _stride(nodes, 2)
    io.edges, io.edges_stride = _p(edges), _stride(edges, 2)
    io.out_states, io.out_states_stride = _p(out_states), _stride(out_states, 2)
    io.receivers, io.senders = _p(receivers), _p(senders)
    io.edge_index_stride = _stride(receivers, 1)
    io.n_env = int(n_env)
    return io


@torch.library.custom_op("dgppo::env_reset_states", mutates_args=("obstacles", "nodes", "edges", "out_states",
                                                                   "receivers", "senders"))
def env_reset_states(cfg: int, key: Optional[Tensor], seed: int, env_offset: int, n_env: int,
                     obstacles: Optional[Tensor], ray_dirs: Tensor, nodes: Tensor, edges: Tensor, out_states: Tensor,
                     receivers: Tensor, senders: Tensor) -> None:
    """env_reset's sampling half: obstacle records and agent / goal state rows (configs without the
    persistent rollout kernel: the full reset).  Pair with env_rollout(rebuild_first=True)."""
    _lib.require_gpu(out_states.device, "dgppo::env_reset_states")
    io = _reset_io(key, seed, env_offset, n_env, obstacles, ray_dirs, nodes, edges, out_states, receivers, senders)
    _lib.check(_lib.load().dgppo_env_reset_states(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(out_states)),
               "dgppo_env_reset_states")


env_reset_states.register_fake(_returns_none)


@torch.library.custom_op("dgppo::env_rollout", mutates_args=("obstacles", "nodes", "edges", "states", "receivers",
                                                              "senders", "reward", "cost"))
def env_rollout(cfg: int, rebuild_first: bool, obstacles: Optional[Tensor], actions: Tensor, ray_dirs: Tensor,
                nodes: Tensor, edges: Tensor, states: Tensor, receivers: Tensor, senders: Tensor, reward: Tensor,
                cost: Tensor, reset_first: bool = False, key: Optional[Tensor] = None, seed: int = 0,
                env_offset: int = 0) -> None:
    """T env steps with given actions (T, B, n, A) through time-major graph buffers (T+1, B, ...):
    step t reads graph t and writes graph t+1, reward[t] (T, B), cost[t] (T, B, n, n_cost).
    rebuild_first: graph 0's rows are first built from its agent / goal states (env_reset_states).
    reset_first: env_reset_states (key / seed / env_offset as there; `obstacles` is written) + rebuild_first in the
    same call -- inside the one launch on the persistent Lidar route."""
    _lib.require_gpu(states.device, "dgppo::env_rollout")
    r = _rollout_io(rebuild_first, obstacles, actions, ray_dirs, nodes, edges, states, receivers, senders, reward, cost,
                    reset_first, key, seed, env_offset)
    _lib.check(_lib.load().dgppo_env_rollout(ctypes.byref(env_cfg(cfg)), ctypes.byref(r), _stream(states)),
               "dgppo_env_rollout")


def _rollout_io(rebuild_first, obstacles, actions, ray_dirs, nodes, edges, states, receivers, senders, reward, cost,
                reset_first=False, key=None, seed=0, env_offset=0):
    """The dgppo_env_rollout_io of env_rollout's tensors (env_rollout and env_rollout_plan both build it here)."""
    T = int(actions.shape[0])
    if states.shape[0] != T + 1 or reward.shape[0] != T or cost.shape[0] != T:
        raise ValueError("env_rollout: graph buffers must hold T+1 graphs, actions / reward / cost T steps")
    r = _lib.EnvRolloutIO()
    io = r.step
    io.states, io.states_stride = _p(states), _stride(states[0], 2)
    io.obstacles = _p(obstacles)
    io.obstacles_stride = obstacles.stride(-3) if obstacles is not None else 0
    # per env within a step; an episode of no steps (T = 0) has no action / cost element, so no strides to hold
    io.action, io.action_stride = _p(actions), (_stride(actions, 2) if T else 0)
    io.ray_dirs = _p(ray_dirs)
    io.nodes, io.nodes_stride = _p(nodes), _stride(nodes[0], 2)
    io.edges, io.edges_stride = _p(edges), _stride(edges[0], 2)
    io.out_states, io.out_states_stride = _p(states), _stride(states[0], 2)
    io.receivers, io.senders = _p(receivers), _p(senders)
    io.edge_index_stride = _stride(receivers[0], 1)
    io.reward, io.reward_stride = _p(reward), reward.stride(1)
    io.cost, io.cost_stride = _p(cost), (_stride(cost, 2) if T else 0)
    io.n_env = int(states.shape[1])
    r.T, r.rebuild_first = T, int(bool(rebuild_first))
    r.t_states, r.t_nodes, r.t_edges = states.stride(0), nodes.stride(0), edges.stride(0)
    if receivers.stride(0) != senders.stride(0):
        raise ValueError("env_rollout: receivers and senders need the same time stride")
    r.t_index, r.t_action, r.t_reward, r.t_cost = receivers.stride(0), actions.stride(0), reward.stride(0), cost.stride(0)
    r.reset_first, r.env_offset = int(bool(reset_first)), int(env_offset)
    if key is not None:
        if key.device != states.device or key.numel() != 1 or key.dtype not in (torch.int64, torch.uint64):
            raise ValueError("tensor key must be a 1-element int64 tensor on the env's device")
        r.seed, r.seed_ptr = 0, key.data_ptr()
    else:
        r.seed, r.seed_ptr = int(seed) & 0xFFFFFFFFFFFFFFFF, None
    return r


def env_rollout_plan(cfg: int, rebuild_first: bool, obstacles: Optional[Tensor], actions: Tensor, ray_dirs: Tensor,
                     nodes: Tensor, edges: Tensor, states: Tensor, receivers: Tensor, senders: Tensor, reward: Tensor,
                     cost: Tensor, reset_first: bool = False) -> _lib.EnvRolloutPlan:
    """The route env_rollout would take for these tensors (dgppo_env_rollout_plan: the kernel family, envs per
    workgroup, block sizes, action staging, grid and LDS), without launching anything.  Tensors on any device: only
    their addresses' alignment and strides are read."""
    r = _rollout_io(rebuild_first, obstacles, actions, ray_dirs, nodes, edges, states, receivers, senders, reward, cost,
                    reset_first)
    pl = _lib.EnvRolloutPlan()
    _lib.check(_lib.load().dgppo_env_rollout_plan(ctypes.byref(env_cfg(cfg)), ctypes.byref(r), ctypes.byref(pl)),
               "dgppo_env_rollout_plan")
    return pl


env_rollout.register_fake(_returns_none)


@torch.library.custom_op("dgppo::env_get_graph", mutates_args=("nodes", "edges", "states", "receivers", "senders"))
def env_get_graph(cfg: int, agent: Tensor, goal: Tensor, third: Optional[Tensor], ray_dirs: Tensor, nodes: Tensor,
                  edges: Tensor, states: Tensor, receivers: Tensor, senders: Tensor) -> None:
    """The graph of caller-given states for B envs: agent (B, n, sd), goal (B, n_goal_rows, sd) and `third` (the
    Lidar obstacle records (B, O, 16) / the MPE obstacle states (B, O, 4); None when n_obs == 0) -> the graph rows a
    reset writes.  Nothing is clipped.  Per-env strides are free; the trailing dims must be contiguous."""
    _lib.require_gpu(states.device, "dgppo::env_get_graph")
    io = _lib.EnvGraphIO()
    io.agent, io.agent_stride = _p(agent), _stride(agent, 2)
    io.goal, io.goal_stride = _p(goal), _stride(goal, 2)
    io.third, io.third_stride = _p(third), (_stride(third, 2) if third is not None else 0)
    io.ray_dirs = _p(ray_dirs)
    io.nodes, io.nodes_stride = _p(nodes), _stride(nodes, 2)
    io.edges, io.edges_stride = _p(edges), _stride(edges, 2)
    io.out_states, io.out_states_stride = _p(states), _stride(states, 2)
    io.receivers, io.senders = _p(receivers), _p(senders)
    io.edge_index_stride = _stride(receivers, 1)
    io.n_env = int(agent.shape[0])
    _lib.check(_lib.load().dgppo_env_get_graph(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(states)),
               "dgppo_env_get_graph")


env_get_graph.register_fake(_returns_none)


# ---- sensor in the loop: scan | hits | graph from hits ---------------------------------------------------
@torch.library.custom_op("dgppo::lidar_scan", mutates_args=("alpha",))
def lidar_scan(cfg: int, agent: Tensor, obstacles: Tensor, ray_dirs: Tensor, alpha: Tensor) -> None:
    """The raw LiDAR scan of B envs: agent (B, n, sd) rows and obstacle records (B, O, 16) -> alpha (B, n, R), per
    beam the value get_lidar sorts (1e6 = no return, 0 inside an obstacle, NaN propagates).  Per-env strides are
    free; the trailing dims must be contiguous."""
    _lib.require_gpu(alpha.device, "dgppo::lidar_scan")
    io = _scan_io(agent, obstacles, ray_dirs, alpha)
    _lib.check(_lib.load().dgppo_lidar_scan(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(alpha)),
               "dgppo_lidar_scan")


def _scan_io(agent, obstacles, ray_dirs, alpha) -> "_lib.LidarScanIO":
    """The dgppo_lidar_scan_io of the two scan ops' arguments."""
    io = _lib.LidarScanIO()
    io.agent, io.agent_stride = _p(agent), _stride(agent, 2)
    io.obstacles, io.obstacles_stride = _p(obstacles), _stride(obstacles, 2)
    io.ray_dirs = _p(ray_dirs)
    io.alpha, io.alpha_stride = _p(alpha), _stride(alpha, 2)
    io.n_env = int(agent.shape[0])
    return io


lidar_scan.register_fake(_returns_none)


@torch.library.custom_op("dgppo::lidar_scan_bodies", mutates_args=("alpha",))
def lidar_scan_bodies(cfg: int, agent: Tensor, obstacles: Tensor, ray_dirs: Tensor, alpha: Tensor) -> None:
    """lidar_scan whose beams also return off the other agents' bodies (discs of radius car_radius around columns 0, 1
    of the agent rows): per beam the nearer of the obstacle and the body return, an obstacle NaN propagating."""
    _lib.require_gpu(alpha.device, "dgppo::lidar_scan_bodies")
    _lib.check(_lib.load().dgppo_lidar_scan_bodies(ctypes.byref(env_cfg(cfg)),
                                                   ctypes.byref(_scan_io(agent, obstacles, ray_dirs, alpha)),
                                                   _stream(alpha)), "dgppo_lidar_scan_bodies")


lidar_scan_bodies.register_fake(_returns_none)


@torch.library.custom_op("dgppo::lidar_hits", mutates_args=("hits",))
def lidar_hits(cfg: int, agent: Tensor, alpha: Tensor, ray_dirs: Tensor, hits: Tensor) -> None:
    """Scan to hit points: agent (B, n, sd) rows and the caller's alpha (B, n, R) -> hits (B, n, top_k, 2), the top_k
    smallest alphas in jnp.argsort's order (stable, NaN last, -0 == +0) as points start + ray * alpha."""
    _lib.require_gpu(hits.device, "dgppo::lidar_hits")
    io = _lib.LidarHitsIO()
    io.agent, io.agent_stride = _p(agent), _stride(agent, 2)
    io.alpha, io.alpha_stride = _p(alpha), _stride(alpha, 2)
    io.ray_dirs = _p(ray_dirs)
    io.hits, io.hits_stride = _p(hits), _stride(hits, 3)
    io.n_env = int(agent.shape[0])
    _lib.check(_lib.load().dgppo_lidar_hits(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(hits)),
               "dgppo_lidar_hits")


lidar_hits.register_fake(_returns_none)


@torch.library.custom_op("dgppo::env_get_graph_hits", mutates_args=("nodes", "edges", "states", "receivers",
                                                                     "senders"))
def env_get_graph_hits(cfg: int, agent: Tensor, goal: Tensor, hits: Tensor, nodes: Tensor, edges: Tensor,
                       states: Tensor, receivers: Tensor, senders: Tensor) -> None:
    """env_get_graph with the LiDAR hit rows given: agent (B, n, sd), goal (B, n_goal_rows, sd) and hits
    (B, n, top_k, 2) -> the graph rows (get_graph's lidar_data argument).  No obstacles are read."""
    _lib.require_gpu(states.device, "dgppo::env_get_graph_hits")
    io = _lib.EnvGraphHitsIO()
    io.agent, io.agent_stride = _p(agent), _stride(agent, 2)
    io.goal, io.goal_stride = _p(goal), _stride(goal, 2)
    io.hits, io.hits_stride = _p(hits), _stride(hits, 3)
    io.nodes, io.nodes_stride = _p(nodes), _stride(nodes, 2)
    io.edges, io.edges_stride = _p(edges), _stride(edges, 2)
    io.out_states, io.out_states_stride = _p(states), _stride(states, 2)
    io.receivers, io.senders = _p(receivers), _p(senders)
    io.edge_index_stride = _stride(receivers, 1)
    io.n_env = int(agent.shape[0])
    _lib.check(_lib.load().dgppo_env_get_graph_hits(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(states)),
               "dgppo_env_get_graph_hits")


env_get_graph_hits.register_fake(_returns_none)


@torch.library.custom_op("dgppo::lidar_observe", mutates_args=("nodes", "edges", "states", "receivers", "senders"))
def lidar_observe(cfg: int, agent: Tensor, goal: Tensor, obstacles: Tensor, ray_dirs: Tensor, key: Optional[Tensor],
                  seed: int, env_offset: int, t: int, noise_scale: float, drop_below: float, flags: int,
                  nodes: Tensor, edges: Tensor, states: Tensor, receivers: Tensor, senders: Tensor) -> None:
    """The observed graph of B true states under the LidarNoise sensor model, one launch: lidar_scan, the model
    (utils/sensor.py: flags = OBSERVE_NOISE | OBSERVE_DROPOUT, noise_scale = sigma / sense_range, drop_below =
    Phi^-1(dropout)), lidar_hits and env_get_graph_hits fused.  The draws of beam (b, i, r) are the Philox normals of
    element ((env_offset + b) n + i) R + r under (seed or *key) and the streams of step t.  `key`: optional 1-element
    int64 device tensor read at run time (hipGraph replays)."""
    _observe("lidar_observe", cfg, agent, goal, obstacles, ray_dirs, key, seed, env_offset, t, noise_scale, drop_below,
             flags, nodes, edges, states, receivers, senders)


def _observe(name, cfg, agent, goal, obstacles, ray_dirs, key, seed, env_offset, t, noise_scale, drop_below, flags, nodes,
             edges, states, receivers, senders, *extra) -> None:
    """The body of the three observe ops: the dgppo_lidar_observe_io of their arguments, then the entry dgppo_<name>
    (`extra`: what that entry takes between the io and the stream)."""
    _lib.require_gpu(states.device, "dgppo::" + name)
    io = _lib.LidarObserveIO()
    io.agent, io.agent_stride = _p(agent), _stride(agent, 2)
    io.goal, io.goal_stride = _p(goal), _stride(goal, 2)
    io.obstacles, io.obstacles_stride = _p(obstacles), _stride(obstacles, 2)
    io.ray_dirs = _p(ray_dirs)
    io.nodes, io.nodes_stride = _p(nodes), _stride(nodes, 2)
    io.edges, io.edges_stride = _p(edges), _stride(edges, 2)
    io.out_states, io.out_states_stride = _p(states), _stride(states, 2)
    io.receivers, io.senders = _p(receivers), _p(senders)
    io.edge_index_stride = _stride(receivers, 1)
    io.n_env, io.flags = int(agent.shape[0]), int(flags)
    io.env_offset, io.t = int(env_offset), int(t)
    if key is not None:
        if key.device != states.device or key.numel() != 1 or key.dtype not in (torch.int64, torch.uint64):
            raise ValueError("tensor key must be a 1-element int64 tensor on the env's device")
        io.seed, io.seed_ptr = 0, key.data_ptr()
    else:
        io.seed, io.seed_ptr = int(seed) & 0xFFFFFFFFFFFFFFFF, None
    io.noise_scale, io.drop_below = float(noise_scale), float(drop_below)
    entry = getattr(_lib.load(), "dgppo_" + name)
    _lib.check(entry(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), *extra, _stream(states)), "dgppo_" + name)


lidar_observe.register_fake(_returns_none)


@torch.library.custom_op("dgppo::lidar_observe_los", mutates_args=("nodes", "edges", "states", "receivers", "senders"))
def lidar_observe_los(cfg: int, agent: Tensor, goal: Tensor, obstacles: Tensor, ray_dirs: Tensor,
                      key: Optional[Tensor], seed: int, env_offset: int, t: int, noise_scale: float, drop_below: float,
                      flags: int, nodes: Tensor, edges: Tensor, states: Tensor, receivers: Tensor,
                      senders: Tensor) -> None:
    """lidar_observe that also takes OBSERVE_SIGHT in `flags`: the observed graph with every agent-agent edge whose
    receiver cannot see its sender past the obstacles (lidar_sight) routed to the pad node, in the same launch."""
    _observe("lidar_observe_los", cfg, agent, goal, obstacles, ray_dirs, key, seed, env_offset, t, noise_scale,
             drop_below, flags, nodes, edges, states, receivers, senders)


lidar_observe_los.register_fake(_returns_none)


@torch.library.custom_op("dgppo::lidar_sight", mutates_args=("visible",))
def lidar_sight(cfg: int, agent: Tensor, obstacles: Tensor, visible: Tensor) -> None:
    """Line of sight between the agents of B envs: agent (B, n, sd) rows and obstacle records (B, O, 16) -> visible
    (B, n, n) uint8, 1 where no obstacle edge cuts the segment from receiver i to sender j (the diagonal is 1).
    Per-env strides are free; the trailing dims must be contiguous."""
    _lib.require_gpu(visible.device, "dgppo::lidar_sight")
    if visible.dtype != torch.uint8:
        raise ValueError(f"dgppo::lidar_sight: visible must be uint8, got {visible.dtype}")
    io = _lib.LidarSightIO()
    io.agent, io.agent_stride = _p(agent), _stride(agent, 2)
    io.obstacles, io.obstacles_stride = _p(obstacles), _stride(obstacles, 2)
    io.visible, io.visible_stride = visible.data_ptr(), _stride(visible, 2)
    io.n_env = int(agent.shape[0])
    _lib.check(_lib.load().dgppo_lidar_sight(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(visible)),
               "dgppo_lidar_sight")


lidar_sight.register_fake(_returns_none)


@torch.library.custom_op("dgppo::lidar_observe_fov", mutates_args=("nodes", "edges", "states", "receivers", "senders"))
def lidar_observe_fov(cfg: int, agent: Tensor, goal: Tensor, obstacles: Tensor, ray_dirs: Tensor,
                      key: Optional[Tensor], seed: int, env_offset: int, t: int, noise_scale: float, drop_below: float,
                      flags: int, half_angle_deg: float, nodes: Tensor, edges: Tensor, states: Tensor,
                      receivers: Tensor, senders: Tensor) -> None:
    """lidar_observe_los that also takes OBSERVE_FOV in `flags`: every agent-agent edge whose sender is outside the
    receiver's forward cone of `half_angle_deg` (agent_fov) goes to the pad node as well, in the same launch."""
    _observe("lidar_observe_fov", cfg, agent, goal, obstacles, ray_dirs, key, seed, env_offset, t, noise_scale,
             drop_below, flags, nodes, edges, states, receivers, senders, float(half_angle_deg))


lidar_observe_fov.register_fake(_returns_none)


@torch.library.custom_op("dgppo::lidar_observe_bodies", mutates_args=("nodes", "edges", "states", "receivers", "senders"))
def lidar_observe_bodies(cfg: int, agent: Tensor, goal: Tensor, obstacles: Tensor, ray_dirs: Tensor,
                         key: Optional[Tensor], seed: int, env_offset: int, t: int, noise_scale: float, drop_below: float,
                         flags: int, half_angle_deg: float, nodes: Tensor, edges: Tensor, states: Tensor,
                         receivers: Tensor, senders: Tensor) -> None:
    """lidar_observe_fov that also takes OBSERVE_BODIES in `flags`: the beams return off the other agents' bodies too
    (lidar_scan_bodies' alphas, before the sensor model), in the same launch."""
    _observe("lidar_observe_bodies", cfg, agent, goal, obstacles, ray_dirs, key, seed, env_offset, t, noise_scale,
             drop_below, flags, nodes, edges, states, receivers, senders, float(half_angle_deg))


lidar_observe_bodies.register_fake(_returns_none)


@torch.library.custom_op("dgppo::agent_fov", mutates_args=("in_fov",))
def agent_fov(cfg: int, agent: Tensor, half_angle_deg: float, in_fov: Tensor) -> None:
    """Field of view between the agents of B envs: agent (B, n, sd) rows (columns 2, 3 the heading's cos, sin) ->
    in_fov (B, n, n) uint8, 1 where sender j is inside receiver i's forward cone of `half_angle_deg` by the FoV cost's
    arithmetic (the diagonal is 1).  Per-env strides are free; the trailing dims must be contiguous."""
    _lib.require_gpu(in_fov.device, "dgppo::agent_fov")
    if in_fov.dtype != torch.uint8:
        raise ValueError(f"dgppo::agent_fov: in_fov must be uint8, got {in_fov.dtype}")
    io = _lib.AgentFovIO()
    io.agent, io.agent_stride = _p(agent), _stride(agent, 2)
    io.in_fov, io.in_fov_stride = in_fov.data_ptr(), _stride(in_fov, 2)
    io.half_angle_deg, io.n_env = float(half_angle_deg), int(agent.shape[0])
    _lib.check(_lib.load().dgppo_agent_fov(ctypes.byref(env_cfg(cfg)), ctypes.byref(io), _stream(in_fov)),
               "dgppo_agent_fov")


agent_fov.register_fake(_returns_none)


def _render_args(states: Tensor, receivers: Tensor, senders: Tensor, obstacles: Optional[Tensor], out: Tensor,
                 flags: int) -> _lib.RenderArgs:
    """Check the tensors of a render_frames call and fill its dgppo_render_args."""
    nb = states.dim() - 2
    if nb not in (1, 2) or receivers.dim() != nb + 1 or receivers.shape != senders.shape or \
            receivers.shape[:nb] != states.shape[:nb]:
        raise ValueError("render_frames: states (B[, T], N, sd) with receivers / senders (B[, T], E)")
    if states.dtype != torch.float32 or receivers.dtype != torch.int32 or senders.dtype != torch.int32:
        raise ValueError("render_frames: float32 states and int32 receivers / senders")
    frames = int(states.shape[0]) * (int(states.shape[1]) if nb == 2 else 1)
    if out.dtype != torch.uint8 or out.dim() < 3 or not out.is_contiguous() or out.shape[-1] != 4 or \
            out.shape[-2] != out.shape[-3] or out.numel() != frames * 4 * int(out.shape[-2]) ** 2:
        raise ValueError("render_frames: out must be a contiguous uint8 (frames, S, S, 4) tensor")
    if receivers.stride()[:nb] != senders.stride()[:nb]:
        raise ValueError("render_frames: receivers and senders need the same batch strides")
    a = _lib.RenderArgs()
    for t, inner in ((states, 2), (receivers, 1), (senders, 1)):
        _stride(t, inner)  # raises unless the trailing dims are contiguous
    a.states, a.states_estride, a.states_tstride = _p(states), states.stride(0), (states.stride(1) if nb == 2 else 0)
    a.receivers, a.senders = _p(receivers), _p(senders)
    a.index_estride, a.index_tstride = receivers.stride(0), (receivers.stride(1) if nb == 2 else 0)
    if obstacles is not None:
        if obstacles.dim() != 3 or obstacles.shape[0] != states.shape[0] or obstacles.dtype != torch.float32:
            raise ValueError("render_frames: obstacles must be float32 (B, O, 16), one set per episode")
        _stride(obstacles, 2)
        a.obstacles, a.obstacles_estride = _p(obstacles), obstacles.stride(0)
    a.out = _p(out)
    a.n_frames, a.frames_per_episode = frames, (int(states.shape[1]) if nb == 2 else 1)
    a.size, a.flags = int(out.shape[-2]), int(flags)
    return a


@torch.library.custom_op("dgppo::render_frames", mutates_args=("out",))
def render_frames(cfg: int, states: Tensor, receivers: Tensor, senders: Tensor, obstacles: Optional[Tensor],
                  out: Tensor, flags: int) -> None:
    """Rasterise the frames of a graph batch: states (B, N, sd) or (B, T, N, sd) with receivers / senders (B[, T], E)
    int32 and the Lidar obstacle records (B, O, 16) (one set per episode; None for MPE or n_obs == 0) -> out, a
    contiguous uint8 (B[, T], S, S, 4) RGBA image stack.  The batch strides are free (the (B, T) view of a time-major
    rollout buffer passes without a copy); the trailing dims must be contiguous.  flags bit 0: FoV wedges."""
    _lib.require_gpu(states.device, "dgppo::render_frames")
    _lib.require_gpu(out.device, "dgppo::render_frames")
    a = _render_args(states, receivers, senders, obstacles, out, flags)
    if a.n_frames == 0:
        return
    _lib.check(_lib.load().dgppo_render_frames(ctypes.byref(env_cfg(cfg)), ctypes.byref(a), _stream(states)),
               "dgppo_render_frames")


render_frames.register_fake(_returns_none)


@torch.library.custom_op("dgppo::render_frames_field", mutates_args=("out",))
def render_frames_field(cfg: int, states: Tensor, receivers: Tensor, senders: Tensor, obstacles: Optional[Tensor],
                        values: Tensor, palette: Tensor, extent: List[float], half_range: float, alpha: float,
                        line_halfwidth: float, out: Tensor, flags: int) -> None:
    """render_frames with a scalar field under every other layer: values, contiguous float32 (B[, T], Gy, Gx) on the
    states' device, one grid per frame on the uniform axes spanning extent = (x0, x1, y0, y1); palette, contiguous
    float32 (K, 3) straight sRGB on that device, K bands over [-half_range, half_range]; alpha of the bands on white;
    the black zero line's half-width in world units.  DESIGN.md "Rendering" has the pixel rule."""
    _lib.require_gpu(states.device, "dgppo::render_frames_field")
    _lib.require_gpu(out.device, "dgppo::render_frames_field")
    a = _render_args(states, receivers, senders, obstacles, out, flags)
    nb = states.dim() - 2
    if values.dtype != torch.float32 or values.dim() != nb + 2 or values.shape[:nb] != states.shape[:nb] or \
            not values.is_contiguous() or values.device != states.device:
        raise ValueError("render_frames_field: values must be a contiguous float32 (B[, T], Gy, Gx) tensor on the "
                         "states' device")
    if palette.dtype != torch.float32 or palette.dim() != 2 or palette.shape[1] != 3 or not palette.is_contiguous() or \
            palette.device != states.device:
        raise ValueError("render_frames_field: palette must be a contiguous float32 (K, 3) tensor on the states' "
                         "device")
    if len(extent) != 4:
        raise ValueError("render_frames_field: extent is (x0, x1, y0, y1)")
    f = _lib.RenderField()
    f.values, f.palette = _p(values), _p(palette)
    f.gy, f.gx, f.bands = int(values.shape[-2]), int(values.shape[-1]), int(palette.shape[0])
    f.extent[:] = [float(v) for v in extent]
    f.half_range, f.alpha, f.line_halfwidth = float(half_range), float(alpha), float(line_halfwidth)
    if a.n_frames == 0:
        return
    _lib.check(_lib.load().dgppo_render_frames_field(ctypes.byref(env_cfg(cfg)), ctypes.byref(a), ctypes.byref(f),
                                                     _stream(states)), "dgppo_render_frames_field")


render_frames_field.register_fake(_returns_none)


@torch.library.custom_op("dgppo::render_frames_vmas", mutates_args=("out",))
def render_frames_vmas(cfg: int, states: Tensor, record: Tensor, out: Tensor) -> None:
    """Rasterise the frames of a VMASWheel / VMASReverseTransport graph batch: states (B, 4, 4) or (B, T, 4, 4)
    float32 (agents 0..2, then the body row) and the env record (B, 1, 8), one per episode -> out, a contiguous uint8
    (B[, T], S, S, 4) RGBA image stack.  The states' batch strides are free (the (B, T) view of a time-major rollout
    buffer passes without a copy); the trailing dims must be contiguous.  No edges are drawn, so none are passed."""
    _lib.require_gpu(states.device, "dgppo::render_frames_vmas")
    _lib.require_gpu(out.device, "dgppo::render_frames_vmas")
    nb = states.dim() - 2
    if nb not in (1, 2) or tuple(states.shape[-2:]) != (4, 4) or states.dtype != torch.float32:
        raise ValueError("render_frames_vmas: float32 states (B[, T], 4, 4)")
    if record.dim() != 3 or tuple(record.shape) != (states.shape[0], 1, _lib.DGPPO_VMAS_FIELDS) or \
            record.dtype != torch.float32 or record.device != states.device:
        raise ValueError("render_frames_vmas: record must be float32 (B, 1, 8) on the states' device, one per episode")
    frames = int(states.shape[0]) * (int(states.shape[1]) if nb == 2 else 1)
    if out.dtype != torch.uint8 or out.dim() < 3 or not out.is_contiguous() or out.shape[-1] != 4 or \
            out.shape[-2] != out.shape[-3] or out.numel() != frames * 4 * int(out.shape[-2]) ** 2:
        raise ValueError("render_frames_vmas: out must be a contiguous uint8 (frames, S, S, 4) tensor")
    _stride(states, 2)  # raises unless the trailing dims are contiguous
    _stride(record, 2)
    a = _lib.RenderArgs()
    a.states, a.states_estride, a.states_tstride = _p(states), states.stride(0), (states.stride(1) if nb == 2 else 0)
    a.obstacles, a.obstacles_estride = _p(record), record.stride(0)
    a.out = _p(out)
    a.n_frames, a.frames_per_episode = frames, (int(states.shape[1]) if nb == 2 else 1)
    a.size, a.flags = int(out.shape[-2]), 0
    if a.n_frames == 0:
        return
    _lib.check(_lib.load().dgppo_render_frames_vmas(ctypes.byref(env_cfg(cfg)), ctypes.byref(a), _stream(states)),
               "dgppo_render_frames_vmas")


render_frames_vmas.register_fake(_returns_none)


# ---- GraphTransformer attention core -------------------------------------------------------------------
def _attn_struct(dims, cand, receivers, senders, sidx, x, x_gstride, ef, ef_gstride, q, qt, bk, scale, xa, xa_gstride,
                 pre_W, pre_b, beta=None, beta_ld=0, qt_ld=0) -> _lib.GnnAttnArgs:
    a = _lib.GnnAttnArgs()
    a.G, a.N, a.E, a.n_agents, a.D, a.F, a.H, a.C, a.D0 = (int(v) for v in dims)
    a.cand, a.receivers, a.senders, a.sidx = _p(cand), _p(receivers), _p(senders), _p(sidx)
    a.x, a.x_gstride = _p(x), int(x_gstride)
    a.ef, a.ef_gstride = _p(ef), int(ef_gstride)
    a.q, a.qt, a.bk = _p(q), _p(qt), _p(bk)
    a.scale = float(scale)
    a.xa, a.xa_gstride = _p(xa), int(xa_gstride)
    a.pre_W, a.pre_b = _p(pre_W), _p(pre_b)
    a.beta, a.beta_ld, a.qt_ld = _p(beta), int(beta_ld), int(qt_ld)
    return a


@torch.library.custom_op("dgppo::gnn_attn_fwd", mutates_args=("attn", "xcat"))
def gnn_attn_fwd(dims: List[int], cand: Tensor, receivers: Tensor, senders: Tensor, sidx: Tensor, x: Tensor,
                 x_gstride: int, ef: Tensor, ef_gstride: int, q: Optional[Tensor], qt: Tensor, bk: Tensor,
                 scale: float, xa: Optional[Tensor], xa_gstride: int, pre_W: Optional[Tensor],
                 pre_b: Optional[Tensor], attn: Tensor, xcat: Tensor, beta: Optional[Tensor] = None,
                 beta_ld: int = 0, qt_ld: int = 0) -> None:
    """Per-receiving-agent attention of one GraphTransformer layer (dims = [G, N, E, n, D, F, H, C, D0]):
    attn (G*n, H, C) = segment softmax of (q . k)/sqrt(F) over each agent's candidate edges, xcat
    (G*n, H*(D+5)) = the attention-weighted [sender rows | edge rows | 1] per head (nn/layers.py).
    Q-free form: q None and beta (G*n, H) = q_h . bk_h given (row stride beta_ld); qt_ld = qt's row stride."""
    _lib.require_gpu(qt.device, "dgppo::gnn_attn_fwd")
    a = _attn_struct(dims, cand, receivers, senders, sidx, x, x_gstride, ef, ef_gstride, q, qt, bk, scale, xa,
                     xa_gstride, pre_W, pre_b, beta, beta_ld, qt_ld)
    a.attn, a.xcat = _p(attn), _p(xcat)
    _lib.check(_lib.load().dgppo_gnn_attn_fwd(ctypes.byref(a), _stream(qt)), "dgppo_gnn_attn_fwd")


gnn_attn_fwd.register_fake(_returns_none)


@torch.library.custom_op("dgppo::gnn_attn_bwd", mutates_args=("dqt", "dq", "dbeta", "dxa", "dpre_part", "dx"))
def gnn_attn_bwd(dims: List[int], cand: Tensor, receivers: Tensor, senders: Tensor, sidx: Tensor, x: Tensor,
                 x_gstride: int, ef: Tensor, ef_gstride: int, q: Optional[Tensor], qt: Tensor, bk: Tensor,
                 scale: float, xa: Optional[Tensor], xa_gstride: int, pre_W: Optional[Tensor],
                 pre_b: Optional[Tensor], attn: Tensor, dxcat: Tensor, da_add: Optional[Tensor], dqt: Tensor,
                 dq: Optional[Tensor], dbeta: Tensor, dxa: Optional[Tensor], dxa_gstride: int,
                 dpre_part: Optional[Tensor], beta: Optional[Tensor] = None, beta_ld: int = 0, qt_ld: int = 0,
                 dqt_ld: int = 0, dbeta_ld: int = 0, dx: Optional[Tensor] = None, dx_gstride: int = 0) -> None:
    """Backward of gnn_attn_fwd given dL/dxcat (+ da_add, extra dL/dattn of edge columns past 4): dqt, dq,
    dbeta (dL/d(q . bk)); in agent mode dxa (accumulated, agent senders) and the partial Dense_4
    gradients of the recomputed never-receiving senders (dpre_part, one row per workgroup); otherwise,
    if dx is given, the sender gradient of every node row of x (accumulated, graph stride dx_gstride).
    Q-free form: dq None (not written), dqt / dbeta row strides dqt_ld / dbeta_ld (e.g. one [dqt | dbeta]
    buffer)."""
    _lib.require_gpu(qt.device, "dgppo::gnn_attn_bwd")
    a = _attn_struct(dims, cand, receivers, senders, sidx, x, x_gstride, ef, ef_gstride, q, qt, bk, scale, xa,
                     xa_gstride, pre_W, pre_b, beta, beta_ld, qt_ld)
    a.dqt_ld, a.dbeta_ld = int(dqt_ld), int(dbeta_ld)
    a.attn, a.dxcat, a.da_add = _p(attn), _p(dxcat), _p(da_add)
    a.dqt, a.dq, a.dbeta = _p(dqt), _p(dq), _p(dbeta)
    a.dxa, a.dxa_gstride, a.dpre_part = _p(dxa), int(dxa_gstride), _p(dpre_part)
    a.dx, a.dx_gstride = _p(dx), int(dx_gstride)
    _lib.check(_lib.load().dgppo_gnn_attn_bwd(ctypes.byref(a), _stream(qt)), "dgppo_gnn_attn_bwd")


gnn_attn_bwd.register_fake(_returns_none)


def gnn_attn_partial_blocks(dims, cand, receivers, senders, sidx, x, x_gstride, ef, ef_gstride, q, qt, bk, scale, xa,
                            xa_gstride, pre_W, pre_b, beta=None, beta_ld=0, qt_ld=0) -> int:
    """Rows of the dpre_part workspace gnn_attn_bwd writes for these arguments (host query)."""
    a = _attn_struct(dims, cand, receivers, senders, sidx, x, x_gstride, ef, ef_gstride, q, qt, bk, scale, xa,
                     xa_gstride, pre_W, pre_b, beta, beta_ld, qt_ld)
    return int(_lib.load().dgppo_gnn_attn_partial_blocks(ctypes.byref(a)))


def gnn_attn_plan(bwd: bool, dx=None, dxa=None, **args) -> _lib.GnnAttnPlan:
    """The kernel family, instantiation, grid and LDS bytes gnn_attn_fwd (bwd False) / gnn_attn_bwd (bwd True) take
    for `args`, the dict of GraphTransformer._attn_args, with dx / dxa as the backward call passes them (host query,
    needs no GPU).  ValueError where the call itself would be refused for its shape."""
    a = _attn_struct(**args)
    a.dx, a.dxa = _p(dx), _p(dxa)
    pl = _lib.GnnAttnPlan()
    _lib.check(_lib.load().dgppo_gnn_attn_plan(ctypes.byref(a), int(bool(bwd)), ctypes.byref(pl)),
               "dgppo_gnn_attn_plan")
    return pl


# ---- one GraphTransformer layer forward as one kernel (ABI 11) -------------------------------------------
TAIL_FIELDS = ("W0", "b0", "ln0_s", "ln0_b", "W1", "b1", "ln1_s", "ln1_b", "Wi", "bi", "Wh", "bhn", "Wo", "bo")


def _layer_struct(dims, cand, receivers, senders, sidx, x, x_gstride, ef, ef_gstride, scale, xa, xa_gstride, pre_W,
                  pre_b, QBW, Wcat, Wu, bu, Y, qb=None, attn=None, xcat=None, zmean=None, tail_w=(), tail_h=None,
                  tail_out=None) -> _lib.GnnLayerArgs:
    la = _lib.GnnLayerArgs()
    la.a = _attn_struct(dims, cand, receivers, senders, sidx, x, x_gstride, ef, ef_gstride, None, None, None, scale, xa,
                        xa_gstride, pre_W, pre_b)
    la.a.attn, la.a.xcat = _p(attn), _p(xcat)
    la.QBW, la.qb, la.Wcat, la.Wu, la.bu, la.Y = _p(QBW), _p(qb), _p(Wcat), _p(Wu), _p(bu), _p(Y)
    la.zmean = _p(zmean)
    if tail_out is not None:
        for name, t in zip(TAIL_FIELDS, tail_w):
            setattr(la.tail, name, _p(t))
        la.tail.h_in, la.tail.out = _p(tail_h), _p(tail_out)
        la.tail.n_out, la.tail.on = int(tail_out.shape[-1]), 1
    return la


def gnn_layer_supported(**kw) -> bool:
    """Whether dgppo_gnn_layer_fwd covers this layer call (host query; same keyword arguments as gnn_layer_fwd)."""
    return bool(_lib.load().dgppo_gnn_layer_supported(ctypes.byref(_layer_struct(**kw))))


@torch.library.custom_op("dgppo::gnn_layer_fwd", mutates_args=("Y", "qb", "attn", "xcat", "zmean", "tail_out"))
def gnn_layer_fwd(dims: List[int], cand: Tensor, receivers: Tensor, senders: Tensor, sidx: Tensor, x: Tensor,
                  x_gstride: int, ef: Tensor, ef_gstride: int, scale: float, xa: Optional[Tensor], xa_gstride: int,
                  pre_W: Optional[Tensor], pre_b: Optional[Tensor], QBW: Tensor, Wcat: Tensor, Wu: Tensor, bu: Tensor,
                  Y: Optional[Tensor], qb: Optional[Tensor], attn: Optional[Tensor], xcat: Optional[Tensor],
                  zmean: Optional[Tensor], tail_w: List[Tensor], tail_h: Optional[Tensor],
                  tail_out: Optional[Tensor]) -> None:
    """One GraphTransformer layer forward (dims as gnn_attn_fwd): Y (G*n, F) = relu(xcat Wcat / H + x_i Wu + bu) with
    the attention of gnn_attn_fwd in between and [qt | beta] = [x_i 1] QBW, all in one kernel; qb, attn and xcat are
    optional outputs for the backward (nn/layers.py GraphTransformer.fwd).  Forward-only epilogues: zmean (G, F) the
    per-graph agent mean of Y; tail_out (G*n, n_out) the value head after the layer (MLP -> GRU(tail_h) -> Dense,
    weights tail_w in TAIL_FIELDS order)."""
    dev = (Y if Y is not None else zmean if zmean is not None else tail_out).device
    _lib.require_gpu(dev, "dgppo::gnn_layer_fwd")
    la = _layer_struct(dims, cand, receivers, senders, sidx, x, x_gstride, ef, ef_gstride, scale, xa, xa_gstride, pre_W,
                       pre_b, QBW, Wcat, Wu, bu, Y, qb, attn, xcat, zmean, tail_w, tail_h, tail_out)
    _lib.check(_lib.load().dgppo_gnn_layer_fwd(ctypes.byref(la), _lib.stream_handle(dev)), "dgppo_gnn_layer_fwd")


gnn_layer_fwd.register_fake(_returns_none)


# ---- GAE, clip + Adam ------------------------------------------------------------------------------------
@torch.library.custom_op("dgppo::gae", mutates_args=("Qh", "Ql"))
def gae(hs: Tensor, l: Tensor, Vh: Tensor, Vl: Tensor, Qh: Tensor, Ql: Tensor, gamma: float, lam: float) -> None:
    """Dec-OCP GAE per env: hs (B, T, n, nh) costs, l (B, T) losses, Vh (B, T+1, n, nh), Vl (B, T+1)
    -> Qh (B, T, n, nh), Ql (B, T) (the reference's O(T^2) row scan, literally)."""
    _lib.require_gpu(hs.device, "dgppo::gae")
    for t in (hs, l, Vh, Vl, Qh, Ql):
        if not t.is_contiguous():
            raise ValueError("dgppo::gae needs contiguous tensors")
    B, T, n, nh = hs.shape
    a = _lib.GaeArgs()
    a.B, a.T, a.n_agents, a.n_h = int(B), int(T), int(n), int(nh)
    a.hs, a.l, a.Vh, a.Vl, a.Qh, a.Ql = _p(hs), _p(l), _p(Vh), _p(Vl), _p(Qh), _p(Ql)
    a.gamma = float(gamma)
    setattr(a, "lambda", float(lam))
    _lib.check(_lib.load().dgppo_gae(ctypes.byref(a), _stream(hs)), "dgppo_gae")


gae.register_fake(_returns_none)


@torch.library.custom_op("dgppo::grad_norm", mutates_args=("state",))
def grad_norm(grad: Tensor, state: Tensor) -> None:
    """state[0] = global L2 norm of grad, state[1] = number of non-finite entries (state[2]: Adam count)."""
    _lib.require_gpu(grad.device, "dgppo::grad_norm")
    lib = _lib.load()
    from .nn.kernels import workspace

    ws = workspace(lib.dgppo_loss_workspace_floats(), grad.device, "norm")
    _lib.check(lib.dgppo_grad_norm(_p(grad), int(grad.numel()), _p(state), _p(ws), _stream(grad)), "dgppo_grad_norm")


grad_norm.register_fake(_returns_none)


@torch.library.custom_op("dgppo::adam", mutates_args=("param", "m", "v", "state"))
def adam(param: Tensor, grad: Tensor, m: Tensor, v: Tensor, state: Tensor, lr: float, b1: float, b2: float,
         eps: float, max_norm: float) -> None:
    """g <- g * max_norm / max(max_norm, |g|) and one optax adam step, skipped entirely (apply_if_finite)
    when state[1] (non-finite count from dgppo::grad_norm) is non-zero; state[2] counts applied steps."""
    _lib.require_gpu(param.device, "dgppo::adam")
    _lib.check(_lib.load().dgppo_adam(_p(param), _p(grad), _p(m), _p(v), int(param.numel()), _p(state), float(lr),
                                      float(b1), float(b2), float(eps), float(max_norm), _stream(param)), "dgppo_adam")


adam.register_fake(_returns_none)


# ---- minibatch assembly ---------------------------------------------------------------------------------
@torch.library.custom_op("dgppo::gather_env_steps", mutates_args=("dst",))
def gather_env_steps(src: List[Tensor], dst: List[Tensor], envs: Tensor) -> None:
    """dst[i][e, t] = src[i][envs[e], t] for (B, T, ...) rollout fields (any strides on B and T, e.g. views
    of time-major buffers; contiguous trailing dims; 4-byte dtypes) into contiguous (Bm, T, ...) outputs:
    the reference's `jtu.tree_map(lambda x: x[idx], rollout)` as one launch for up to 8 fields."""
    if not src or len(src) != len(dst) or len(src) > 8:
        raise ValueError("gather_env_steps: 1..8 (src, dst) pairs")
    _lib.require_gpu(envs.device, "dgppo::gather_env_steps")
    if envs.dtype != torch.int64 or envs.dim() != 1:
        raise ValueError("envs must be a 1-d int64 tensor")
    T = int(src[0].shape[1])
    fields = (_lib.GatherField * len(src))()
    for f, a, b in zip(fields, src, dst):
        if a.element_size() != 4 or b.element_size() != 4 or a.dim() < 2 or a.shape[1] != T:
            raise ValueError("gather_env_steps: (B, T, ...) fields of 4-byte elements")
        if tuple(b.shape) != (envs.shape[0],) + tuple(a.shape[1:]) or not b.is_contiguous():
            raise ValueError("gather_env_steps: dst must be contiguous (len(envs), T, ...)")
        inner = 1
        for d in range(a.dim() - 1, 1, -1):
            if a.shape[d] != 1 and a.stride(d) != inner:
                raise ValueError("gather_env_steps: trailing dims must be contiguous")
            inner *= a.shape[d]
        f.src, f.dst, f.row_elems = _p(a), _p(b), inner
        f.src_tstride, f.src_estride = a.stride(1), a.stride(0)
    if envs.shape[0] == 0:  # an empty selection gathers nothing (an empty tensor has no address to pass)
        return
    _lib.check(_lib.load().dgppo_gather_env_steps(fields, len(src), _p(envs), int(envs.shape[0]), T, _stream(envs)),
               "dgppo_gather_env_steps")


gather_env_steps.register_fake(_returns_none)
