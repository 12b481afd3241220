"""MultiAgentEnv: the reference's env plugin API (dgppo/env/base.py:30-150), batched over envs.

Differences from the reference, all deliberate:
  * `reset(key, n_env)` / `step(graph, action)` take and return env-batched tensors (leading B);
    the reference's per-env functions are `jax.vmap`-ed by the algorithm instead.
  * `step` runs ONE fused HIP kernel (dgppo_env_step in libdgppo_hip.so) that does dynamics,
    LiDAR, reward, cost and the padded graph build; `reset` runs dgppo_env_reset.
  * `PARAMS` is copied per instance (the reference mutates the class dict in make_env).
There is no CPU fallback: without the HIP library every call raises NativeLibraryError.
"""
from __future__ import annotations

import copy
import ctypes
from abc import ABC
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from .. import _lib, ops
from ..utils.graph import GraphsTuple


class StepResult(NamedTuple):
    graph: GraphsTuple
    reward: torch.Tensor  # (B,)
    cost: torch.Tensor  # (B, n, n_cost)
    done: torch.Tensor  # (B,) bool, always False (fixed-horizon episodes)
    info: dict


class RolloutResult(NamedTuple):
    Tp1_graph: GraphsTuple
    T_action: torch.Tensor
    T_reward: torch.Tensor
    T_cost: torch.Tensor
    T_done: torch.Tensor
    T_info: dict
    T_rnn_state: torch.Tensor


class MultiAgentEnv(ABC):
    PARAMS: dict = {}
    ENGINE: int = _lib.DGPPO_ENGINE_LIDAR
    GOAL_MODE: int = _lib.DGPPO_GOAL_SPREAD

    AGENT = 0
    GOAL = 1
    OBS = 2

    # node columns a never-receiving node can have nonzero (None: all); the GNN's agent-mode layers read only
    # these when the nodes are wider than the attention kernels' raw-row limit (nn/layers.py GraphBatch)
    nonagent_feature_cols = None

    def __init__(self, num_agents: int, area_size: float, max_step: int = 256, dt: float = 0.03,
                 params: Optional[dict] = None, device=None):
        self._num_agents = int(num_agents)
        self._dt = dt
        self._params = copy.deepcopy(self.PARAMS if params is None else params)
        self._t = 0
        self._max_step = max_step
        self._area_size = area_size
        self.num_goals = self._n_goals()  # goal node rows (the line / formation variants: landmarks)
        self.device = torch.device(device) if device is not None else (
            torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu"))
        self._cfg = self._make_cfg()
        self._cfg_handle = ops.register_env_cfg(self._cfg, owner=self)  # the torch.ops.dgppo env ops take this handle
        self._dev_cache = {}

    def _n_goals(self) -> int:
        return self._num_agents

    # ---- reference properties --------------------------------------------------------------
    @property
    def params(self) -> dict:
        return self._params

    @property
    def num_agents(self) -> int:
        return self._num_agents

    @property
    def area_size(self) -> float:
        return self._area_size

    @property
    def dt(self) -> float:
        return self._dt

    @property
    def max_episode_steps(self) -> int:
        return self._max_step

    @property
    def n_cost(self) -> int:
        return 2

    @property
    def cost_components(self) -> Tuple[str, ...]:
        return "agent collisions", "obs collisions"

    @property
    def state_dim(self) -> int:
        return 4

    @property
    def node_dim(self) -> int:
        return self.state_dim + 3

    @property
    def edge_dim(self) -> int:
        return 4

    @property
    def action_dim(self) -> int:
        return 2

    def state_lim(self, state=None):
        raise NotImplementedError

    def action_lim(self):
        return -torch.ones(self.action_dim), torch.ones(self.action_dim)

    def clip_state(self, state: torch.Tensor) -> torch.Tensor:
        lo, hi = self.state_lim(state)
        return torch.minimum(torch.maximum(state, lo.to(state)), hi.to(state))

    def clip_action(self, action: torch.Tensor) -> torch.Tensor:
        lo, hi = self.action_lim()
        return torch.minimum(torch.maximum(action, lo.to(action)), hi.to(action))

    # ---- graph geometry --------------------------------------------------------------------
    @property
    def n_obs(self) -> int:
        return int(self._params["n_obs"])

    @property
    def n_nodes(self) -> int:
        return int(self._cfg.n_nodes)

    @property
    def n_edges(self) -> int:
        return int(self._cfg.n_edges)

    @property
    def cfg(self) -> _lib.EnvCfg:
        return self._cfg

    def _obstacle_fields(self) -> int:
        return 0

    def _obstacle_rows(self) -> int:
        """Rows of the per-env obstacle buffer (env_states records the step kernels read)."""
        return max(self.n_obs, 1)

    def _make_cfg(self) -> _lib.EnvCfg:
        p = self._params
        c = _lib.EnvCfg()
        c.engine = self.ENGINE
        c.goal_mode = self.GOAL_MODE
        c.n_agents = self._num_agents
        c.n_obs = int(p["n_obs"])
        c.n_rays = int(p.get("n_rays", 0))
        c.top_k = int(p.get("top_k_rays", 0))
        c.state_dim = self.state_dim
        c.node_dim = self.node_dim
        c.dt = self._dt
        c.comm_radius = p["comm_radius"]
        c.car_radius = p["car_radius"]
        c.obs_radius = p.get("obs_radius", 0.0)
        c.area_size = self._area_size
        c.dist2goal = p["dist2goal"]
        lo, hi = p.get("obs_len_range", [0.1, 0.3])
        c.obs_len_lo, c.obs_len_hi = lo, hi
        c.obs_theta_lo, c.obs_theta_hi = self._obs_theta_range()
        # derived constants in Python float64 arithmetic, rounded once (as the reference does)
        r, cr = p["car_radius"], p["comm_radius"]
        orr = p.get("obs_radius", 0.0)
        mpe = self.ENGINE == _lib.DGPPO_ENGINE_MPE
        c.c_agent_cost = r * 2
        c.c_obs_cost = (r + orr) if mpe else r
        c.c_self_dist = cr + 1
        c.c_lidar_active = cr - 1e-1
        md = 2 * r if mpe else 2.2 * r
        c.c_min_dist = md
        c.c_inside_r = md / 2
        c.c_mpe_obs_agent = r + orr
        c.c_mpe_obs_goal = r * 2 + orr
        c.c_mpe_obs_lo = r * 3
        c.c_mpe_obs_hi = self._area_size - r * 3
        c.n_goals = self.num_goals if self.num_goals != self._num_agents else 0
        self._engine_cfg(c)
        _lib.check(_lib.load().dgppo_env_cfg_finalize(ctypes.byref(c)), "dgppo_env_cfg_finalize")
        return c

    def _engine_cfg(self, c: _lib.EnvCfg) -> None:
        """Engine-specific cfg fields (hook for subclasses), set before dgppo_env_cfg_finalize."""

    def _obs_theta_range(self):
        return 0.0, 2 * np.pi

    # ---- device constants -------------------------------------------------------------------
    def _ray_table(self, device):
        key = ("rays", str(device))
        if key not in self._dev_cache:
            self._dev_cache[key] = ray_table(int(self._params.get("n_rays", 1) or 1),
                                             float(self._params["comm_radius"])).to(device)
        return self._dev_cache[key]

    def _count_scalars(self, device):
        key = ("counts", str(device))
        if key not in self._dev_cache:  # built once: no per-step fill kernels in a captured rollout
            self._dev_cache[key] = (torch.tensor(self.n_nodes, dtype=torch.int32, device=device),
                                    torch.tensor(self.n_edges, dtype=torch.int32, device=device))
        return self._dev_cache[key]

    def node_type_row(self, device=None) -> torch.Tensor:
        device = device or self.device
        key = ("node_type", str(device))
        if key not in self._dev_cache:
            n, ng, N = self._num_agents, self.num_goals, self.n_nodes
            t = -torch.ones(N, dtype=torch.int32)
            t[:n] = self.AGENT
            t[n:n + ng] = self.GOAL
            t[n + ng:N - 1] = self.OBS
            self._dev_cache[key] = t.to(device)
        return self._dev_cache[key]

    def agent_candidates(self, device=None) -> torch.Tensor:
        """(n, C) int32: for each agent i, the edge ids of the padded layout whose receiver may be i
        (agent-agent row i, its goal edge(s), its lidar hits / obstacle edges).  The GNN kernels
        keep a candidate iff receivers[e] == i at run time (masked edges point at the pad node)."""
        device = device or self.device
        key = ("cand", str(device))
        if key not in self._dev_cache:
            n, ng = self._num_agents, self.num_goals
            spread = self.GOAL_MODE == _lib.DGPPO_GOAL_SPREAD
            n_ag = n * ng if spread else n
            mpe = self.ENGINE == _lib.DGPPO_ENGINE_MPE
            k = self.n_obs if mpe else (int(self._params.get("top_k_rays", 0)) if self.n_obs > 0 else 0)
            rows = []
            for i in range(n):
                r = [i * n + j for j in range(n)]
                r += [n * n + i * ng + j for j in range(ng)] if spread else [n * n + i]
                r += [n * n + n_ag + i * k + h for h in range(k)]
                rows.append(r)
            self._dev_cache[key] = torch.tensor(rows, dtype=torch.int32).to(device)
        return self._dev_cache[key]

    # ---- buffers ----------------------------------------------------------------------------
    def empty_graph(self, batch_shape, device=None) -> GraphsTuple:
        """Allocate an uninitialised batched graph (the kernel fills every element)."""
        device = device or self.device
        bs = tuple(batch_shape) if isinstance(batch_shape, (tuple, list)) else (int(batch_shape),)
        N, E = self.n_nodes, self.n_edges
        f32 = dict(dtype=torch.float32, device=device)
        i32 = dict(dtype=torch.int32, device=device)
        nodes = torch.empty(bs + (N, self.node_dim), **f32)
        states = torch.empty(bs + (N, self.state_dim), **f32)
        edges = torch.empty(bs + (E, self.edge_dim), **f32)
        recv = torch.empty(bs + (E,), **i32)
        send = torch.empty(bs + (E,), **i32)
        return self._assemble(nodes, edges, states, recv, send, None)

    def _assemble(self, nodes, edges, states, recv, send, obstacles) -> GraphsTuple:
        bs = tuple(nodes.shape[:-2])
        dev = nodes.device
        n_node, n_edge = self._count_scalars(dev)
        n_node, n_edge = n_node.expand(bs), n_edge.expand(bs)
        node_type = self.node_type_row(dev).expand(bs + (self.n_nodes,))
        env_states = self._env_states(states, obstacles)
        return GraphsTuple(n_node, n_edge, nodes, edges, states, recv, send, node_type, env_states)

    def _env_states(self, states, obstacles):
        raise NotImplementedError

    @staticmethod
    def _env_stride(t: torch.Tensor, inner: int) -> int:
        """Per-env element stride of t, requiring the trailing `inner` elements to be contiguous."""
        tail = 1
        for d in range(t.dim() - 1, t.dim() - 1 - inner, -1):
            if t.stride(d) != tail:
                raise ValueError("trailing dims must be contiguous")
            tail *= t.shape[d]
        return t.stride(t.dim() - 1 - inner) if t.dim() > inner else tail

    # ---- reset / step ------------------------------------------------------------------------
    def reset(self, key=0, n_env: int = 1, env_offset: int = 0, out: Optional[GraphsTuple] = None,
              obstacles_out: Optional[torch.Tensor] = None) -> GraphsTuple:
        """Batched `vmap(env.reset)`: env b samples from Philox keyed (key, env_offset + b).

        `key` is an int, or a 1-element uint64/int64 device tensor read by the kernel at run time
        (so a captured hipGraph can be replayed with fresh keys)."""
        dev = self.device if out is None else out.nodes.device
        _lib.require_gpu(dev, "env.reset")
        g = self.empty_graph((n_env,), dev) if out is None else out
        ob = obstacles_out
        if ob is None and self._obstacle_fields() > 0:
            ob = torch.empty((n_env, self._obstacle_rows(), self._obstacle_fields()), dtype=torch.float32, device=dev)
        tkey = key if isinstance(key, torch.Tensor) else None
        seed = 0 if tkey is not None else int(key) & 0xFFFFFFFFFFFFFFFF
        torch.ops.dgppo.env_reset(self._cfg_handle, tkey, seed if seed < 2 ** 63 else seed - 2 ** 64,
                                  int(env_offset), int(n_env), ob, self._ray_table(dev), g.nodes, g.edges, g.states,
                                  g.receivers, g.senders)
        return self._assemble(g.nodes, g.edges, g.states, g.receivers, g.senders, ob)

    def reset_states(self, key, n_env: int, env_offset: int = 0, out: Optional[GraphsTuple] = None,
                     obstacles_out: Optional[torch.Tensor] = None) -> GraphsTuple:
        """The sampling half of `reset` (torch.ops.dgppo.env_reset_states): obstacles and the agent / goal
        state rows only; `rollout_into(..., rebuild_first=True)` builds graph 0 from them.  Configs
        without the persistent rollout kernel get the full reset."""
        dev = self.device if out is None else out.nodes.device
        _lib.require_gpu(dev, "env.reset_states")
        g = self.empty_graph((n_env,), dev) if out is None else out
        ob = obstacles_out
        if ob is None and self._obstacle_fields() > 0:
            ob = torch.empty((n_env, self._obstacle_rows(), self._obstacle_fields()), dtype=torch.float32, device=dev)
        tkey = key if isinstance(key, torch.Tensor) else None
        seed = 0 if tkey is not None else int(key) & 0xFFFFFFFFFFFFFFFF
        torch.ops.dgppo.env_reset_states(self._cfg_handle, tkey, seed if seed < 2 ** 63 else seed - 2 ** 64,
                                         int(env_offset), int(n_env), ob, self._ray_table(dev), g.nodes, g.edges,
                                         g.states, g.receivers, g.senders)
        return self._assemble(g.nodes, g.edges, g.states, g.receivers, g.senders, ob)

    def rollout_into(self, buf: GraphsTuple, obstacles: Optional[torch.Tensor], actions: torch.Tensor,
                     rewards: torch.Tensor, costs: torch.Tensor, rebuild_first: bool = False, reset_key=None,
                     env_offset: int = 0) -> None:
        """T env steps with the given actions (T, B, n, A) in one call (torch.ops.dgppo.env_rollout): buf is
        a time-major (T+1, B, ...) graph buffer, step t reads buf[t] and writes buf[t+1], rewards[t],
        costs[t] -- the env half of the reference's rollout scan (trainer/utils.py:45-55).
        reset_key (an int, or a 1-element int64 device tensor read at run time): the call first resets the envs as
        `reset_states(reset_key, env_offset=env_offset)` + rebuild_first would -- `obstacles` receives the records
        -- inside the same launch where the persistent Lidar kernel runs."""
        _lib.require_gpu(buf.states.device, "env.rollout")
        n, A = self._num_agents, self.action_dim
        T = actions.shape[0]
        if actions.shape[-2:] != (n, A) or buf.states.shape[0] != T + 1 or buf.states.dim() != 4:
            raise ValueError("rollout_into: actions (T, B, n, A) and a (T+1, B, N, sd) graph buffer")
        tkey = reset_key if isinstance(reset_key, torch.Tensor) else None
        seed = 0 if tkey is not None or reset_key is None else int(reset_key) & 0xFFFFFFFFFFFFFFFF
        torch.ops.dgppo.env_rollout(self._cfg_handle, bool(rebuild_first), obstacles, actions,
                                    self._ray_table(buf.states.device), buf.nodes, buf.edges, buf.states,
                                    buf.receivers, buf.senders, rewards, costs, reset_key is not None, tkey,
                                    seed if seed < 2 ** 63 else seed - 2 ** 64, int(env_offset))

    def step_into(self, graph: GraphsTuple, action: torch.Tensor, out: GraphsTuple,
                  reward: torch.Tensor, cost: torch.Tensor) -> GraphsTuple:
        """One fused HIP step (torch.ops.dgppo.env_step) writing into caller-owned buffers (views into a
        rollout buffer)."""
        _lib.require_gpu(graph.states.device, "env.step")
        if graph.states.dim() != 3:
            raise ValueError("step expects one leading env axis: states (B, N, state_dim)")
        B = graph.states.shape[0]
        n = self._num_agents
        if action.shape[-2:] != (n, self.action_dim):
            raise ValueError(f"action must be (B, {n}, {self.action_dim}), got {tuple(action.shape)}")
        if graph.states.shape[-2:] != (self.n_nodes, self.state_dim):
            raise ValueError("graph does not match this env's layout")
        if action.dtype != torch.float32:
            action = action.float()
        A = self.action_dim
        action = action if action.stride(-1) == 1 and action.stride(-2) == A else action.contiguous()
        ob = self._obstacles_of(graph)
        torch.ops.dgppo.env_step(self._cfg_handle, graph.states, ob, action, self._ray_table(graph.states.device),
                                 out.nodes, out.edges, out.states, out.receivers, out.senders, reward, cost)
        return self._assemble(out.nodes, out.edges, out.states, out.receivers, out.senders, ob)

    # ---- graphs of caller-given states ------------------------------------------------------------
    def _third_name(self) -> str:
        return "obstacle" if self._obstacle_fields() > 0 else "obs"

    def state_rows(self, state, what: str = "get_graph: state", third_optional: bool = False):
        """Check an env state tuple's shapes and return (agent (B, n, sd), goal (B, n_goal_rows, sd), third, B), third
        = the (B, O, F) obstacle tensor the graph kernel reads (None when n_obs == 0): the Lidar records (F = 16; a
        Rectangle or its packed tensor) or the MPE obstacle states (F = 4).  A mismatch raises a ValueError naming the
        field as `what`.<field>.  third_optional: a missing / None third passes as None (sensor-only states)."""
        if not isinstance(state, tuple) or len(state) < 2:
            raise ValueError(f"{what} must be the env's (agent, goal, {self._third_name()}) state tuple")
        agent, goal = state[0], state[1]
        n, sd = self._num_agents, self.state_dim
        for name, t, rows in (("agent", agent, n), ("goal", goal, self.num_goals)):
            if not isinstance(t, torch.Tensor) or t.dim() != 3 or tuple(t.shape[1:]) != (rows, sd):
                got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"{what}.{name} must be (B, {rows}, {sd}), got {got}")
        B = int(agent.shape[0])
        if goal.shape[0] != B:
            raise ValueError(f"{what}.goal must be ({B}, {self.num_goals}, {sd}), got {tuple(goal.shape)}")
        third = None
        if self.n_obs > 0:
            third = state[2] if len(state) > 2 else None
            third = getattr(third, "packed", third)
            if third is None and third_optional:
                return agent, goal, None, B
            fields = self._obstacle_fields() or sd
            if not isinstance(third, torch.Tensor) or tuple(third.shape) != (B, self.n_obs, fields):
                got = tuple(third.shape) if isinstance(third, torch.Tensor) else type(third).__name__
                raise ValueError(f"{what}.{self._third_name()} must be ({B}, {self.n_obs}, {fields}), got {got}")
        return agent, goal, third, B

    def get_graph(self, state, out: Optional[GraphsTuple] = None, *, lidar_data: Optional[torch.Tensor] = None
                  ) -> GraphsTuple:
        """Batched `vmap(env.get_graph)` with get_lidar_data (dgppo/env/base.py:137, lidar_env/base.py:227-271,
        mpe/base.py:211-241): the graph of the caller's own state, one HIP launch (torch.ops.dgppo.env_get_graph).

        `state` is this env's state tuple with one leading env axis: (agent (B, n, sd), goal (B, n_goal_rows, sd),
        obstacle), the obstacle a Rectangle / packed (B, O, 16) tensor (Lidar), the (B, O, 4) obstacle states (MPE),
        or None when n_obs == 0.  `graph.env_states` of any graph of this env is a valid argument.  Nothing is
        clipped.  The returned graph carries the obstacles, so `env.step(env.get_graph(s), a)` works.

        lidar_data (B, n, top_k, 2), Lidar envs only: the graph is built from these hit points instead of a ray cast
        (the reference's get_graph(state, lidar_data); torch.ops.dgppo.env_get_graph_hits).  The state's obstacle may
        then be None (a sensor-only graph: `env.step` on it raises) or given (carried on the graph for `step`)."""
        if lidar_data is not None:
            return self._get_graph_hits(state, out, lidar_data)
        agent, goal, third, B = self.state_rows(state)
        dev = agent.device if out is None else out.nodes.device
        _lib.require_gpu(dev, "env.get_graph")
        _lib.require_gpu(agent.device, "env.get_graph")

        def rows_of(name, t):  # fp32 on the graph's device, rows contiguous (views of a graph's states pass as they are)
            if t.device != dev:
                raise ValueError(f"get_graph: state.{name} is on {t.device}, the graph on {dev}")
            t = t if t.dtype == torch.float32 else t.float()
            return t if t.stride(-1) == 1 and t.stride(-2) == t.shape[-1] else t.contiguous()

        agent, goal = rows_of("agent", agent), rows_of("goal", goal)
        if third is not None:
            third = rows_of(self._third_name(), third)
        g = self.empty_graph((B,), dev) if out is None else out
        if g.states.dim() != 3 or g.states.shape[0] != B:
            raise ValueError(f"get_graph: out must hold {B} graphs")
        torch.ops.dgppo.env_get_graph(self._cfg_handle, agent, goal, third, self._ray_table(dev), g.nodes, g.edges,
                                      g.states, g.receivers, g.senders)
        return self._assemble(g.nodes, g.edges, g.states, g.receivers, g.senders,
                              third if self._obstacle_fields() > 0 else None)

    def get_lidar_data(self, agent_states: torch.Tensor, obstacles) -> torch.Tensor:
        """Batched get_lidar_data (lidar_env/base.py:126-140): (B, n, top_k, 2) hit points of the agents at
        `agent_states` (B, n, sd) among `obstacles` -- the hit rows of that state's graph."""
        if self._obstacle_fields() == 0 or self.n_obs == 0:
            raise ValueError("get_lidar_data: this env has no LiDAR")
        if not isinstance(agent_states, torch.Tensor) or agent_states.dim() != 3:
            raise ValueError(f"get_lidar_data: agent_states must be (B, {self._num_agents}, {self.state_dim})")
        n, ng, k = self._num_agents, self.num_goals, int(self._params["top_k_rays"])
        goal = agent_states.new_zeros((agent_states.shape[0], ng, self.state_dim))
        g = self.get_graph((agent_states, goal, obstacles))
        return g.states[:, n + ng:n + ng + n * k, :2].reshape(-1, n, k, 2)

    # ---- sensor in the loop: scan | hits | graph from hits ------------------------------------------
    def _require_lidar(self, what: str) -> None:
        if self.ENGINE in self._VMAS_ENGINES:
            raise NotImplementedError(f"{what}: the VMAS envs have no LiDAR sensor model")
        if self._obstacle_fields() == 0 or self.n_obs == 0:
            raise ValueError(f"{what}: this env has no LiDAR")

    @staticmethod
    def _sensor_arg(what: str, name: str, t, shape, dev=None) -> torch.Tensor:
        """A float32 tensor of exactly `shape` (on `dev` when given) with contiguous rows, else a ValueError naming it."""
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape):
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"{what}: {name} must be {tuple(shape)}, got {got}")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: {name} must be float32, got {t.dtype}")
        if dev is not None and t.device != dev:
            raise ValueError(f"{what}: {name} is on {t.device}, expected {dev}")
        tail = 1  # the per-env stride is free (views of a rollout buffer); the dims behind it must be contiguous
        for d in range(t.dim() - 1, 0, -1):
            if t.stride(d) != tail:
                return t.contiguous()
            tail *= t.shape[d]
        return t

    def _sensor_agents(self, what: str, agent_states) -> torch.Tensor:
        if not isinstance(agent_states, torch.Tensor) or agent_states.dim() != 3:
            got = tuple(agent_states.shape) if isinstance(agent_states, torch.Tensor) else type(agent_states).__name__
            raise ValueError(f"{what}: agent_states must be (B, {self._num_agents}, {self.state_dim}), got {got}")
        B = int(agent_states.shape[0])
        return self._sensor_arg(what, "agent_states", agent_states, (B, self._num_agents, self.state_dim))

    def lidar_scan(self, agent_states: torch.Tensor, obstacles, bodies: bool = False) -> torch.Tensor:
        """The raw scan (torch.ops.dgppo.lidar_scan): alpha (B, n, R) of the agents at `agent_states` (B, n, sd)
        among `obstacles` (a Rectangle or its packed (B, O, 16) tensor): per beam the fraction of the sensing range
        to the nearest obstacle edge, 1e6 where nothing is hit, 0 for an agent inside an obstacle -- the values
        get_lidar_data ranks (env/utils.py:115-130).  `lidar_hits(agent_states, alpha)` turns them (or an edited
        copy: utils/sensor.py) into hit points.

        bodies: the beams also return off the other agents' bodies, discs of radius car_radius
        (torch.ops.dgppo.lidar_scan_bodies): per beam the nearer of the obstacle and the body return, 0 where the
        discs overlap; a NaN or infinite row returns nothing, an obstacle NaN propagates.  False takes exactly the
        path without it.  The env's own step, reward and cost never see bodies."""
        from ..utils.sensor import bodies_option

        what = "lidar_scan"
        self._require_lidar(what)
        op = torch.ops.dgppo.lidar_scan_bodies if bodies_option(self, what, bodies) else torch.ops.dgppo.lidar_scan
        agent = self._sensor_agents(what, agent_states)
        B = int(agent.shape[0])
        ob = self._sensor_arg(what, "obstacles", getattr(obstacles, "packed", obstacles),
                              (B, self.n_obs, self._obstacle_fields()), agent.device)
        _lib.require_gpu(agent.device, "env.lidar_scan")
        alpha = torch.empty((B, self._num_agents, int(self._params["n_rays"])), dtype=torch.float32,
                            device=agent.device)
        op(self._cfg_handle, agent, ob, self._ray_table(agent.device), alpha)
        return alpha

    def lidar_hits(self, agent_states: torch.Tensor, alpha: torch.Tensor) -> torch.Tensor:
        """Scan to hit points (torch.ops.dgppo.lidar_hits): (B, n, top_k, 2), the top_k smallest of `alpha` (B, n, R)
        per agent in the reference's order (stable argsort, NaN last), each the point start + ray * alpha.
        `lidar_hits(a, lidar_scan(a, ob))` is `get_lidar_data(a, ob)` bit for bit."""
        what = "lidar_hits"
        self._require_lidar(what)
        agent = self._sensor_agents(what, agent_states)
        B, n = int(agent.shape[0]), self._num_agents
        alpha = self._sensor_arg(what, "alpha", alpha, (B, n, int(self._params["n_rays"])), agent.device)
        _lib.require_gpu(agent.device, "env.lidar_hits")
        hits = torch.empty((B, n, int(self._params["top_k_rays"]), 2), dtype=torch.float32, device=agent.device)
        torch.ops.dgppo.lidar_hits(self._cfg_handle, agent, alpha, self._ray_table(agent.device), hits)
        return hits

    def line_of_sight(self, agent_states: torch.Tensor, obstacles) -> torch.Tensor:
        """Which agents see each other past the obstacles (torch.ops.dgppo.lidar_sight): bool (B, n, n), entry
        [b, i, j] False where an edge of some obstacle cuts the segment from agent i to agent j of env b, by the scan's
        per-edge arithmetic (Rectangle.raytracing's alpha and beta both in [0, 1]).  The diagonal is True, coincident
        agents see each other, agents do not occlude.  `utils.sensor.mask_unseen(graph, visible)` applies it to a
        graph; `observe(..., occlusion=True)` does both in its one launch."""
        what = "line_of_sight"
        self._require_lidar(what)
        agent = self._sensor_agents(what, agent_states)
        B, n = int(agent.shape[0]), self._num_agents
        ob = self._sensor_arg(what, "obstacles", getattr(obstacles, "packed", obstacles),
                              (B, self.n_obs, self._obstacle_fields()), agent.device)
        _lib.require_gpu(agent.device, "env.line_of_sight")
        visible = torch.empty((B, n, n), dtype=torch.uint8, device=agent.device)
        torch.ops.dgppo.lidar_sight(self._cfg_handle, agent, ob, visible)
        return visible.view(torch.bool)

    def field_of_view(self, agent_states: torch.Tensor, half_angle_deg: float) -> torch.Tensor:
        """Which agents lie in each other's camera cone (torch.ops.dgppo.agent_fov): bool (B, n, n), entry [b, i, j]
        True where agent j of env b is inside the forward cone of half angle `half_angle_deg` (0 < deg <= 180) around
        agent i's heading (columns 2, 3 of its row, used as given), by the FoV cost's own fp32 arithmetic: at
        `params["fov_angle_deg"]`, `[b, i, i + 1] == (cost[b, i, 2] < 0)` of LidarOmniTarget bit for bit.  The diagonal
        is True, a NaN row sees no one and is seen by no one, coincident agents see each other exactly when the cone's
        cosine is <= 0 (the formula's quirk), and there is no range test.  Only the envs with a heading; no obstacles
        are needed.  `utils.sensor.mask_unseen(graph, in_fov)` applies it to a graph; `observe(..., fov=deg)` does both
        in its one launch."""
        from ..utils.sensor import cone_angle

        what = "field_of_view"
        cone_angle(self, what, float("nan") if half_angle_deg is None else half_angle_deg)  # the env, then the domain
        agent = self._sensor_agents(what, agent_states)
        B, n = int(agent.shape[0]), self._num_agents
        _lib.require_gpu(agent.device, "env.field_of_view")
        in_fov = torch.empty((B, n, n), dtype=torch.uint8, device=agent.device)
        torch.ops.dgppo.agent_fov(self._cfg_handle, agent, float(half_angle_deg), in_fov)
        return in_fov.view(torch.bool)

    def _get_graph_hits(self, state, out: Optional[GraphsTuple], lidar_data) -> GraphsTuple:
        what = "get_graph"
        self._require_lidar(what + ": lidar_data")
        agent, goal, third, B = self.state_rows(state, third_optional=True)
        dev = agent.device if out is None else out.nodes.device
        n, sd = self._num_agents, self.state_dim
        agent = self._sensor_arg(what, "state.agent", agent, (B, n, sd), dev)
        goal = self._sensor_arg(what, "state.goal", goal, (B, self.num_goals, sd), dev)
        hits = self._sensor_arg(what, "lidar_data", lidar_data, (B, n, int(self._params["top_k_rays"]), 2), dev)
        if third is not None:  # not read here: carried on the graph for step
            third = self._sensor_arg(what, "state.obstacle", third, (B, self.n_obs, self._obstacle_fields()), dev)
        _lib.require_gpu(dev, "env.get_graph")
        g = self.empty_graph((B,), dev) if out is None else out
        if g.states.dim() != 3 or g.states.shape[0] != B:
            raise ValueError(f"get_graph: out must hold {B} graphs")
        torch.ops.dgppo.env_get_graph_hits(self._cfg_handle, agent, goal, hits, g.nodes, g.edges, g.states,
                                           g.receivers, g.senders)
        return self._assemble(g.nodes, g.edges, g.states, g.receivers, g.senders, third)

    def observe(self, state, t: int, *, sigma: float, dropout: float, seed, env_offset: int = 0,
                out: Optional[GraphsTuple] = None, occlusion: bool = False, fov=None,
                bodies: bool = False) -> GraphsTuple:
        """The OBSERVED graph of the true `state` (get_graph's tuple, obstacles required) at step `t` under the
        range-noise / beam-dropout sensor model of utils/sensor.py, in one HIP launch (torch.ops.dgppo.lidar_observe):
        bit for bit `get_graph(state, lidar_data=lidar_hits(agent, LidarNoise(sigma, dropout, seed,
        sense_range=comm_radius)(lidar_scan(agent, obstacle), t)))`, with env b's draws taken at row env_offset + b of
        the noise streams (ranks of a multi-GPU run pass rank * n_env).  seed: an int, or a 1-element int64 device
        tensor read at run time (replays of a captured rollout draw new noise).  sigma = dropout = 0 is the true
        graph.  `out` may be the graph whose env_states are `state`.  LidarLine runs the chained launches instead of
        the fused kernel (same results).

        occlusion: obstacles also hide agents from each other -- every agent-agent edge whose receiver has no line of
        sight to its sender goes to the pad node, `mask_unseen(observe(...), line_of_sight(agent, obstacle))` bit for
        bit, in the same launch (torch.ops.dgppo.lidar_observe_los).  False takes exactly the path without it.

        fov: a half angle in degrees (LidarBicycleTarget and LidarOmniTarget only) -- every agent-agent edge whose sender
        is outside the receiver's forward cone goes to the pad node as well, `mask_unseen(observe(...),
        field_of_view(agent, fov) [& line_of_sight(agent, obstacle)])` bit for bit, in the same launch
        (torch.ops.dgppo.lidar_observe_fov).  The beams stay omnidirectional.  None and 180 take exactly the paths
        without it.

        bodies: the beams also return off the other agents' bodies -- `lidar_scan(agent, obstacle, bodies=True)` in
        place of the scan above, in the same launch (torch.ops.dgppo.lidar_observe_bodies): a neighbour whose edge is
        hidden or out of range still shows up as an anonymous hit row.  False takes exactly the paths without it."""
        from ..utils.sensor import Sensing, bodies_option, drop_below

        what = "observe"
        sensing = Sensing.of(self, what, sigma, dropout, occlusion, fov)  # checks the env and all four options
        bodies = bodies_option(self, what, bodies)
        sigma, dropout, fov = sensing.sigma, sensing.dropout, sensing.fov
        sense_range = float(self._params["comm_radius"])
        t, env_offset = int(t), int(env_offset)
        if t < 0 or env_offset < 0:
            raise ValueError(f"observe: t and env_offset must be >= 0, got {t} and {env_offset}")
        agent, goal, third, B = self.state_rows(state, what + ": state")
        dev = agent.device if out is None else out.nodes.device
        n, sd = self._num_agents, self.state_dim
        agent = self._sensor_arg(what, "state.agent", agent, (B, n, sd), dev)
        goal = self._sensor_arg(what, "state.goal", goal, (B, self.num_goals, sd), dev)
        third = self._sensor_arg(what, "state.obstacle", third, (B, self.n_obs, self._obstacle_fields()), dev)
        tkey = seed if isinstance(seed, torch.Tensor) else None
        if tkey is not None and (tkey.device != dev or tkey.numel() != 1 or tkey.dtype != torch.int64):
            raise ValueError("observe: a tensor seed must be a 1-element int64 tensor on the env's device")
        _lib.require_gpu(dev, "env.observe")
        g = self.empty_graph((B,), dev) if out is None else out
        if g.states.dim() != 3 or g.states.shape[0] != B:
            raise ValueError(f"observe: out must hold {B} graphs")
        if self.cfg.variant != _lib.DGPPO_VARIANT_NONE:
            model = sensing.model(sense_range)
            if not occlusion:
                return self._observe_chained(model, agent, goal, third, t, seed, env_offset, g, bodies)
            from ..utils.sensor import mask_unseen

            visible = self.line_of_sight(agent, third)  # before the graph is written: `out` may alias the state
            return mask_unseen(self._observe_chained(model, agent, goal, third, t, seed, env_offset, g, bodies), visible)
        iseed = 0 if tkey is not None else int(seed) & 0xFFFFFFFFFFFFFFFF
        flags = (_lib.OBSERVE_NOISE if sigma > 0.0 else 0) | (_lib.OBSERVE_DROPOUT if dropout > 0.0 else 0)
        op = torch.ops.dgppo.lidar_observe
        if occlusion:
            op, flags = torch.ops.dgppo.lidar_observe_los, flags | _lib.OBSERVE_SIGHT
        head = (self._cfg_handle, agent, goal, third, self._ray_table(dev), tkey,
                iseed if iseed < 2 ** 63 else iseed - 2 ** 64, env_offset, t, sigma / sense_range,
                drop_below(dropout))
        if bodies:
            flags |= _lib.OBSERVE_BODIES | (_lib.OBSERVE_FOV if fov is not None else 0)
            torch.ops.dgppo.lidar_observe_bodies(*head, flags, 180.0 if fov is None else fov, g.nodes, g.edges, g.states,
                                                 g.receivers, g.senders)
        elif fov is not None:  # the heading envs have no variant: always the fused kernel
            torch.ops.dgppo.lidar_observe_fov(*head, flags | _lib.OBSERVE_FOV, fov, g.nodes, g.edges, g.states,
                                              g.receivers, g.senders)
        else:
            op(*head, flags, g.nodes, g.edges, g.states, g.receivers, g.senders)
        return self._assemble(g.nodes, g.edges, g.states, g.receivers, g.senders, third)

    def _observe_chained(self, model, agent, goal, third, t, seed, env_offset, g, bodies: bool = False) -> GraphsTuple:
        """observe by the three launches with LidarNoise's arithmetic between them (the variant envs)."""
        from ..nn import kernels as K
        from ..utils.sensor import NO_RETURN

        alpha = self.lidar_scan(agent, third, bodies=True) if bodies else self.lidar_scan(agent, third)
        B = alpha.shape[0]
        seen = alpha
        if model.sigma > 0.0 or model.dropout > 0.0:
            kw = dict(seed_tensor=seed) if isinstance(seed, torch.Tensor) else dict(seed=int(seed))
            z = torch.empty((env_offset + B,) + tuple(alpha.shape[1:]), dtype=torch.float32, device=alpha.device)
            if model.sigma > 0.0:
                K.normal_(z, stream_id=model.STREAM_BASE + 2 * t, **kw)
                noisy = torch.clamp_min(alpha + z[env_offset:] * (model.sigma / model.sense_range), 0.0)
                seen = torch.where(alpha <= 1.0, noisy, alpha)
            if model.dropout > 0.0:
                K.normal_(z, stream_id=model.STREAM_BASE + 2 * t + 1, **kw)
                drop = (z[env_offset:] < model._drop_below) & ~torch.isnan(alpha)
                seen = torch.where(drop, torch.full_like(alpha, NO_RETURN), seen)
        return self._get_graph_hits((agent, goal, third), g, self.lidar_hits(agent, seen))

    def get_reward(self, graph: GraphsTuple, action: torch.Tensor) -> torch.Tensor:
        """Reward (B,) of taking `action` in `graph` (lidar_spread.py:35-52, ...): the step kernel evaluates it."""
        return self.step(graph, action).reward

    def _obstacles_of(self, graph: GraphsTuple) -> Optional[torch.Tensor]:
        return None

    def step(self, graph: GraphsTuple, action: torch.Tensor, get_eval_info: bool = False) -> StepResult:
        """Batched `vmap(env.step)` (lidar_env/base.py:151-174, mpe/base.py:137-158)."""
        B = graph.states.shape[:-2]
        out = self.empty_graph(B, graph.states.device)
        reward = torch.empty(B, dtype=torch.float32, device=graph.states.device)
        cost = torch.empty(B + (self._num_agents, self.n_cost), dtype=torch.float32, device=graph.states.device)
        g = self.step_into(graph, action, out, reward, cost)
        done = torch.zeros(B, dtype=torch.bool, device=graph.states.device)
        return StepResult(g, reward, cost, done, {})

    # ---- rendering -----------------------------------------------------------------------------------
    _VMAS_ENGINES = (_lib.DGPPO_ENGINE_VMAS_WHEEL, _lib.DGPPO_ENGINE_VMAS_TRANSPORT)

    def render_frames(self, graph: GraphsTuple, size: Optional[int] = None, dpi: int = 100,
                      viz_opts: Optional[dict] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The scene of every graph of `graph` (batch shape (B,) or (B, T), e.g. the strided `rollout.graph` view) as a
        uint8 RGBA image (*batch, S, S, 4) on the graph's device, S = size or 10 * dpi (the reference's 10 in figure):
        one HIP launch over (frame, pixel tile) (torch.ops.dgppo.render_frames; DESIGN.md "Rendering" has the pixel
        rule and the layers).  viz_opts={"fov": False} leaves out the FoV wedges LidarOmniTarget draws by default.
        `out` reuses a contiguous uint8 buffer of that shape.  There is no host path: a CPU graph raises.
        viz_opts={"field": FieldLayer} (utils/field.py) draws a scalar field per frame -- hard-edged colour bands and a
        black zero line -- under every other layer (torch.ops.dgppo.render_frames_field): this project's door to the
        picture the reference draws for viz_opts["cbf"] / ["Vh"], keys that stay unbuilt here."""
        viz_opts = viz_opts or {}
        for key in ("cbf", "Vh"):
            if key in viz_opts:
                raise NotImplementedError(f"viz_opts[{key!r}] (the reference's contour overlay): not built")
        _lib.require_gpu(graph.states.device, "env.render_frames")
        states, recv, send = graph.states, graph.receivers, graph.senders
        bs, out = self._frame_buffer(states, size, dpi, out)
        ob = self._obstacles_of(graph) if self._obstacle_fields() > 0 else None
        if ob is not None and len(bs) == 2:  # one obstacle set per episode: the (B, T) views expand it over T
            if ob.shape[1] > 1 and ob.stride(1) != 0:
                raise ValueError("render_frames: a (B, T) graph needs one obstacle set per episode")
            ob = ob[:, 0]
        flags = _lib.RENDER_FOV if viz_opts.get("fov", True) else 0
        field = viz_opts.get("field")
        if field is None:
            torch.ops.dgppo.render_frames(self._cfg_handle, states, recv, send, ob, out, flags)
            return out
        from ..utils.field import FIELD_ALPHA, FieldLayer, palette_tensor

        if not isinstance(field, FieldLayer):
            raise ValueError(f"render_frames: viz_opts['field'] must be a FieldLayer, got {type(field).__name__}")
        if tuple(field.values.shape[:-2]) != bs or field.values.device != states.device:
            raise ValueError(f"render_frames: the field's values must be {bs + ('Gy', 'Gx')} on {states.device}, got "
                             f"{tuple(field.values.shape)} on {field.values.device}")
        torch.ops.dgppo.render_frames_field(self._cfg_handle, states, recv, send, ob, field.values,
                                            palette_tensor(field.bands, states.device), list(field.extent),
                                            field.half_range, FIELD_ALPHA, self._area_size / 480.0, out, flags)
        return out

    def _frame_buffer(self, states: torch.Tensor, size: Optional[int], dpi: int, out: Optional[torch.Tensor]):
        """(batch shape, the uint8 (*batch, S, S, 4) image stack) of a render_frames call: `out`, checked, or new."""
        bs = tuple(states.shape[:-2])
        if len(bs) not in (1, 2) or tuple(states.shape[-2:]) != (self.n_nodes, self.state_dim):
            raise ValueError("render_frames: graph must have batch shape (B,) or (B, T) and this env's layout")
        S = int(size) if size else 10 * int(dpi)
        if S < 1:
            raise ValueError(f"render_frames: image size must be >= 1, got {S}")
        shape = bs + (S, S, 4)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=states.device)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != states.device:
            raise ValueError(f"render_frames: out must be a uint8 {shape} tensor on {states.device}")
        return bs, out

    def render_video(self, rollout, video_path, Ta_is_unsafe=None, viz_opts: Optional[dict] = None, dpi: int = 100,
                     episode: int = 0, max_frame_bytes: int = 1 << 30) -> str:
        """The reference's render_video (dgppo/env/base.py:141, plot.py render_lidar / render_mpe) for episode
        `episode` of a batched Rollout: the T frames of rollout.graph[episode] are rasterised on the GPU
        (render_frames, in chunks whose device buffer stays within max_frame_bytes) and copied to the host, where
        Pillow draws the header band above the scene (per-component max cost, reward, unsafe agents, kk) and the
        agent indices and encodes an animated GIF at 30 fps.  A `.mp4` suffix is rewritten to `.gif` (no ffmpeg);
        the path written is returned.  Ta_is_unsafe: (T, n) booleans (test.py: any(cost >= 0)).
        viz_opts={"field": FieldLayer} with values (T, Gy, Gx) draws that field under every frame's scene, one
        half_range for the whole episode, and writes its label centred in the header."""
        import pathlib

        try:
            from PIL import Image, ImageDraw, ImageFont
        except ImportError as e:
            raise ImportError("render_video needs Pillow for the text and the GIF; env.render_frames returns the "
                              "frames without it") from e
        g = rollout.graph
        if g.states.dim() != 4 or g.states.shape[1] < 1:
            raise ValueError("render_video: rollout.graph must have batch shape (B, T) with T >= 1")
        T, n, S = int(g.states.shape[1]), self._num_agents, 10 * int(dpi)
        band = S // 8
        per = max(1, int(max_frame_bytes) // (S * S * 4))
        ob = self._obstacles_of(g) if self._obstacle_fields() > 0 else None
        costs = rollout.costs[episode].amax(dim=1).double().cpu().numpy()  # (T, n_cost) max over agents
        rewards = rollout.rewards[episode].double().cpu().numpy()
        pos = g.states[episode, :, :n, :2].double().cpu().numpy()  # (T, n, 2)
        unsafe = None if Ta_is_unsafe is None else np.asarray(
            Ta_is_unsafe.cpu() if isinstance(Ta_is_unsafe, torch.Tensor) else Ta_is_unsafe).astype(bool)
        px = max(6, band // (self._header_line_count() + 1))
        frames, h = [], self._area_size / S
        lpx = max(px, int(1.4 * float(self._params.get("car_radius", 0.05)) / h))  # labels: about the agent's radius
        try:
            font, label_font = ImageFont.load_default(size=px), ImageFont.load_default(size=lpx)
        except (TypeError, OSError):  # a Pillow without the scalable default font
            font = label_font = ImageFont.load_default()
            lpx = px
        host = self._header_host(g, episode)
        field = (viz_opts or {}).get("field")
        if field is not None and (not hasattr(field, "sliced") or tuple(field.values.shape[:-2]) != (T,)):
            raise ValueError(f"render_video: viz_opts['field'] must be a FieldLayer with values ({T}, Gy, Gx)")
        for t0 in range(0, T, per):
            t1 = min(T, t0 + per)
            if field is not None:
                viz_opts = dict(viz_opts, field=field.sliced(slice(t0, t1)))
            sub = self._assemble(g.nodes[episode, t0:t1], g.edges[episode, t0:t1], g.states[episode, t0:t1],
                                 g.receivers[episode, t0:t1], g.senders[episode, t0:t1],
                                 None if ob is None else ob[episode, t0:t1])
            rgb = self.render_frames(sub, size=S, viz_opts=viz_opts)[..., :3].cpu().numpy()
            for t in range(t0, t1):
                im = Image.new("RGB", (S, S + band), "white")
                im.paste(Image.fromarray(rgb[t - t0], "RGB"), (0, band))
                d = ImageDraw.Draw(im)
                left, right = self._header_text(host, t, costs[t], rewards[t])
                if left:
                    d.multiline_text((S // 50, 0), left, fill="black", font=font, spacing=0)
                if unsafe is not None and t < len(unsafe):
                    right = right + ["Unsafe: [" + " ".join(str(i) for i in np.where(unsafe[t])[0]) + "]"]  # one line
                for i, s in enumerate(right):
                    d.text((S - S // 100 - d.textlength(s, font=font), i * px), s, fill="black", font=font)
                if field is not None and field.label:
                    d.text(((S - d.textlength(field.label, font=font)) / 2, 0), field.label, fill="black", font=font)
                for i in range(n if self._labels_agents else 0):
                    x, y = pos[t, i]
                    if np.isfinite(x) and np.isfinite(y) and 0 <= x <= self._area_size and 0 <= y <= self._area_size:
                        d.text((x / h - d.textlength(str(i), font=label_font) / 2, band + S - y / h - 0.6 * lpx), str(i),
                               fill="black", font=label_font)
                frames.append(im.convert("P", palette=Image.Palette.ADAPTIVE, colors=64))
        path = pathlib.Path(video_path)
        if path.suffix.lower() != ".gif":
            path = path.with_suffix(".gif")
        path.parent.mkdir(parents=True, exist_ok=True)
        frames[0].save(path, save_all=True, append_images=frames[1:], duration=1000 // 30, loop=0, optimize=False)
        return str(path)

    _labels_agents = True  # render_video writes each agent's index at its centre

    def _header_line_count(self) -> int:
        """Text lines the header band of render_video has room for."""
        return 2 + len(self.cost_components)

    def _header_host(self, graph: GraphsTuple, episode: int):
        """Host copies of what _header_text reads beyond costs and rewards (taken once per video)."""
        return None

    def _header_text(self, host, t: int, costs_t, reward_t):
        """Frame t's header of render_video: (the left block, the right-aligned lines top to bottom)."""
        left = "Cost:\n" + "\n".join(f"    {nm}: {costs_t[i]:5.4f}" for i, nm in enumerate(self.cost_components))
        return left + f"\nReward: {reward_t:5.4f}", [f"kk={t:04}"]

    def get_cost(self, graph: GraphsTuple) -> torch.Tensor:
        """Cost of a graph (lidar_env/base.py:180-207): the step kernel evaluates it on its input."""
        zero = torch.zeros(graph.states.shape[:-2] + (self._num_agents, self.action_dim), device=graph.states.device)
        return self.step(graph, zero).cost


def ray_table(n_rays: int, sense_range: float) -> torch.Tensor:
    """(R, 2) per-ray end offsets (cos th * range, sin th * range) with th = jnp.linspace(-pi,
    pi - 2pi/R, R) (env/utils.py:51-55), computed by dgppo_ray_table in the native library."""
    out = torch.empty((n_rays, 2), dtype=torch.float32)
    _lib.check(_lib.load().dgppo_ray_table(int(n_rays), float(sense_range), ctypes.c_void_p(out.data_ptr())),
               "dgppo_ray_table")
    return out
