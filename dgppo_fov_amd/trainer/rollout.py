"""Device-resident rollout driver: the reference's `rollout` / `test_rollout`
(dgppo/trainer/utils.py:22-86: reset, then lax.scan of (actor, env.step) over T steps) as a fixed
sequence of HIP launches over preallocated TIME-MAJOR HBM buffers, optionally captured once into
a hipGraph and replayed (one host call per episode instead of ~25T launches).

Buffers are time-major, (T+1, B, ...), so the graph of step t is one contiguous (B, ...) block
that the env-step and GNN kernels read and write without copies; the Rollout handed to the
algorithm exposes the reference's (B, T, ...) leading dims as permuted views.

Actor carry semantics follow the reference exactly:
  stochastic `rollout`   rnn_states[t] = carry BEFORE acting on graph t (utils.py:186-192)
  deterministic `test_rollout` rnn_states[t] = carry AFTER acting on graph t (utils.py:211-218)
"""
from __future__ import annotations

from typing import Optional

import ctypes

import torch

from .. import _lib
from ..env.base import MultiAgentEnv
from ..nn import kernels as K
from ..nn.layers import GraphBatch
from ..utils.graph import GraphsTuple
from ..utils.sensor import Sensing, bodies_option, mask_unseen
from .data import Rollout


MAX_ENV_ROWS = 1 << 30  # env rows (env_offset + env) a run may address: see check_env_offset


def check_env_offset(env_offset: int, n_env: int) -> int:
    """The policy's sampling streams are (env_offset << 32) | t and the sensor's 2^62 + 2t (+ 1), bit 63 being the
    generator's domain bit: they stay disjoint while env_offset < 2^30.  Raises ValueError unless
    0 <= env_offset and env_offset + n_env <= 2^30; returns env_offset as an int."""
    env_offset, n_env = int(env_offset), int(n_env)
    if env_offset < 0 or env_offset + n_env > MAX_ENV_ROWS:
        raise ValueError(f"env_offset must be >= 0 with env_offset + n_env <= 2^30 (the policy's noise streams "
                         f"would meet the sensor's), got env_offset {env_offset}, n_env {n_env}")
    return env_offset


class RolloutEngine:
    MODE_RANDOM, MODE_SAMPLE, MODE_DET = -1, 1, 0

    def __init__(self, env: MultiAgentEnv, n_env: int, T: Optional[int] = None, device=None, env_offset: int = 0,
                 actor=None, mode: int = -1, lanes: int = 1, fused: bool = True, init_state=None):
        """actor: an ActorNet (or None); mode: MODE_SAMPLE (stochastic policy, sample_action),
        MODE_DET (deterministic policy, get_action) or MODE_RANDOM (keep `self.actions` as given).
        lanes: split the envs into that many contiguous slices, each running its T (act, step) pairs
        on its own HIP stream after the shared reset, so one slice's launch ramp and store drain
        overlap the other's compute (envs are independent: results are identical).  With an actor
        this needs the fused policy step (it reads only the prepared query-key workspace); the T
        sampling-noise tensors are drawn up front with the same Philox stream ids.
        fused: an env-only (MODE_RANDOM, one lane) rollout runs as one dgppo_env_rollout call with reset_first -- on
        the persistent Lidar route one launch that samples the envs and runs all T steps (else reset + T step
        launches; identical results).
        init_state: the env's state tuple (agent, goal, obstacle) for the n_env envs (env.get_graph's argument);
        when given, every run starts from that scene instead of a reset (the key then only seeds the policy
        noise).  The fp32 device tensors are read in place on every run, so editing them between runs -- also
        between replays of a captured engine -- runs the new scene.
        env_offset: the first of this engine's n_env rows in the run's noise streams (rank * n_env on a multi-GPU
        run); 0 <= env_offset, env_offset + n_env <= 2^30 (check_env_offset), else ValueError."""
        self.env_offset = check_env_offset(env_offset, n_env)  # before anything is allocated
        self.env = env
        self.B = int(n_env)
        self.T = int(T or env.max_episode_steps)
        self.device = torch.device(device) if device is not None else env.device
        self.actor = actor
        self.mode = mode if actor is not None else self.MODE_RANDOM
        B, T, n, dev = self.B, self.T, env.num_agents, self.device
        self.buf = env.empty_graph((T + 1, B), dev)
        nf = env._obstacle_fields()
        self.init_state = None
        if init_state is not None:  # the steps read the scene's own Lidar records
            self.init_state, self.obstacles = self._check_init_state(init_state)
        else:
            self.obstacles = (torch.empty((B, env._obstacle_rows(), nf), dtype=torch.float32, device=dev) if nf
                              else None)
        self.actions = torch.zeros((T, B, n, env.action_dim), dtype=torch.float32, device=dev)
        self.rewards = torch.empty((T, B), dtype=torch.float32, device=dev)
        self.costs = torch.empty((T, B, n, env.n_cost), dtype=torch.float32, device=dev)
        self.dones = torch.zeros((T, B), dtype=torch.bool, device=dev)
        self.key = torch.zeros(1, dtype=torch.int64, device=dev)
        if actor is not None:
            self.W = actor.carry_width  # carry floats per agent: (rnn_layers, carries, 64) flattened
            self.rnn = torch.zeros((T + 1, B, n, self.W), dtype=torch.float32, device=dev)
            self.log_pis = torch.zeros((T, B, n), dtype=torch.float32, device=dev)
            self.noise = torch.empty((B * n, env.action_dim), dtype=torch.float32, device=dev)
        self._hip_graph = None
        self.fused = bool(fused)
        self.lanes = int(lanes)
        if self.lanes > 1 and B % self.lanes:
            raise ValueError(f"n_env {B} is not a multiple of lanes {self.lanes}")
        if self.lanes > 1 and actor is not None and actor._fused_args(self._batch(0)) is None:
            self.lanes = 1  # the unfused actor path shares GEMM workspaces: one stream only
        if self.lanes > 1:
            self._streams = [torch.cuda.Stream(dev) for _ in range(self.lanes)]
            if self.mode == self.MODE_SAMPLE:
                self.noise_all = torch.empty((T, B * n, env.action_dim), dtype=torch.float32, device=dev)

    def _check_init_state(self, state):
        """The scene as the kernels will read it on every run: env.get_graph's shapes for n_env envs, fp32 tensors
        on the engine's device with contiguous rows (anything else would be copied, and a captured engine would
        replay the copy).  Returns (state, the Lidar obstacle records or None)."""
        agent, goal, third, B = self.env.state_rows(state, "init_state")
        names = ("agent", "goal", self.env._third_name())
        for name, t in zip(names, (agent, goal, third)):
            if t is None:
                continue
            if t.shape[0] != self.B:
                raise ValueError(f"init_state.{name} must hold {self.B} envs, got {tuple(t.shape)}")
            if t.dtype != torch.float32 or t.device != self.device:
                raise ValueError(f"init_state.{name} must be a float32 tensor on {self.device}, got {t.dtype} on "
                                 f"{t.device}")
            if t.stride(-1) != 1 or t.stride(-2) != t.shape[-1]:
                raise ValueError(f"init_state.{name} must have contiguous rows, got strides {tuple(t.stride())}")
        return tuple(state), (third if self.env._obstacle_fields() > 0 else None)

    def graph_at(self, t: int) -> GraphsTuple:
        b = self.buf
        return self.env._assemble(b.nodes[t], b.edges[t], b.states[t], b.receivers[t], b.senders[t], self.obstacles)

    def _batch(self, t: int, sl=slice(None)) -> GraphBatch:
        b = self.buf
        return GraphBatch.of(self.env, b.nodes[t][sl], b.edges[t][sl], b.receivers[t][sl], b.senders[t][sl])

    def _act_slice(self, t: int, sl: slice, k: int):
        n, A, w = self.env.num_agents, self.env.action_dim, sl.stop - sl.start
        h = self.rnn[t][sl].view(w * n, self.W)
        kw = dict(action_out=self.actions[t][sl].view(-1, A), h_out=self.rnn[t + 1][sl].view(w * n, self.W), prepare=False)
        if self.mode == self.MODE_SAMPLE:
            self.actor.act(self._batch(t, sl), h, 1, noise=self.noise_all[t][k * w * n:(k + 1) * w * n],
                           log_pi_out=self.log_pis[t][sl].view(-1), **kw)
        else:
            self.actor.act(self._batch(t, sl), h, 0, **kw)

    def _act(self, t: int):
        env = self.env
        g = self._batch(t)
        n = env.num_agents
        h = self.rnn[t].view(self.B * n, self.W)
        if self.mode == self.MODE_SAMPLE:
            # per-step, per-shard Philox stream (env_offset, t) -> disjoint noise across ranks, drawn inside the
            # fused policy step (K.normal_ into self.noise first on the unfused path)
            self.actor.act(g, h, 1, noise=self.noise, action_out=self.actions[t].view(-1, env.action_dim),
                           log_pi_out=self.log_pis[t].view(-1), h_out=self.rnn[t + 1].view(self.B * n, self.W),
                           prepare=t == 0, noise_seed=self.key, noise_stream=(self.env_offset << 32) | t)
        else:
            self.actor.act(g, h, 0, action_out=self.actions[t].view(-1, env.action_dim),
                           h_out=self.rnn[t + 1].view(self.B * n, self.W), prepare=t == 0)

    def _run(self):
        env = self.env
        if self.init_state is not None:  # graph 0 of the caller's scene in place of the reset
            cur = env.get_graph(self.init_state, out=self.graph_at(0))
            if self.mode == self.MODE_RANDOM and self.lanes == 1 and self.fused:
                env.rollout_into(self.buf, self.obstacles, self.actions, self.rewards, self.costs)
            elif self.lanes > 1:
                self._run_lanes()
            else:
                for t in range(self.T):
                    if self.mode != self.MODE_RANDOM:
                        self._act(t)
                    cur = env.step_into(cur, self.actions[t], self.graph_at(t + 1), self.rewards[t], self.costs[t])
            return
        if self.mode == self.MODE_RANDOM and self.lanes == 1 and self.fused:
            # env-only rollout: ONE call, on the persistent Lidar route one launch -- each wave samples its env (the
            # states-only reset), builds graph 0 and runs all T steps; other configs launch the reset, then their
            # rollout kernel or step loop, inside the call
            env.rollout_into(self.buf, self.obstacles, self.actions, self.rewards, self.costs, reset_key=self.key,
                             env_offset=self.env_offset)
            return
        cur = env.reset(self.key, n_env=self.B, env_offset=self.env_offset, out=self.graph_at(0),
                        obstacles_out=self.obstacles)
        if self.lanes > 1:
            self._run_lanes()
            return
        for t in range(self.T):
            if self.mode != self.MODE_RANDOM:
                self._act(t)
            cur = env.step_into(cur, self.actions[t], self.graph_at(t + 1), self.rewards[t], self.costs[t])

    def _run_lanes(self):
        env, b, main = self.env, self.buf, torch.cuda.current_stream(self.device)
        w = self.B // self.lanes
        if self.actor is not None:
            fa = self.actor._fused_args(self._batch(0))  # not None: checked in __init__
            K._chk(_lib.load().dgppo_policy_prepare(ctypes.byref(fa), _lib.stream_handle(self.device)),
                   "dgppo_policy_prepare")
            if self.mode == self.MODE_SAMPLE:
                for t in range(self.T):
                    K.normal_(self.noise_all[t], stream_id=(self.env_offset << 32) | t, seed_tensor=self.key)
        for k, s in enumerate(self._streams):
            sl = slice(k * w, (k + 1) * w)
            obst = self.obstacles[sl] if self.obstacles is not None else None
            at = lambda t: env._assemble(b.nodes[t][sl], b.edges[t][sl], b.states[t][sl],  # noqa: E731
                                         b.receivers[t][sl], b.senders[t][sl], obst)
            s.wait_stream(main)
            with torch.cuda.stream(s):
                cur = at(0)
                for t in range(self.T):
                    if self.actor is not None:
                        self._act_slice(t, sl, k)
                    cur = env.step_into(cur, self.actions[t][sl], at(t + 1), self.rewards[t][sl], self.costs[t][sl])
        for s in self._streams:
            main.wait_stream(s)

    def capture(self):
        """Record reset + T x (actor, step) into one hipGraph (after one eager warm-up run)."""
        self._run()
        torch.cuda.synchronize(self.device)
        g = K.hold_for_graph(torch.cuda.CUDAGraph())
        with torch.cuda.graph(g):
            self._run()
        self._hip_graph = g
        return self

    def run(self, key: int) -> Rollout:
        self.key.fill_(int(key))
        if self._hip_graph is not None:
            self._hip_graph.replay()
        else:
            self._run()
        return self.rollout()

    def rollout(self, graphs: Optional[GraphsTuple] = None) -> Rollout:
        """(B, T, ...) views of the time-major buffers (Rollout of dgppo/trainer/data.py).  graphs: another (T+1, B)
        graph buffer to take `graph` and `next_graph` from (default: the engine's true graphs)."""
        b, T = self.buf if graphs is None else graphs, self.T

        def view(sl):
            tr = lambda x: x[sl].transpose(0, 1)  # noqa: E731
            return self.env._assemble(tr(b.nodes), tr(b.edges), tr(b.states), tr(b.receivers), tr(b.senders),
                                      self.obstacles)

        rnn = None
        log_pis = None
        if self.actor is not None:
            # (B, T, rnn_layers, n, carries, 64): rnn_states[t] = carry before (stochastic) / after (deterministic)
            # step t; a view of the (T+1, B, n, W) buffer
            sl = slice(0, T) if self.mode == self.MODE_SAMPLE else slice(1, T + 1)
            rs = self.actor.gru
            rnn = self.rnn[sl].transpose(0, 1).unflatten(-1, (rs.layers, rs.carries, 64)).movedim(-4, -3)
            log_pis = self.log_pis.transpose(0, 1) if self.mode == self.MODE_SAMPLE else None
        return Rollout(view(slice(0, T)), self.actions.transpose(0, 1), rnn, self.rewards.transpose(0, 1),
                       self.costs.transpose(0, 1), self.dones.transpose(0, 1), log_pis, view(slice(1, T + 1)))


class _ObservedRolloutEngine(RolloutEngine):
    """What the two sensor engines share: per step the actor acts on an OBSERVED graph, kept in the time-major buffer
    `obs`, while env.step_into advances the TRUE graph in `buf` and writes the true reward and cost.  `sensing` is the
    utils.sensor.Sensing record the engine was built from or for (None: nothing beyond the subclass's own sensor); its
    `occlusion` and `fov` are attributes here.  MODE_DET or MODE_SAMPLE with an actor, one lane, a Lidar env with
    obstacles."""

    @staticmethod
    def _need_actor(what: str, actor, mode: int) -> None:
        if actor is None or mode not in (RolloutEngine.MODE_DET, RolloutEngine.MODE_SAMPLE):
            raise ValueError(f"{what}: needs an actor in MODE_DET or MODE_SAMPLE")

    def __init__(self, what: str, sensing: Optional[Sensing], final_obs: bool, env: MultiAgentEnv, n_env: int, T, device,
                 env_offset: int, actor, mode: int, init_state):
        env._require_lidar(what)
        super().__init__(env, n_env, T, device, env_offset, actor, mode, lanes=1, init_state=init_state)
        self.sensing = sensing
        self.occlusion, self.fov = (sensing.occlusion, sensing.fov) if sensing is not None else (False, None)
        # time-major, like buf; with final_obs one more graph, observed from the final true state
        self.obs = env.empty_graph((self.T + int(final_obs), self.B), self.device)

    def _observed_at(self, t: int) -> GraphsTuple:
        b = self.obs
        return self.env._assemble(b.nodes[t], b.edges[t], b.states[t], b.receivers[t], b.senders[t], self.obstacles)

    def _batch(self, t: int, sl=slice(None)) -> GraphBatch:  # the actor's input: the observed graph of step t
        b = self.obs
        return GraphBatch.of(self.env, b.nodes[t][sl], b.edges[t][sl], b.receivers[t][sl], b.senders[t][sl])

    def _run(self):
        env = self.env
        if self.init_state is not None:
            cur = env.get_graph(self.init_state, out=self.graph_at(0))
        else:
            cur = env.reset(self.key, n_env=self.B, env_offset=self.env_offset, out=self.graph_at(0),
                            obstacles_out=self.obstacles)
        for t in range(self.T):
            self._observe(t)
            self._act(t)
            cur = env.step_into(cur, self.actions[t], self.graph_at(t + 1), self.rewards[t], self.costs[t])

    @property
    def observed(self) -> GraphsTuple:
        """The graphs the actor saw (and with them the final one where the engine observes it), batch shape (B, T) or
        (B, T + 1): views of the time-major buffer."""
        b = self.obs
        tr = lambda x: x.transpose(0, 1)  # noqa: E731
        return self.env._assemble(tr(b.nodes), tr(b.edges), tr(b.states), tr(b.receivers), tr(b.senders),
                                  self.obstacles)


def _identity_sensor(alpha, t):
    return alpha


class SensorRolloutEngine(_ObservedRolloutEngine):
    """RolloutEngine with a LiDAR sensor model between the world and the policy.

    Per step t: alpha = env.lidar_scan(agent_t, obstacles); alpha_obs = sensor(alpha, t); the OBSERVED graph is
    env.get_graph(true state_t, lidar_data=env.lidar_hits(agent_t, alpha_obs)); the actor acts on it; env.step_into
    advances the TRUE graph (true obstacles, true ray cast) and writes the true reward and cost.  So the truth
    depends on the observation through the actions only, `run` returns the true Rollout (metrics and videos mean
    what they meant), and the observed graphs are `engine.observed`, batch shape (B, T).

    sensor: a callable (alpha (B, n, R), t) -> alpha_obs of the same shape, dtype and device (utils/sensor.py has
    LidarNoise; `lambda a, t: a` reproduces the plain engine bit for bit).  occlusion: obstacles also hide agents from
    each other -- each observed graph then goes through utils.sensor.mask_unseen with env.line_of_sight of the true
    state, and `sensor` may be None (the identity).  fov: a half angle in degrees (the envs with a heading) -- the
    senders outside the receiver's camera cone are hidden too (env.field_of_view, ANDed into the same mask); None and
    180 mean no cone, and `sensor` may be None here as well.  sensing: a utils.sensor.Sensing in place of occlusion and
    fov, and of `sensor` when that is None (the record's LidarNoise, seed 0).  bodies: the scan is
    env.lidar_scan(..., bodies=True), whose beams also return off the other agents' bodies, and `sensor` may be None
    once more; the true graph's scan stays the obstacle-only one.  No hipGraph capture (a sensor is arbitrary Python)."""

    def __init__(self, env: MultiAgentEnv, n_env: int, T: Optional[int] = None, device=None, env_offset: int = 0,
                 actor=None, mode: int = RolloutEngine.MODE_DET, sensor=None, init_state=None,
                 occlusion: bool = False, fov=None, sensing: Optional[Sensing] = None, bodies: bool = False):
        what = "SensorRolloutEngine"
        if sensing is None:
            sensing = Sensing.of(env, what, occlusion=occlusion, fov=fov)
        bodies = bodies_option(env, what, bodies)
        if sensor is None and sensing is not None:
            sensor = sensing.model(float(env.params["comm_radius"]))
        if sensor is None and bodies:
            sensor = _identity_sensor
        if not callable(sensor):
            raise ValueError("SensorRolloutEngine: sensor must be a callable (alpha, t) -> alpha_obs")
        self._need_actor(what, actor, mode)
        super().__init__(what, sensing, False, env, n_env, T, device, env_offset, actor, mode, init_state)
        self.sensor, self.bodies = sensor, bodies

    def _observe(self, t: int):
        env, n = self.env, self.env.num_agents
        agent = self.buf.states[t][:, :n]
        goal = self.buf.states[t][:, n:n + env.num_goals]
        scan = env.lidar_scan(agent, self.obstacles, bodies=True) if self.bodies else env.lidar_scan(agent, self.obstacles)
        alpha_obs = self.sensor(scan, t)
        seen = env.get_graph((agent, goal, self.obstacles), out=self._observed_at(t),
                             lidar_data=env.lidar_hits(agent, alpha_obs))
        if self.occlusion or self.fov is not None:
            vis = env.line_of_sight(agent, self.obstacles) if self.occlusion else None
            if self.fov is not None:
                cone = env.field_of_view(agent, self.fov)
                vis = cone if vis is None else vis & cone
            mask_unseen(seen, vis)

    def capture(self):
        raise NotImplementedError("SensorRolloutEngine: hipGraph capture of the sensor loop is not built")


class NoisyLidarRolloutEngine(_ObservedRolloutEngine):
    """RolloutEngine under the LidarNoise sensor model (utils/sensor.py), the sensor one fused launch per step
    (env.observe, torch.ops.dgppo.lidar_observe), so the whole rollout captures into a hipGraph: what training under
    the sensor model runs.  SensorRolloutEngine(sensor=LidarNoise(sigma, dropout, seed=key)) is its definition; this
    engine gives the same bits.

    Per step t: obs[t] = env.observe(true state_t, t) into a time-major buffer of T + 1 observed graphs; the actor acts
    on obs[t]; env.step_into advances the TRUE graph and writes the true reward and cost.  After the loop obs[T] is
    observed from the final true state (the update's final-value graph).  The noise seed is the engine's key tensor --
    a replay with a new key draws new noise -- under the sensor's stream ids (2^62 + 2t, + 1), which cannot collide
    with the policy's (env_offset << 32) | t while env_offset < 2^30 (check_env_offset refuses more); env b's beams
    draw at row env_offset + b.  occlusion: env.observe(..., occlusion=True), the agents hidden from each other by
    obstacles dropped from every observed graph in the same launch.  fov: env.observe(..., fov=deg), the senders outside
    the receiver's camera cone dropped as well (the envs with a heading; None and 180: no cone).  sensing: a
    utils.sensor.Sensing in place of the four keywords.  bodies: env.observe(..., bodies=True), the beams returning off
    the other agents' bodies too.

    `run` returns the true Rollout; `observed_rollout()` the Rollout the algorithms train on: graph and next_graph
    the observed ones, every other field the true run's."""

    def __init__(self, env: MultiAgentEnv, n_env: int, T: Optional[int] = None, device=None, env_offset: int = 0,
                 actor=None, mode: int = RolloutEngine.MODE_SAMPLE, sigma: float = 0.0, dropout: float = 0.0,
                 init_state=None, occlusion: bool = False, fov=None, sensing: Optional[Sensing] = None,
                 bodies: bool = False):
        what = "NoisyLidarRolloutEngine"
        self._need_actor(what, actor, mode)
        if sensing is None:
            sensing = Sensing.of(env, what, sigma, dropout, occlusion, fov)
        self.bodies = bodies_option(env, what, bodies)
        super().__init__(what, sensing, True, env, n_env, T, device, env_offset, actor, mode, init_state)
        self.sigma, self.dropout = sensing.sigma or 0.0, sensing.dropout or 0.0

    def _observe(self, t: int):
        env, n = self.env, self.env.num_agents
        s = self.buf.states[t]
        env.observe((s[:, :n], s[:, n:n + env.num_goals], self.obstacles), t, sigma=self.sigma, dropout=self.dropout,
                    seed=self.key, env_offset=self.env_offset, out=self._observed_at(t), occlusion=self.occlusion,
                    fov=self.fov, **({"bodies": True} if self.bodies else {}))

    def _run(self):
        super()._run()
        self._observe(self.T)

    def observed_rollout(self) -> Rollout:
        """The last run as the algorithms read it: graph = obs[0:T] and next_graph = obs[1:T+1] as (B, T) views,
        actions, carries, log_pis, rewards, costs and dones the true run's."""
        return self.rollout(self.obs)
