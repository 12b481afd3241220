"""Shared pieces of the env tests: graph comparison, adversarial Lidar scenes (pure NumPy, so the CPU tests can run
them through the oracle alone), the oracle chain of a whole rollout and its bit-for-bit comparison, and the case
table of test_rollout_oracle_gpu.py (held to dgppo_env_rollout_plan by test_env_rollout_plan_cpu.py)."""
from types import SimpleNamespace

import numpy as np

from oracle import env as O

GRAPH_FIELDS = ("nodes", "edges", "states", "receivers", "senders")
CHAIN_FIELDS = GRAPH_FIELDS + ("reward", "cost")


def _np(t):
    return t.detach().cpu().numpy()


def assert_graph_equal(g, ref, what=""):
    for f in ("nodes", "edges", "states"):
        a, b = _np(getattr(g, f)), ref[f]
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        bad = ~((a == b) | (np.isnan(a) & np.isnan(b)))
        assert not bad.any(), f"{what} {f}: {bad.sum()} mismatches, first at {np.argwhere(bad)[0]}: {a[bad][:4]} vs {b[bad][:4]}"
    np.testing.assert_array_equal(_np(g.receivers), ref["receivers"], err_msg=f"{what} receivers")
    np.testing.assert_array_equal(_np(g.senders), ref["senders"], err_msg=f"{what} senders")


def oracle_third(spec, g):
    if spec.engine == O.ENGINE_MPE:
        return None
    return _np(g.env_states.obstacle.packed) if spec.n_obs > 0 else np.zeros((_np(g.states).shape[0], 0, 16), np.float32)


def adversarial_lidar_scene(spec, states, ob, seed):
    """Inputs aimed at the wave kernel's exact ray culling: tiny / huge / ineligible
    obstacles, edges exactly parallel to a ray, NaN and far-away corners, agents at corners and
    centres (inside -> alpha 0), agents crowded around one obstacle (> k hits), NaN actions.
    `states` (B, N, sd) and `ob` (B, 3, 16) are a reset's arrays (from the GPU env or from O.env_reset); returns the
    scene's (states, obstacles, actions).  Env b is of kind b % 8."""
    rng = np.random.default_rng(seed)
    states = states.copy()
    ob = ob.copy()
    B = states.shape[0]
    n = spec.n
    rays = O.ray_table(spec.n_rays, 0.5)
    kind = np.arange(B) % 8
    for b in range(B):
        k = kind[b]
        if k == 0:  # random sizes spanning eligibility (rho <= 0.5) and tiny boxes, exact axis angles
            wh = rng.choice([1e-4, 0.05, 0.3, 0.69, 0.9], size=(3, 2))
            th = rng.choice([0.0, np.pi / 2, np.pi, rng.uniform(0, 2 * np.pi)], size=3)
            ob[b] = O.make_rectangles(rng.uniform(0, 1.5, (3, 2)), wh[:, 0], wh[:, 1], th)
        elif k == 1:  # agents exactly on corners / centres of obstacles
            for i in range(n):
                o = i % 3
                p = ob[b, o, 8 + 2 * (i % 4):10 + 2 * (i % 4)] if i < 4 else ob[b, o, :2]
                states[b, i, :2] = np.clip(p, 0, 1.5)
                states[b, i, 2:4] = 0.0
        elif k == 2:  # obstacle 0 = parallelogram whose first edge is exactly 2 x ray r
            r = rng.integers(0, spec.n_rays)
            c = states[b, 0, :2] + rays[(r + 8) % spec.n_rays] * 0.6
            e1 = rays[r] * np.float32(2.0)
            e2 = rays[(r + 8) % spec.n_rays] * np.float32(0.5)
            p0 = c.astype(np.float32)
            pts = np.stack([p0, p0 - e1, p0 - e1 - e2, p0 - e2]).astype(np.float32)
            ob[b, 0, 8:] = pts.reshape(-1)
            ob[b, 0, :2] = pts.mean(0)
        elif k == 3:  # NaN corner and far / huge obstacles
            ob[b, 0, 8] = np.nan
            ob[b, 1, 8:] = ob[b, 1, 8:] + np.float32(1e3)
            ob[b, 2, 8:] = ob[b, 2, 8:] * np.float32(3.0)
        elif k == 4:  # everyone crowded around obstacle 0
            states[b, :n, :2] = ob[b, 0, :2] + rng.uniform(-0.25, 0.25, (n, 2)).astype(np.float32)
            states[b, :n, :2] = np.clip(states[b, :n, :2], 0, 1.5)
        elif k == 5:  # agent on the ray line through a corner
            r = rng.integers(0, spec.n_rays)
            states[b, 0, :2] = np.clip(ob[b, 1, 8:10] - rays[r] * np.float32(0.5), 0, 1.5)
            states[b, 0, 2:4] = 0.0
    a = rng.uniform(-1, 1, (B, n, spec.ad)).astype(np.float32)
    a[kind == 1] = 0.0
    a[kind == 5, 0] = 0.0
    a[6, 0, 0] = np.nan
    if spec.ad == 3:  # LidarOmniTarget: coincident agents (FoV norm 0), non-unit headings, rates at the
        # limits, huge / non-finite alpha
        for b in np.nonzero(kind == 6)[0]:
            states[b, 1, :2] = states[b, 0, :2]
            states[b, :n, 2:4] = [0.3, 0.4]
        for b in np.nonzero(kind == 7)[0]:
            states[b, :n, 6] = rng.choice([-99.0, 0.0, 99.0], size=n)
            states[b, :n, 4:6] = rng.choice([-1.9, 2.5], size=(n, 2))
        a[7, 1, 2] = 1e30
        a[15, 2, 2] = -np.inf
        a[23, 3, 2] = np.nan
    return states, ob, a


# ---- a whole rollout against the oracle ------------------------------------------------------------------------
def oracle_chain(spec, states0, third, actions):
    """T = len(actions) oracle steps from graph 0's `states0` (B, N, sd): every field stacked over t -- graph t + 1
    (nodes, edges, states, receivers, senders), reward[t] and cost[t], each (T, B, ...).  `third`: the Lidar obstacle
    records (None for MPE, whose obstacles are state rows).  NaN rows stay NaN for the rest of the chain."""
    out = {f: [] for f in CHAIN_FIELDS}
    states = np.asarray(states0, np.float32)
    with np.errstate(all="ignore"):
        for a in actions:
            ref = O.env_step(spec, states, third, a)
            for f in CHAIN_FIELDS:
                out[f].append(ref[f])
            states = ref["states"]
    return {f: np.stack(v) for f, v in out.items()}


def _bits_differ(a, b):
    """Elementwise: not the same bits and not both NaN."""
    if a.dtype.kind == "f":
        return (a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b))
    return a != b


def first_chain_mismatch(got, chain):
    """(step, field, env, index within the env's rows) of the first element of `got` that differs from the oracle
    chain, None when every one matches.  `got`: nodes / edges / states / receivers / senders (T + 1, B, ...) rollout
    buffers (graph t + 1 is compared with the chain's step t), reward (T, B) and cost (T, B, n, n_cost), as NumPy
    arrays in a mapping.  Steps are searched in order, within a step the fields in CHAIN_FIELDS order."""
    T = chain["reward"].shape[0]
    for t in range(T):
        for f in CHAIN_FIELDS:
            a = np.ascontiguousarray(got[f][t + 1] if f in GRAPH_FIELDS else got[f][t])
            b = np.ascontiguousarray(chain[f][t])
            assert a.shape == b.shape and a.dtype == b.dtype, (t, f, a.shape, b.shape, a.dtype, b.dtype)
            bad = _bits_differ(a, b)
            if bad.any():
                at = tuple(int(i) for i in np.argwhere(bad)[0])
                return t, f, at[0], at[1:]
    return None


def assert_chain_equal(got, chain, what=""):
    """Every field of every step by bits (NaN equal to NaN, as assert_graph_equal; reward and cost with the same NaN
    pattern and equal elsewhere); reports the first failing (step, field, env, index)."""
    bad = first_chain_mismatch(got, chain)
    if bad is not None:
        t, f, env, idx = bad
        a = (got[f][t + 1] if f in GRAPH_FIELDS else got[f][t])[(env,) + idx]
        b = chain[f][t][(env,) + idx]
        raise AssertionError(f"{what}: first mismatch at step {t}, field {f}, env {env}, index {idx}: {a!r} vs "
                             f"oracle {b!r}")


def host_buffers(buf, rewards, costs):
    """The mapping first_chain_mismatch takes, from a rollout's device buffers."""
    got = {f: _np(getattr(buf, f)) for f in GRAPH_FIELDS}
    got["reward"], got["cost"] = _np(rewards), _np(costs)
    return got


# ---- the adversarial chain of test_rollout_oracle_gpu.py (c) ----------------------------------------------------
ADV_B, ADV_T, ADV_SEED = 256, 6, 77


def adversarial_chain_inputs(spec, agent, goal, ob, seed=ADV_SEED, T=ADV_T):
    """The rollout form of adversarial_lidar_scene: graph 0's agent / goal rows and obstacles of B envs (kinds b % 8)
    and T steps of actions -- the scene's own actions (a NaN at env 6) at t = 0, uniform +-1.5 after, a second NaN at
    t = 3 in env 9 (an agent row turns NaN mid-episode and stays NaN), an inf and a -1e30 at t = 4."""
    B, n = agent.shape[0], spec.n
    rows = np.concatenate([agent, goal], 1)
    rows, ob, a0 = adversarial_lidar_scene(spec, rows, ob, seed)
    rng = np.random.default_rng(seed + 1)
    acts = rng.uniform(-1.5, 1.5, (T, B, n, spec.ad)).astype(np.float32)
    if spec.ad == 3:
        acts[..., 2] *= 1000.0
    acts[0] = a0
    acts[3, 9, 2, 1] = np.nan
    acts[4, 10, 0, 0] = np.inf
    acts[4, 11, 1, 1] = -1e30
    return rows[:, :n].copy(), rows[:, n:].copy(), ob, acts


def full_lists_scene(spec, agent, goal, ob):
    """16 LidarSpread envs for 8 envs per workgroup: envs 0..7 keep every (agent, obstacle, ray) triple on the ray-cast
    item list (8 x 768 pooled items, the list at capacity) -- none of their obstacles is eligible for culling: a NaN
    corner, corners 1e3 away, a circumradius 8 x >= 0.07 > 0.5 -- and envs 8..15 have 0.1-wide eligible obstacles near
    (1.9, 1.9), turned 0.1 rad so that no edge is parallel to a ray, with every agent inside [0, 1]^2: farther than a
    ray's length (0.5) from every corner for the 6 steps, so no triple survives."""
    agent, ob = agent.copy(), ob.copy()
    for b in range(8):
        ob[b, 0, 8] = np.nan
        ob[b, 1, 8:] = ob[b, 1, 8:] + np.float32(1e3)
        c = np.tile(ob[b, 2, :2], 4)
        ob[b, 2, 8:] = (ob[b, 2, 8:] - c) * np.float32(8.0) + c
    far = O.make_rectangles(np.array([[1.9, 1.9], [1.9, 1.7], [1.7, 1.9]], np.float32), np.full(3, 0.1, np.float32),
                            np.full(3, 0.1, np.float32), np.full(3, 0.1, np.float32))
    for b in range(8, 16):
        ob[b] = far
        agent[b, :, :2] *= np.float32(2.0 / 3.0)
    return agent, goal, ob


FULL_LISTS_KEY = 31


def full_lists_inputs(spec, agent, goal, ob):
    """full_lists_scene of a reset (key FULL_LISTS_KEY, 16 envs) with its ADV_T steps of actions."""
    agent, goal, ob = full_lists_scene(spec, agent, goal, ob)
    return agent, goal, ob, chain_actions(spec, ADV_T, agent.shape[0], seed=6)


def chain_actions(spec, T, B, seed):
    """Uniform +-1.5 actions (T, B, n, ad), the Omni angular component x1000 (clipped at +-1000)."""
    a = np.random.default_rng(seed).uniform(-1.5, 1.5, (T, B, spec.n, spec.ad)).astype(np.float32)
    if spec.ad == 3:
        a[..., 2] *= 1000.0
    return a


# ---- the GPU case table ---------------------------------------------------------------------------------------
LIDAR_IDS = ("LidarSpread", "LidarTarget", "LidarBicycleTarget", "LidarOmniTarget")
_S838 = (256, 8, 3, 32, 8)


def _case(eid, n, obs, B, T, route, wpg=0, mode=0, rebuild=True, size=None, stage=0, pre=0, layout="aligned",
          actions="uniform", scene="reset"):
    """One GPU case and, next to it, what dgppo_env_rollout_plan must answer for it.  wpg: the forced envs per
    workgroup (0 = automatic); mode: dgppo_env_set_step_kernel; rebuild: rebuild_first; size / stage: BLOCK's SizeTag
    and staging flag; pre: a REBUILD launch precedes; layout: "aligned" or "t_edges+2" (per-step edge stride a
    multiple of 4 floats plus 2)."""
    return SimpleNamespace(eid=eid, n=n, obs=obs, B=B, T=T, route=route, wpg=wpg, mode=mode, rebuild=rebuild,
                           size=size, stage=stage, pre=pre, layout=layout, actions=actions, scene=scene)


def _cases():
    c = {}
    for eid in LIDAR_IDS:
        for w in (1, 4, 8):
            for rb in (True, False):  # (a) every Lidar wave instantiation, both ways into graph 0
                c[f"a-{eid}-w{w}-{'rebuild' if rb else 'loaded'}"] = _case(eid, 8, 3, 19, 33, "LIDAR_WAVE", wpg=w,
                                                                           rebuild=rb)
            for rb in (True, False):  # (c) the adversarial scenes through the persistent kernel
                c[f"c-{eid}-w{w}-{'rebuild' if rb else 'loaded'}"] = _case(eid, 8, 3, ADV_B, ADV_T, "LIDAR_WAVE",
                                                                           wpg=w, rebuild=rb, scene="adversarial")
    c["c-LidarSpread-w8-full-lists"] = _case("LidarSpread", 8, 3, 16, ADV_T, "LIDAR_WAVE", wpg=8, rebuild=True,
                                             scene="full-lists")
    # (b) episode lengths
    c["b-LidarSpread-w8-T128"] = _case("LidarSpread", 8, 3, 17, 128, "LIDAR_WAVE", wpg=8)
    c["b-LidarOmniTarget-w4-T128"] = _case("LidarOmniTarget", 8, 3, 17, 128, "LIDAR_WAVE", wpg=4)
    for T in (1, 15, 16, 17, 32):
        c[f"b-LidarBicycleTarget-w4-T{T}"] = _case("LidarBicycleTarget", 8, 3, 9, T, "LIDAR_WAVE", wpg=4)
    # (d) the other persistent kernels
    sp = dict(actions="uniform+nan+inf")
    c["d-block-LidarSpread-n8"] = _case("LidarSpread", 8, 3, 9, 17, "BLOCK", mode=1, size=_S838, stage=1, **sp)
    c["d-block-LidarSpread-n8-adversarial"] = _case("LidarSpread", 8, 3, ADV_B, ADV_T, "BLOCK", mode=1, size=_S838,
                                                    stage=1, rebuild=False, scene="adversarial")
    c["d-block-LidarSpread-n32-staged"] = _case("LidarSpread", 32, 8, 3, 24, "BLOCK", size=(256, 32, 8, 32, 8),
                                                stage=1, **sp)
    c["d-block-LidarSpread-n32-prefetched"] = _case("LidarSpread", 32, 8, 3, 128, "BLOCK", size=(256, 32, 8, 32, 8),
                                                    stage=0, **sp)
    c["d-block-LidarTarget-n4"] = _case("LidarTarget", 4, 2, 9, 17, "BLOCK", size=(128, 0, -1, 0, 0), stage=1, **sp)
    c["d-block-LidarBicycleTarget-n9"] = _case("LidarBicycleTarget", 9, 1, 9, 17, "BLOCK", size=(256, 0, -1, 0, 0),
                                               stage=1, **sp)
    c["d-block-MPETarget-n3-o0"] = _case("MPETarget", 3, 0, 9, 17, "BLOCK", size=(64, 3, 0, 0, 0), stage=1, **sp)
    c["d-block-MPESpread-n5-o2"] = _case("MPESpread", 5, 2, 9, 17, "BLOCK", size=(64, 0, -1, 0, 0), stage=1, **sp)
    c["d-block-MPESpread-n3-o3"] = _case("MPESpread", 3, 3, 9, 17, "BLOCK", mode=1, size=(64, 3, 3, 0, 0), stage=1,
                                         **sp)
    # ... and the engine / goal instantiations of each SizeTag the list above leaves out (B = 5)
    for eid, n, o, mode, size in (("LidarBicycleTarget", 4, 2, 0, (128, 0, -1, 0, 0)),
                                  ("LidarBicycleTarget", 32, 8, 0, (256, 32, 8, 32, 8)),
                                  ("LidarBicycleTarget", 8, 3, 1, _S838),
                                  ("LidarSpread", 3, 2, 0, (128, 0, -1, 0, 0)),
                                  ("LidarSpread", 9, 1, 0, (256, 0, -1, 0, 0)),
                                  ("LidarTarget", 9, 1, 0, (256, 0, -1, 0, 0)),
                                  ("LidarTarget", 32, 8, 0, (256, 32, 8, 32, 8)),
                                  ("LidarTarget", 8, 3, 1, _S838),
                                  ("MPESpread", 3, 0, 0, (64, 3, 0, 0, 0)),
                                  ("MPETarget", 5, 2, 0, (64, 0, -1, 0, 0)),
                                  ("MPETarget", 3, 3, 1, (64, 3, 3, 0, 0))):
        c[f"d-block-{eid}-n{n}-o{o}"] = _case(eid, n, o, 3 if n == 32 else 5, 17, "BLOCK", mode=mode, size=size,
                                             stage=1, **sp)
    for eid in ("MPESpread", "MPETarget"):
        for T in (33, 128):
            c[f"d-mpe-wave-{eid}-T{T}"] = _case(eid, 3, 3, 9, T, "MPE_WAVE", wpg=4, **sp)
    c["d-rebuild-then-block"] = _case("LidarSpread", 8, 3, 9, 17, "BLOCK", size=_S838, stage=1, pre=1,
                                      layout="t_edges+2", **sp)
    # (e) the automatic threshold (compared with the step kernel; first and last 32 envs with the oracle)
    c["e-auto-2049"] = _case("LidarSpread", 8, 3, 2049, 3, "LIDAR_WAVE", wpg=0)
    c["e-auto-2047"] = _case("LidarSpread", 8, 3, 2047, 3, "LIDAR_WAVE", wpg=0)
    return c


CASES = _cases()
AUTO_WPG = {"e-auto-2049": 8, "e-auto-2047": 4}  # what the plan answers with nothing forced


class RolloutBuffers:
    """Rollout buffers with guard envs and guard steps around the used slice: every graph field is allocated
    (T + 3, B + 2 * PAD, ...) (reward / cost (T + 2, ...)) and used as [1:T + 2, PAD:PAD + B]; PAD = 4 keeps every
    row of the used slice as aligned as the allocation.  layout "t_edges+2": the edge buffer's per-step stride is a
    multiple of 4 floats plus 2 (its base stays 16-byte aligned).  Everything is prefilled with a sentinel (a NaN
    with a payload / a negative index);
    `assert_guards_untouched` then demands those bits back outside the slice."""
    PAD = 4
    F_SENT = np.array([0x7FC0BEEF], np.uint32).view(np.float32)[0]
    I_SENT = -0x1234567

    def __init__(self, env, B, T, device, layout="aligned"):
        import torch

        P, n = self.PAD, env.num_agents
        self.env, self.B, self.T = env, B, T
        W = B + 2 * P
        N, E = env.n_nodes, env.n_edges
        f32 = dict(dtype=torch.float32, device=device)
        self.full = {}

        def strides(inner):
            return tuple(int(np.prod(inner[i + 1:])) for i in range(len(inner)))

        def alloc(name, steps, inner, int32=False, tail=0):
            # tail: extra floats per step; the same number leads the allocation, so step 1 (the first used) starts
            # on a 16-byte boundary again
            row = int(np.prod(inner))
            per_step = W * row + tail
            flat = torch.empty(tail + steps * per_step, dtype=torch.int32 if int32 else torch.float32, device=device)
            (flat if int32 else flat.view(torch.int32)).fill_(
                self.I_SENT if int32 else int(np.array([self.F_SENT]).view(np.int32)[0]))
            self.full[name] = flat
            return flat.as_strided((steps, W) + tuple(inner), (per_step, row) + strides(inner), tail)

        tail = 2 if layout == "t_edges+2" else 0
        assert layout in ("aligned", "t_edges+2")
        whole = dict(nodes=alloc("nodes", T + 3, (N, env.node_dim)),
                     edges=alloc("edges", T + 3, (E, env.edge_dim), tail=tail),
                     states=alloc("states", T + 3, (N, env.state_dim)),
                     receivers=alloc("receivers", T + 3, (E,), int32=True),
                     senders=alloc("senders", T + 3, (E,), int32=True),
                     reward=alloc("reward", T + 2, ()),
                     cost=alloc("cost", T + 2, (n, env.n_cost)))
        self.whole = whole
        used = {k: (v[1:T + 2, P:P + B] if k in GRAPH_FIELDS else v[1:T + 1, P:P + B]) for k, v in whole.items()}
        self.buf = env._assemble(used["nodes"], used["edges"], used["states"], used["receivers"], used["senders"], None)
        self.rewards, self.costs = used["reward"], used["cost"]

    def graph0(self, obstacles=None):
        b = self.buf
        return self.env._assemble(b.nodes[0], b.edges[0], b.states[0], b.receivers[0], b.senders[0], obstacles)

    def host(self):
        return host_buffers(self.buf, self.rewards, self.costs)

    def assert_guards_untouched(self, what=""):
        P, B, T = self.PAD, self.B, self.T
        for name, flat in self.full.items():
            a = flat.cpu().numpy().view(np.uint32 if flat.dtype.itemsize == 4 else np.uint8)
            w = self.whole[name]
            sent = (np.array([self.I_SENT], np.int32) if name in ("receivers", "senders")
                    else np.array([self.F_SENT], np.float32)).view(np.uint32)[0]
            touched = a != sent
            # the used slice, as a mask over the flat allocation
            mask = np.zeros(a.shape, bool)
            steps = T + 1 if name in GRAPH_FIELDS else T
            row = int(np.prod(w.shape[2:])) if w.dim() > 2 else 1
            for t in range(1, 1 + steps):
                lo = w.storage_offset() + t * w.stride(0) + P * row
                mask[lo:lo + B * row] = True
            bad = touched & ~mask
            assert not bad.any(), (f"{what}: {name} written outside the used slice at flat index "
                                   f"{np.argwhere(bad)[0][0]}")


# ---- plans of cases ---------------------------------------------------------------------------------------------
class forced:
    """with forced(wpg, mode): dgppo_env_set_rollout_wpg / dgppo_env_set_step_kernel, restored on exit."""

    def __init__(self, wpg=0, mode=0):
        self.wpg, self.mode = wpg, mode

    def __enter__(self):
        from dgppo_fov_amd import _lib

        lib = _lib.load()
        self.prev_wpg = lib.dgppo_env_set_rollout_wpg(self.wpg)
        self.prev_mode = lib.dgppo_env_set_step_kernel(self.mode)
        assert self.prev_wpg >= 0 and self.prev_mode >= 0
        return self

    def __exit__(self, *exc):
        from dgppo_fov_amd import _lib

        lib = _lib.load()
        lib.dgppo_env_set_rollout_wpg(self.prev_wpg)
        lib.dgppo_env_set_step_kernel(self.prev_mode)
        return False


def plan_of(env, buf, obstacles, actions, rewards, costs, rebuild_first):
    """ops.env_rollout_plan on exactly the tensors env.rollout_into passes to ops.env_rollout."""
    from dgppo_fov_amd import ops

    return ops.env_rollout_plan(env._cfg_handle, bool(rebuild_first), obstacles, actions,
                                env._ray_table(buf.states.device), buf.nodes, buf.edges, buf.states, buf.receivers,
                                buf.senders, rewards, costs)


def plan_key(env, pl):
    """The coverage key of a plan: (route, WPG, engine, goal, SizeTag, stage, rebuild)."""
    return (pl.route_name, pl.wpg, int(env.cfg.engine), int(env.cfg.goal_mode), pl.size_tag, pl.stage, pl.rebuild)


def assert_case_plan(name, case, pl):
    """The plan names the route, WPG, SizeTag, staging flag and REBUILD launch written next to the case."""
    wpg = AUTO_WPG.get(name, case.wpg)
    got = (pl.route_name, pl.wpg, pl.size_tag, pl.stage, pl.rebuild)
    assert got == (case.route, wpg, case.size, case.stage, case.pre), (name, got)
    assert (pl.grid - 1) * max(pl.wpg, 1) < case.B <= pl.grid * max(pl.wpg, 1), (name, pl.grid)


def case_tensors(env, case, device):
    """(RolloutBuffers, obstacles or None, zeroed actions) of a case on `device`."""
    import torch

    rb = RolloutBuffers(env, case.B, case.T, device, case.layout)
    nf = env._obstacle_fields()
    ob = torch.zeros((case.B, env._obstacle_rows(), nf), dtype=torch.float32, device=device) if nf else None
    acts = torch.zeros((case.T, case.B, env.num_agents, env.action_dim), dtype=torch.float32, device=device)
    return rb, ob, acts
