"""InforMARL (dgppo/algo/informarl.py): the GNN PPO baseline DGPPO extends — policy + Vl only, the
costs entering the GAE loss with weight `cost_weight` (informarl.py:318-340):

  l = -reward + w * sum_a sum_h max(cost, 0),  w = cost_weight (x5 at 50% and x5 at 75% of train_steps
  when cost_schedule, informarl.py:189-198);
  (Qh, Ql) = compute_dec_ocp_gae(costs, l, Vh = Vl broadcast, Vl);  Al = Ql - Vl;
  A = -(Al - mean_t Al) / (std_t Al + 1e-8) for every agent;
  per minibatch: update_Vl (l2 to Ql) and update_policy (clipped PPO + entropy), clip + Adam each.

Same kernels as DGPPO (GNN / GRU / TanhNormal / GAE / losses / Adam) plus dgppo_cost_shaped_loss and
dgppo_informarl_advantages.  The Vh network DGPPO builds is allocated but never used or stepped.
"""
from __future__ import annotations

import torch

from ..nn import kernels as K
from ..trainer.rollout import Rollout
from .dgppo import PREPASS_GRAPHS, DGPPO, _Phases


class InforMARL(DGPPO):
    NETS = ("Vl", "policy")  # Vh's parameters and Adam state stay as built (they are in the checkpoints)
    CONCURRENT = False

    def __init__(self, *args, cost_weight: float = 0.0, cost_schedule: bool = False, **kwargs):
        super().__init__(*args, **kwargs)
        self.cost_weight, self.cost_schedule = float(cost_weight), bool(cost_schedule)

    @property
    def config(self) -> dict:
        c = dict(super().config)
        c.update(cost_weight=self.cost_weight, cost_schedule=self.cost_schedule)
        for k in ("alpha", "cbf_eps", "cbf_weight", "cbf_schedule", "Vh_gnn_layers", "lr_Vh"):
            c.pop(k, None)
        return c

    @property
    def get_Vh(self):
        """InforMARL has no constraint-value function (the reference's informarl.py defines no get_Vh): the name
        DGPPO provides is absent here, so `hasattr(algo, "get_Vh")` is False.  HCBF-CRPO defines its own."""
        raise AttributeError(f"{type(self).__name__} has no get_Vh")

    def cost_weight_at(self, step: int) -> float:
        """optax.piecewise_constant_schedule(cost_weight, {0.5 T: 5, 0.75 T: 5}) (informarl.py:189-198)."""
        w = self.cost_weight
        if self.cost_schedule:
            if step >= int(self.train_steps * 0.5):
                w *= 5
            if step >= int(self.train_steps * 0.75):
                w *= 5
        return w

    def _targets(self, rollout: Rollout, Vl: torch.Tensor, step: int):
        """GAE on the cost-shaped loss with Vh = Vl broadcast, normalised advantages (informarl.py:324-340).
        Returns Ql (B, T), A (B, T, n) and extra info entries."""
        env, dev = self._env, self.device
        B, T = rollout.rewards.shape
        n = self._n_agents
        costs = rollout.costs.contiguous()
        l = torch.empty((B, T), device=dev)
        K.cost_shaped_loss(rollout.rewards.contiguous(), costs, self.cost_weight_at(step), l)
        Vh = Vl[:, :, None, None].expand(B, T + 1, n, env.n_cost).contiguous()
        Qh = torch.empty((B, T, n, env.n_cost), device=dev)
        Ql = torch.empty((B, T), device=dev)
        K.gae(costs, l, Vh, Vl, Qh, Ql, self.gamma, self.gae_lambda)
        A = torch.empty((B, T, n), device=dev)
        K.informarl_advantages(Ql, Vl, A)
        if self.trace is not None:
            self.trace.update(Vl=Vl.clone(), l=l.clone(), Ql=Ql.clone(), A=A.clone())
        return Ql, A, {}

    def update(self, rollout: Rollout, step: int) -> dict:
        B, T = rollout.rewards.shape
        chunk = max(1, min(B, PREPASS_GRAPHS // T))
        L = self.rnn_step
        ph = _Phases(self.device)
        ph.mark()
        info, extra = {}, {}
        self._flat_reduce = True  # one all-reduce of the whole gradient buffer per minibatch
        for _ in range(self.epoch_ppo):
            # Vl scan over the whole episode + final Vl (informarl.py:310-322)
            Vl = self._vl_all(rollout, chunk)
            Ql, A, extra = self._targets(rollout, Vl, step)
            # minibatches (informarl.py:342-355)
            for bi, envs in self._minibatches(B, T):
                S = len(bi) * (T // L)
                self.grad_flat.zero_()
                g, acts, lp_old, adv, tgt = self._mb_rows(envs, rollout.graph, rollout.actions, rollout.log_pis, A, Ql)
                tgt = tgt.view(S, L)
                acts, lp_old, adv = acts.view(-1, self._action_dim), lp_old.view(-1), adv.view(-1)
                vl_loss, stats = self._mb_step([
                    lambda pending: self._vl_pass(g, tgt, S, L, ph, pending),
                    lambda pending: self._pi_pass(g, acts, lp_old, adv, S, L, ph, pending)], ph)
                self._trace_mb(bi, vl_loss=vl_loss, stats=stats)
                info = {"Vl/loss": vl_loss, "Vl/max_target": tgt.max(), "Vl/min_target": tgt.min(),
                        "policy/stats": stats, "policy/log_pi_min": lp_old.min()}
        self._flat_reduce = False
        ph.report()
        info.update(extra)
        out = self._finish_info(info)
        for k in ("Vh/grad_Vh_norm", "Vh/grad_Vh_has_nan"):
            out.pop(k, None)
        return out
