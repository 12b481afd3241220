"""The attention kernel families the bench configurations do not reach (csrc/attn.hip: the block forward, the block
and wave backward at their other instantiations, the above-64 KB LDS opt-in) against the float64 per-edge reference.

Each case is a two-layer layers.GNN built directly on a ParamSpace with a msg_dim / n_heads the kernels' tuned
paths do not cover, run forward and backward on 6 env graphs (S = 2 sequences of L = 3 steps) and compared with
oracle.nets_t.gnn: the agents' outputs and every parameter gradient, with test_nets_gpu's bounds (outputs
|gpu - ref| <= 1e-5 + 1e-5 |ref|, gradients <= 2e-5 max|ref| + 1e-6 per tensor).

Which family each layer's forward / backward launch takes is NOT asked of the library here (this file runs unchanged
against a library without dgppo_gnn_attn_plan); tests/test_attn_plan_cpu.py evaluates this table through the plan on
the CPU and checks that it reaches every (family, direction) pair and the cp / dm instantiations it is meant to.
`fused` says which layers' forward goes through the fused layer kernel instead of dgppo_gnn_attn_fwd."""
import numpy as np
import pytest
import torch

from dgppo_fov_amd.nn.layers import GNN, ParamSpace
from oracle import nets_t as R
from test_nets_gpu import _close, _grad_close, _graphs, _walk

pytestmark = pytest.mark.gpu

S, L = 2, 3

# key: (env id, agents, obstacles, GNN keyword arguments, fused forward per layer)
CASES = {
    # 2 heads: block forward <32, 8> / <32, 32>, wave backward at the same; layer 2 has pre_W (dpre_part rows)
    "spread8_h2": ("LidarSpread", 8, 3, dict(n_heads=2), (False, False)),
    # msg_dim 40: layer 2 is D = 40, the DM = 64 instantiations
    "spread8_d40": ("LidarSpread", 8, 3, dict(msg_dim=40), (True, False)),
    # 9 candidates: CP = 8 is too narrow, CP = 16
    "mpe3_h2": ("MPESpread", 3, 3, dict(n_heads=2), (False, False)),
    # 4 candidates: CP = 8
    "mpetarget3_h2": ("MPETarget", 3, 0, dict(n_heads=2), (False, False)),
    # C = 72, D = 40: block forward and backward <128, 64>; the backward's LDS is past 64 KB
    "spread32_d40": ("LidarSpread", 32, 8, dict(msg_dim=40), (False, False)),
    # 10-wide first layer with 33 candidates: wave backward <64, 32>
    "omni24": ("LidarOmniTarget", 24, 3, dict(), (False, False)),
    # the tuned row-block pair, unfused (10-wide edges): <16> first layer, <32> second
    "omni3": ("LidarOmniTarget", 3, 2, dict(), (False, False)),
}


def build_gnn(env, device, kw, seed=3):
    """A two-layer GNN with nonzero biases (so every bias gradient path carries signal)."""
    ps = ParamSpace()
    net = GNN(ps, "gnn", env.node_dim, 2, edge_dim=env.edge_dim, **kw)
    ps.build(device)
    rng = np.random.default_rng(seed)
    net.init_host(rng)
    for layer in net.layers:
        for b in ("bq", "bk", "bu"):
            v = layer.v(b)
            v.copy_(torch.from_numpy((0.1 * rng.standard_normal(tuple(v.shape))).astype(np.float32)))
    return ps, net


@pytest.mark.parametrize("key", list(CASES))
def test_gnn_fwd_bwd_matches_float64(cuda, key):
    eid, n, obs, kw, fused = CASES[key]
    env, gb, host = _graphs(cuda, eid, n, obs, S, L, seed=5)
    ps, net = build_gnn(env, cuda, kw)
    Y, caches = net.fwd(gb)
    assert tuple(bool(layer.last_fused) for layer in net.layers) == fused  # which forwards the fused kernel took
    p = R.to_t(net.flax(), requires_grad=True)
    ref = R.gnn(p, host, n, msg_dim=kw.get("msg_dim", 32), n_heads=kw.get("n_heads", 3))
    torch.cuda.synchronize()
    _close(Y.cpu().numpy(), ref.detach().numpy().reshape(S * L * n, -1), what=f"{key} output")
    w = np.random.default_rng(7).standard_normal((S * L * n, 64))
    (ref.reshape(S * L * n, -1) * torch.tensor(w)).sum().backward()
    ps.zero_grad()
    net.bwd(caches, torch.tensor(w, dtype=torch.float32, device=cuda), gb)
    torch.cuda.synchronize()
    ps.swap_views()
    g = net.flax()
    ps.swap_views()
    for path, a, b in _walk(g, R.grads(p)):
        _grad_close(a, b, f"{key} grad {path}")
