"""Host-side layer logic that needs no GPU: the flax <-> kernel parameter layout of GraphTransformer for
4- and 10-wide edges (Dense_3 split into Wcat's edge rows + Wex), and GraphBatch's wide-node views."""
import numpy as np
import pytest
import torch

from dgppo_fov_amd.nn.layers import GraphBatch, GraphTransformer, ParamSpace


@pytest.mark.parametrize("ED", [4, 10])
def test_graph_transformer_flax_roundtrip(ED):
    ps = ParamSpace()
    L = GraphTransformer(ps, "t", 10, 32, 3, ED)
    ps.build("cpu")
    L.init_host(np.random.default_rng(0))
    d = L.flax()
    rng = np.random.default_rng(1)
    for k in ("Dense_0", "Dense_1", "Dense_2", "Dense_3", "Dense_4"):
        for kk in d[k]:
            d[k][kk] = rng.standard_normal(d[k][kk].shape).astype(np.float32)
    assert d["Dense_3"]["kernel"].shape == (ED, 96)
    L.load_flax(d)
    back = L.flax()
    for k in d:
        for kk in d[k]:
            assert np.array_equal(back[k][kk], d[k][kk]), (k, kk)
    if ED > 4:  # Wex row h*EX + j = Dense_3 row 4 + j, head h's column block
        wex = L.v("Wex").numpy()
        assert np.array_equal(wex[1 * (ED - 4) + 2], d["Dense_3"]["kernel"][4 + 2, 32:64])


def test_omni_graph_batch_views():
    """LidarOmniTarget graphs (oracle reset): never-receiving nodes are zero outside
    nonagent_feature_cols, so the agent-mode layers' compressed raw rows lose nothing; edge views split
    at column 4; nodes wider than 8 without raw_cols are refused."""
    from dgppo_fov_amd.env.lidar_env.lidar_omni_target import LidarOmniTarget
    from oracle import env as OE

    cols = LidarOmniTarget.nonagent_feature_cols
    n = 3
    spec = OE.Spec("LidarOmniTarget", n, 2)
    ag, gl, third = OE.env_reset(spec, 5, 4)
    g = OE.initial_graph(spec, ag, gl, third)
    nodes, edges = g["nodes"], g["edges"]
    mask = np.ones(nodes.shape[2], bool)
    mask[list(cols)] = False
    assert np.abs(nodes[:, n:][..., mask]).max() == 0
    assert np.abs(nodes[:, n:][..., list(cols)]).max() > 0
    G = nodes.shape[0]
    cand = torch.zeros((n, 4), dtype=torch.int32)
    args = (torch.from_numpy(nodes), torch.from_numpy(edges), torch.from_numpy(g["receivers"]),
            torch.from_numpy(g["senders"]), n, cand)
    gb = GraphBatch(*args, raw_cols=cols)
    raw, c = gb.sender_raw
    assert raw.shape == (G, nodes.shape[1], len(cols)) and raw.is_contiguous()
    assert torch.equal(raw, torch.from_numpy(nodes[..., list(cols)].copy()))
    assert torch.equal(gb.edges_head, torch.from_numpy(edges[..., :4].copy()))
    assert torch.equal(gb.edges_x, torch.from_numpy(edges[..., 4:].copy()))
    with pytest.raises(NotImplementedError):
        GraphBatch(*args).sender_raw


@pytest.mark.parametrize("eid", ["LidarSpread", "LidarOmniTarget"])  # 4-wide and 10-wide edges
def test_graph_batch_of_matches_constructor(eid):
    """GraphBatch.of flattens any leading batch dims of the four fields and takes the agent count, candidate table
    and raw_cols from the env: the same batch as the constructor calls it replaces, for an env-major (B, T) rollout
    (DGPPO._graph_batch), env slices of the (B, T) view of a time-major buffer (DGPPO._graphs) and the last step of
    a (B, T + 1) buffer (DGPPO._last_graph)."""
    from dgppo_fov_amd.env import make_env

    B, T, n = 2, 3, 2
    env = make_env(eid, n, num_obs=2, device="cpu")
    N, E = env.n_nodes, env.n_edges
    assert env.edge_dim == (10 if eid == "LidarOmniTarget" else 4)
    rng = np.random.default_rng(3)

    def fields(*lead):
        return (torch.from_numpy(rng.standard_normal(lead + (N, env.node_dim)).astype(np.float32)),
                torch.from_numpy(rng.standard_normal(lead + (E, env.edge_dim)).astype(np.float32)),
                torch.from_numpy(rng.integers(0, N, lead + (E,)).astype(np.int32)),
                torch.from_numpy(rng.integers(0, N, lead + (E,)).astype(np.int32)))

    def ctor(nodes, edges, recv, send):  # the call every site wrote out
        return GraphBatch(nodes, edges, recv, send, n, env.agent_candidates(torch.device("cpu")),
                          raw_cols=env.nonagent_feature_cols)

    def same(a, b, G):
        for k in ("nodes", "edges", "receivers", "senders"):
            x, y = getattr(a, k), getattr(b, k)
            assert x.is_contiguous() and x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), k
        assert (a.G, a.N, a.E, a.C, a.n) == (b.G, b.N, b.E, b.C, b.n) == (G, N, E, env.agent_candidates().shape[1], n)
        assert a.cand is b.cand and a.raw_cols == b.raw_cols == env.nonagent_feature_cols

    # (B, T, ...) contiguous: the gathered minibatch rows
    f = fields(B, T)
    same(GraphBatch.of(env, *f), ctor(*(x.view(B * T, *x.shape[2:]) for x in f)), B * T)
    # a (T, B) buffer viewed as (B, T), sliced by env: the prepass's env chunks of the engine's rollout
    f = [x.transpose(0, 1) for x in fields(T, B)]
    for sl in (slice(0, 1), slice(1, 2), slice(0, 2)):
        Be = sl.stop - sl.start
        old = ctor(*(x[sl].contiguous().view(Be * T, *x.shape[2:]) for x in f))
        same(GraphBatch.of(env, *(x[sl] for x in f)), old, Be * T)
    # [:, -1] of a (B, T + 1, ...) buffer: the final value's graphs
    f = fields(B, T + 1)
    same(GraphBatch.of(env, *(x[:, -1] for x in f)), ctor(*(x[:, -1] for x in f)), B)
