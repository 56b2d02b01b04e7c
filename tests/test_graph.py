"""Host-side graph construction and positional encoding: bit-exact against the networkx
restatement of the reference's rule (oracle/graph_rule_nx.py; reference job_runner.py:1319-1344,
1712-1801, 1882)."""
import re

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import graph_rule_nx as R
from spgnn_amd import graph as G
from spgnn_amd import posenc, synthetic


def _trees(ns, seed=0):
    rng = np.random.default_rng(seed)
    return [synthetic.random_tree_adj(n, rng) for n in ns]


@pytest.mark.parametrize("n", [1, 2, 3, 21, 128, 177])
def test_edge_rule_matches_networkx(n):
    adj = _trees([n], seed=n)[0]
    u, v = G.edges_from_adj(adj)
    ru, rv = R.edges_spgnn(adj)
    assert np.array_equal(u, ru) and np.array_equal(v, rv)
    gu, gv = R.edges_gcn(adj)               # the GCN/GAT runner's path yields the same list
    assert np.array_equal(u, gu) and np.array_equal(v, gv)
    assert u.shape[0] == 3 * n - 2          # E = 3n - 2


def test_dglgraph_from_networkx_then_add_self_loops():
    adj = _trees([40], seed=3)[0]
    Gd = nx.DiGraph(adj)
    g = G.DGLGraph(Gd)
    g = G.remove_self_loop(g)
    g.add_edges(g.nodes(), g.nodes())
    u, v = R.edges_spgnn(adj)
    assert np.array_equal(g._src, u) and np.array_equal(g._dst, v)
    Gu = nx.Graph(adj); Gu.remove_edges_from(nx.selfloop_edges(Gu))
    g2 = G.DGLGraph(Gu); g2.add_edges(g2.nodes(), g2.nodes())
    assert np.array_equal(g2._src, u) and np.array_equal(g2._dst, v)


def test_batch_offsets_and_csc_bit_exact():
    adjs = _trees([5, 1, 33, 150, 2], seed=5)
    graphs = [G.graph_from_adj(a) for a in adjs]
    for i, g in enumerate(graphs):
        g.ndata["fvs"] = torch.full((g.number_of_nodes(), 3), float(i))
    bg = G.batch(graphs)
    rs, rd = R.batch_edges([R.edges_spgnn(a) for a in adjs], [a.shape[0] for a in adjs])
    assert np.array_equal(bg._src, rs) and np.array_equal(bg._dst, rd)
    assert bg.batch_size == 5 and bg.batch_num_nodes_list == [5, 1, 33, 150, 2]
    assert bg.batch_num_edges_list == [3 * n - 2 for n in (5, 1, 33, 150, 2)]
    assert torch.equal(bg.ndata["fvs"][:, 0], torch.cat([torch.full((a.shape[0],), float(i)) for i, a in enumerate(adjs)]))
    csc = G.build_csc_numpy(bg._src, bg._dst, bg.number_of_nodes())
    indptr, indices, eid = R.csc_stable(rs, rd, bg.number_of_nodes())
    assert np.array_equal(csc["indptr"], indptr) and np.array_equal(csc["indices"], indices)
    assert np.array_equal(csc["eid"], eid)
    # CSR side + slot map: edge k of out-list of u is (u -> out_indices[k]) stored at CSC slot out_pos[k]
    for u in range(bg.number_of_nodes()):
        for k in range(csc["out_indptr"][u], csc["out_indptr"][u + 1]):
            slot = csc["out_pos"][k]
            v = csc["out_indices"][k]
            assert csc["indices"][slot] == u and csc["indptr"][v] <= slot < csc["indptr"][v + 1]
    # in-neighbour order of v: ascending tree neighbours, then v itself
    for v in range(bg.number_of_nodes()):
        nb = csc["indices"][csc["indptr"][v]:csc["indptr"][v + 1]]
        assert nb[-1] == v and np.all(np.diff(nb[:-1]) > 0)


def test_unbatch_round_trip_and_edge_cases():
    adjs = _trees([7, 30, 4], seed=6)
    graphs = [G.graph_from_adj(a) for a in adjs]
    for g in graphs:
        g.ndata["y"] = torch.arange(g.number_of_nodes())
    parts = G.unbatch(G.batch(graphs))
    for a, b in zip(graphs, parts):
        assert np.array_equal(a._src, b._src) and np.array_equal(a._dst, b._dst)
        assert torch.equal(a.ndata["y"], b.ndata["y"])
    with pytest.raises(ValueError):
        G.batch([])
    with pytest.raises(ValueError):
        graphs[0].ndata["bad"] = torch.zeros(3)
    with pytest.raises(ValueError):
        graphs[0].add_edges([0], [999])
    e = G.TreeGraph(None, 0)                     # empty graph
    assert e.number_of_nodes() == 0 and e.number_of_edges() == 0
    assert G.build_csc_numpy(e._src, e._dst, 0)["indptr"].tolist() == [0]
    assert int(graphs[1].in_degrees().sum()) == graphs[1].number_of_edges()


def test_to_networkx_and_adjacency():
    adj = _trees([12], seed=8)[0]
    g = G.graph_from_adj(adj, add_self_loops=False)
    Gx = G.to_networkx(g)
    assert sorted(Gx.edges()) == sorted(zip(g._src.tolist(), g._dst.tolist()))
    A = g.adjacency_matrix().to_dense().numpy()
    ref = adj.astype(np.float32) - np.eye(12, dtype=np.float32)
    assert np.array_equal(A, ref)
    assert np.array_equal(g.adjacency_matrix(scipy_fmt="csr").toarray(), ref)


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_positional_encoding_matches_networkx(seed):
    rng = np.random.default_rng(100 + seed)
    s = synthetic.synthetic_tree(int(rng.integers(30, 160)), rng)
    a1 = posenc.anchors_from_cnn_prediction(s["fvs_out"], s["adj"], 39)
    a2 = R.anchors_from_cnn_prediction(s["fvs_out"], s["adj"], 39)
    assert a1 == a2 and len(a1) == 39
    pe1, d1 = posenc.distance_pos_enc(s["adj"], a1)
    pe2, d2 = R.distance_pos_enc(s["adj"], a2)
    assert d1 == d2
    assert np.array_equal(pe1, pe2) and pe1.dtype == np.float32 and pe1.shape == (s["adj"].shape[0], 39)
    assert posenc.anchors_from_cnn_prediction(s["fvs_out"], s["adj"], 21) == a1[:21]


def test_synthetic_workload_shape():
    samples = synthetic.synthetic_trees(4, rank=0)
    again = synthetic.synthetic_trees(4, rank=0)
    other = synthetic.synthetic_trees(4, rank=1)
    for a, b in zip(samples, again):
        assert all(np.array_equal(a[k], b[k]) for k in a)              # seeded, reproducible
    assert not np.array_equal(samples[0]["fvs"][:50], other[0]["fvs"][:50])
    for s in samples:
        n = s["adj"].shape[0]
        assert 120 <= n <= 180 and s["fvs"].shape == (n, 1024) and s["fvs_out"].shape == (n, 22)
        assert (s["fvs"] >= 0).all() and s["adj"].dtype == np.uint8
        up = np.triu(s["adj"], 1)
        assert (up.sum(0)[1:] == 1).all() and up.sum(1).max() <= 3      # one parent < child, fan-out <= 3
        assert sorted(s["labels"][s["labels"] > 0].tolist()) == list(range(1, 22))
    bg = synthetic.batch_from_samples(samples)
    assert bg.ndata["pos_enc"].shape == (bg.number_of_nodes(), 39)
    assert bg.number_of_edges() == 3 * bg.number_of_nodes() - 2 * 4


def test_tree_downstream_graph_mode_follows_the_reference_rule():
    """GRAPH_MODE == "tree_downstream" (reference job_runner.py:1334-1336: nx.DiGraph(np.triu(adj)), self loops removed, then
    g.add_edges(nodes, nodes)): parent -> child edges only.  Bit-exact against the networkx restatement, for symmetric trees
    and for an adjacency matrix that is already upper triangular (job_runner.py:1329-1332: the same directed graph in either
    mode); no config of the reference selects it, the boundary still has it."""
    from oracle import graph_rule_nx as R
    rng = np.random.default_rng(3)
    for n in (1, 2, 7, 33, 150):
        adj = synthetic.random_tree_adj(n, rng)
        u, v = G.edges_from_adj(adj, graph_mode="tree_downstream")
        ru, rv = R.edges_gcn(adj, "tree_downstream")
        assert np.array_equal(u, ru) and np.array_equal(v, rv)
        assert u.shape[0] == 2 * n - 1 and (u <= v).all()                  # n - 1 parent -> child edges + n self loops
        tri = np.triu(adj)
        for mode in G.GRAPH_MODES:
            u2, v2 = G.edges_from_adj(tri, graph_mode=mode)
            ru2, rv2 = R.edges_gcn(tri, mode)
            assert np.array_equal(u2, ru2) and np.array_equal(v2, rv2) and np.array_equal(u2, u)
    with pytest.raises(ValueError):
        G.edges_from_adj(np.eye(3), graph_mode="upstream")
    g = G.graph_from_adj(synthetic.random_tree_adj(20, rng), graph_mode="tree_downstream")
    assert g.number_of_edges() == 39


def test_degree_edge_batch_layout():
    """tests/util.DEGREE_EDGE_TREES (the fused SPGNN level's degree edges, test_hip_lspe.py): the degrees the builder promises
    are the graph's, in both directions, with the statistics the host checks before it picks the fused kernels; every degree
    1..8 occurs; degree 1 sits next to degree 8 inside one wave of 16- and of 32-lane teams (4 and 2 nodes per wave), a 16-lane
    wave holds four different degrees, and N leaves a partial last block (16, 8 or 4 nodes per block)."""
    from tests.util import DEGREE_EDGE_TREES, degree_edge_batch, exact_degrees, tree_adj_from_child_counts
    adjs, deg = degree_edge_batch()
    g = G.batch([G.graph_from_adj(a) for a in adjs])
    N = g.number_of_nodes()
    assert N == deg.shape[0] and N % 16 != 0
    csc = g.csc()
    assert np.array_equal((csc.indptr[1:] - csc.indptr[:-1]).numpy(), deg)
    assert np.array_equal((csc.out_indptr[1:] - csc.out_indptr[:-1]).numpy(), deg)
    assert (csc.min_in_degree, csc.max_in_degree, csc.min_out_degree, csc.max_out_degree) == (1, 8, 1, 8)
    assert set(deg.tolist()) == set(range(1, 9))
    for per in (4, 2):
        waves = [set(deg[i:i + per].tolist()) for i in range(0, N, per)]
        assert any({1, 8} <= w for w in waves), per
    assert any(len(set(deg[i:i + 4].tolist())) == 4 for i in range(0, N, 4))
    for c in DEGREE_EDGE_TREES:                    # each tree: a tree (n - 1 undirected edges, connected) of the promised degrees
        a = tree_adj_from_child_counts(c)
        n = a.shape[0]
        assert np.array_equal(a, a.T) and np.all(np.diag(a) == 1) and (a.sum() - n) == 2 * (n - 1)
        assert np.array_equal(a.sum(0), exact_degrees(c))
        assert nx.is_connected(nx.from_numpy_array(a))
    with pytest.raises(ValueError):
        tree_adj_from_child_counts([1, 0, 2])      # node 2 is never reached
    # past the fast path (test_hip_degree_edges.py): degrees 9 and 10 in both directions, in a 16-lane wave and a 32-lane wave
    # with degree 1, and in a 16-lane wave with degree 8
    from tests.util import PAST_FAST_PATH_TREES, past_fast_path_batch, star_edges, zero_in_degree_edges
    adjs, deg = past_fast_path_batch()
    g = G.batch([G.graph_from_adj(a) for a in adjs])
    N = g.number_of_nodes()
    csc = g.csc()
    assert N == deg.shape[0] and N % 16 != 0
    assert np.array_equal((csc.indptr[1:] - csc.indptr[:-1]).numpy(), deg)
    assert np.array_equal((csc.out_indptr[1:] - csc.out_indptr[:-1]).numpy(), deg)
    assert (csc.min_in_degree, csc.max_in_degree, csc.min_out_degree, csc.max_out_degree) == (1, 10, 1, 10)
    assert {1, 2, 8, 9, 10} <= set(deg.tolist())
    assert any({1, 10} <= set(deg[i:i + 2].tolist()) for i in range(0, N, 2))
    assert any({1, 8, 10} <= set(deg[i:i + 4].tolist()) for i in range(0, N, 4))
    assert any({8, 9} <= set(deg[i:i + 4].tolist()) for i in range(0, N, 4))
    for c in PAST_FAST_PATH_TREES:
        a = tree_adj_from_child_counts(c)
        assert np.array_equal(a.sum(0), exact_degrees(c)) and nx.is_connected(nx.from_numpy_array(a))
    # zero in-degree (not a tree): in-degrees 0..9, zero-degree nodes beside degree-9 ones, the last node isolated
    s, d, n = zero_in_degree_edges()
    csc = G.TreeGraph((s, d), n).csc()
    ind = (csc.indptr[1:] - csc.indptr[:-1]).numpy()
    outd = (csc.out_indptr[1:] - csc.out_indptr[:-1]).numpy()
    assert set(ind.tolist()) == set(range(10)) and ind[-1] == 0 and outd[-1] == 0 and (outd == 0).sum() == 1
    assert any(ind[i] == 9 and ind[i + 1] == 0 for i in range(n - 1))
    assert csc.min_in_degree == 0 and csc.max_in_degree == 9
    # stars on either side of the one-byte argmax limit (in-degree <= 254)
    for k, root in ((253, 254), (254, 255)):
        s, d, n = star_edges(k)
        csc = G.TreeGraph((s, d), n).csc()
        ind = (csc.indptr[1:] - csc.indptr[:-1]).numpy()
        assert ind[0] == root and csc.max_in_degree == root and csc.max_out_degree == root and (ind[1:] == 2).all()


def test_gat_geometry_rule_covers_every_instance(lib):
    """tests/util.pick_gat restates the vector GAT kernels' geometry rule (spgnn_rows.h pick_team, spgnn_kernels.hip pick_gat):
    it agrees with the library's host queries over a grid of shapes, every instance it reaches is a case of SPGNN_FOR_R_CH (teams
    narrower than a wave only with R <= 4: launch_small_team has no other instances), and the row-kernel shapes of
    test_hip_degree_edges.py select every instance plus the scalar fallback.  A change to the dispatch fails here rather than
    leaving an instance untested."""
    import os
    import re
    from tests.util import GAT_INSTANCE_SHAPES, pick_gat, pick_team
    src = open(os.path.join(os.path.dirname(G.__file__), "csrc", "spgnn_kernels.hip")).read()
    macro = src[src.index("#define SPGNN_FOR_R_CH"):]
    macro = macro[:macro.index("default:")]
    cases = {(int(a), int(b)) for a, b in re.findall(r"X\((\d+), (\d+)\)", macro)}
    assert len(cases) == 14
    reached = set()
    for H in range(1, 17):
        for D in range(1, 2049):
            inst = pick_gat(H, D)
            assert bool(lib.spgnn_gat_can_fuse_mean(H, D)) == (inst is not None and inst[2] >= 1), (H, D)
            if inst is not None:
                T, R, CH = inst
                assert (R, CH) in cases and T in (16, 32, 64) and (T == 64 or R <= 4), (H, D, inst)
                assert H * D == 4 * T * R
                reached.add(inst)
    for F_ in range(1, 2049):
        assert bool(lib.spgnn_spmm_max_u8_supported(F_)) == (pick_team(F_, True) is not None), F_
    assert {(R, CH) for _, R, CH in reached} == cases                       # no dead case in the switch
    tested = [pick_gat(H, D) for H, D in GAT_INSTANCE_SHAPES]
    assert set(tested) - {None} == reached and None in tested, sorted(reached - set(tested))
    assert len(reached) == 20


def _launcher_rule(src: str, fn: str, kernel: str, limit: str):
    """The J -> instance rule of launcher ``fn`` as its source writes it: the ``J <= n`` chain, the instance each branch launches
    (``kernel``: a regex whose group is the instance) and the largest J it accepts (``limit``: the regex of its refusal)."""
    body = src[src.index(f"\nint {fn}(") if f"\nint {fn}(" in src else src.index(f"\nstatic int {fn}("):]
    body = body[:body.index("\n}\n")]
    cuts = [int(n) for n in re.findall(r"if \(J <= (\d+)\)", body)]
    insts = [int(n) for n in re.findall(kernel, body)]
    top = int(re.search(limit, body).group(1))
    assert len(insts) == len(cuts) + 1 and cuts == sorted(cuts) and top > cuts[-1], (fn, cuts, insts, top)
    return lambda J: None if not 1 <= J <= top else next((i for c, i in zip(cuts, insts) if J <= c), insts[-1])


def test_head_fold_rule_covers_every_instance():
    """tests/util.fold_instance / act_bwd_proj_instance / act_bwd_proj_wgrad_instance restate the classifier-width dispatch of
    spgnn_linear_mean_fold_fwd / _bwd (spgnn_gemm.hip), spgnn_act_bwd_proj and spgnn_act_bwd_proj_wgrad (spgnn_kernels.hip): they
    agree with the launchers' sources, and the widths test_hip_head_fold.py runs select every instance of each, with J on both
    sides of every edge.  A change to a dispatch rule fails here rather than leaving an instance untested."""
    import os
    from tests.util import (ACT_BWD_PROJ_J, ACT_BWD_PROJ_WGRAD_J, FOLD_J, act_bwd_proj_instance, act_bwd_proj_wgrad_instance,
                            fold_instance)
    csrc = os.path.join(os.path.dirname(G.__file__), "csrc")
    gemm = open(os.path.join(csrc, "spgnn_gemm.hip")).read()
    kern = open(os.path.join(csrc, "spgnn_kernels.hip")).read()
    kfoldj = re.search(r"constexpr int kFoldJ = (\d+);", gemm).group(1)   # the fold launchers refuse J > gemm::kFoldJ
    gemm = gemm.replace("gemm::kFoldJ", kfoldj)
    cases = [
        (gemm, "spgnn_linear_mean_fold_fwd", r"linear_mean_fold_fwd_kernel<(\d+)>", r"J > (\d+)",
         fold_instance, FOLD_J),
        (gemm, "spgnn_linear_mean_fold_bwd", r"linear_mean_fold_bwd_kernel<(\d+)>", r"J > (\d+)",
         fold_instance, FOLD_J),
        (kern, "act_bwd_proj_launch", r"X\((\d+)\)", r"J > (\d+)", act_bwd_proj_instance, ACT_BWD_PROJ_J),
        (kern, "spgnn_act_bwd_proj_wgrad", r"X\((\d+)\)", r"J > (\d+)", act_bwd_proj_wgrad_instance, ACT_BWD_PROJ_WGRAD_J),
    ]
    for src, fn, kernel, limit, rule, tested in cases:
        lib_rule = _launcher_rule(src, fn, kernel, limit)
        assert [lib_rule(J) for J in range(0, 41)] == [rule(J) for J in range(0, 41)], fn
        every = {rule(J) for J in range(1, 41)} - {None}
        assert {rule(J) for J in tested} == every, (fn, sorted(every))
        for jp in every:                                                   # both sides of every edge between instances
            if rule(jp + 1) is not None:
                assert jp in tested and jp + 1 in tested, (fn, jp)
        assert 1 in tested and max(J for J in range(1, 41) if rule(J) is not None) in tested, fn
