"""Shared helpers for the parity tests."""
import numpy as np
import torch


def rel_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """Normwise relative error max|a-b| / max|b| (the 1e-5 bar of BASELINE.json.north_star)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    denom = b.abs().max().item()
    return (a - b).abs().max().item() / (denom if denom > 0 else 1.0)


def mixed_err(a: torch.Tensor, b: torch.Tensor) -> float:
    """Elementwise mixed error max_i |a_i - b_i| / (|b_i| + rms(b)): a value of e means every element satisfies
    |a - b| <= e * |b| + e * rms(b) - small elements are held to the tensor's typical magnitude, not to its maximum
    (the normwise ``rel_err`` says nothing about them)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    rms = b.pow(2).mean().sqrt().item()
    return ((a - b).abs() / (b.abs() + (rms if rms > 0 else 1.0))).max().item()


def keep_scale_host(seed: int, idx: np.ndarray, p: float) -> np.ndarray:
    """Bit-exact host copy of the kernels' counter-based attention-dropout mask
    (spgnn_kernels.hip keep_scale): returns 1/(1-p) where kept, 0 where dropped."""
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx.astype(np.uint64) + np.uint64(1))) & M
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M
        z = z ^ (z >> np.uint64(31))
    u = (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.where(u >= np.float32(p), np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0)).astype(np.float32)


def keep4_scale_host(seed: int, N: int, widths, p: float) -> np.ndarray:
    """Host copy of spgnn_cat_dropout's mask for sources of the given widths: one 64-bit hash per group of four
    columns of a source, 16 bits per element."""
    total = int(sum(widths))
    out = np.zeros((N, total), dtype=np.float32)
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    thr = np.uint64(int(np.float32(p) * np.float32(65536.0)))
    rows = np.arange(N, dtype=np.int64)[:, None]
    off = 0
    for w in widths:
        c = np.arange(0, w, 4, dtype=np.int64)[None, :]
        idx = (rows * total + off + c).astype(np.uint64)
        with np.errstate(over="ignore"):
            z = (np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx + np.uint64(1))) & M
            z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M
            z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M
            z = z ^ (z >> np.uint64(31))
        for j in range(4):
            cols = off + c[0] + j
            ok = cols < off + w
            bits = (z >> np.uint64(16 * j)) & np.uint64(0xFFFF)
            out[:, cols[ok]] = np.where(bits[:, ok] >= thr, np.float32(1.0) / (np.float32(1.0) - np.float32(p)), np.float32(0.0))
        off += w
    return out


def spgnn_host_masks(plan, model, g):
    """The dropout multipliers of ONE training-mode forward of GATPSPGNN, rebuilt on the host from the forward's own seed plan
    (spgnn_amd.models.GATPSPGNN._seed_plan: per level the next structure layer's feature dropout over cat[h_s, h_p], the
    structure / position layer's attention dropout, the next position layer's feature dropout) with the bit-exact host
    copies of the kernels' counter hashes (above) - in the oracle's layout: {(kind, stream, layer): multiplier}."""
    csc = g.csc()
    N, E = g.number_of_nodes(), csc.num_edges
    eid = csc.eid.cpu().numpy()
    head = model.gat
    drop = {}

    def attn(seed, H, p):
        slot = keep_scale_host(seed, np.arange(E * H), p).reshape(E, H)          # CSC slot order -> edge-id order
        edge = np.empty_like(slot)
        edge[eid] = slot
        return torch.from_numpy(edge)
    for l, d in enumerate(plan):
        s_layer, p_layer = head.gat_layers[l], head.pgnn_layers[l]
        w_s, w_p = s_layer._num_heads * s_layer._out_feats, p_layer._num_heads * p_layer._out_feats
        if d["fp"] > 0:
            drop[("feat", "s", l + 1)] = torch.from_numpy(keep4_scale_host(d["fseed"], N, (w_s, w_p), d["fp"]))
        if d["ps"] > 0:
            drop[("attn", "s", l)] = attn(d["seed_s"], s_layer._num_heads, d["ps"])
        if d["pp"] > 0:
            drop[("attn", "p", l)] = attn(d["seed_p"], p_layer._num_heads, d["pp"])
        if d["fp2"] > 0:
            drop[("feat", "p", l + 1)] = torch.from_numpy(keep4_scale_host(d["fseed2"], N, (w_p,), d["fp2"]))
    return drop


def tree_batch_edges(ns, seed=0):
    from spgnn_amd import synthetic
    from spgnn_amd.graph import edges_from_adj
    rng = np.random.default_rng(seed)
    srcs, dsts, off = [], [], 0
    for n in ns:
        u, v = edges_from_adj(synthetic.random_tree_adj(n, rng))
        srcs.append(u + off); dsts.append(v + off); off += n
    return np.concatenate(srcs), np.concatenate(dsts), off


def mix64_host(seed: int, idx: np.ndarray) -> np.ndarray:
    """Host copy of the kernels' counter hash (spgnn_kernels.hip mix64)."""
    M = np.uint64(0xFFFFFFFFFFFFFFFF)
    with np.errstate(over="ignore"):
        z = (np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * (idx.astype(np.uint64) + np.uint64(1))) & M
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & M
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & M
        return z ^ (z >> np.uint64(31))


def sample_neighbors_host(indptr, indices, eid, seeds, fanout, seed):
    """Bit-exact host copy of spgnn_sample_neighbors (selection sampling over the CSC slots of every seed):
    returns (src parent ids, parent edge ids, per-seed counts), edges grouped by seed."""
    src, eids, cnt = [], [], []
    for v in seeds:
        b, d = int(indptr[v]), int(indptr[v + 1] - indptr[v])
        k = d if fanout is None or fanout < 0 or fanout > d else fanout
        r = (mix64_host(seed, np.arange(b, b + d, dtype=np.int64)) >> np.uint64(32)).astype(np.uint64)
        m = 0
        for i in range(d):
            if m >= k:
                break
            left, need = d - i, k - m
            take = need >= left or int((int(r[i]) * left) >> 32) < need
            if take:
                src.append(int(indices[b + i])); eids.append(int(eid[b + i])); m += 1
        cnt.append(m)
    return np.array(src, np.int64), np.array(eids, np.int64), np.array(cnt, np.int64)


def tree_adj_from_child_counts(counts) -> np.ndarray:
    """adj (n, n) uint8 = I + A + A^T of the tree whose node i (breadth-first ids, root 0) has ``counts[i]`` children; nodes
    past the end of ``counts`` are leaves.  With the self loop every node's in- and out-degree is then exactly
    counts[i] + 1 (+ 1 for its parent unless it is the root)."""
    n = 1 + int(sum(counts))
    adj = np.eye(n, dtype=np.uint8)
    nxt = 1
    for i, c in enumerate(counts):
        if i >= nxt:
            raise ValueError(f"child counts leave node {i} unreached")
        adj[i, nxt:nxt + c] = 1
        adj[nxt:nxt + c, i] = 1
        nxt += c
    return adj


def exact_degrees(counts) -> np.ndarray:
    """The in- (= out-) degrees tree_adj_from_child_counts(counts) gives its nodes, self loop included."""
    n = 1 + int(sum(counts))
    c = np.zeros(n, dtype=np.int64)
    c[:len(counts)] = counts
    return c + 1 + (np.arange(n) > 0)


# Batched trees at the degree edges of the fused SPGNN level (spgnn_lspe.hip: 1 <= degree <= 8 in both directions), as
# breadth-first child counts per tree.  [] is a one-node tree: its only edge is the self loop (degree 1; in a tree of two or
# more nodes every node has a neighbour besides itself).  The layout puts degrees 1 and 8 side by side in the teams of one
# wave at every team width (the kernels' __any(k0 < deg) exit), see test_graph.test_degree_edge_batch_layout.
DEGREE_EDGE_TREES = (
    [7] + [6] * 7,                              # root: 7 children; its children: parent + 6 children; all + self loop = 8
    [],                                         # ids 50 (degree 1), 51 (the next root, degree 8) share a 32-lane wave
    [7] + [6, 0, 5, 1, 4, 2, 3] * 3,            # consecutive ids of degree 8, 8, 2, 7, 3, 6, 4, 5, ...
    [], [],
    [1, 0],                                     # a two-node tree: degree 2 + 2
    [],
    [3, 6, 6, 6] + [0, 1] * 5,
    [],
)


def degree_edge_batch():
    """-> (list of adjs, per-node degrees) of DEGREE_EDGE_TREES, batched in order."""
    adjs = [tree_adj_from_child_counts(c) for c in DEGREE_EDGE_TREES]
    return adjs, np.concatenate([exact_degrees(c) for c in DEGREE_EDGE_TREES])
