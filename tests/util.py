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


# Batched trees just past the 8-slot fast path of the traversal kernels (kMaxFast, spgnn_rows.h): in- and out-degrees 9 and 10
# (the general CSC walk) next to degree 8 and degree 1 (the fast path) in the same wave, see
# test_graph.test_past_the_fast_path_batch_layout.
PAST_FAST_PATH_TREES = (
    [8, 7, 6, 8, 0, 2],                         # root 9; children of degree 9, 8, 10, 2, 4
    [],                                         # id 32: a one-node tree (degree 1) beside the next root (degree 10) ...
    [9] + [6, 8, 7, 0] + [0] * 5 + [1],         # ... then 8, 10, 9, 2: a 16-lane wave of degrees 1, 10, 8, 10
    [6, 7],                                     # degree 7 root beside a degree 9 child
    [],
    [7] + [6] * 7,                              # degree 8 throughout
    [],
)


def past_fast_path_batch():
    """-> (list of adjs, per-node degrees) of PAST_FAST_PATH_TREES, batched in order."""
    adjs = [tree_adj_from_child_counts(c) for c in PAST_FAST_PATH_TREES]
    return adjs, np.concatenate([exact_degrees(c) for c in PAST_FAST_PATH_TREES])


def zero_in_degree_edges():
    """(src, dst, n) of a directed graph that is not a tree: nodes without in-edges (among them the last node, whose padded
    neighbour row the host builder clamps to the last edge) and without out-edges, next to nodes of in-degree 1..9."""
    n = 40
    src, dst = [], []
    for v in range(n - 1):
        k = v % 11 - 1                                  # in-degree -1 -> 0, then 0..9 (no self loops)
        for j in range(max(k, 0)):
            src.append((v + 3 + 5 * j) % (n - 1)); dst.append(v)
    return np.array(src, np.int64), np.array(dst, np.int64), n


def star_edges(k: int):
    """(src, dst, n) of a star with k children, self loops included: the root's in- and out-degree is k + 1."""
    s = np.concatenate([np.zeros(k, np.int64), np.arange(1, k + 1), np.arange(k + 1)])
    d = np.concatenate([np.arange(1, k + 1), np.zeros(k, np.int64), np.arange(k + 1)])
    return s, d, k + 1


def oracle_gat(layer, src, dst, n, x, act, dtype=torch.float32, attn_keep=None):
    """The oracle's GATConv (oracle.dgl_cpu.gat_conv) on a copy of ``layer``'s parameters and ``x`` in ``dtype``, as leaves:
    -> (rst (N, H, D), a (E, H) per edge id, x leaf, {name: parameter leaf})."""
    from oracle import dgl_cpu as O
    from spgnn_amd import nn as snn
    sd = {k: v.detach().cpu().to(dtype).requires_grad_(True) for k, v in layer.state_dict().items()}
    xo = x.detach().cpu().to(dtype).requires_grad_(True)
    rst, a = O.gat_conv(src, dst, n, xo, sd["fc.weight"], sd["attn_l"], sd["attn_r"], sd.get("res_fc.weight"),
                        sd.get("bias"), layer.negative_slope, act, attn_keep,
                        residual_identity=isinstance(layer.res_fc, snn.Identity))
    return rst, a, xo, sd


BF16_ULP = 2.0 ** -8       # bf16: 8 significant bits, round to nearest: relative rounding error <= 2^-9, one ulp = 2^-8


def close_to_model(x, ref, what, frac=0.02):
    """x (HIP, bf16 storage) against the bf16 storage model (oracle.dgl_cpu.Bf16Storage): normwise within two bf16 ulp, and all
    but a small fraction of the elements within fp32-accumulation noise of the model (the rest crossed a bf16 rounding
    boundary somewhere upstream).  -> the normwise error max|x - ref| / max|ref|."""
    x, ref = x.detach().float().cpu().double(), ref.detach().double().cpu()
    scale = ref.abs().max().item() or 1.0
    d = (x - ref).abs()
    assert d.max().item() <= 2 * BF16_ULP * scale, (what, d.max().item() / scale)
    off = (d > 1e-4 * scale).double().mean().item()
    assert off <= frac, (what, off)
    return d.max().item() / scale


# Python restatement of the vector GAT kernels' geometry rule (spgnn_rows.h pick_team, spgnn_kernels.hip pick_gat): an (H, D)
# layer runs the instance (T lanes per node, R float4 chunks per lane, CH chunks per head; CH = 0: heads narrower than the
# team), or None: the scalar fallback.  test_graph.test_gat_geometry_rule_covers_every_instance keeps it equal to the library.
def pick_team(width: int, narrow: bool = False):
    if width <= 0 or width & 3:
        return None
    q = width >> 2
    if narrow and q <= 64 and q % 16 == 0 and q // 16 in (1, 2, 4):
        return 16, q // 16
    for t in (64, 32, 16):
        if q % t == 0 and q // t in (1, 2, 4, 8):
            return t, q // t
    return None


def pick_gat(H: int, D: int):
    if D % 4:
        return None
    tr = pick_team(H * D, H in (1, 2))
    if tr is None:
        return None
    T, R = tr
    if D % (4 * T) == 0:
        CH = D // (4 * T)
        return (T, R, CH) if CH in (1, 2, 4, 8) and R % CH == 0 else None
    if (4 * T) % D == 0 and ((D // 4) & (D // 4 - 1)) == 0:
        return T, R, 0
    return None


# One (H, D) per vector GAT instance (the narrowest layer that selects it), plus a scalar-fallback shape last: the geometries of
# the row-kernel tests in test_hip_degree_edges.py.
GAT_INSTANCE_SHAPES = (
    (2, 32), (1, 64), (2, 64), (1, 128), (2, 128), (1, 256),          # 16-lane teams: (16, 1, 0) .. (16, 4, 4)
    (4, 32),                                                           # (32, 1, 0)
    (4, 64), (4, 128), (2, 256), (1, 512),                             # (64, 1, 0) (64, 2, 0..2)
    (8, 128), (4, 256), (2, 512), (1, 1024),                           # (64, 4, 0..4)
    (16, 128), (8, 256), (4, 512), (2, 1024), (1, 2048),               # (64, 8, 0..8)
    (3, 5),                                                            # scalar fallback
)


def gat_raw_inputs(n, H, D, dtype, seed):
    """Random [ft | res] rows (dtype), scores [el | er], bias and output gradient of an (H, D) GATConv traversal."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    y = (torch.randn(n, 2 * H * D, device="cuda", generator=gen)).to(dtype)          # [ft | res]
    s = torch.randn(n, 2 * H, device="cuda", generator=gen)
    bias = torch.randn(H * D, device="cuda", generator=gen) * 0.1
    g_out = torch.randn(n, H * D, device="cuda", generator=gen).to(dtype)
    return y, s, bias, g_out


def run_gat_raw_fp32(csc, y, s, bias, g_out, H, D, act, p, od, score):
    """One forward + backward of the fp32 GAT traversals through ops.gat_fwd_raw / gat_bwd_raw (row or tile kernels, whatever
    ops.tile_plan picks): attention dropout p, the consumer's output dropout od, the score term with ``score``."""
    from spgnn_amd import ops
    HD = H * D
    ft, res = y[:, :HD], y[:, HD:]
    total = HD + 8
    buf = torch.zeros(y.shape[0], total, device="cuda")
    out_drop = (od, 77, total, 4) if od > 0 else None
    out_view = buf[:, 4:4 + HD] if od > 0 else None
    blk = ops.new_scale_block("cuda")
    out, _, attn = ops.gat_fwd_raw(csc, ft, s[:, :H], s[:, H:], res, bias, H, D, 0.2, act, p, 1234, out=out_view, out_drop=out_drop,
                                   out_absmax=blk)
    g_y = torch.zeros_like(y)
    g_s = torch.zeros_like(s)
    blk2 = ops.new_scale_block("cuda")
    al = torch.randn(HD, device="cuda", generator=torch.Generator(device="cuda").manual_seed(3)) if score else None
    ar = torch.randn(HD, device="cuda", generator=torch.Generator(device="cuda").manual_seed(4)) if score else None
    g_e = ops.gat_bwd_raw(csc, ft, s[:, :H], s[:, H:], attn, g_out, out if act != ops.ACT_NONE else None, H, D, 0.2, act, p, 1234,
                          g_y[:, HD:], g_y[:, :HD], g_s[:, :H], g_s[:, H:], absmax=blk2, score_l=al, score_r=ar, out_drop=out_drop)
    return dict(out=out.clone(), attn=attn, g_y=g_y, g_s=g_s, g_e=g_e, blk=blk.clone(), blk2=blk2.clone())


# Python restatement of the J -> template instance rules of the output-head kernels (the launchers in spgnn_gemm.hip and
# spgnn_kernels.hip): the classifier width J rounded up to the next instance, None where the launcher refuses J.
# test_graph.test_head_fold_rule_covers_every_instance keeps them equal to the sources and checks that the shapes of
# test_hip_head_fold.py select every instance.
def fold_instance(J: int):
    """spgnn_linear_mean_fold_fwd / _bwd: JP = 8 / 16 / 24 / 32."""
    return None if not 1 <= J <= 32 else next(jp for jp in (8, 16, 24, 32) if J <= jp)


def act_bwd_proj_instance(J: int):
    """spgnn_act_bwd_proj: JP = 8 / 16 / 24 / 32."""
    return None if not 1 <= J <= 32 else next(jp for jp in (8, 16, 24, 32) if J <= jp)


def act_bwd_proj_wgrad_instance(J: int):
    """spgnn_act_bwd_proj_wgrad: JP = 8 / 16 / 24."""
    return None if not 1 <= J <= 24 else next(jp for jp in (8, 16, 24) if J <= jp)


FOLD_J = (1, 8, 9, 16, 17, 22, 24, 25, 32)          # every instance and both sides of each of its edges
ACT_BWD_PROJ_J = (1, 8, 9, 16, 17, 24, 25, 32)
ACT_BWD_PROJ_WGRAD_J = (1, 8, 9, 16, 17, 24)
