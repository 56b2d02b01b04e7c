"""Distance-preserving and compactness losses on the position stream ``p`` of the SPGNN training step (reference
job_runner.py:1827-1865 ``dist_pos_loss``, on when the settings set ``USE_DIST_LOSS``; the step's loss becomes
``CE + d + 0.1 c``, job_runner.py:1901-1903).

* :class:`PosLossTables` - per loader batch, on the device: per-tree hop-distance tables (uint16), diameters, the "last
  node per label" table and the 64-row block list of the pair kernel (spgnn_pos_loss_tables).  Kept on the graph; on a
  batch arena they are rebuilt into the same storage whenever a batch is loaded, so a captured step replays on them.
* :class:`PosLossState` - the running mean ``M`` of the label rows and its step counter (device tensors), and
  :meth:`PosLossState.run`: d, c, the seed gradient ``g_p`` and the update of ``M`` in two launches (spgnn_pos_losses).
* :func:`reference_pos_losses` - the reference's arithmetic restated in plain torch (CPU, any dtype; autograd gives the
  gradient).  Test and documentation only: the package has no CPU path for the step.

One deliberate difference: the reference fills the statistics rows of labels absent from a tree with unseeded
``torch.rand``.  Here that noise is a counter hash of (seed, step counter, tree, label, column) - :func:`noise` rebuilds it
on the host - so a captured step replays deterministically.
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

__all__ = ["C_WEIGHT", "NUM_LABELS", "PosLossTables", "PosLossState", "pos_losses", "noise", "tree_sizes", "hop_tables_host",
           "reference_pos_losses"]

C_WEIGHT = 0.1          # loss = CE + d + 0.1 * c (job_runner.py:1903)
NUM_LABELS = 21         # labels 1 .. NR_CLASS - 1 (job_runner.py:1835-1840)
ROWS = 64               # rows per block of the pair kernel
_M64 = (1 << 64) - 1


def _mix64(seed: int, idx):
    """spgnn_internal.h mix64 (splitmix64 finaliser over seed + golden * (idx + 1)), vectorised over numpy uint64 ``idx``."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed & _M64) + np.uint64(0x9E3779B97F4A7C15) * (np.asarray(idx, dtype=np.uint64) + np.uint64(1))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def noise(seed: int, step: int, num_trees: int, num_labels: int, D: int) -> np.ndarray:
    """(num_trees, num_labels, D) float32: the uniform [0, 1) rows the kernel uses for absent labels at ``step`` (the
    number of running-mean updates before this one)."""
    s = int(_mix64(seed, np.uint64(step)))
    idx = np.arange(num_trees * num_labels * D, dtype=np.uint64)
    z = _mix64(s, idx)
    return ((z >> np.uint64(40)).astype(np.float64) / 16777216.0).astype(np.float32).reshape(num_trees, num_labels, D)


def tree_sizes(g) -> List[int]:
    """Node counts of ``g``'s trees; on a batch-arena graph the trailing pad component is not a tree."""
    nn = [int(x) for x in g.batch_num_nodes_list]
    if getattr(g, "arena", None) is not None and getattr(g, "num_real_nodes", None) is not None:
        nn = nn[:-1]
    return nn


def hop_tables_host(adj: np.ndarray):
    """Host restatement of the table kernel for one tree: BFS parent / depth from node 0, hop distance of every pair from
    the lowest common ancestor.  -> ((n, n) int64 hop distances, diameter)."""
    a = np.asarray(adj) != 0
    n = a.shape[0]
    depth = np.full(n, -1, dtype=np.int64)
    parent = np.full(n, -1, dtype=np.int64)
    depth[0] = 0
    frontier = [0]
    while frontier:
        nxt = []
        for u in frontier:
            for v in np.nonzero(a[u] | a[:, u])[0]:
                if v != u and depth[v] < 0:
                    depth[v], parent[v] = depth[u] + 1, u
                    nxt.append(int(v))
        frontier = nxt
    if (depth < 0).any():
        raise ValueError("graph is not connected")
    D = np.zeros((n, n), dtype=np.int64)
    for i in range(n):
        for j in range(n):
            x, y, dx, dy = i, j, depth[i], depth[j]
            while dx > dy:
                x, dx = parent[x], dx - 1
            while dy > dx:
                y, dy = parent[y], dy - 1
            while x != y:
                x, y, dx = parent[x], parent[y], dx - 1
            D[i, j] = depth[i] + depth[j] - 2 * dx
    return D, int(D.max())


def reference_pos_losses(p: torch.Tensor, sizes: Sequence[int], hops: Sequence[np.ndarray], y: torch.Tensor,
                         mean: Optional[torch.Tensor], noise_rows: torch.Tensor, num_labels: int = NUM_LABELS):
    """job_runner.py:1827-1865 in plain torch: -> (d, c, new_mean).  ``hops[t]``: (n_t, n_t) hop distances of tree t (its
    diameter is their maximum); ``mean``: the running mean (None on the first step); ``noise_rows``: (B, num_labels, D) -
    the rows of absent labels (the reference's torch.rand, :func:`noise` here)."""
    stats = noise_rows.to(device=p.device, dtype=p.dtype).clone()
    y = y.cpu()
    d_all, c_all = [], []
    off = 0
    for t, n in enumerate(sizes):
        pt, yt = p[off:off + n], y[off:off + n]
        off += n
        mapping = {int(yt[i]): i for i in range(n) if int(yt[i]) != 0}        # the last node per label wins
        keys = sorted(set(range(1, num_labels + 1)) & set(mapping))
        rows = []
        for L in range(1, num_labels + 1):
            if L in mapping:
                stats[t, L - 1] = pt[mapping[L]]
                rows.append(pt[mapping[L]])
        if mean is not None and rows:
            m = mean.to(device=p.device, dtype=p.dtype)
            c = ((torch.stack(rows) - m[torch.as_tensor(keys, device=p.device) - 1]) ** 2).sum()
        else:
            c = p.new_zeros(())
        h = np.asarray(hops[t])
        diam = int(h.max())
        enc = (h.astype(np.float64) / float(diam)).astype(np.float32) if diam > 0 else np.zeros_like(h, dtype=np.float32)
        x = pt.unsqueeze(0).repeat(n, 1, 1)
        z = pt.unsqueeze(1).repeat(1, n, 1)
        aff = torch.exp(-1.0 * torch.abs(x - z).sum(dim=2))
        d_all.append(F.smooth_l1_loss(aff, torch.exp(-torch.from_numpy(enc).to(device=p.device, dtype=p.dtype))))
        c_all.append(c)
    d = torch.stack(d_all).mean()
    c = torch.stack(c_all).mean()
    m = stats.mean(dim=0).detach()
    new_mean = m if mean is None else 0.15 * mean.to(device=p.device, dtype=p.dtype) + 0.85 * m
    return d, c, new_mean


class PosLossTables:
    """Device tables of one batched graph (see the module doc).  Build with :meth:`of` (cached on the graph)."""

    def __init__(self, g, num_labels: int = NUM_LABELS):
        self.device = g.csc().out_indptr.device
        if self.device.type != "cuda":
            raise RuntimeError("pos losses run on a ROCm device (reference_pos_losses is the CPU restatement)")
        self.num_labels = num_labels
        nn = tree_sizes(g)
        self.max_trees = len(nn)
        self.block_cap = int(sum(-(-n // ROWS) for n in nn))
        if getattr(g, "arena", None) is not None:               # every batch of the class fits: sum ceil(n/64) <= N/64 + B
            self.block_cap = int(g.arena.n_cap // ROWS + self.max_trees + 1)
        self.nmax_cap = 0
        self.dist_cap = 0
        self.gen = 0                                             # grows whenever storage had to be re-allocated
        self.g_p_bufs = []                                       # seed-gradient buffers of the steps using these tables
        self._alloc(nn)
        self.load(g)

    @classmethod
    def of(cls, g, num_labels: int = NUM_LABELS) -> "PosLossTables":
        t = g.__dict__.get("_pos_loss_tables")
        if t is None:
            t = g.__dict__["_pos_loss_tables"] = cls(g, num_labels)
            if getattr(g, "_stable_storage", False):
                g._refresh_hooks.append(lambda: t.load(g))
        return t

    def _alloc(self, nn):
        dev, B = self.device, self.max_trees
        need = int(sum(n * n for n in nn))
        self.dist_cap = max(need, int(self.dist_cap * 1.25))
        self.nmax_cap = max(max(nn) if nn else 0, self.nmax_cap)
        self.dist = torch.zeros((max(self.dist_cap, 1),), dtype=torch.int16, device=dev)     # uint16 payload
        i64 = torch.zeros((2 * B + 1,), dtype=torch.int64, device=dev)
        self.tree_ptr, self.dist_off = i64[:B + 1], i64[B + 1:]
        self.diam = torch.zeros((max(B, 1),), dtype=torch.int32, device=dev)
        self.label_node = torch.full((max(B, 1) * self.num_labels,), -1, dtype=torch.int32, device=dev)
        i32 = torch.zeros((2 * self.block_cap + 1,), dtype=torch.int32, device=dev)
        self.blocks, self.num_trees = i32[:2 * self.block_cap], i32[2 * self.block_cap:]
        self.gen += 1

    def load(self, g) -> None:
        """(Re)build the tables of the batch now in ``g`` (into the same storage where it fits)."""
        nn = tree_sizes(g)
        if len(nn) != self.max_trees:
            raise ValueError(f"pos losses: the tables were built for {self.max_trees} trees, the batch has {len(nn)}")
        if any(n > 2048 for n in nn):
            raise ValueError("pos losses: trees of at most 2048 nodes")
        sizes = np.asarray(nn, dtype=np.int64)
        need = int((sizes * sizes).sum())
        if need > self.dist_cap or (sizes.max(initial=0) > self.nmax_cap):
            self._alloc(nn)                                      # new addresses: captures made on the old ones are stale
        ptr = np.concatenate([[0], np.cumsum(sizes)])
        off = np.concatenate([[0], np.cumsum(sizes * sizes)[:-1]]) if len(sizes) else np.zeros(0, np.int64)
        blocks = np.full((self.block_cap, 2), -1, dtype=np.int32)
        q = 0
        for t, n in enumerate(nn):
            for r0 in range(0, n, ROWS):
                blocks[q] = (t, r0)
                q += 1
        assert q <= self.block_cap
        host_i64 = torch.from_numpy(np.concatenate([ptr, off]).astype(np.int64))
        host_i32 = torch.from_numpy(np.concatenate([blocks.reshape(-1), [len(nn)]]).astype(np.int32))
        self.tree_ptr.copy_(host_i64[:self.max_trees + 1])
        self.dist_off.copy_(host_i64[self.max_trees + 1:])
        self.blocks.copy_(host_i32[:-1])
        self.num_trees.copy_(host_i32[-1:])
        for b in self.g_p_bufs:
            b.zero_()
        y = g.ndata["y"]
        if y.dtype != torch.int64 or not y.is_contiguous():
            if getattr(g, "_stable_storage", False):     # a captured step addresses the labels: no per-load copy
                raise ValueError("pos losses on a batch arena need ndata['y'] as a contiguous int64 tensor")
            y = y.to(torch.int64).contiguous()
        self._y = y
        csc = g.csc()
        from . import _capi
        with torch.cuda.device(self.device):
            _capi.check(_capi.load().spgnn_pos_loss_tables(
                csc.out_indptr.data_ptr(), csc.out_indices.data_ptr(), self.tree_ptr.data_ptr(), self.dist_off.data_ptr(),
                self._y.data_ptr(), self.num_labels, self.max_trees, int(sizes.max(initial=0)), self.dist.data_ptr(),
                self.diam.data_ptr(), self.label_node.data_ptr(), torch.cuda.current_stream(self.device).cuda_stream),
                "spgnn_pos_loss_tables")

    def hops(self, t: int) -> np.ndarray:
        """Tree t's (n, n) hop-distance table, read back (tests)."""
        ptr = self.tree_ptr.cpu().numpy()
        off = int(self.dist_off[t])
        n = int(ptr[t + 1] - ptr[t])
        return self.dist[off:off + n * n].cpu().numpy().view(np.uint16).astype(np.int64).reshape(n, n)


class PosLossState:
    """Running mean of the label rows (``cached_mean_pos_enc``, job_runner.py:1522, 1858-1862) and its counter."""

    def __init__(self, D: int, device, seed: int = 0, num_labels: int = NUM_LABELS):
        self.D, self.num_labels = int(D), num_labels
        self.seed = (int(seed) * 0xD1B54A32D192ED03 + 0x8CB92BA72F3D8DD7) & ((1 << 63) - 1)
        self.mean = torch.zeros((num_labels, self.D), dtype=torch.float32, device=device)
        self.state = torch.zeros((2,), dtype=torch.int64, device=device)       # [updates so far, scratch]
        self.losses = torch.zeros((2,), dtype=torch.float32, device=device)    # [d, c] of the last step
        self._bufs = {}

    def _buffers(self, tables: PosLossTables, N: int):
        key = (id(tables), tables.gen, N)
        hit = self._bufs.get(key)
        if hit is None:
            for k in [k for k in self._bufs if k[0] == id(tables)]:
                old = self._bufs.pop(k)[0]
                tables.g_p_bufs[:] = [b for b in tables.g_p_bufs if b is not old]
            g_p = torch.zeros((N, (self.D + 3) // 4 * 4), dtype=torch.float32, device=self.mean.device)[:, :self.D]
            parts = torch.zeros((2 * tables.block_cap,), dtype=torch.float32, device=self.mean.device)
            hit = self._bufs[key] = (g_p, parts, tables)
            tables.g_p_bufs.append(g_p)          # zeroed on every batch load: rows the kernel does not write (pad) stay 0
        return hit[0], hit[1]

    def run(self, tables: PosLossTables, p: torch.Tensor, weight_sum: Optional[torch.Tensor] = None,
            loss_num: Optional[torch.Tensor] = None) -> torch.Tensor:
        """d and c of ``p`` into :attr:`losses`, the running mean updated, ``loss_num += weight_sum * (d + 0.1 c)`` when
        given.  -> g_p = weight_sum * d(d + 0.1 c)/dp (N, D), a buffer reused by later calls on the same tables."""
        from . import _capi
        if p.dim() != 2 or p.shape[1] != self.D or p.dtype != torch.float32 or p.stride(1) != 1:
            raise ValueError(f"p must be (N, {self.D}) float32 with unit column stride")
        N = p.shape[0]
        g_p, parts = self._buffers(tables, N)
        dev = p.device
        with torch.cuda.device(dev):
            _capi.check(_capi.load().spgnn_pos_losses(
                p.data_ptr(), p.stride(0), self.D, tables._y.data_ptr(), tables.tree_ptr.data_ptr(), tables.dist_off.data_ptr(),
                tables.dist.data_ptr(), tables.diam.data_ptr(), tables.label_node.data_ptr(), self.num_labels,
                tables.blocks.data_ptr(), tables.block_cap, tables.num_trees.data_ptr(), tables.max_trees, tables.nmax_cap,
                self.mean.data_ptr(), self.state.data_ptr(), self.seed, weight_sum.data_ptr() if weight_sum is not None else None,
                C_WEIGHT, g_p.data_ptr(), g_p.stride(0), parts.data_ptr(), loss_num.data_ptr() if loss_num is not None else None,
                self.losses.data_ptr(), torch.cuda.current_stream(dev).cuda_stream), "spgnn_pos_losses")
        return g_p

    def state_dict(self) -> dict:
        return {"mean": self.mean.detach().cpu().clone(), "updates": int(self.state[0].item()), "seed": self.seed}

    def load_state_dict(self, sd: dict) -> None:
        self.mean.copy_(sd["mean"].to(self.mean.device, torch.float32))
        self.state[0].fill_(int(sd["updates"]))
        self.seed = int(sd.get("seed", self.seed))


def pos_losses(g, p: torch.Tensor, state: PosLossState, weight_sum: Optional[torch.Tensor] = None,
               loss_num: Optional[torch.Tensor] = None):
    """The op: -> (d, c, g_p) for the position-stream output ``p`` of batched graph ``g`` (d, c: device scalars, views of
    ``state.losses``; g_p with ``weight_sum`` folded in, 1 when None).  Updates ``state``'s running mean."""
    g_p = state.run(PosLossTables.of(g, state.num_labels), p, weight_sum, loss_num)
    return state.losses[0], state.losses[1], g_p
