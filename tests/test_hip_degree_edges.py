"""The neighbour traversals of spgnn_kernels.hip and spgnn_tile.hip at the degree edges of their 8-slot fast path (kMaxFast,
spgnn_rows.h: nodes of 1..8 edges load all eight slots unconditionally, padded slots re-read the last edge with weight 0; every
other degree walks the CSC), against the fp64 oracle.  The airway trees of the other tests stay at degrees 2..5.

Fixtures (tests/util.py): DEGREE_EDGE_TREES (degrees 1..8 exact, 1 beside 8 in one wave), PAST_FAST_PATH_TREES (9 and 10 beside
8 and 1), a zero-in-degree graph (in-degrees 0..9, the last node isolated) and stars of 253 / 254 children (root in-degree 254 /
255: either side of the one-byte argmax of spmm_max).  Tolerances are those of test_hip_layers.py (fp32: 1e-5 forward, 5e-5
gradients) and test_hip_bf16.py (bf16 storage model: two ulp normwise, at most 2 % of the elements off)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dgl_cpu as O
from spgnn_amd import graph as G
from spgnn_amd import nn as snn
from spgnn_amd import ops, ops_bf16
from tests.util import (GAT_INSTANCE_SHAPES, close_to_model, degree_edge_batch, keep4_scale_host, keep_scale_host, oracle_gat,
                        past_fast_path_batch, pick_gat, rel_err, run_gat_raw_fp32, gat_raw_inputs, star_edges,
                        zero_in_degree_edges)

pytestmark = pytest.mark.gpu
FWD_TOL, GRAD_TOL = 1e-5, 5e-5
P_ATTN, SEED = 0.1, 0x5EED5EED


def _fixture(name):
    """-> (TreeGraph on the device, src, dst (int64 CPU tensors, edge-id order), N)."""
    if name in ("degree_edge", "past_fast_path"):
        adjs, _ = (degree_edge_batch if name == "degree_edge" else past_fast_path_batch)()
        g = G.batch([G.graph_from_adj(a) for a in adjs])
        s, d = g.edges()
        s, d, n = np.asarray(s, np.int64), np.asarray(d, np.int64), g.number_of_nodes()
    elif name == "zero_in_degree":
        s, d, n = zero_in_degree_edges()
        g = G.TreeGraph((s, d), n)
    else:
        s, d, n = star_edges(int(name.split("_")[1]))
        g = G.TreeGraph((s, d), n)
    return g.to("cuda"), torch.as_tensor(s), torch.as_tensor(d), n


FIXTURES = ("degree_edge", "past_fast_path", "zero_in_degree", "star_253", "star_254")


def _keep_edge(csc, H):
    """The kernels' attention-dropout multipliers (CSC slot order on the device) in edge-id order, as the oracle takes them."""
    E = csc.num_edges
    slot = keep_scale_host(SEED, np.arange(E * H), P_ATTN).reshape(E, H)
    edge = np.empty_like(slot)
    edge[csc.eid.cpu().numpy()] = slot
    return torch.from_numpy(edge)


def _check_gat_layer(layer, g, src, dst, n, x, act, mean, monkeypatch, bf16=False):
    """One training-mode forward (attention dropout on, fixed seed) + backward of ``layer`` against fp64: output, the returned
    attention per edge id (attn_drop(edge_softmax), what was aggregated), the input and every parameter gradient.
    -> {what: normwise error}."""
    monkeypatch.setattr(snn, "_draw_seed", lambda: SEED)
    H, D = layer._num_heads, layer._out_feats
    csc = g.csc()
    keep = _keep_edge(csc, H)
    xg = (ops_bf16.cast_rows(x) if bf16 else x.clone()).requires_grad_(True)
    layer.zero_grad()
    out, a_ret = layer(g, xg, get_attention=True, mean_heads=mean)
    cot = torch.randn(out.shape, generator=torch.Generator().manual_seed(H * 1000 + D))
    cot = cot.to(torch.bfloat16).float() if out.dtype == torch.bfloat16 else cot
    (out.float() * cot.cuda()).sum().backward()
    errs = {}
    if not bf16:
        ref, a_ref, xo, sd = oracle_gat(layer, src, dst, n, x, act, torch.float64, attn_keep=keep)
        ref = ref.mean(1) if mean else ref
        (ref * cot.double()).sum().backward()
        errs["out"] = rel_err(out, ref)
        assert errs["out"] < FWD_TOL, errs
        errs["attn"] = rel_err(a_ret.squeeze(-1), a_ref * keep.double())
        assert errs["attn"] < FWD_TOL, errs
        errs["g_x"] = rel_err(xg.grad, xo.grad)
        for name, p in layer.named_parameters():
            errs[name] = rel_err(p.grad, sd[name].grad)
        assert max(v for k, v in errs.items() if k not in ("out", "attn")) < GRAD_TOL, errs
        return errs
    # bf16 rows: the storage model (fp64 arithmetic, bf16 rounding at the storage points), as test_hip_bf16.py
    fused = mean and ops.can_fuse_mean(H, D)
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in layer.state_dict().items()}
    x64 = x.detach().cpu().to(torch.bfloat16).double().requires_grad_()
    r, a_ref = O.gat_conv(src, dst, n, x64, sd["fc.weight"], sd["attn_l"], sd["attn_r"], sd.get("res_fc.weight"), sd["bias"], 0.2,
                          act, keep.double(), residual_identity=isinstance(layer.res_fc, snn.Identity), storage=O.Bf16Storage,
                          store_out=not fused)
    r = r.mean(1) if mean else r.flatten(1)
    if mean and not fused:
        r = O.Bf16Storage.store(r)
    r.backward(cot.double().reshape(r.shape))
    errs["out"] = close_to_model(out.reshape(r.shape), r, "out")
    errs["attn"] = close_to_model(a_ret.squeeze(-1), a_ref * keep.double(), "attn")    # scores from the product's fp32 accumulators
    errs["g_x"] = close_to_model(xg.grad, O._rb(x64.grad), "g_x")
    for k, p in layer.named_parameters():
        errs[k] = close_to_model(p.grad, sd[k].grad, k, frac=1.0 if k.startswith("attn") else 0.05)
    return errs


@pytest.mark.parametrize("H,D", GAT_INSTANCE_SHAPES)
def test_gat_row_kernels_fp32_at_the_degree_edges(H, D, monkeypatch):
    """gat_fwd_vec / gat_bwd_dst / gat_bwd_src (fp32) at every team instance of SPGNN_FOR_R_CH and the scalar fallback, on
    degrees 1..8 (fast path) and 9 / 10 (CSC walk) beside each other, with the padded neighbour rows and without, attention
    dropout on, and with the fused head mean (the MEAN instance) where the geometry takes it."""
    monkeypatch.setattr(snn, "AGGREGATE_FIRST", False)                  # project-first for every width: the row kernels
    monkeypatch.setattr(ops, "TILE_KERNELS", False)
    torch.manual_seed(H * 100 + D)
    fin = 24
    layer = snn.GATConv(fin, D, H, 0.0, P_ATTN, 0.2, True, F.elu).cuda().train()
    with torch.no_grad():
        layer.bias.normal_(0, 0.1)
    fuse_mean = ops.can_fuse_mean(H, D)
    assert fuse_mean == (pick_gat(H, D) is not None and pick_gat(H, D)[2] >= 1)
    for name in ("degree_edge", "past_fast_path"):
        g, src, dst, n = _fixture(name)
        x = torch.randn(n, fin, device="cuda")
        for ell in (True, False):
            monkeypatch.setattr(ops, "USE_ELL", ell)
            for mean in ((False, True) if fuse_mean else (False,)):
                ops.KernelTimer.start()
                _check_gat_layer(layer, g, src, dst, n, x, F.elu, mean, monkeypatch)
                used = {k[0] for k in ops.KernelTimer.stop()}
                assert {"gat_fwd", "gat_bwd_dst", "gat_bwd_src"} <= used, (name, ell, mean, used)


@pytest.mark.parametrize("H,D", [(2, 64), (4, 64), (1, 256)])
def test_gat_row_kernels_on_nodes_without_in_edges(H, D, monkeypatch):
    """Zero in-degree at a vector geometry (test_hip_layers' edge case runs H=2, D=4: the scalar kernel): the rows of nodes
    without in-edges are residual + bias, nodes without out-edges get no gradient from the aggregation; in-degrees up to 9."""
    monkeypatch.setattr(snn, "AGGREGATE_FIRST", False)
    monkeypatch.setattr(ops, "TILE_FORCE", True)                         # tile_plan must refuse this graph by itself
    assert pick_gat(H, D) is not None
    torch.manual_seed(H + D)
    g, src, dst, n = _fixture("zero_in_degree")
    assert ops.tile_plan(g.csc(), H, D, 4, "fwd") is None and ops.tile_plan(g.csc(), H, D, 4, "src") is None
    layer = snn.GATConv(20, D, H, 0.0, P_ATTN, 0.2, True, torch.tanh, allow_zero_in_degree=True).cuda().train()
    with torch.no_grad():
        layer.bias.normal_(0, 0.1)
    x = torch.randn(n, 20, device="cuda")
    for ell in (True, False):
        monkeypatch.setattr(ops, "USE_ELL", ell)
        _check_gat_layer(layer, g, src, dst, n, x, torch.tanh, False, monkeypatch)


BF16_SHAPES = [(1, 64), (2, 128), (4, 64), (2, 256), (4, 256)]        # (16,1,1) (16,4,2) (64,1,0) (64,2,1) (64,4,1)


@pytest.mark.parametrize("H,D", BF16_SHAPES)
def test_gat_row_kernels_bf16_at_the_degree_edges(H, D, monkeypatch):
    """The bf16-storage row kernels (template ST = bf16s) on the same graphs, attention dropout on, against the bf16 storage
    model: normwise two ulp, at most 2 % of the elements beyond fp32 noise."""
    monkeypatch.setattr(ops, "TILE_KERNELS", False)
    torch.manual_seed(H * 10 + D)
    fin = 96                                                             # a Linear residual, as in BASELINE config 4
    layer = snn.GATConv(fin, D, H, 0.0, P_ATTN, 0.2, True, F.elu).cuda().train()
    with torch.no_grad():
        layer.bias.normal_(0, 0.05)
    for name in ("degree_edge", "past_fast_path"):
        g, src, dst, n = _fixture(name)
        x = torch.randn(n, fin).to(torch.bfloat16).float().cuda()
        for ell in (True, False):
            monkeypatch.setattr(ops, "USE_ELL", ell)
            _check_gat_layer(layer, g, src, dst, n, x, F.elu, False, monkeypatch, bf16=True)


@pytest.mark.parametrize("fin,H,D", [(64, 4, 128), (100, 2, 128), (192, 1, 256), (256, 4, 320), (512, 2, 640),
                                     (1024, 1, 2048), (1024, 4, 1040)])
def test_aggregate_first_form_at_the_degree_edges(fin, H, D, monkeypatch):
    """gat_agg_fwd / gat_agg_bwd_dst / gat_agg_bwd_src (inputs narrower than a head) across their dispatch: 16-lane teams with
    1..3 chunks (F <= 192), 64-lane teams with 1 / 2 / 4 chunks (F <= 256 / 512 / 1024); against fp64 and against the
    project-first form, attention dropout on, on degrees 1..10."""
    monkeypatch.setattr(ops, "TILE_KERNELS", False)
    monkeypatch.setattr(snn, "_draw_seed", lambda: SEED)
    torch.manual_seed(fin + H + D)
    layer = snn.GATConv(fin, D, H, 0.0, P_ATTN, 0.2, True, F.elu).cuda().train()
    with torch.no_grad():
        layer.bias.normal_(0, 0.1)
    for name in ("degree_edge", "past_fast_path"):
        g, src, dst, n = _fixture(name)
        x = torch.randn(n, fin, device="cuda")
        cot = torch.randn(n, H, D, device="cuda")
        results = {}
        for form in (True, False):
            monkeypatch.setattr(snn, "AGGREGATE_FIRST", form)
            ops.KernelTimer.start()
            xg = x.clone().requires_grad_(True)
            layer.zero_grad()
            out = layer(g, xg)
            (out * cot).sum().backward()
            used = {k[0] for k in ops.KernelTimer.stop()}
            assert ({"gat_agg_fwd", "gat_agg_bwd_dst", "gat_agg_bwd_src"} <= used) == form, (form, used)
            assert ("gat_fwd" in used) != form
            results[form] = [out.detach(), xg.grad] + [q.grad.clone() for q in layer.parameters()]
        ref, _, xo, sd = oracle_gat(layer, src, dst, n, x, F.elu, torch.float64, attn_keep=_keep_edge(g.csc(), H))
        (ref * cot.cpu().double()).sum().backward()
        names = ["out", "x"] + [k for k, _ in layer.named_parameters()]
        want = [ref, xo.grad] + [sd[k].grad for k in names[2:]]
        for form in (True, False):
            for nm, got, w in zip(names, results[form], want):
                assert rel_err(got, w) < (FWD_TOL if nm == "out" else GRAD_TOL), (name, form, nm, rel_err(got, w))
        for nm, a, b in zip(names, results[True], results[False]):
            assert rel_err(a, b) < GRAD_TOL, (name, nm)


@pytest.mark.parametrize("H,D", [(2, 64), (1, 128), (2, 128)])
@pytest.mark.parametrize("cap", [192, 12])
def test_tile_kernels_at_the_degree_edges(H, D, cap, monkeypatch):
    """The LDS tile kernels (fwd / dst / src, fp32) on degrees 1..8 against the row kernels - forward, attention and g_pre bit
    for bit, the rest to 2e-6 as test_hip_tile.py - with whole trees in a tile and with 12-node tiles (a degree-8 node's
    children straddle a tile boundary: the global-load path)."""
    g, _, _, n = _fixture("degree_edge")
    csc = g.csc()
    y, s, bias, g_out = gat_raw_inputs(n, H, D, torch.float32, seed=H + D)
    monkeypatch.setattr(ops, "TILE_FORCE", False); monkeypatch.setattr(ops, "TILE_KERNELS", False)
    ref = run_gat_raw_fp32(csc, y, s, bias, g_out, H, D, ops.ACT_ELU, P_ATTN, 0.1, True)
    monkeypatch.setattr(ops, "TILE_FORCE", True)
    monkeypatch.setattr(ops, "TILE_NODES", cap)
    assert all(ops.tile_plan(csc, H, D, 4, kind) is not None for kind in ("fwd", "dst", "src"))
    if cap < 192:
        tp = csc.tiles(cap)[0].cpu().numpy()
        ip, ind = csc.indptr.cpu().numpy(), csc.indices.cpu().numpy()
        split = [v for v in range(n) if ip[v + 1] - ip[v] == 8 and
                 len({int(np.searchsorted(tp, u, side="right")) for u in ind[ip[v]:ip[v + 1]]}) > 1]
        assert split, "no degree-8 node has neighbours in two tiles"
    got = run_gat_raw_fp32(csc, y, s, bias, g_out, H, D, ops.ACT_ELU, P_ATTN, 0.1, True)
    HD = H * D
    assert torch.equal(got["out"], ref["out"]) and torch.equal(got["attn"], ref["attn"])
    assert torch.equal(got["g_y"][:, HD:], ref["g_y"][:, HD:])
    assert rel_err(got["g_e"], ref["g_e"]) < 2e-6 and rel_err(got["g_s"], ref["g_s"]) < 2e-6
    assert rel_err(got["g_y"][:, :HD], ref["g_y"][:, :HD]) < 2e-6


def _spy_tile_plan(monkeypatch):
    """Wrap ops.tile_plan: -> the list it appends (kind, elem_bytes, planned) to on every call."""
    seen = []
    real = ops.tile_plan

    def spy(csc, H, D, eb, kind="src"):
        r = real(csc, H, D, eb, kind)
        seen.append((kind, eb, r is not None))
        return r
    monkeypatch.setattr(ops, "tile_plan", spy)
    return seen


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("cap", [192, 12])
def test_tile_layers_against_the_oracle(bf16, cap, monkeypatch):
    """GATConv layers with every traversal forced onto tiles (fp32 and bf16 rows) on degrees 1..8 against fp64 / the bf16
    storage model; on degrees 9..10 and on the zero-in-degree graph tile_plan refuses (the tile kernels have no CSC walk) and
    the layer still matches on the row kernels."""
    monkeypatch.setattr(snn, "AGGREGATE_FIRST", False)
    monkeypatch.setattr(ops, "TILE_FORCE", True)
    monkeypatch.setattr(ops, "TILE_NODES", cap)
    H, D, fin = 2, 64, 96
    torch.manual_seed(cap + bf16)
    layer = snn.GATConv(fin, D, H, 0.0, P_ATTN, 0.2, True, F.elu, allow_zero_in_degree=True).cuda().train()
    with torch.no_grad():
        layer.bias.normal_(0, 0.05)
    seen = _spy_tile_plan(monkeypatch)
    for name in ("degree_edge", "past_fast_path", "zero_in_degree"):
        g, src, dst, n = _fixture(name)
        x = torch.randn(n, fin).to(torch.bfloat16).float().cuda()
        seen.clear()
        _check_gat_layer(layer, g, src, dst, n, x, F.elu, False, monkeypatch, bf16=bf16)
        kinds = {k for k, _, on in seen if on}
        if name == "degree_edge":
            assert kinds == {"fwd", "dst", "src"}, seen
        else:
            assert seen and not kinds, seen


def _spmm_ref(src, dst, n, xo, ws, wd, eps):
    agg = O.spmm_sum(src, dst, xo if ws is None else xo * ws.unsqueeze(1), n)
    agg = agg if wd is None else agg * wd.unsqueeze(1)
    return agg if eps is None else (1 + eps) * xo + agg


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("F_", [64, 256, 7])                    # 16-lane teams, 64-lane teams, the scalar kernel
def test_spmm_sum_at_the_degree_edges(name, F_):
    """spmm_sum plain, weighted (GCN's degree scales, GIN's eps) and in its dropout form (bias + dropout epilogue) against fp64."""
    torch.manual_seed(F_)
    g, src, dst, n = _fixture(name)
    csc = g.csc()
    ws, wd = csc.out_degrees_f().clamp(min=1).pow(-0.5), csc.in_degrees_f().clamp(min=1).pow(-0.5)
    x0 = torch.randn(n, F_, device="cuda")
    cot = torch.randn(n, F_, dtype=torch.float64)
    for form in ("plain", "weighted", "drop") if F_ % 4 == 0 else ("plain", "weighted"):    # dropout form: F % 4 == 0
        x = x0.clone().requires_grad_(True)
        xo = x0.cpu().double().requires_grad_(True)
        eps = torch.tensor([0.25], device="cuda", requires_grad=True)
        epo = eps.detach().cpu().double().requires_grad_(True)
        if form == "plain":
            out, ref = ops.spmm_sum(csc, x), _spmm_ref(src, dst, n, xo, None, None, None)
        elif form == "weighted":
            out = ops.spmm_sum(csc, x, ws, wd, eps)
            ref = _spmm_ref(src, dst, n, xo, ws.cpu().double(), wd.cpu().double(), epo)
        else:
            b = torch.randn(F_, device="cuda") * 0.1
            out = ops.spmm_sum(csc, x, None, wd, eps, bias=b, act=ops.ACT_NONE, drop=(0.1, 4242))
            keep = torch.from_numpy(keep4_scale_host(4242, n, (F_,), 0.1)).double()
            ref = (_spmm_ref(src, dst, n, xo, None, wd.cpu().double(), epo) + b.cpu().double()) * keep
        assert rel_err(out, ref) < FWD_TOL, (form, rel_err(out, ref))
        (out * cot.float().cuda()).sum().backward()
        (ref * cot).sum().backward()
        assert rel_err(x.grad, xo.grad) < GRAD_TOL, (form, rel_err(x.grad, xo.grad))
        if form != "plain":
            assert rel_err(eps.grad, epo.grad) < GRAD_TOL, form


@pytest.mark.parametrize("name", FIXTURES)
@pytest.mark.parametrize("F_", [64, 256, 7])
def test_spmm_max_at_the_degree_edges(name, F_, monkeypatch):
    """spmm_max against the oracle, both argmax forms (one byte: position inside the in-edge list, for in-degrees <= 254; int32
    CSC slots otherwise): the maximum exactly, the gradient routed to exactly one maximising edge per (node, column) - with
    distinct values the oracle's, with every edge tied one edge each; the byte and int32 forms bit for bit the same."""
    torch.manual_seed(F_ + 1)
    g, src, dst, n = _fixture(name)
    csc = g.csc()
    u8_ok = csc.max_in_degree <= 254 and bool(ops._capi.load().spgnn_spmm_max_u8_supported(F_))
    if name == "star_253":
        assert u8_ok == (F_ % 4 == 0)
    if name == "star_254":
        assert not u8_ok
    has_in = (csc.indptr[1:] - csc.indptr[:-1]).cpu() > 0
    x_distinct = torch.randperm(n * F_).float().view(n, F_) / (n * F_) - 0.5          # no ties: one argmax per (node, column)
    cot = torch.randn(n, F_)
    res = {}
    for compact in (True, False):
        monkeypatch.setattr(ops, "COMPACT_MAX_ARG", compact)
        x = x_distinct.cuda().requires_grad_(True)
        y = ops.spmm_max(csc, x)
        assert y.grad_fn.u8 == (compact and u8_ok)
        xo = x_distinct.double().requires_grad_(True)
        ref = O.spmm_max(src, dst, xo, n)
        assert torch.equal(y.cpu().double(), ref.detach())
        (y * cot.cuda()).sum().backward(); (ref * cot.double()).sum().backward()
        assert rel_err(x.grad, xo.grad) < GRAD_TOL                                       # the same addends, fp32 sums
        xt = torch.ones(n, F_, device="cuda", requires_grad=True)                       # every in-edge ties
        yt = ops.spmm_max(csc, xt)
        assert torch.equal(yt.cpu(), has_in.float().unsqueeze(1).expand(n, F_))
        yt.sum().backward()
        assert torch.equal(xt.grad.sum(0).cpu(), torch.full((F_,), float(has_in.sum())))   # each dst routes its grad once
        res[compact] = (y.detach().clone(), x.grad.clone(), xt.grad.clone())
    for a, b in zip(res[True], res[False]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", FIXTURES)
def test_device_ell_rows_equal_the_host_formula(name):
    """DeviceCSC.ell's device builders (spgnn_ell_rows, and spgnn_ell_rows_both of the batch arena) against the host torch
    formula nbr8[v, k] = indices[min(indptr[v] + min(k, max(deg(v) - 1, 0)), E - 1)]: zero-degree nodes (their row points at
    the next node's edges) and a last node of degree 0 (clamped to the last edge) included."""
    from spgnn_amd import _capi
    g, _, _, n = _fixture(name)
    dev = g.csc()
    host = g.cpu().csc()
    want = [t.numpy() for t in host.ell()]
    got = [t.cpu().numpy() for t in dev.ell()]
    for w, gt in zip(want, got):
        assert w.shape == (n, 8) and np.array_equal(w, gt)
    E = dev.num_edges
    ptr = dev.indptr.cpu().numpy().astype(np.int64)
    deg = ptr[1:] - ptr[:-1]
    pos = np.minimum(ptr[:-1, None] + np.minimum(np.arange(8)[None, :], np.maximum(deg - 1, 0)[:, None]), E - 1)
    assert np.array_equal(want[0], dev.indices.cpu().numpy()[pos])
    both = [torch.empty((n, 8), dtype=torch.int32, device="cuda") for _ in range(3)]
    _capi.check(_capi.load().spgnn_ell_rows_both(dev.indptr.data_ptr(), dev.indices.data_ptr(), dev.out_indptr.data_ptr(),
                                                  dev.out_indices.data_ptr(), dev.out_pos.data_ptr(), n, E, both[0].data_ptr(),
                                                  both[1].data_ptr(), both[2].data_ptr(), torch.cuda.current_stream().cuda_stream),
                "spgnn_ell_rows_both")
    for w, b in zip(want, both):
        assert np.array_equal(w, b.cpu().numpy())
