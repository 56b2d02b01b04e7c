"""The fused SPGNN level (spgnn_lspe_fwd / _bwd_dst / _bwd_src: structure GATConv + position GATConv of reference
models.py:472-484 in ONE traversal) against the two-layer form it replaces and against the oracle.

* forward: bit for bit equal to the two-layer form (same arithmetic per element, same masks from one seed plan), in eval mode
  and with every dropout on;
* backward: the per-edge dots are summed over a different team geometry (3 heads per team instead of 2 and 1), so gradients
  agree to fp32 rounding: <= 2e-6 normwise here (tolerance written below), and they match the oracle like every other
  configuration (tests/test_hip_models.py runs st_pgat_spgnn_3 through this path);
* graphs the kernels do not take (a node of degree > 8) fall back to the two-layer form;
* every geometry the kernels accept (D = 64 / 128 / 256: T = 16 / 32 / 64 lanes, bwd_src RR = 1 / 2 / 4) in model variants with
  identity position residuals, the degree edges 1 and 8 side by side in one wave, training mode with its masks rebuilt on the
  host, both routes of the scores and the split-GEMM scales the kernels emit - all against the fp64 oracle or exactly.
"""
import numpy as np
import pytest
import torch

from oracle import dgl_cpu as O
from spgnn_amd import models, ops, synthetic
from spgnn_amd.configs import class_weight_list, get_config
from spgnn_amd.graph import TreeGraph
from spgnn_amd.train import masked_weighted_ce
from tests.util import rel_err, spgnn_host_masks

pytestmark = pytest.mark.gpu
GRAD_TOL = 2e-6      # fused vs two-layer gradients, normwise relative (fp32 summation order only)


def _model(seed=0, hiddens=None):
    """st_pgat_spgnn_3's model; ``hiddens``: other level widths (num_hiddens = pos_hiddens, so every level stays fusable)."""
    cfg = get_config("st_pgat_spgnn_3")
    if hiddens is not None:
        cfg.MODEL.update(num_hiddens=list(hiddens), pos_hiddens=list(hiddens))
    torch.manual_seed(seed)
    model = models.build_model(cfg.MODEL).cuda()
    model.init(None)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
    model.set_gcn_only()
    return cfg, model


def _run(model, g, cfg, fused, train, monkeypatch, seed=77):
    monkeypatch.setattr(models, "FUSE_LSPE", fused)
    model.train(train)
    for p in model.parameters():
        p.grad = None
    torch.manual_seed(seed)                       # the seed plan draws from torch's CPU generator
    outs = model(g)
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS), device="cuda")
    y = g.ndata["y"]
    mask = (torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5).cuda()
    # the position output h_p enters the loss too, so both consumers of every level's position rows carry a gradient
    loss = masked_weighted_ce(outs[0], y, mask, w) + 1e-3 * outs[2].square().sum() + 1e-4 * outs[1].square().mean()
    loss.backward()
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return [o.detach().clone() for o in outs], grads, float(loss.detach())


@pytest.mark.parametrize("train", [False, True])
def test_fused_level_equals_two_layer_form(train, monkeypatch):
    cfg, model = _model()
    g = synthetic.make_batch(5, rank=2, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    assert model.gat._lspe_ok(g, torch.empty(1, 8, device="cuda"), g.ndata["pos_enc"])
    timed = {}
    ops.KernelTimer.start()
    o_f, g_f, l_f = _run(model, g, cfg, True, train, monkeypatch)
    timed["fused"] = {k[0] for k in ops.KernelTimer.stop()}
    ops.KernelTimer.start()
    o_u, g_u, l_u = _run(model, g, cfg, False, train, monkeypatch)
    timed["two"] = {k[0] for k in ops.KernelTimer.stop()}
    assert {"lspe_fwd", "lspe_bwd_dst", "lspe_bwd_src"} <= timed["fused"] and "lspe_fwd" not in timed["two"]
    for a, b in zip(o_f, o_u):                    # logits, node embedding, position embedding: bit for bit
        assert torch.equal(a, b)
    assert l_f == l_u
    assert set(g_f) == set(g_u)
    gmax = max(float(v.abs().max()) for v in g_u.values())
    for n in g_u:
        tiny = float((g_f[n] - g_u[n]).abs().max()) < 1e-7 * gmax
        # with feature dropout on, the two-layer form keeps the position rows un-dropped for tanh' while the fused form
        # recovers them as stored * (1 - p): one more rounding per element
        assert rel_err(g_f[n], g_u[n]) < (4 * GRAD_TOL if train else GRAD_TOL) or tiny, (n, rel_err(g_f[n], g_u[n]))


def test_pair_launches_leave_the_step_bitwise_unchanged(monkeypatch):
    """ops.PAIR_GEMMS: a level's two projections / weight gradients / input gradients as one launch each - outputs and every
    gradient equal the separate launches bit for bit, and the paired step has the fewer launches."""
    cfg, model = _model(3)
    g = synthetic.make_batch(4, rank=1, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    res, names = [], []
    for pair in (True, False):
        monkeypatch.setattr(ops, "PAIR_GEMMS", pair)
        monkeypatch.setattr(ops, "PAIR_SCORE_GRADS", pair)          # ... and the two attention-vector gradient passes
        ops.KernelTimer.start()
        res.append(_run(model, g, cfg, True, True, monkeypatch))
        names.append([k[0] for k in ops.KernelTimer.sequence])
        ops.KernelTimer.stop()
    assert "gemm_nt_pair" in names[0] and "gemm_tn_pair" in names[0] and "gemm_nt_pair" not in names[1]
    assert "scores_bwd_w_pair" in names[0] and "scores_bwd_w_pair" not in names[1]
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert set(res[0][1]) == set(res[1][1])
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


def test_fused_level_matches_oracle_gradients(monkeypatch):
    """fwd + all parameter gradients of the fused path against the CPU oracle (eval-mode arithmetic), with the position
    output inside the loss so that the second gradient path of every level is exercised."""
    cfg, model = _model(seed=3)
    g = synthetic.make_batch(3, rank=4, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    outs, grads, _ = _run(model, g, cfg, True, False, monkeypatch)
    src, dst = g.cpu().edges()
    sd = {k: v.detach().cpu().double().requires_grad_(v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    ref = O.net_forward(cfg.KIND, sd, src, dst, g.number_of_nodes(), g.ndata["fvs"].cpu().double(), g.ndata["pos_enc"].cpu().double())
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS)).double()
    y = g.ndata["y"].cpu()
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5
    (O.masked_weighted_ce(ref[0], y, mask, w) + 1e-3 * ref[2].square().sum() + 1e-4 * ref[1].square().mean()).backward()
    for o, r in zip(outs, ref):
        assert rel_err(o, r) < 1e-5
    gmax = max(float(v.grad.abs().max()) for v in sd.values() if v.grad is not None)
    for n, gr in grads.items():
        tiny = float((gr.cpu().double() - sd[n].grad).abs().max()) < 1e-7 * gmax
        assert rel_err(gr, sd[n].grad) < 1e-4 or tiny, (n, rel_err(gr, sd[n].grad))


def test_high_degree_graph_takes_the_two_layer_form(monkeypatch):
    """A node with more than 8 neighbours: the fused kernels are not used (they assume degree <= 8) and the model still
    matches the oracle."""
    cfg, model = _model(seed=1)
    n = 40
    src = np.concatenate([np.zeros(n - 1, dtype=np.int64), np.arange(1, n), np.arange(n)])     # a star + self loops
    dst = np.concatenate([np.arange(1, n), np.zeros(n - 1, dtype=np.int64), np.arange(n)])
    g = TreeGraph((src, dst), n).to("cuda")
    torch.manual_seed(0)
    g.ndata["fvs"] = torch.relu(torch.randn(n, 1024, device="cuda"))
    g.ndata["pos_enc"] = torch.rand(n, cfg.POS_ENC_DIM, device="cuda")
    model.eval()
    assert not model.gat._lspe_ok(g, torch.empty(1, 8, device="cuda"), g.ndata["pos_enc"])
    ops.KernelTimer.start()
    with torch.no_grad():
        outs = model(g)
    assert "lspe_fwd" not in {k[0] for k in ops.KernelTimer.stop()}
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    ref = O.net_forward(cfg.KIND, sd, torch.from_numpy(src), torch.from_numpy(dst), n, g.ndata["fvs"].cpu(), g.ndata["pos_enc"].cpu())
    for o, r in zip(outs, ref):
        assert rel_err(o, r) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# every geometry the kernels accept, against the fp64 oracle
# ---------------------------------------------------------------------------------------------------------------------
# level widths D -> team geometry (spgnn_lspe.hip lspe_geometry): T = 16 (two table registers per lane), 32 or 64 lanes per
# node in the forward and bwd_dst; bwd_src on 16-lane teams with RR = D / 64 chunks per lane
WIDTHS = {
    "w64-64-64": (64, 64, 64),          # every level at T = 16, bwd_src with RR = 1
    "w256-256-64": (256, 256, 64),      # two T = 64 levels in a row
    "w128-64-64": (128, 64, 64),        # a level whose next level is narrower
}
SHIPPED = (256, 128, 64)
ROUTES = {"scores-in-kernel": True, "scores-from-parts": False}
DROP_KEYS = [("attn", "p", 1), ("attn", "s", 1), ("attn", "s", 2), ("feat", "p", 1), ("feat", "s", 1), ("feat", "s", 2)]


def _degree_edge_graph(seed=0):
    """tests/util.DEGREE_EDGE_TREES as one batch: nodes of every degree 1..8 (one-node trees included) side by side, N not a
    multiple of 16 (a partial last block at every team width).  The anchor rule of the distance encoding needs at least 21
    nodes per tree (posenc.anchors_from_cnn_prediction refuses smaller ones), so the one-node trees have no encoding: every
    node gets a stand-in in [0, 1), 39 wide in rows of 40 like the encoding's.  The kernels do not depend on where it came from."""
    from spgnn_amd import graph as G
    from tests.util import degree_edge_batch
    adjs, deg = degree_edge_batch()
    g = G.batch([G.graph_from_adj(a) for a in adjs]).to("cuda")
    N = g.number_of_nodes()
    gen = torch.Generator().manual_seed(seed)
    g.ndata["fvs"] = torch.relu(torch.randn(N, 1024, generator=gen)).cuda()
    pe = torch.zeros(N, 40)
    pe[:, :39] = torch.rand(N, 39, generator=gen)
    g.ndata["pos_enc"] = pe.cuda()[:, :39]
    g.ndata["y"] = torch.randint(0, 22, (N,), generator=gen).cuda()
    return g, deg


def _fused_step(model, g, cfg, train, pos_in_loss, monkeypatch, seed=77):
    """One forward + backward through the fused levels with gradients into fvs and pos_enc too.
    -> (outputs, {name: gradient} incl. "fvs" / "pos_enc", seed plan, {kernel key: launches})."""
    monkeypatch.setattr(models, "FUSE_LSPE", True)
    model.train(train)
    for p in model.parameters():
        p.grad = None
    x_in = {k: g.ndata[k].detach().requires_grad_(True) for k in ("fvs", "pos_enc")}
    for k, t in x_in.items():
        g.ndata[k] = t
    plans = []
    orig = model.gat._seed_plan

    def recording_plan():
        plans.append(orig())
        return plans[-1]
    model.gat._seed_plan = recording_plan
    try:
        assert model.gat._lspe_ok(g, g.ndata["fvs"], g.ndata["pos_enc"])
        ops.KernelTimer.start()
        torch.manual_seed(seed)                   # the seed plan draws from torch's CPU generator
        outs = model(g)
        loss = _loss(outs, g, cfg, pos_in_loss, masked_weighted_ce, "cuda")
        loss.backward()
        timed = {k: len(v) for k, v in ops.KernelTimer.stop().items()}
    finally:
        ops.KernelTimer.enabled = False
        del model.gat._seed_plan
    assert len(plans) == 1
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    for k, t in x_in.items():
        grads[k] = t.grad.detach().clone()
        g.ndata[k] = t.detach()
    return [o.detach().clone() for o in outs], grads, plans[0], timed


def _loss(outs, g, cfg, pos_in_loss, ce, dev):
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS), dtype=outs[0].dtype, device=dev)
    y = g.ndata["y"].to(dev)
    mask = (torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5).to(dev)
    loss = ce(outs[0], y, mask, w) + 1e-4 * outs[1].square().mean()
    # with the position output in the loss, the last level's bwd_dst takes a gradient of its second copy (g_xp) too
    return loss + 1e-3 * outs[2].square().sum() if pos_in_loss else loss


def _assert_fused_ran(timed, widths, pos_in_loss):
    """Every level went through spgnn_lspe_fwd / _bwd_dst / _bwd_src at its width (keys: (kernel, N, E, D[, g_xp given]))."""
    launched = lambda name: sorted(k[3:] for k, n in timed.items() if k[0] == name for _ in range(n))
    assert launched("lspe_fwd") == sorted((w,) for w in widths)
    assert launched("lspe_bwd_src") == sorted((w,) for w in widths)
    assert launched("lspe_bwd_dst") == sorted([(w, 1) for w in widths[:-1]] + [(widths[-1], int(pos_in_loss))])


def _assert_matches_oracle(model, g, cfg, outs, grads, pos_in_loss, drop=None):
    """Outputs (logits, node embedding, position embedding) 1e-5 normwise against the fp64 oracle; every parameter gradient
    and the gradients of fvs / pos_enc 1e-4 normwise, or within 1e-7 of the largest gradient."""
    src, dst = g.cpu().edges()
    sd = {k: v.detach().cpu().double().requires_grad_(v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    x64 = {k: g.ndata[k].detach().cpu().double().requires_grad_(True) for k in ("fvs", "pos_enc")}
    ref = O.net_forward(cfg.KIND, sd, src, dst, g.number_of_nodes(), x64["fvs"], x64["pos_enc"],
                        drop=None if drop is None else {k: m.double() for k, m in drop.items()})
    _loss(ref, g, cfg, pos_in_loss, O.masked_weighted_ce, "cpu").backward()
    assert len(outs) == len(ref) == 3
    for i, (o, r) in enumerate(zip(outs, ref)):
        assert o.shape == r.shape and rel_err(o, r) < 1e-5, (i, rel_err(o, r))
    ref_grads = {n: sd[n].grad for n in sd if sd[n].grad is not None}
    ref_grads.update({k: t.grad for k, t in x64.items()})
    assert set(grads) == set(ref_grads), set(grads) ^ set(ref_grads)
    gmax = max(float(v.abs().max()) for v in ref_grads.values())
    for n, gr in grads.items():
        tiny = float((gr.cpu().double() - ref_grads[n]).abs().max()) < 1e-7 * gmax
        assert rel_err(gr, ref_grads[n]) < 1e-4 or tiny, (n, rel_err(gr, ref_grads[n]))
    for k in x64:                                  # the input gradients are really checked, not waved through as tiny
        assert float(ref_grads[k].abs().max()) > 1e-5 * gmax, k


@pytest.mark.parametrize("route", ROUTES.values(), ids=ROUTES.keys())
@pytest.mark.parametrize("pos_in_loss", [True, False], ids=["pos-in-loss", "pos-not-in-loss"])
@pytest.mark.parametrize("widths", WIDTHS.values(), ids=WIDTHS.keys())
def test_model_variant_matches_the_fp64_oracle(widths, pos_in_loss, route, monkeypatch):
    """GATPositionSPGNNNet at level widths the shipped config does not have, eval mode: all three outputs, every parameter
    gradient and the gradients of fvs and pos_enc against the fp64 oracle, on both routes of the scores.  Each variant has a
    level whose position layer is as wide as its input - an identity residual (DGL GATConv adds the input itself)."""
    cfg, model = _model(seed=21, hiddens=widths)
    assert any(type(l.res_fc).__name__ == "Identity" for l in model.gat.pgnn_layers)
    monkeypatch.setattr(ops, "LSPE_SCORES_IN_KERNEL", route)
    g = synthetic.make_batch(3, rank=5, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    outs, grads, _, timed = _fused_step(model, g, cfg, False, pos_in_loss, monkeypatch)
    _assert_fused_ran(timed, widths, pos_in_loss)
    _assert_matches_oracle(model, g, cfg, outs, grads, pos_in_loss)


@pytest.mark.parametrize("route", ROUTES.values(), ids=ROUTES.keys())
@pytest.mark.parametrize("widths", [WIDTHS["w64-64-64"], SHIPPED], ids=["w64-64-64", "shipped"])
def test_degree_edge_graph_matches_the_fp64_oracle(widths, route, monkeypatch):
    """Degree 8 (a full 24-entry (slot, head) table, the last gather pair of slots 6 and 7), degree 1 (a node whose only edge
    is its self loop) and teams of different degrees in one wave, N not a multiple of 16 - against the fp64 oracle."""
    monkeypatch.setattr(ops, "LSPE_SCORES_IN_KERNEL", route)
    cfg, model = _model(seed=22, hiddens=widths)
    g, deg = _degree_edge_graph()
    N = g.number_of_nodes()
    assert N % 16 != 0 and N == deg.shape[0]
    csc = g.csc("cuda")
    assert (csc.min_in_degree, csc.max_in_degree, csc.min_out_degree, csc.max_out_degree) == (1, 8, 1, 8)
    assert np.array_equal((csc.indptr[1:] - csc.indptr[:-1]).cpu().numpy(), deg)
    outs, grads, _, timed = _fused_step(model, g, cfg, False, True, monkeypatch)
    _assert_fused_ran(timed, widths, True)
    _assert_matches_oracle(model, g, cfg, outs, grads, True)


DROPOUT_CASES = {**{k: (w, "trees") for k, w in WIDTHS.items()}, "w64-64-64-degree-edges": (WIDTHS["w64-64-64"], "degree")}


@pytest.mark.parametrize("widths,graph", DROPOUT_CASES.values(), ids=[f"dropout-{k}" for k in DROPOUT_CASES])
def test_training_mode_with_dropout_matches_the_fp64_oracle(widths, graph, monkeypatch):
    """Training mode, feature and attention dropout on (rate 0.1 where the reference places it): the forward's seed plan is
    recorded, every mask rebuilt on the host bit for bit (tests/util.spgnn_host_masks) and handed to the oracle; the same
    bars as in eval mode."""
    cfg, model = _model(seed=23, hiddens=widths)
    g = synthetic.make_batch(3, rank=6, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM) if graph == "trees" else _degree_edge_graph(1)[0]
    outs, grads, plan, timed = _fused_step(model, g, cfg, True, True, monkeypatch)
    _assert_fused_ran(timed, widths, True)
    assert [(d["fp"], d["ps"], d["pp"], d["fp2"]) for d in plan] == [(0.1, 0.0, 0.0, 0.1), (0.1, 0.1, 0.1, 0.0), (0.0, 0.1, 0.0, 0.0)]
    drop = spgnn_host_masks(plan, model, g)
    assert sorted(drop) == DROP_KEYS
    for k, m in drop.items():
        assert 0.8 < float((m > 0).float().mean()) < 0.97, k
    _assert_matches_oracle(model, g, cfg, outs, grads, True, drop=drop)


@pytest.mark.parametrize("graph", ["trees", "degree-edges"])
@pytest.mark.parametrize("widths", [*WIDTHS.values(), SHIPPED], ids=[*WIDTHS.keys(), "shipped"])
def test_score_routes_are_bitwise_equal(widths, graph, monkeypatch):
    """ops.LSPE_SCORES_IN_KERNEL: el / er summed inside spgnn_lspe_fwd from the GEMMs' score partials (PARTS) or by
    spgnn_scores_from_parts before it - the same additions in the same order, so the outputs and (the backward reads the
    same el / er and attention) every gradient are equal bit for bit.  Training mode: dropout on."""
    cfg, model = _model(seed=24, hiddens=widths)
    g = synthetic.make_batch(2, rank=7, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM) if graph == "trees" else _degree_edge_graph(2)[0]
    res = []
    for route in (True, False):
        monkeypatch.setattr(ops, "LSPE_SCORES_IN_KERNEL", route)
        res.append(_fused_step(model, g, cfg, True, True, monkeypatch))
        _assert_fused_ran(res[-1][3], widths, True)
    # the route really switched: without PARTS each level runs spgnn_scores_from_parts once per layer
    parts = [sorted(k[1:] for k, n in r[3].items() if k[0] == "scores_from_parts" for _ in range(n)) for r in res]
    extra = list(parts[1])
    for k in parts[0]:
        extra.remove(k)
    assert sorted(extra) == sorted((g.number_of_nodes(), H, D) for D in widths for H in (2, 1))
    for a, b in zip(res[0][0], res[1][0]):
        assert torch.equal(a, b)
    assert set(res[0][1]) == set(res[1][1])
    for n in res[0][1]:
        assert torch.equal(res[0][1][n], res[1][1][n]), n


@pytest.mark.parametrize("widths", WIDTHS.values(), ids=WIDTHS.keys())
def test_fused_levels_emit_exact_scales(widths, monkeypatch):
    """The split-GEMM scales the fused kernels fold up on the way equal an absmax pass over what they wrote (as
    test_hip_layers.test_emitted_scales_equal_an_absmax_pass checks for the other kernels): the forward's tags on the next
    level's inputs buf (N, 3D) and xp (N, D), and the backward's blocks over the GEMM-gradient buffers [g_ft | g_pre] of
    both layers (bwd_dst folds g_pre, bwd_src g_ft), which the weight- and input-gradient products take as their scale."""
    cfg, model = _model(seed=25, hiddens=widths)
    g = synthetic.make_batch(3, rank=8, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    fwd, bwd, log, active = [], [], [], [False]
    orig_level, orig_bwd = ops.lspe_level, ops._LspeLevelFn.backward

    def level(csc, x_s, x_p, w_s, w_p, attn_s, attn_p, bias_s, bias_p, D, cfg_):
        buf, xp = orig_level(csc, x_s, x_p, w_s, w_p, attn_s, attn_p, bias_s, bias_p, D, cfg_)
        for t in (buf, xp):
            tag = t._spgnn_scale
            assert tag[0] == t._version
            fwd.append((D, t.shape[1], ops.scale_value(tag[1]), float(ops.pow2_scale(t.detach()))))
        return buf, xp

    def recording(cls):
        class Rec(cls):
            def __init__(self, a, b, scale_a=None, *args, **kw):
                if active[0]:
                    log.append((a, scale_a))
                super().__init__(a, b, scale_a, *args, **kw)
        return Rec

    def backward(ctx, *grads):
        start = len(log)
        active[0] = True
        try:
            out = orig_bwd(ctx, *grads)
        finally:
            active[0] = False
        seen = {a.data_ptr(): (a, sc) for a, sc in log[start:]}
        assert len(seen) == 2, len(seen)           # one gradient buffer per layer, each consumed by its products
        for a, sc in seen.values():
            assert sc is not None and sc.numel() > 1
            bwd.append((ctx.D, a.shape[1], ops.scale_value(sc), float(ops.pow2_scale(a))))
        return out
    monkeypatch.setattr(ops, "lspe_level", level)
    monkeypatch.setattr(ops, "NtProblem", recording(ops.NtProblem))
    monkeypatch.setattr(ops, "TnProblem", recording(ops.TnProblem))
    monkeypatch.setattr(ops._LspeLevelFn, "backward", staticmethod(backward))
    model.train(True)
    for k in ("fvs", "pos_enc"):                   # input gradients: every level's both layers run their input-gradient product
        g.ndata[k] = g.ndata[k].detach().requires_grad_(True)
    torch.manual_seed(7)
    outs = model(g)
    _loss(outs, g, cfg, True, masked_weighted_ce, "cuda").backward()
    assert sorted((D, c) for D, c, _, _ in fwd) == sorted([(D, 3 * D) for D in widths] + [(D, D) for D in widths])
    # [g_ft | g_pre]: 4D wide for the structure layer; 2D for the position layer, D (g_ft alone) with an identity residual
    p_width = [2 * D if isinstance(l.res_fc, torch.nn.Linear) else D for D, l in zip(widths, model.gat.pgnn_layers)]
    assert sorted((D, c) for D, c, _, _ in bwd) == sorted([(D, 4 * D) for D in widths] + list(zip(widths, p_width)))
    for D, c, tagged, absmax in fwd + bwd:
        assert tagged == absmax, (D, c, tagged, absmax)
