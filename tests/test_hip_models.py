"""Model-level parity (every exp_settings config) of the HIP path against the CPU oracle, at the
configs' full layer widths on a few synthetic trees, plus size-independent properties at the
BASELINE batch size (512 trees)."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import dgl_cpu as O
from spgnn_amd import models, synthetic
from spgnn_amd.configs import CONFIGS, class_weight_list, get_config
from spgnn_amd.train import TrainStep, masked_weighted_ce
from tests.util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-5     # BASELINE.json north_star: logits within 1e-5 (fp32, relative) of the DGL-CPU forward


def _build(name, seed=0):
    cfg = get_config(name)
    torch.manual_seed(seed)
    model = models.build_model(cfg.MODEL).cuda()
    model.init(None)
    with torch.no_grad():                       # non-trivial biases/eps so their paths are exercised
        for n, p in model.named_parameters():
            if n.endswith("bias") or n.endswith("eps"):
                p.normal_(0, 0.05)
    model.set_gcn_only()
    return cfg, model


def _oracle(cfg, model, g, grad=False):
    src, dst = g.cpu().edges()
    sd = {k: v.detach().cpu().clone().requires_grad_(grad and v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    pe = g.ndata["pos_enc"].cpu() if "pos_enc" in g.ndata else None
    return O.net_forward(cfg.KIND, sd, src, dst, g.number_of_nodes(), g.ndata["fvs"].cpu(), pe), sd


@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_config_forward_matches_oracle(name):
    cfg, model = _build(name)
    g = synthetic.make_batch(3, rank=7, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    model.eval()
    with torch.no_grad():
        outs = model(g)
    refs, _ = _oracle(cfg, model, g)
    assert len(outs) == len(refs)
    for o, r in zip(outs, refs):
        assert o.shape == r.shape and rel_err(o, r) < TOL
    assert outs[0].shape == (g.number_of_nodes(), 22)


@pytest.mark.parametrize("name", ["st_gcn_3", "st_gin_3", "st_sage_3", "st_gat_3"])
def test_small_batches_on_the_librarys_own_products(name, monkeypatch):
    """below ops.MIN_GEMM_ROWS = 512 rows the dense layers of rows D / E / F (and the linear-mean output
    layer) go to torch.mm, so the 2-3-tree parity cases never touched spgnn_gemm_*.  With the threshold at 1 the same small
    batch runs the library's matrix-core kernels - ragged row tiles, one-tile weight gradients - forward and loss gradients
    against the oracle."""
    from spgnn_amd import ops as _ops
    monkeypatch.setattr(_ops, "MIN_GEMM_ROWS", 1)
    cfg, model = _build(name, seed=9)
    g = synthetic.make_batch(2, rank=5, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    assert g.number_of_nodes() < 512
    model.eval()
    _ops.KernelTimer.start()
    outs = model(g)
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS))
    y = g.ndata["y"]
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(3)) < 0.5
    loss = masked_weighted_ce(outs[0], y, mask.cuda(), w.cuda())
    loss.backward()
    ran = {k[0] for k in _ops.KernelTimer.stop()}
    assert "gemm_nt" in ran and ("gemm_tn" in ran or name == "st_gat_3"), ran
    refs, sd = _oracle(cfg, model, g, grad=True)
    for o, r in zip(outs, refs):
        assert rel_err(o, r) < TOL
    O.masked_weighted_ce(refs[0], y.cpu(), mask, w).backward()
    bad = []
    for n, p in model.named_parameters():
        if p.requires_grad and p.grad is not None and sd[n].grad is not None:
            e = rel_err(p.grad, sd[n].grad)
            if e >= 1e-4 and not (cfg.KIND == "sage" and (p.grad.cpu().double() - sd[n].grad.double()).norm() / sd[n].grad.double().norm() < 5e-3):
                bad.append((n, e))
    assert not bad, bad


@pytest.mark.parametrize("name,trees", [("st_pgat_spgnn_3", 2), ("st_pgat_spgnnnl_3", 2), ("st_gat_3", 2), ("st_gcn_3", 2), ("st_gin_3", 2),
                                        ("st_sage_3", 2), ("st_gat_6_nr", 2),
                                        # >= 512 nodes: the dense layers of rows D / E / F take the matrix-core products with their
                                        # epilogues, emitted scales, prepared weights, SAGE's K-concatenated output layer and folded classifier
                                        ("st_gcn_3", 5), ("st_gin_3", 5), ("st_sage_3", 5)])
def test_config_loss_gradients_match_oracle(name, trees):
    cfg, model = _build(name, seed=1)
    g = synthetic.make_batch(trees, rank=3, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    assert trees == 2 or g.number_of_nodes() >= 512
    model.eval()                                  # dropout off; gradients still flow
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS))
    y = g.ndata["y"]
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5
    loss = masked_weighted_ce(model(g)[0], y, mask.cuda(), w.cuda())
    loss.backward()
    refs, sd = _oracle(cfg, model, g, grad=True)
    ref_loss = O.masked_weighted_ce(refs[0], y.cpu(), mask, w)
    ref_loss.backward()
    assert rel_err(loss, ref_loss) < TOL
    # gradients: judged against an fp64 evaluation of the oracle.  The HIP path must be within 1e-4 of the
    # fp32 oracle, or (tiny-magnitude gradients where fp32 itself is noisy) no further from fp64 than 5x the
    # fp32 oracle's own distance (the score vectors' gradients are sums of ~1e-6 terms of mixed sign).
    src, dst = g.cpu().edges()
    sd64 = {k: v.detach().cpu().double().requires_grad_(v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    pe = g.ndata["pos_enc"].cpu().double() if "pos_enc" in g.ndata else None
    out64 = O.net_forward(cfg.KIND, sd64, src, dst, g.number_of_nodes(), g.ndata["fvs"].cpu().double(), pe)[0]
    O.masked_weighted_ce(out64, y.cpu(), mask, w.double()).backward()
    gmax = max(float(v.grad.abs().max()) for v in sd64.values() if v.grad is not None)
    for n, p in model.named_parameters():
        if p.requires_grad and not (p.grad is None and sd[n].grad is None):     # (GINNet's auxiliary heads are unused)
            assert sd[n].grad is not None and p.grad is not None, n
            e32 = rel_err(p.grad, sd[n].grad)
            if cfg.KIND == "sage" and e32 >= 1e-4:
                # max-pool routing is discontinuous: when two neighbours' pooled values differ by less than the
                # fp32 noise between rocBLAS and MKL (~1e-7 relative), GPU and CPU legitimately pick different
                # winners for that (node, feature); one flip moves one row of fc_pool's gradient (measured:
                # 0.3 % of entries, relative L2 error 1.5e-3) and perturbs everything upstream of it slightly.
                # A routing bug gives O(1) errors; tests/test_hip_layers.py checks the routing bit-exactly on
                # tie-free data.  So here: the error must stay small in L2.
                d = (p.grad.cpu().double() - sd[n].grad.double())
                assert d.norm() / sd[n].grad.double().norm() < 5e-3, (n, e32)
                continue
            # ... or the tensor sits below the fp32 resolution of the computation it comes from: the score vectors'
            # gradients in the position stream are ~1e-6 (softmax is shift-invariant in er up to the LeakyReLU kink, so
            # they are near-total cancellations of ~1e-2 terms) and move by 1e-4 relative when el/er change by one ulp.
            tiny = (p.grad.cpu().double() - sd64[n].grad).abs().max() < 1e-7 * gmax
            assert e32 < 1e-4 or tiny or rel_err(p.grad, sd64[n].grad) < 5 * rel_err(sd[n].grad, sd64[n].grad) + 1e-6, (n, e32)


@pytest.mark.parametrize("embedding_in_loss", [False, True])
def test_linear_mean_fold_kernels_equal_the_torch_assembly(embedding_in_loss, monkeypatch):
    """ops.FUSE_LINEAR_MEAN_FOLD: W_comb / b_mean / P / c0 and the way back to g_W_fc / g_W_res / g_bias / g_Wc in one launch
    each (spgnn_linear_mean_fold_fwd / _bwd) against the torch / rocBLAS assembly they replace - logits, embedding and every
    parameter gradient, on the folded route (only the logits in the loss) and the ordinary one (the embedding too)."""
    from spgnn_amd import ops
    cfg, model = _build("st_gat_3", seed=2)
    g = synthetic.make_batch(5, rank=1, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    assert g.number_of_nodes() >= 512
    model.eval()
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS), device="cuda")
    y = g.ndata["y"]
    mask = (torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5).cuda()
    res = []
    for fused in (True, False):
        monkeypatch.setattr(ops, "FUSE_LINEAR_MEAN_FOLD", fused)
        for p_ in model.parameters():
            p_.grad = None
        ops.KernelTimer.start()
        out = model(g)
        loss = masked_weighted_ce(out[0], y, mask, w)
        if embedding_in_loss:
            loss = loss + 1e-3 * out[1].square().mean()
        loss.backward()
        ops.KernelTimer.stop()
        res.append(([o.detach().clone() for o in out[:2]], {n: p_.grad.clone() for n, p_ in model.named_parameters() if p_.grad is not None}))
    for a, b in zip(res[0][0], res[1][0]):
        assert rel_err(a, b) < 2e-6
    assert set(res[0][1]) == set(res[1][1])
    gmax = max(float(v.abs().max()) for v in res[1][1].values())
    for n in res[1][1]:
        a, b = res[0][1][n], res[1][1][n]
        assert rel_err(a, b) < 2e-5 or float((a - b).abs().max()) < 1e-7 * gmax, (n, rel_err(a, b))


@pytest.mark.parametrize("trees", [2, 64])
def test_st_gat_3_with_eight_heads_matches_oracle(trees):
    """BASELINE.json words config 2 as "st_gat_3 (3-layer 8-head GAT)"; the reference's st_gat_3 has 2 heads
    (exp_settings/st_gat_3.py:101-102).  H is a run-time parameter here: the same model with num_heads = 8 (hidden layers
    8 x 256 / 8 x 128 / 8 x 64, output 2 x 1024), forward and loss gradients against the oracle at model level - on a 2-tree
    batch and at BASELINE config 2's own batch of 64 trees."""
    cfg = get_config("st_gat_3")
    torch.manual_seed(0)
    model = models.build_model({**cfg.MODEL, "num_heads": 8}).cuda()
    model.init(None)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
    model.set_gcn_only(); model.eval()
    assert model.state_dict()["gat.gat_layers.0.fc.weight"].shape == (2048, 1024)
    g = synthetic.make_batch(trees, rank=6, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS))
    y = g.ndata["y"]
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5
    outs = model(g)
    masked_weighted_ce(outs[0], y, mask.cuda(), w.cuda()).backward()
    refs, sd = _oracle(cfg, model, g, grad=True)
    O.masked_weighted_ce(refs[0], y.cpu(), mask, w).backward()
    assert rel_err(outs[0], refs[0]) < TOL and rel_err(outs[1], refs[1]) < TOL
    gmax = max(float(v.grad.abs().max()) for v in sd.values() if v.grad is not None)
    for n, p in model.named_parameters():
        if p.requires_grad:
            tiny = float((p.grad.cpu() - sd[n].grad).abs().max()) < 1e-7 * gmax
            assert rel_err(p.grad, sd[n].grad) < 1e-4 or tiny, n


@pytest.mark.parametrize("name", ["st_pgat_spgnn_3", "st_gat_3", "st_gat_6_nr"])
def test_fused_output_dropout_equals_separate_pass(name, monkeypatch):
    """Training mode (feature + attention dropout on): hidden layers writing their rows straight into the next layer's
    input buffer under that layer's feature dropout (nn.GATConv fuse_out + ops.fill_cols_dropout) against the separate
    concat + dropout pass (reference models.py:477-481 order of operations).  Every seed draw returns one constant, so both
    forms see identical masks whatever the order of the draws: the forward pass must agree to rounding (the stored rows are
    the same products), the gradients to fp32 noise (the activation derivative is recovered from stored * (1 - p))."""
    from spgnn_amd import nn as snn
    monkeypatch.setattr(snn, "_draw_seed", lambda: 424242)
    monkeypatch.setattr(models, "_draw_seed", lambda: 424242)
    cfg, model = _build(name, seed=2)
    model.train()
    g = synthetic.make_batch(3, rank=8, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS)).cuda()
    y = g.ndata["y"]
    mask = (torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5).cuda()
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(models, "FUSE_OUTPUT_DROPOUT", fused)
        model.zero_grad(set_to_none=True)
        logits = model(g)[0]
        masked_weighted_ce(logits, y, mask, w).backward()
        res[fused] = (logits.detach().clone(), {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    assert rel_err(res[True][0], res[False][0]) < 1e-6
    gmax = max(float(v.abs().max()) for v in res[False][1].values())
    for n, gref in res[False][1].items():
        tiny = float((res[True][1][n] - gref).abs().max()) < 1e-7 * gmax
        assert rel_err(res[True][1][n], gref) < 2e-5 or tiny, n
    # the keep rate of what the next layer reads: fraction of zeros in a fused buffer ~ p (plus ELU's exact zeros: none)
    monkeypatch.setattr(models, "FUSE_OUTPUT_DROPOUT", True)


def test_state_dict_keys_follow_dgl_layout():
    """Checkpoint compatibility: parameter names/shapes as DGL's layers."""
    _, m = _build("st_pgat_spgnn_3")
    sd = m.state_dict()
    assert sd["gat.gat_layers.0.fc.weight"].shape == (512, 1063)
    assert sd["gat.gat_layers.0.res_fc.weight"].shape == (512, 1063)
    assert sd["gat.gat_layers.0.attn_l"].shape == (1, 2, 256) and sd["gat.gat_layers.0.bias"].shape == (512,)
    assert sd["gat.pgnn_layers.1.attn_r"].shape == (1, 1, 128) and sd["gat.pgnn_layers.0.fc.weight"].shape == (256, 39)
    assert sd["gat.gat_layers.3.fc.weight"].shape == (2048, 192) and sd["gnn_out.weight"].shape == (22, 1024)
    assert sum(p.numel() for p in m.parameters()) == 2501078
    for name, count in [("st_gat_3", 1931926), ("st_gat_6", 2031382), ("st_gcn_3", 392662), ("st_sage_3", 1898838)]:
        assert sum(p.numel() for p in _build(name)[1].parameters()) == count, name
    _, m = _build("st_gcn_3"); assert m.state_dict()["gcn.gcn_layers.0.weight"].shape == (1024, 256)
    _, m = _build("st_gin_3")
    assert {"gin.gin_layers.0.eps", "gin.gin_layers.0.apply_func.0.weight", "gin.gin_layers.3.apply_func.3.bias",
            "gnn_lobe_out.weight"} <= set(m.state_dict())
    _, m = _build("st_sage_3")
    assert m.state_dict()["sage.g_layers.0.fc_pool.weight"].shape == (1024, 1024)
    assert not any(k.startswith("gat.") and "res_fc" in k for k in _build("st_gat_3_nr")[1].state_dict())


def test_train_step_matches_torch_sgd_on_oracle():
    """Harness parity: given the same mask draws, three TrainStep steps equal three
    torch.optim.SGD(momentum) steps on the oracle's loss."""
    cfg, model = _build("st_gat_3", seed=2)
    model.eval()
    g = synthetic.make_batch(2, rank=1, device="cuda", pos_enc_dim=None)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    src, dst = g.cpu().edges()
    ref_p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()}
    opt = torch.optim.SGD(list(ref_p.values()), lr=0.01, momentum=0.9)
    ts = TrainStep(model, w, cfg.SAMPLING_RATE, 0.01, 0.9)
    gen = torch.Generator().manual_seed(11)
    y = g.ndata["y"].cpu()
    for _ in range(3):
        draws = torch.rand(y.shape[0], generator=gen)
        loss = ts.step(g, draws.cuda())
        opt.zero_grad()
        mask = draws < torch.where(y != 0, torch.tensor(1.0), torch.tensor(cfg.SAMPLING_RATE))
        ref = O.masked_weighted_ce(O.net_forward("gat", ref_p, src, dst, y.shape[0], g.ndata["fvs"].cpu())[0], y, mask,
                                   torch.tensor(w))
        ref.backward(); opt.step()
        assert rel_err(loss, ref) < TOL
    for k, v in model.named_parameters():
        assert rel_err(v, ref_p[k]) < 1e-5, k


# ---- size-independent properties at the BASELINE batch size -----------------------------------------
@pytest.fixture(scope="module")
def big():
    cfg, model = _build("st_pgat_spgnn_3")
    model.eval()
    samples = synthetic.synthetic_trees(512, rank=0)
    return cfg, model, samples, synthetic.batch_from_samples(samples, "cuda", 39)


def test_full_batch_equals_per_tree_and_is_deterministic(big):
    cfg, model, samples, g = big
    assert g.batch_size == 512 and g.number_of_edges() == 3 * g.number_of_nodes() - 2 * 512
    with torch.no_grad():
        a = model(g)[0]
        b = model(g)[0]
        assert torch.equal(a, b)                                    # no atomics: bitwise reproducible
        offs = np.cumsum([0] + g.batch_num_nodes_list)
        for i in (0, 255, 511):                                     # block-diagonal: tree i alone gives the same rows
            gi = synthetic.batch_from_samples(samples[i:i + 1], "cuda", 39)
            assert rel_err(a[offs[i]:offs[i + 1]], model(gi)[0]) < TOL
    refs, _ = _oracle(cfg, model, synthetic.batch_from_samples(samples[:2], "cuda", 39))
    assert rel_err(a[:offs[2]], refs[0]) < TOL                      # and those rows match the oracle


def test_full_batch_backward_is_bitwise_reproducible(big):
    """No atomics and no order-dependent reductions: at the BASELINE batch size every gradient must repeat bit for bit
    (the check that exposed the packed-op / cross-lane read hazard, DESIGN.md §4.1: a few wrong 16-lane sums per
    million elements, different on every run)."""
    cfg, model, samples, g = big
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS), device="cuda")
    y = g.ndata["y"]
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(1)).cuda() < 0.5
    runs = []
    for _ in range(3):
        model.zero_grad(set_to_none=True)
        masked_weighted_ce(model(g)[0], y, mask, w).backward()
        runs.append({n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None})
    model.zero_grad(set_to_none=True)
    for n in runs[0]:
        assert torch.equal(runs[0][n], runs[1][n]) and torch.equal(runs[1][n], runs[2][n]), n


def test_full_batch_attention_rows_sum_to_one_and_linearity(big):
    from spgnn_amd import ops
    _, _, _, g = big
    csc = g.csc()
    N, H, D = csc.num_nodes, 2, 256
    torch.manual_seed(0)
    ft1, ft2 = torch.randn(N, H * D, device="cuda"), torch.randn(N, H * D, device="cuda")
    el, er = torch.randn(N, H, device="cuda"), torch.randn(N, H, device="cuda")
    o1, _, attn = ops.gat_fwd_raw(csc, ft1, el, er, None, None, H, D, 0.2, 0)
    o2 = ops.gat_fwd_raw(csc, ft2, el, er, None, None, H, D, 0.2, 0)[0]
    o12 = ops.gat_fwd_raw(csc, ft1 + ft2, el, er, None, None, H, D, 0.2, 0)[0]
    assert rel_err(o12, o1 + o2) < 1e-5                             # linear in ft for fixed scores
    seg = torch.repeat_interleave(torch.arange(N, device="cuda"), (csc.indptr[1:] - csc.indptr[:-1]).long())
    sums = torch.zeros(N, H, device="cuda").index_add_(0, seg, attn)
    assert (sums - 1).abs().max().item() < 1e-5                     # softmax over in-neighbours
    const = torch.randn(1, H * D, device="cuda").expand(N, -1).contiguous()
    oc = ops.gat_fwd_raw(csc, const, el, er, None, None, H, D, 0.2, 0)[0]
    assert rel_err(oc, const) < 1e-5                                # constant rows: out == ft


def test_graph_replay_matches_eager_and_refreshes_dropout():
    """TrainStep.capture: replays of the captured step train like eager steps; with dropout on, successive
    replays draw different attention-dropout masks (device seed counter) and losses stay finite."""
    from spgnn_amd import ops as _ops
    cfg, model = _build("st_gat_3", seed=3)
    g = synthetic.make_batch(4, rank=2, device="cuda", pos_enc_dim=None)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    model.eval()                                           # deterministic arithmetic: replay == eager
    eager = copy.deepcopy(model)
    ts_g = TrainStep(model, w, 1.0, 1e-3, 0.9)             # sampling rate 1: the mask does not depend on the RNG
    ts_e = TrainStep(eager, w, 1.0, 1e-3, 0.9)
    ts_g.capture(g, warmup=2)                              # two eager warm-up steps; the capture itself executes nothing
    for _ in range(3):
        lg = ts_g.replay()
    for _ in range(5):
        le = ts_e.step(g)
    assert torch.isfinite(lg) and rel_err(lg, le) < 1e-5
    n = ts_g.bucket.numel
    assert rel_err(ts_g.bucket.flat_param[:n], ts_e.bucket.flat_param[:n]) < 1e-6     # 2 + 3 steps == 5 steps
    _ops.DROPOUT_SEED_OFFSET = None
    # fresh attention-dropout masks per replay
    cfg, model = _build("st_gat_3", seed=4)
    model.train()
    ts = TrainStep(model, w, 1.0, 0.0, 0.0)                # lr 0: parameters frozen, only the masks change
    ts.capture(g, warmup=1)
    l1 = float(ts.replay()); l2 = float(ts.replay()); l3 = float(ts.replay())
    assert len({l1, l2, l3}) == 3 and all(np.isfinite([l1, l2, l3]))
    _ops.DROPOUT_SEED_OFFSET = None


def test_wide_range_products_model_parity_and_the_auto_policy(monkeypatch):
    """ops.GEMM_WIDE (SPGNN_GEMM_WIDE, round 4): the flagship model with every split product in its wide-range form - logits
    and loss gradients against the oracle at the usual bars - and TrainStep(range_policy="auto"): once the range monitor's
    counter moves, the next loader batch switches the process to the wide form and drops the narrow captures."""
    from spgnn_amd import ops as _ops
    monkeypatch.setattr(_ops, "GEMM_WIDE", True)
    cfg, model = _build("st_pgat_spgnn_3", seed=10)
    g = synthetic.make_batch(5, rank=6, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    model.eval()
    outs = model(g)
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS))
    y = g.ndata["y"]
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(4)) < 0.5
    masked_weighted_ce(outs[0], y, mask.cuda(), w.cuda()).backward()
    refs, sd = _oracle(cfg, model, g, grad=True)
    for o, r in zip(outs, refs):
        assert rel_err(o, r) < TOL
    O.masked_weighted_ce(refs[0], y.cpu(), mask, w).backward()
    for n, p in model.named_parameters():
        if p.requires_grad and p.grad is not None and sd[n].grad is not None and float(sd[n].grad.abs().max()) > 1e-6:
            assert rel_err(p.grad, sd[n].grad) < 1e-4, n
    # the policy: narrow until the monitor reports, wide afterwards
    monkeypatch.setattr(_ops, "GEMM_WIDE", False)
    cfg, model = _build("st_gat_3", seed=11)
    model.eval()
    ts = TrainStep(model, class_weight_list(cfg.CLASS_WEIGHTS), 1.0, 1e-3, 0.9, range_policy="auto")
    g1 = synthetic.make_batch(4, rank=1, device="cuda", pos_enc_dim=None)
    l1 = float(ts.run_batch(g1, 4, granule=1024))
    assert not _ops.GEMM_WIDE and len(ts._captures) == 1
    _ops.scale_pool(g1.device).violations.add_(1)            # what spgnn_step_begin does when a product flagged its operand
    l2 = float(ts.run_batch(g1, 4, granule=1024))
    assert _ops.GEMM_WIDE and len(ts._captures) == 1 and np.isfinite([l1, l2]).all()
    assert abs(l2 - l1) < 0.5 * abs(l1)                       # training continued from the same parameters
    _ops.DROPOUT_SEED_OFFSET = None


@pytest.mark.parametrize("name,bf16", [("st_pgat_spgnn_3", False), ("st_gat_3", False), ("st_gat_6", True)])
def test_deferred_attention_vector_gradients_are_bit_identical(name, bf16, monkeypatch):
    """ops.AttnGradQueue (round 4): a training step collects every GATConv's attention-vector gradient pass during backward
    and runs them as ONE spgnn_scores_bwd_w_multi launch afterwards.  The flat gradient bucket - every parameter's gradient,
    attn_l / attn_r included - is bit for bit what the per-layer launches give, and an eager ``loss.backward()`` outside a
    step (no queue) still fills the attention vectors' gradients through autograd."""
    from spgnn_amd import ops as _ops
    cfg, model = _build(name, seed=8)
    if bf16:
        models.set_storage_dtype(model, torch.bfloat16)
    model.eval()
    g = synthetic.make_batch(5, rank=2, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    grads = []
    for defer in (True, False):
        monkeypatch.setattr(_ops, "DEFER_ATTN_GRADS", defer)
        ts = TrainStep(copy.deepcopy(model), w, 1.0, 1e-3, 0.9)
        ts._front(g)
        grads.append(ts.bucket.flat_grad.clone())
        names = [n for n, p in ts.model.named_parameters() if p.requires_grad]
        assert any("attn_l" in n for n in names)
    assert torch.equal(grads[0], grads[1])
    assert _ops.ATTN_GRAD_QUEUE is None
    m2 = copy.deepcopy(model)
    m2(g)[0].square().mean().backward()                       # plain autograd: the layers run their own passes
    for n, p in m2.named_parameters():
        if "attn_" in n and p.requires_grad and "lobe" not in n and "lung" not in n:
            assert p.grad is not None and torch.isfinite(p.grad).all(), n
    _ops.DROPOUT_SEED_OFFSET = None


@pytest.mark.parametrize("name,bf16", [("st_pgat_spgnn_3", False), ("st_pgat_spgnnnl_3", False), ("st_gat_3", False), ("st_gat_1", False),
                                       ("st_gat_6", True), ("st_gcn_3", False), ("st_gin_3", False), ("st_sage_3", False)])
def test_step_wide_deferred_sums_are_bit_identical(name, bf16, monkeypatch):
    """ops.StepSums (round 4): inside a training step the split-K reductions behind the weight gradients wait for ONE launch
    after the backward pass.  That is only sound for outputs nothing reads before then - a gradient that feeds another
    autograd node, or one of two gradients of the same parameter (the aggregate-first output layer's fc.weight), must stay
    in its node's own launch (SumJobs(local=True)).  Every model family: the flat gradient bucket with the step-wide queue
    equals the one without it bit for bit, over two steps (the second starts from parameters the first one moved)."""
    from spgnn_amd import ops as _ops
    cfg, model = _build(name, seed=9)
    if bf16:
        models.set_storage_dtype(model, torch.bfloat16)
    model.eval()
    g = synthetic.make_batch(6, rank=3, device="cuda", pos_enc_dim=getattr(cfg, "POS_ENC_DIM", None))
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    out = []
    monkeypatch.setattr(_ops, "DEBUG_POISON_DEFERRED", True)      # deferred outputs start as NaN: an early read cannot pass unnoticed
    for defer in (True, False):
        monkeypatch.setattr(_ops, "DEFER_STEP_SUMS", defer)
        ts = TrainStep(copy.deepcopy(model), w, 1.0, 1e-3, 0.9)
        ts.step(g)
        ts._front(g)
        out.append((ts.bucket.flat_grad.clone(), ts.bucket.flat_param.clone()))
        assert _ops.STEP_SUMS is None
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[0][0]).all() and float(out[0][0].abs().max()) > 0
    _ops.DROPOUT_SEED_OFFSET = None


def test_two_gatconvs_sharing_their_attention_vectors_get_the_summed_gradient(monkeypatch):
    """AttnGradQueue.flush ADDS to a parameter that already holds a gradient or that two recorded passes share;
    under the step-wide queue those sums were still unfilled memory at that point.  Two GATConv layers of st_gat_3 share
    attn_l / attn_r (same shape): the step's gradient for the shared vectors must equal plain autograd's (which adds the two
    layers' contributions), with the deferred outputs poisoned with NaN so that an early read cannot pass."""
    from spgnn_amd import ops as _ops
    cfg, model = _build("st_gat_6", seed=12)
    model.eval()
    layers = model.gat.gat_layers
    a, b = layers[3], layers[4]                                   # two 128 -> 2 x 64 hidden layers
    assert a.attn_l.shape == b.attn_l.shape
    b.attn_l, b.attn_r = a.attn_l, a.attn_r                       # shared parameters
    g = synthetic.make_batch(5, rank=4, device="cuda", pos_enc_dim=None)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    monkeypatch.setattr(_ops, "DEBUG_POISON_DEFERRED", True)
    got = {}
    for defer in (True, False):
        monkeypatch.setattr(_ops, "DEFER_ATTN_GRADS", defer)
        monkeypatch.setattr(_ops, "DEFER_STEP_SUMS", defer)
        m = copy.deepcopy(model)
        assert m.gat.gat_layers[4].attn_l is m.gat.gat_layers[3].attn_l
        ts = TrainStep(m, w, 1.0, 1e-3, 0.9)
        ts._front(g)
        got[defer] = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    for n, v in got[False].items():
        assert torch.isfinite(got[True][n]).all(), n
        scale = float(v.abs().max()) + 1e-30
        assert float((got[True][n] - v).abs().max()) <= 2e-6 * scale, n      # (a + b) vs (b + a): fp32 rounding only
    shared = got[True]["gat.gat_layers.3.attn_l"]
    assert float(shared.abs().max()) > 0
    _ops.DROPOUT_SEED_OFFSET = None


def test_step_wide_sums_raise_when_autograd_copied_an_unfilled_gradient(monkeypatch):
    """the step-wide queue is sound only while autograd takes every deferred output over untouched.  The first step
    of a TrainStep proves that for its model (deferred outputs start as NaN; a NaN in the gathered bucket = an early read).
    A gradient hook on a weight makes autograd hand the hook's result - computed from the unfilled tensor - on instead: the
    step must raise, not train on garbage.  (fc.weight's gradient is one of two views of a deferred output, the other being
    res_fc.weight's: a storage-level check alone would not see this.)"""
    from spgnn_amd import ops as _ops
    cfg, model = _build("st_gat_3", seed=13)
    model.eval()
    g = synthetic.make_batch(4, rank=5, device="cuda", pos_enc_dim=None)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    ts = TrainStep(copy.deepcopy(model), w, 1.0, 1e-3, 0.9)
    ts._front(g)                                                   # sound as built: the proof passes and is not repeated
    assert not ts._verify_deferred and torch.isfinite(ts.bucket.flat_grad).all()
    m2 = copy.deepcopy(model)
    h = m2.gat.gat_layers[1].fc.weight.register_hook(lambda gr: gr * 1.0)
    ts2 = TrainStep(m2, w, 1.0, 1e-3, 0.9)
    with pytest.raises(RuntimeError, match="deferred split-K gradient sum"):
        ts2._front(g)
    assert _ops.STEP_SUMS is None and _ops.ATTN_GRAD_QUEUE is None and not _ops.DEBUG_POISON_DEFERRED
    monkeypatch.setattr(_ops, "DEFER_STEP_SUMS", False)           # the documented way out
    ts3 = TrainStep(m2, w, 1.0, 1e-3, 0.9)
    ts3._front(g)
    h.remove()
    assert torch.isfinite(ts3.bucket.flat_grad).all()
    # a sole-alias gradient that autograd replaced is also caught by the per-step storage check (no host read)
    monkeypatch.setattr(_ops, "DEFER_STEP_SUMS", True)
    m4 = copy.deepcopy(model)
    ts4 = TrainStep(m4, w, 1.0, 1e-3, 0.9)
    ts4._front(g)
    h = m4.gnn_out.weight.register_hook(lambda gr: gr * 1.0)
    try:
        ts4._front(g)
        caught = False
    except RuntimeError:
        caught = True
    h.remove()
    print("storage-level check caught a hook on the classifier weight:", caught)
    _ops.DROPOUT_SEED_OFFSET = None


@pytest.mark.parametrize("N,C", [(1000, 22), (1, 22), (257, 3), (4096, 64)])
def test_fused_masked_ce_matches_cross_entropy(N, C):
    """spgnn_masked_ce == F.cross_entropy(pre[mask], y[mask], weight=w) (reference job_runner.py:1896-1900): loss
    value, and the gradient it leaves behind, against the oracle's formulation and against torch's own op."""
    from spgnn_amd import ops
    torch.manual_seed(N + C)
    logits = (torch.randn(N, C, device="cuda") * 3).requires_grad_(True)
    y = torch.randint(0, C, (N,), device="cuda")
    w = torch.rand(C, device="cuda") + 0.1
    p = torch.where(y != 0, torch.tensor(1.0, device="cuda"), torch.tensor(0.15, device="cuda"))
    draws = torch.rand(N, device="cuda")
    if N == 1:
        draws.zero_()
    mask = draws < p
    nd = ops.masked_ce_sums(logits, y, draws, p, w)
    loss = nd[0] / nd[1]
    loss.backward()
    lo = logits.detach().cpu().double().requires_grad_(True)
    ref = O.masked_weighted_ce(lo, y.cpu(), mask.cpu(), w.cpu().double())
    ref.backward()
    assert rel_err(loss, ref) < 1e-6 and rel_err(logits.grad, lo.grad) < 1e-5
    lt = logits.detach().clone().requires_grad_(True)
    ref_t = torch.nn.functional.cross_entropy(lt[mask], y[mask], weight=w)
    ref_t.backward()
    assert rel_err(loss, ref_t) < 1e-6 and rel_err(logits.grad, lt.grad) < 1e-5


def _mask_draws_host(seed: int, offset: int, n: int) -> np.ndarray:
    """Host restatement of spgnn_masked_ce_step's draw: 24 bits of mix64(seed + 0xD1B54A32D192ED03 * offset, i) / 2^24."""
    M = (1 << 64) - 1
    out = np.empty(n, dtype=np.float32)
    sd = (seed + 0xD1B54A32D192ED03 * offset) & M
    for i in range(n):
        z = (sd + 0x9E3779B97F4A7C15 * (i + 1)) & M
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        z ^= z >> 31
        out[i] = np.float32(z >> 40) * np.float32(1.0 / 16777216.0)
    return out


def test_masked_ce_draws_its_own_mask_and_sums_in_the_last_workgroup():
    """draws=None: the kernel's counter-hash mask (restated on the host) gives the sums of the explicit-draws call bit for
    bit, moves with the device step counter, is uniform, and the last-workgroup totals are repeatable launch after launch."""
    from spgnn_amd import ops
    torch.manual_seed(5)
    N, C = 5000, 22
    logits = torch.randn(N, C, device="cuda") * 2
    y = torch.randint(0, C, (N,), device="cuda")
    w = torch.rand(C, device="cuda") + 0.1
    p = torch.where(y != 0, torch.tensor(1.0, device="cuda"), torch.tensor(0.15, device="cuda"))
    ctr = torch.tensor([3], dtype=torch.int64, device="cuda")
    seed = 0x1234567890ABCDEF & ((1 << 62) - 1)
    prev = ops.DROPOUT_SEED_OFFSET
    try:
        ops.DROPOUT_SEED_OFFSET = ctr
        out = torch.zeros(2, device="cuda")
        a = [t.clone() for t in ops.masked_ce_sums(logits, y, None, p, w, out=out, draw_seed=seed)]
        host = torch.from_numpy(_mask_draws_host(seed, 3, N)).cuda()
        b = ops.masked_ce_sums(logits, y, host, p, w)
        assert float(a[0]) == float(b[0]) and float(a[1]) == float(b[1]) and float(out[1]) == float(a[1])
        for _ in range(20):                                       # arrival order of the workgroups must not show
            c = ops.masked_ce_sums(logits, y, None, p, w, draw_seed=seed)
            assert float(c[0]) == float(a[0]) and float(c[1]) == float(a[1])
        ctr.add_(1)
        d = ops.masked_ce_sums(logits, y, None, p, w, draw_seed=seed)
        assert float(d[1]) != float(a[1])
    finally:
        ops.DROPOUT_SEED_OFFSET = prev
    u = _mask_draws_host(seed, 0, 20000)
    assert abs(float(u.mean()) - 0.5) < 0.01 and abs(float((u < 0.15).mean()) - 0.15) < 0.01 and u.min() >= 0.0 and u.max() < 1.0
    ref = O.masked_weighted_ce(logits.cpu().double(), y.cpu(), (host < p).cpu(), w.cpu().double())
    assert rel_err(a[0] / a[1], ref) < 1e-6
    # unit_grad: the stored gradient is handed on as it is
    lg = logits.clone().requires_grad_(True)
    n1 = ops.masked_ce_sums(lg, y, host, p, w, unit_grad=True)[0]
    torch.autograd.backward(n1, torch.ones((), device="cuda"))
    lg2 = logits.clone().requires_grad_(True)
    ops.masked_ce_sums(lg2, y, host, p, w)[0].backward()
    assert torch.equal(lg.grad, lg2.grad)
    # ... and, for the node that produced the logits, carries its own column sums (the classifier bias' gradient), formed by the
    # kernel's last workgroup in block order
    seen = {}

    class Probe(torch.autograd.Function):
        @staticmethod
        def forward(ctx, t):
            return t.clone()

        @staticmethod
        def backward(ctx, g_):
            seen["attr"] = getattr(g_, "_spgnn_colsum", None)
            seen["cs"] = ops.column_sums(g_)
            return g_

    lg3 = logits.clone().requires_grad_(True)
    n3 = ops.masked_ce_sums(Probe.apply(lg3), y, host, p, w, unit_grad=True)[0]
    torch.autograd.backward(n3, torch.ones((), device="cuda"))
    assert seen["attr"] is not None and seen["cs"] is seen["attr"]
    assert rel_err(seen["cs"], lg2.grad.double().sum(0)) < 1e-6
    assert ops.column_sums(lg2.grad).shape == (C,) and getattr(lg2.grad, "_spgnn_colsum", None) is None


# ---- the N > 1 step as HIP-graph replays: two processes on the one GPU, gloo carrying the CUDA tensors ----------------
def _dp_graph_worker(rank, world, port, ret):
    import torch.distributed as dist
    from spgnn_amd import models, synthetic
    from spgnn_amd.configs import class_weight_list, get_config
    from spgnn_amd.train import TrainStep
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = get_config("st_pgat_spgnn_3")
    out = {}
    for mode in ("eager", "graph"):
        torch.manual_seed(0)
        model = models.build_model(cfg.MODEL).cuda()
        model.init(None); model.set_gcn_only(); model.eval()          # deterministic arithmetic: replay == eager
        g = synthetic.make_batch(3, rank=rank, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
        ts = TrainStep(model, class_weight_list(cfg.CLASS_WEIGHTS), 1.0, 0.05, 0.9, seed=5)   # sampling rate 1: no draws
        if mode == "eager":
            losses = [float(ts.step(g)) for _ in range(5)]
        else:
            ts.capture(g, warmup=2)                                   # two eager steps, then three replays
            losses = [float(ts.replay()) for _ in range(3)]
        out[mode] = (losses, ts.bucket.flat_param[:ts.bucket.numel].detach().cpu().clone())
    ret[rank] = out
    dist.destroy_process_group()


def test_two_rank_graph_replay_equals_two_rank_eager():
    """TrainStep.capture with world_size 2: the front graph, the eager all-reduces, the back graph.  Both ranks end
    with the same parameters, equal to those of five eagerly issued 2-rank steps (RCCL is replaced by gloo here: two
    ranks cannot share one GPU under RCCL; the graphs and their hand-over are what is tested)."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(_dp_graph_worker, args=(2, port, ret), nprocs=2, join=True)
    for r in (0, 1):
        le, pe = ret[r]["eager"]
        lg, pg = ret[r]["graph"]
        assert all(np.isfinite(le)) and all(np.isfinite(lg))
        assert np.allclose(le[2:], lg, rtol=1e-5), (le, lg)
        assert torch.allclose(pe, pg, rtol=1e-5, atol=1e-7)
    assert torch.equal(ret[0]["graph"][1], ret[1]["graph"][1])      # replicas stay identical


def _dp_cycle_worker(rank, world, port, ret):
    import torch.distributed as dist
    from spgnn_amd import models, synthetic
    from spgnn_amd.configs import class_weight_list, get_config
    from spgnn_amd.train import TrainStep
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg = get_config("st_gat_3")
    out = {}
    for mode in ("eager", "cycle"):
        torch.manual_seed(0)
        model = models.build_model(cfg.MODEL).cuda()
        model.init(None); model.set_gcn_only(); model.eval()
        ts = TrainStep(model, class_weight_list(cfg.CLASS_WEIGHTS), 1.0, 0.02, 0.9, seed=5)
        losses = []
        for b in range(3):                                            # three loader batches; rank 1's are larger (other size classes)
            g = synthetic.make_batch(3 + rank + (b % 2), rank=10 * b + rank, device="cuda", pos_enc_dim=None)
            if mode == "eager":
                for _ in range(4):
                    l = ts.step(g)
            else:
                l = ts.run_batch(g, 4, granule=512)                   # the first batch of a class: 3 warm-up steps + 1 replay
            losses.append(float(l))
        out[mode] = (losses, ts.bucket.flat_param[:ts.bucket.numel].detach().cpu().clone(), len(ts._captures))
    ret[rank] = out
    dist.destroy_process_group()


def test_two_rank_loader_batch_cycle_equals_two_rank_eager():
    """The loader-batch cycle with world_size 2 (gloo on the one GPU): every rank pads its own batches into its own size classes
    and captures when IT meets a new class - a rank replaying while its peer is warming up still issues exactly one all-reduce
    per step, so the collectives line up; losses and parameters follow the eager 2-rank run and the replicas stay identical."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(_dp_cycle_worker, args=(2, port, ret), nprocs=2, join=True)
    for r in (0, 1):
        le, pe, _ = ret[r]["eager"]
        lc, pc, ncap = ret[r]["cycle"]
        assert ncap >= 1 and all(np.isfinite(le)) and all(np.isfinite(lc))
        assert np.allclose(le, lc, rtol=1e-4), (le, lc)
        assert rel_err(pc, pe) < 1e-4                                 # normwise: padding moves fp32 summation order (tests/test_arena.py)
    assert torch.equal(ret[0]["cycle"][1], ret[1]["cycle"][1])


def test_sage_feature_dropout_in_the_previous_layers_epilogue(monkeypatch):
    """SAGE in training mode: layer l + 1's feature dropout applied by layer l's last product (models.FUSE_SAGE_DROP) - same
    seeds, same masks: logits equal the layer-by-layer form bit for bit, gradients to the rounding of ELU's recovered value."""
    from spgnn_amd import synthetic
    cfg = get_config("st_sage_3")
    g = synthetic.make_batch(8, rank=3, device="cuda", pos_enc_dim=None)
    res = {}
    for fused in (True, False):
        monkeypatch.setattr(models, "FUSE_SAGE_DROP", fused)
        torch.manual_seed(0)
        model = models.build_model(cfg.MODEL).cuda(); model.init(None); model.set_gcn_only(); model.train(True)
        torch.manual_seed(5)
        logits, emb = model(g)
        (logits * torch.linspace(-1, 1, logits.shape[1], device="cuda")).sum().backward()
        res[fused] = (logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None})
    assert torch.equal(res[True][0], res[False][0])
    assert set(res[True][1]) == set(res[False][1]) and len(res[True][1]) >= 20
    for n in res[True][1]:
        assert rel_err(res[True][1][n], res[False][1][n]) < 2e-6, n
    kept = float((res[True][0] != 0).float().mean())
    assert kept > 0.99


def test_bench_two_rank_rehearsal_through_self_launch():
    """`python3 bench.py --gpus 2` with no launcher and no WORLD_SIZE: bench.py starts both ranks itself (before any GPU call),
    they run the whole N > 1 flow of the training step on the one GPU of this box (SPGNN_BENCH_REHEARSAL=1: gloo moves the
    bucket, RCCL refuses two ranks per device), rank 0 prints ONE line with n_gpus 2, and the flat keys the driver's record
    keeps are there.  The numbers of a rehearsal mean nothing; the protocol is what is checked."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SPGNN_BENCH_REHEARSAL="1")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "3", "--trees", "8",
                        "--no-secondary"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["steps"] == 4 and out["warmup"] == 3 and out["scaling"] == "weak"
    c = out["config"]
    assert c["comm_world_size"] == 2 and c["comm_backend"].startswith("gloo") and c["global_trees"] == 16
    assert c["launch"] == "hip-graph replay", c.get("capture_error")
    assert c["allreduce_ms_p50"] > 0.0 and 4 * 2501080 <= c["comm_bucket_bytes"] <= 4 * 2501080 + 64       # 2 501 078 parameters + the two loss slots, 16-byte parameter starts
    assert out["value"] > 0 and np.isfinite(out["loss"])
    assert out["roofline"]["hbm_frac"] > 0 and out["roofline"]["hbm_ms_per_step"] > 0


def test_bench_real_launcher_and_rccl_with_one_rank():
    """The REAL (non-rehearsal) N > 1 launcher path as far as one GPU allows: SPGNN_BENCH_FORCE_LAUNCH=1
    makes `bench.py --gpus 1` take self_launch - whose parent counts GPUs from /sys and never calls torch.cuda - and its one
    child initialise the "nccl" (= RCCL) process group at world size 1, run the multi-rank step (two HIP graphs around the
    real TrainStep._reduce -> dist.all_reduce on the flat bucket) and report the collective on the line."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, SPGNN_BENCH_FORCE_LAUNCH="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "SPGNN_BENCH_REHEARSAL", "SPGNN_BENCH_DRY", "SPGNN_BENCH_CHILD"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "3", "--trees", "8",
                        "--no-secondary", "--no-cpu-baseline"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    c = out["config"]
    assert out["n_gpus"] == 1 and c["comm_world_size"] == 1 and c["comm_backend"].startswith("nccl"), c
    assert c["launch"] == "hip-graph replay", c.get("capture_error")
    assert c["allreduce_ms_p50"] > 0.0 and 4 * 2501080 <= c["comm_bucket_bytes"] <= 4 * 2501080 + 64
    assert out["value"] > 0 and np.isfinite(out["loss"])
    # ... and the all-reduce with one rank changes nothing: the same run without the forced exchange gives the same loss
    env2 = {k: v for k, v in env.items() if k != "SPGNN_BENCH_FORCE_LAUNCH"}
    r2 = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "3", "--trees", "8",
                         "--no-secondary", "--no-cpu-baseline"], env=env2, capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0, r2.stderr[-3000:]
    out2 = json.loads([ln for ln in r2.stdout.splitlines() if ln.strip()][0])
    assert out2["config"]["comm_backend"].startswith("none") and out2["loss"] == pytest.approx(out["loss"], rel=1e-6)


@pytest.mark.parametrize("name,trees", [("st_pgat_spgnn_3", 5), ("st_gin_3", 5), ("st_pgat_spgnn_3", 40)])
def test_classifier_weight_gradient_rides_in_act_bwd_proj(name, trees, monkeypatch):
    """ops.ACT_BWD_PROJ_WGRAD (round 5): the classifier's weight gradient g_logits^T mean_h(out) (reference gnn_out on the head
    mean, models.py:482, 1125) is formed by spgnn_act_bwd_proj_wgrad from the rows that pass reads anyway, instead of a second
    pass over the (N, 1024) head mean.  Every other gradient is bit-identical; gnn_out.weight differs by summation order only."""
    from spgnn_amd import ops as _ops
    cfg, model = _build(name, seed=21)
    model.eval()
    g = synthetic.make_batch(trees, rank=7, device="cuda", pos_enc_dim=getattr(cfg, "POS_ENC_DIM", None))
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    got = {}
    for ride in (True, False):
        monkeypatch.setattr(_ops, "ACT_BWD_PROJ_WGRAD", ride)
        m = copy.deepcopy(model)
        ts = TrainStep(m, w, 1.0, 1e-3, 0.9)
        ts._front(g)
        got[ride] = {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}
    assert "gnn_out.weight" in got[True]
    for n, v in got[False].items():
        if n == "gnn_out.weight":
            assert rel_err(got[True][n], v) < 2e-6 and float(v.abs().max()) > 0, (n, rel_err(got[True][n], v))
        else:
            assert torch.equal(got[True][n], v), n
    _ops.DROPOUT_SEED_OFFSET = None


@pytest.mark.parametrize("name,trees,min_rows", [("st_pgat_spgnn_3", 6, 1), ("st_gat_3", 6, 1), ("st_pgat_spgnnnl_3", 5, 1), ("st_gin_3", 5, 1),
                                                   ("st_pgat_spgnn_3", 230, 32768)])
def test_side_stream_weight_gradients_are_bit_identical(name, trees, min_rows, monkeypatch):
    """ops.SideLaunch (round 5): a training step issues its weight-gradient products on a side stream, behind the input-gradient
    products, so that they run next to the following level's traversals.  Only the ORDER of launches and the stream change:
    the flat gradient bucket and the parameters after two steps are bit for bit those of the single-stream step - eagerly issued
    and as HIP-graph replays (which leave the side stream out unless ops.OVERLAP_TN_IN_GRAPHS) - with the deferred outputs poisoned
    with NaN so that a sum reading a partial before the join could not pass."""
    from spgnn_amd import ops as _ops
    cfg, model = _build(name, seed=17)
    model.eval()                                     # (the layers' dropout seeds come from torch's global generator: two step objects
    g = synthetic.make_batch(trees, rank=8, device="cuda", pos_enc_dim=getattr(cfg, "POS_ENC_DIM", None))   # would draw different masks)
    assert g.number_of_nodes() >= min_rows
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    monkeypatch.setattr(_ops, "OVERLAP_TN_MIN_ROWS", min_rows)
    monkeypatch.setattr(_ops, "DEBUG_POISON_DEFERRED", True)
    got = {}
    for side in (True, False):
        monkeypatch.setattr(_ops, "OVERLAP_TN", side)
        ts = TrainStep(copy.deepcopy(model), w, cfg.SAMPLING_RATE, 1e-3, 0.9, seed=3)
        ts.step(g); ts._front(g)
        eager = (ts.bucket.flat_grad.clone(), ts.bucket.flat_param.clone())
        ts2 = TrainStep(copy.deepcopy(model), w, cfg.SAMPLING_RATE, 1e-3, 0.9, seed=3)
        ts2.capture(g, warmup=1)
        ts2.replay(); ts2.replay()
        torch.cuda.synchronize()
        got[side] = (eager, ts2.bucket.flat_param.clone(), float(ts2._static_loss))
        assert _ops.TN_SIDE is None
    assert torch.equal(got[True][0][0], got[False][0][0]) and torch.equal(got[True][0][1], got[False][0][1])
    assert torch.isfinite(got[True][0][0]).all() and float(got[True][0][0].abs().max()) > 0
    assert torch.equal(got[True][1], got[False][1]) and got[True][2] == got[False][2]
    _ops.DROPOUT_SEED_OFFSET = None


@pytest.mark.gpu
def test_training_step_splits_its_node_data_once_per_batch():
    """Guard for a silent regression (docs/HISTORY.md, round 5): the products of a TRAINING step must find the pre-split image of
    the batch's constant node data (ops.const_operand) - the test that skips it for single inference passes may not look at
    torch.is_grad_enabled(), which is False inside every autograd.Function.forward."""
    from spgnn_amd import models, ops, synthetic
    from spgnn_amd.configs import class_weight_list, get_config
    from spgnn_amd.train import TrainStep
    cfg = get_config("st_pgat_spgnn_3")
    torch.manual_seed(0)
    model = models.build_model(cfg.MODEL).cuda()
    model.init(None)
    model.set_gcn_only()
    g = synthetic.make_batch(4, rank=0, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    ts = TrainStep(model, class_weight_list(cfg.CLASS_WEIGHTS), cfg.SAMPLING_RATE, 1e-4, 0.9)
    ts.step(g)
    consts = [t for t in list(g._tensor_cache.values()) + list(g.ndata.values()) if getattr(t, "_spgnn_const", False)]
    assert consts and ops.A_PRESPLIT and ops.PRESPLIT_B
    split = [t for t in consts if getattr(t, "_spgnn_aps", None)]
    assert split, "no constant node-data tensor carries a pre-split image after a training step"
    model.eval()
    g2 = synthetic.make_batch(4, rank=1, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    with torch.no_grad():
        model(g2)                                   # a single inference pass: no split pass, no image
    assert not [t for t in list(g2._tensor_cache.values()) + list(g2.ndata.values()) if getattr(t, "_spgnn_aps", None)]
