"""bf16-STORAGE path (BASELINE.json config 4: "st_gat_6 deep GAT, batch=512 trees, bf16").

The reference is fp32 only, so there is no reference result in bf16; what is checked is
  (1) the kernels against an exact model of what they are meant to do: the oracle with bf16 rounding applied at the
      product's storage points (``oracle.dgl_cpu.Bf16Storage``: inputs, weights fed to the GEMMs, ft / res / out and the
      gradients g_pre / g_ft / g_x), arithmetic in between in fp64.  The HIP path differs from that model only by fp32
      accumulation order, which can move a value across a bf16 rounding boundary (one ulp = 2^-8 relative of THAT
      element); tolerance below: normwise 2^-7 per tensor, and a small fraction of elements off by more than fp32 noise;
  (2) the distance to the true fp64 oracle, bounded by what bf16 storage costs: <= 4x the distance of the storage model
      itself to fp64 (+ a floor), stated per test.
The fp32 path stays the parity path (tests/test_hip_models.py, 1e-5)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import dgl_cpu as O
from spgnn_amd import models, nn as snn, ops, ops_bf16, synthetic
from spgnn_amd.configs import class_weight_list, get_config
from spgnn_amd.graph import TreeGraph
from spgnn_amd.train import TrainStep, masked_weighted_ce
from tests.util import close_to_model as _close_to_model
from tests.util import rel_err, tree_batch_edges

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
ULP = 2.0 ** -8            # bf16: 8 significant bits, round to nearest: relative rounding error <= 2^-9, one ulp = 2^-8


def _rows(x):
    return ops_bf16.cast_rows(x.float().cuda())


# ----------------------------------------------------------------------------------------------------------------
# GEMMs
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", [(1, 4, 8), (77, 64, 32), (300, 128, 64), (513, 256, 128), (1000, 512, 1063),
                                   (2049, 132, 40), (4100, 1024, 200), (131, 4096, 128)])
def test_gemm_nt_bf16_exact_on_integers(M, N, K):
    """fp32 output, small-integer operands: every product and partial sum is exact, so any tile / fragment / ragged-K
    (K % 64 != 0, chunks redirected to the zero line) / edge-row mistake shows as an integer error."""
    g = torch.Generator().manual_seed(M * 7 + N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    b = torch.randint(-3, 4, (N, K), generator=g).float()
    out = ops_bf16.gemm_nt(_rows(a), _rows(b), out_f32=True)
    assert torch.equal(out.cpu(), a @ b.t())
    out16 = ops_bf16.gemm_nt(_rows(a), _rows(b))
    assert out16.dtype == BF and torch.equal(out16.float().cpu(), (a @ b.t()).to(BF).float())


@pytest.mark.parametrize("M,N,K", [(300, 128, 64), (1000, 512, 1063), (2049, 132, 40), (777, 1024, 200), (260, 260, 264),
                                   (260, 260, 8), (300, 132, 96), (515, 256, 104), (300, 128, 160), (258, 64, 192)])
def test_gemm_nt_bf16_every_tile_variant(M, N, K):
    """128 x 128, 256 x 128 and 256 x 256 (waves of 128 x 64) block tiles: exact on integers, bit-identical to each other on
    random data with bias + ELU and with the score partials, fp32 and bf16 results, ragged rows / columns / K; 1 to 34 k
    stages of 32 (the kernels keep 3 or 4 stages in flight and peel the last: fewer stages than buffers, as many, one more)."""
    g = torch.Generator().manual_seed(M + N + K)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    b = torch.randint(-3, 4, (N, K), generator=g).float()
    for tile in (2, 4, 5):
        assert torch.equal(ops_bf16.gemm_nt(_rows(a), _rows(b), out_f32=True, tile=tile).cpu(), a @ b.t()), tile
    ar, br = _rows(torch.randn(M, K, generator=g)), _rows(torch.randn(N, K, generator=g) / 8)
    bias = torch.randn(N, generator=g).cuda()
    ref32 = ops_bf16.gemm_nt(ar, br, out_f32=True, bias=bias, act=ops.ACT_ELU, tile=2)
    ref16 = ops_bf16.gemm_nt(ar, br, bias=bias, act=ops.ACT_ELU, tile=2)
    for tile in (4, 5):
        assert torch.equal(ops_bf16.gemm_nt(ar, br, out_f32=True, bias=bias, act=ops.ACT_ELU, tile=tile), ref32), tile
        assert torch.equal(ops_bf16.gemm_nt(ar, br, bias=bias, act=ops.ACT_ELU, tile=tile).view(torch.int16), ref16.view(torch.int16)), tile
    C = N // 64 * 64
    if C:
        sl, sr = torch.randn(C, generator=g).cuda(), torch.randn(C, generator=g).cuda()
        parts = {}
        for tile in (2, 4, 5):
            parts[tile] = torch.empty((M, C // 64, 2), dtype=torch.float32, device="cuda")
            ops_bf16.gemm_nt(ar, br, score_l=sl, score_r=sr, score_out=parts[tile], tile=tile)
        assert torch.equal(parts[4], parts[2]) and torch.equal(parts[5], parts[2])


def test_gemm_nt_bf16_asymmetric_identity():
    """A = I with an asymmetric B: catches a transposed output / fragment map (cdna_hip_programming.md §3)."""
    n = 256
    a = torch.eye(n)
    b = (torch.arange(n)[:, None] * 3 + torch.arange(n)[None, :] % 7).float() % 64      # asymmetric, exact in bf16
    out = ops_bf16.gemm_nt(_rows(a), _rows(b), out_f32=True)
    assert torch.equal(out.cpu(), b.t())


@pytest.mark.parametrize("M,N,K,act", [(700, 256, 192, ops.ACT_NONE), (700, 128, 256, ops.ACT_ELU), (90, 64, 64, ops.ACT_RELU)])
def test_gemm_nt_bf16_random_bias_act(M, N, K, act):
    g = torch.Generator().manual_seed(3)
    a = torch.randn(M, K, generator=g).to(BF).float()
    b = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF).float()
    bias = torch.randn(N, generator=g) * 0.1
    ref = a.double() @ b.double().t() + bias.double()
    ref = {ops.ACT_NONE: ref, ops.ACT_ELU: F.elu(ref), ops.ACT_RELU: F.relu(ref)}[act]
    out32 = ops_bf16.gemm_nt(_rows(a), _rows(b), out_f32=True, bias=bias.cuda(), act=act)
    assert rel_err(out32, ref) < 2e-6                                   # fp32 accumulation of exact bf16 products
    out16 = ops_bf16.gemm_nt(_rows(a), _rows(b), bias=bias.cuda(), act=act)
    d = (out16.float().cpu().double() - ref).abs()
    assert (d <= ULP * ref.abs() + 1e-6).all()                          # the stored value is the rounding of an fp32-accurate sum


def test_gemm_nt_bf16_score_partials():
    """el / er partials from the values AS STORED (bf16-rounded ft), per 64-column block."""
    M, K, HD, R = 333, 128, 256, 512
    g = torch.Generator().manual_seed(5)
    a = torch.randn(M, K, generator=g).to(BF).float()
    b = (torch.randn(R, K, generator=g) / K ** 0.5).to(BF).float()
    sl, sr = torch.randn(HD, generator=g), torch.randn(HD, generator=g)
    parts = torch.empty((M, HD // 64, 2), device="cuda")
    y = ops_bf16.gemm_nt(_rows(a), _rows(b), score_l=sl.cuda(), score_r=sr.cuda(), score_out=parts)
    ft = y[:, :HD].float().cpu().double()
    ref_l = (ft * sl.double()).view(M, HD // 64, 64).sum(-1)
    ref_r = (ft * sr.double()).view(M, HD // 64, 64).sum(-1)
    assert rel_err(parts[..., 0], ref_l) < 2e-6 and rel_err(parts[..., 1], ref_r) < 2e-6
    # heads of exactly one 64-column block: the direct [el | er] layout holds the same numbers, the product is unchanged
    for Md in (M, 3000):
        ad = torch.randn(Md, K, generator=g).to(BF).float()
        p2 = torch.empty((Md, HD // 64, 2), device="cuda")
        y2 = ops_bf16.gemm_nt(_rows(ad), _rows(b), score_l=sl.cuda(), score_r=sr.cuda(), score_out=p2)
        s = torch.full((Md, 2 * (HD // 64)), float("nan"), device="cuda")
        yd = ops_bf16.gemm_nt(_rows(ad), _rows(b), score_l=sl.cuda(), score_r=sr.cuda(), score_out=s, score_direct=True)
        assert torch.equal(yd, y2) and torch.equal(s, ops.scores_from_parts(p2, HD // 64, 64))


@pytest.mark.parametrize("R,M,N", [(1, 8, 8), (500, 128, 64), (4097, 256, 128), (9000, 512, 1063), (20000, 1024, 40),
                                   (777, 200, 136)])
def test_gemm_tn_bf16_exact_on_integers(R, M, N):
    g = torch.Generator().manual_seed(R + M + N)
    a = torch.randint(-2, 3, (R, M), generator=g).float()
    b = torch.randint(-2, 3, (R, N), generator=g).float()
    out, cs = ops_bf16.gemm_tn(_rows(a), _rows(b), want_colsum=True)
    assert torch.equal(out.cpu(), a.t() @ b)
    assert torch.equal(cs.cpu(), a.sum(0))
    assert torch.equal(ops_bf16.gemm_tn(_rows(a), _rows(b)).cpu(), a.t() @ b)


def test_weight_operands_and_cast():
    g = torch.Generator().manual_seed(1)
    wa, wb = torch.randn(96, 1063, generator=g), torch.randn(32, 1063, generator=g)
    w, wt = ops_bf16.weight_operands(wa.cuda(), wb.cuda(), want_t=True)
    ref = torch.cat([wa, wb]).to(BF)
    assert ops_bf16.rows_ok(w) and ops_bf16.rows_ok(wt)
    assert torch.equal(w.cpu(), ref) and torch.equal(wt.cpu(), ref.t())
    # pad columns are zero (the GEMMs read whole 8-element chunks)
    assert w.stride(0) == 1064 and float(w._base[:, 1063:].abs().max()) == 0.0
    x = torch.randn(50, 39, generator=g)
    xb = ops_bf16.cast_rows(x.cuda())
    assert torch.equal(xb.cpu(), x.to(BF)) and xb.stride(0) == 40 and float(xb._base[:, 39:].abs().max()) == 0.0


def test_prepared_weights_bf16_one_launch_equals_one_per_layer():
    """ops_bf16.prepared_weights: every project-first layer's bf16 operands from ONE spgnn_weight_cat_bf16_multi launch, bit for
    bit those of a spgnn_weight_cat_bf16 call per layer (ragged widths, with and without a second block / a transpose); inside
    the block weight_operands launches nothing and hands out the prepared buffers."""
    g = torch.Generator().manual_seed(3)
    shapes = [((512, 1063), (512, 1063), False), ((256, 1024), (256, 1024), True), ((128, 128), None, True), ((96, 39), (40, 39), True),
              ((64, 250), None, False)]
    ws = [(torch.randn(a, generator=g).cuda(), None if b is None else torch.randn(b, generator=g).cuda(), t) for a, b, t in shapes]
    single = [ops_bf16.weight_operands(a, b, t) for a, b, t in ws]
    with ops_bf16.prepared_weights(ws):
        for (a, b, t), (w1, t1) in zip(ws, single):
            w, wt = ops_bf16.weight_operands(a, b, t)
            assert (id(a), id(b) if b is not None else 0) in ops_bf16._PREP_ACTIVE
            assert torch.equal(w, w1) and ops_bf16.rows_ok(w) and torch.equal(w._base, w1._base)      # pad columns too
            assert (wt is None) == (not t) and (wt is None or (torch.equal(wt, t1) and torch.equal(wt._base, t1._base)))
            if t:                                                   # a transpose prepared but not asked for
                assert ops_bf16.weight_operands(a, b, False)[1] is None
    assert not ops_bf16._PREP_ACTIVE


def test_cat_dropout_bf16_matches_fp32_mask():
    """Same counter hash as the fp32 kernel: equal keep masks; backward multiplies by the same mask."""
    N, w1, w2, p, seed = 257, 64, 128, 0.3, 1234
    g = torch.Generator().manual_seed(2)
    a, b = torch.randn(N, w1, generator=g), torch.randn(N, w2, generator=g)
    y32 = ops.cat_dropout((a.cuda(), b.cuda()), p, seed)
    ab, bb = _rows(a).requires_grad_(), _rows(b).requires_grad_()
    y16 = ops_bf16.cat_dropout((ab, bb), p, seed)
    assert ops_bf16.rows_ok(y16)
    keep = (y32 != 0).cpu()
    ref = torch.cat([a.to(BF).float(), b.to(BF).float()], 1) * keep / (1 - p)
    assert torch.equal(y16.float().cpu(), ref.to(BF).float())
    go = torch.randn(N, w1 + w2, generator=g).to(BF)
    y16.backward(go.cuda())
    gref = (go.float() * keep / (1 - p)).to(BF).float()
    assert torch.equal(ab.grad.float().cpu(), gref[:, :w1]) and torch.equal(bb.grad.float().cpu(), gref[:, w1:])


# ----------------------------------------------------------------------------------------------------------------
# GATConv layer: HIP bf16 path vs the storage model (fp64 arithmetic, bf16 rounding at the storage points)
# ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F_in,H,D,res,act,mean", [(128, 2, 64, True, "elu", False), (256, 2, 128, True, "elu", False),
                                                   (64, 1, 64, False, None, False), (128, 2, 1024, True, None, True),
                                                   (64, 4, 128, False, None, True), (200, 2, 512, True, None, True),
                                                   (1024, 2, 256, True, "elu", False), (96, 4, 64, True, "tanh", True)])
def test_gat_layer_bf16_matches_storage_model(F_in, H, D, res, act, mean):
    src, dst, n = tree_batch_edges([37, 61, 150, 9], seed=4)
    g = TreeGraph((src, dst), n, device="cuda")
    actf = {"elu": F.elu, "tanh": torch.tanh, None: None}[act]
    torch.manual_seed(F_in + H + D)
    layer = snn.GATConv(F_in, D, H, 0.0, 0.0, 0.2, res, actf).cuda()
    with torch.no_grad():
        layer.bias.normal_(0, 0.05)
    x = torch.randn(n, F_in).to(BF).float()
    xb = _rows(x).requires_grad_()
    out = layer(g, xb, mean_heads=mean)
    out = out if mean else out.flatten(1)
    go = torch.randn(out.shape, generator=torch.Generator().manual_seed(9))
    go = go if out.dtype == torch.float32 else go.to(BF).float()
    out.backward(go.cuda().to(out.dtype))
    # storage model in fp64
    lm = mean and act is None and O.linear_mean_form(H, D, F_in, res)
    fused = lm or (mean and ops.can_fuse_mean(H, D))   # a head narrower than a team: per-head rows are stored, torch takes the mean
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in layer.state_dict().items()}
    x64 = x.double().requires_grad_()
    if lm:
        # output layer without activation: the product takes the linear-mean form (ops_bf16.gat_layer_linear_mean)
        r = O.gat_conv_linear_mean(torch.as_tensor(src), torch.as_tensor(dst), n, x64, sd["fc.weight"], sd["attn_l"], sd["attn_r"],
                                   sd.get("res_fc.weight"), sd["bias"], 0.2, storage=O.Bf16Storage)[0]
    else:
        r = O.gat_conv(torch.as_tensor(src), torch.as_tensor(dst), n, x64, sd["fc.weight"], sd["attn_l"], sd["attn_r"],
                       sd.get("res_fc.weight"), sd["bias"], 0.2, actf, storage=O.Bf16Storage, store_out=not fused)[0]
        r = r.mean(1) if mean else r.flatten(1)
    if mean and not fused:
        r = O.Bf16Storage.store(r)
    r.backward(go.double())
    assert out.dtype == (torch.float32 if fused else BF)
    _close_to_model(out, r, "out")
    _close_to_model(xb.grad, O._rb(x64.grad), "g_x")
    for k, p in layer.named_parameters():
        # attn_l / attn_r gradients are sums over all nodes of g_el * ft: cancellation-heavy (the softmax is shift invariant
        # in er up to the LeakyReLU kink), so single rounding-boundary flips upstream move many of their elements by more
        # than fp32 noise; they keep the normwise 2-ulp bound only
        _close_to_model(p.grad, sd[k].grad, k, frac=1.0 if k.startswith("attn") else 0.05)


@pytest.mark.parametrize("emb_in_loss", [False, True])
def test_linear_with_joined_classifier_bf16(emb_in_loss):
    """ops_bf16._LinearClassifierBf16Fn against fp64 on the SAME bf16 operands: folded route (no (N, C) gradient, nothing
    rounded but the bf16 gradient rows g_x) and ordinary route (the (N, C) gradient rounded to bf16 once)."""
    torch.manual_seed(5 + emb_in_loss)
    N, K, C, J = 700, 384, 1024, 22
    x32 = torch.randn(N, K).to(BF).float()
    xb = _rows(x32).requires_grad_()
    w = (torch.randn(C, K, device="cuda") / 16).requires_grad_()
    b = torch.randn(C, device="cuda", requires_grad=True)
    wc = (torch.randn(J, C, device="cuda") / 32).requires_grad_()
    bc = torch.randn(J, device="cuda", requires_grad=True)
    y, logits = ops_bf16._LinearClassifierBf16Fn.apply(xb, w, b, wc, bc)
    cl, cy = torch.randn(N, J, device="cuda"), torch.randn(N, C, device="cuda")
    ((logits * cl).sum() + ((y * cy).sum() if emb_in_loss else 0.0)).backward()
    S = O.Bf16Storage
    rx, rw, rb_, rwc, rbc = (t.detach().double().cpu().requires_grad_() for t in (x32, w, b, wc, bc))
    ry = S.round_grad(rx) @ S.store_fwd(rw).t() + rb_
    if emb_in_loss:
        ry = S.round_grad(ry)
    rl = ry @ rwc.t() + rbc
    ((rl * cl.double().cpu()).sum() + ((ry * cy.double().cpu()).sum() if emb_in_loss else 0.0)).backward()
    assert rel_err(y, ry) < 1e-5 and rel_err(logits, rl) < 1e-5
    _close_to_model(xb.grad, rx.grad, "g_x")
    for name, got, want in (("w", w, rw), ("b", b, rb_), ("w_cls", wc, rwc), ("b_cls", bc, rbc)):
        assert rel_err(got.grad, want.grad) < (2 * ULP if emb_in_loss else 1e-4), name


# ----------------------------------------------------------------------------------------------------------------
# model level: st_gat_6 (BASELINE config 4) and st_gat_3
# ----------------------------------------------------------------------------------------------------------------
def _build(name, seed=0):
    cfg = get_config(name)
    torch.manual_seed(seed)
    model = models.build_model(cfg.MODEL).cuda()
    model.init(None)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if n.endswith("bias"):
                p.normal_(0, 0.05)
    model.set_gcn_only()
    models.set_storage_dtype(model, BF)
    return cfg, model


def _oracle_logits(cfg, model, g, dtype, storage, grad=False):
    src, dst = g.cpu().edges()
    sd = {k: v.detach().cpu().to(dtype).requires_grad_(grad and v.dtype.is_floating_point) for k, v in model.state_dict().items()}
    return O.net_forward(cfg.KIND, sd, src, dst, g.number_of_nodes(), g.ndata["fvs"].cpu().to(dtype), None, storage=storage), sd


@pytest.mark.parametrize("name,trees", [("st_gat_6", 3), ("st_gat_3", 3), ("st_gat_6", 64)])
def test_bf16_model_forward_and_gradients(name, trees):
    """(st_gat_6, 64): BASELINE config 4's model against its storage-model oracle at the reference's TRAIN_BATCH_SIZE, not only
    on a 3-tree batch."""
    cfg, model = _build(name)
    g = synthetic.make_batch(trees, rank=5, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    model.eval()
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS))
    y = g.ndata["y"]
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5
    logits, emb = model(g)
    loss = masked_weighted_ce(logits, y, mask.cuda(), w.cuda())
    loss.backward()
    assert logits.dtype == torch.float32 and emb.dtype == torch.float32
    (m_logits, m_emb), sd_m = _oracle_logits(cfg, model, g, torch.float64, O.Bf16Storage, grad=True)
    O.masked_weighted_ce(m_logits, y.cpu(), mask, w.double()).backward()
    (t_logits, t_emb), sd_t = _oracle_logits(cfg, model, g, torch.float64, None, grad=True)
    O.masked_weighted_ce(t_logits, y.cpu(), mask, w.double()).backward()
    # (1) against the storage model.  Rounding-boundary flips upstream perturb downstream layers, so at model level the
    # bound is a small multiple of one ulp rather than fp32 noise: normwise 4 ulp on embeddings and logits.
    assert rel_err(emb, m_emb) < 4 * ULP and rel_err(logits, m_logits) < 4 * ULP
    # (2) against the true fp64 oracle: no worse than 4x what bf16 storage itself costs (model vs truth), floor 2 ulp
    cost = rel_err(m_logits, t_logits)
    assert rel_err(logits, t_logits) < 4 * cost + 2 * ULP, (rel_err(logits, t_logits), cost)
    assert rel_err(logits, t_logits) < 0.05            # absolute sanity bound: 7 layers of 2^-9 relative rounding noise
    # (3) gradients: against an ENVELOPE MEASURED ON THE STORAGE MODEL ITSELF (flat bounds of 0.5 / 0.05 could hide
    # a real error behind conditioning).  The HIP path differs from the model only by fp32 accumulation order, which moves a
    # few per cent of the stored values across a bf16 rounding boundary (measured: 3.7 % of a layer's input elements are one
    # ulp apart).  So the model is re-run FLIP_TRIALS times with that perturbation injected - every store rounds to nearest
    # and then 4 % of the elements are moved one ulp up or down - and each parameter's gradient may deviate from the
    # unperturbed model by at most ENV_FACTOR x the largest deviation those trials show for THAT tensor (floor: 2 ulp).  The
    # attention-vector gradients (sums of g_el[n] * row[n] with sum_n g_el ~ 0: they see only differences between rows)
    # get a wide envelope because they ARE that sensitive, every weight a tight one (< 1 %); a sign or indexing error moves a
    # tensor by O(1) of its norm whatever its conditioning.
    env = _flip_envelope(cfg, model, g, y, mask, w, {n: sd_m[n].grad for n, p in model.named_parameters() if p.requires_grad})
    report = []
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        gm = sd_m[n].grad
        e_model = rel_err(p.grad, gm)
        report.append((n, e_model, env[n]))
        assert e_model < ENV_FACTOR * env[n] + 2 * ULP, (n, e_model, env[n])
        assert e_model < 0.6, (n, e_model)                 # and never anywhere near a sign error, whatever the envelope says
    if os.environ.get("SPGNN_BF16_REPORT"):
        for n, e, v in report:
            print(f"{n:45s} hip-vs-model {e:9.3e}   envelope {v:9.3e}   ratio {e / max(v, 1e-12):6.2f}")


# Twelve trials, not four: the deviation of an attention vector's gradient is dominated by DISCRETE events - a flip that moves
# one edge's el + er across the LeakyReLU kink changes its slope from 1 to 0.2 - so its distribution over trials is bimodal
# (st_gat_3 output layer, attn_l: median 0.02-0.05, but 0.177 in the trials where the event occurs - exactly the HIP path's
# own deviation, 0.177; attn_r: 0.274 both ways; tools/env_diag.py).  The maximum over twelve trials at either flip rate sees it.
FLIP_RATE, FLIP_TRIALS, ENV_FACTOR = 0.04, 12, 1.5


def _flip_envelope(cfg, model, g, y, mask, w, grads_model, trials=None, dtype=torch.float64):
    """Per-parameter max over FLIP_TRIALS of the gradient's normwise deviation when every bf16 store of the storage-model
    oracle additionally moves FLIP_RATE of its elements by one ulp (what a different fp32 accumulation order does to values
    that sit near a rounding boundary)."""
    orig = O._rb
    gen = torch.Generator().manual_seed(1234)

    def flipping(x):
        r = orig(x)
        m = torch.rand(r.shape, generator=gen) < FLIP_RATE
        up = torch.rand(r.shape, generator=gen) < 0.5
        ulp1 = torch.ldexp(torch.ones_like(r), torch.frexp(r)[1] - 8)          # spacing of bf16 at r (8 significant bits)
        return torch.where(m & (r != 0), orig(r + torch.where(up, ulp1, -ulp1)), r)
    env = {n: 0.0 for n in grads_model}
    try:
        O._rb = flipping
        for _ in range(trials or FLIP_TRIALS):
            (lg, _e), sd = _oracle_logits(cfg, model, g, dtype, O.Bf16Storage, grad=True)
            O.masked_weighted_ce(lg, y.cpu(), mask, w.to(dtype)).backward()
            for n in env:
                env[n] = max(env[n], rel_err(sd[n].grad, grads_model[n]))
    finally:
        O._rb = orig
    return env


@pytest.mark.parametrize("name", ["st_gat_6", "st_gat_3"])
def test_bf16_output_layer_exact_on_its_own_inputs(name):
    """The output layer inside the model (linear-mean form): fed the HIP path's own input rows and incoming gradient, the
    storage model reproduces its output and every parameter gradient to fp32-accumulation noise - whatever distance the
    model-level test sees on this layer's gradients is upstream rounding flips, not the kernels."""
    cfg, model = _build(name)
    g = synthetic.make_batch(3, rank=5, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    model.eval()
    layer = model.gat.gat_layers[-1]
    cap, inner = {}, layer._forward

    def spy(graph, feat, *a, **k):
        cap["x"] = feat.detach().float().cpu()
        out = inner(graph, feat, *a, **k)
        t = out[0] if isinstance(out, tuple) else out
        cap["out"] = t.detach().float().cpu()
        return out

    layer._forward = spy
    y = g.ndata["y"]
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < 0.5
    logits, _ = model(g)
    logits.register_hook(lambda gr: cap.__setitem__("g", gr.detach().float().cpu()))
    masked_weighted_ce(logits, y, mask.cuda(), torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS)).cuda()).backward()
    src, dst = g.cpu().edges()
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in layer.state_dict().items()}
    wc, bc = (t.detach().cpu().double().requires_grad_() for t in (model.gnn_out.weight, model.gnn_out.bias))
    _, H, D = sd["attn_l"].shape
    assert O.linear_mean_form(H, D, cap["x"].shape[1], "res_fc.weight" in sd)
    # the *Net's classifier is joined to the layer's node: only the logits carry a gradient, the product's is never stored
    r = O.gat_conv_linear_mean(src, dst, g.number_of_nodes(), cap["x"].double(), sd["fc.weight"], sd["attn_l"], sd["attn_r"],
                               sd.get("res_fc.weight"), sd["bias"], 0.2, storage=O.Bf16Storage, round_out_grad=False)[0]
    F.linear(r, wc, bc).backward(cap["g"].double())
    assert rel_err(cap["out"], r) < 2e-4          # a stored z element may sit on a bf16 rounding boundary (fp32 vs fp64 sums)
    for k, p in layer.named_parameters():
        assert rel_err(p.grad, sd[k].grad) < 1e-3, (k, rel_err(p.grad, sd[k].grad))
    assert rel_err(model.gnn_out.weight.grad, wc.grad) < 1e-3 and rel_err(model.gnn_out.bias.grad, bc.grad) < 1e-5


def test_bf16_train_step_tracks_fp32_and_replays():
    """The full training step (dropout on) on bf16 storage follows the fp32-storage step taken from the same weights with
    the same mask / dropout draws (identical counter hashes in both paths) within bf16 noise, keeps fp32 master weights,
    and runs as HIP-graph replays."""
    losses = {}
    for dt in (torch.float32, BF):
        cfg, model = _build("st_gat_6", seed=11)
        models.set_storage_dtype(model, dt)
        g = synthetic.make_batch(6, rank=1, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
        model.train()
        torch.manual_seed(77)                       # the host-side seed draws of the dropout hashes
        step = TrainStep(model, class_weight_list(cfg.CLASS_WEIGHTS), cfg.SAMPLING_RATE, 1e-3, 0.9, seed=3)
        losses[dt] = [float(step.step(g)) for _ in range(6)]
        assert all(p.dtype == torch.float32 for p in model.parameters())
    a, b = np.array(losses[torch.float32]), np.array(losses[BF])
    assert np.isfinite(b).all() and np.abs(a - b).max() < 0.03 * np.abs(a).max(), (a, b)
    step.capture(g)                                  # the bf16 step, captured
    l2 = [float(step.replay()) for _ in range(4)]
    assert np.isfinite(l2).all() and max(l2) < 2 * a.max()


def test_bf16_config_4_at_512_trees_with_the_tile_kernels_against_the_storage_model(monkeypatch):
    """BASELINE config 4 AT ITS FULL SIZE - st_gat_6, bf16 rows, 512 trees (N = 76 410: above
    ops.TILE_MIN_NODES, so the src-major halves run on the LDS-tile kernels of csrc/spgnn_tile.hip, as shipped) - forward, loss
    and every gradient against the storage-model oracle (O.Bf16Storage, fp64 arithmetic with bf16 storage points), the same
    rule as the 64-tree case of test_bf16_model_forward_and_gradients with a 4-trial flip envelope (4 more oracle passes at
    this size: ~1 min of CPU)."""
    from spgnn_amd import ops as _ops
    cfg, model = _build("st_gat_6")
    g = synthetic.make_batch(512, rank=0, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    assert g.number_of_nodes() >= _ops.TILE_MIN_NODES
    model.eval()
    tiled = []
    real_plan = _ops.tile_plan

    def spy(csc, H, D, elem_bytes, kind="src"):
        r = real_plan(csc, H, D, elem_bytes, kind)
        if r is not None:
            tiled.append((kind, elem_bytes, H, D))
        return r
    monkeypatch.setattr(_ops, "tile_plan", spy)
    w = torch.tensor(class_weight_list(cfg.CLASS_WEIGHTS))
    y = g.ndata["y"]
    mask = torch.rand(y.shape[0], generator=torch.Generator().manual_seed(5)) < torch.where(y.cpu() != 0, torch.tensor(1.0), torch.tensor(cfg.SAMPLING_RATE))
    logits, emb = model(g)
    loss = masked_weighted_ce(logits, y, mask.cuda(), w.cuda())
    loss.backward()
    monkeypatch.undo()
    assert {t[:2] for t in tiled} == {("src", 2)} and len(tiled) >= 6, tiled       # the shipped dispatch: src-major halves of the bf16 layers
    # fp32 oracle arithmetic at this size (an fp64 pass over 76 410 nodes takes over a minute on the host, six are needed):
    # its 2^-24 noise is far below the bf16 storage points' 2^-9 that the comparison is about
    OD = torch.float32
    (m_logits, m_emb), sd_m = _oracle_logits(cfg, model, g, OD, O.Bf16Storage, grad=True)
    m_loss = O.masked_weighted_ce(m_logits, y.cpu(), mask, w.to(OD))
    m_loss.backward()
    with torch.no_grad():
        (t_logits, t_emb), _sd_t = _oracle_logits(cfg, model, g, OD, None)
    assert rel_err(emb, m_emb) < 4 * ULP and rel_err(logits, m_logits) < 4 * ULP
    cost = rel_err(m_logits, t_logits)
    assert rel_err(logits, t_logits) < 4 * cost + 2 * ULP and rel_err(logits, t_logits) < 0.05
    assert rel_err(loss, m_loss) < 2 * ULP
    env = _flip_envelope(cfg, model, g, y, mask, w, {n: sd_m[n].grad for n, p in model.named_parameters() if p.requires_grad}, trials=4, dtype=OD)
    worst = (None, 0.0, 0.0)
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        e_model = rel_err(p.grad, sd_m[n].grad)
        if e_model / max(env[n], 2 * ULP) > worst[1] / max(worst[2], 2 * ULP) or worst[0] is None:
            worst = (n, e_model, env[n])
        # four trials see less of the envelope than twelve: twice the factor of the 64-tree test
        assert e_model < 2 * ENV_FACTOR * env[n] + 2 * ULP, (n, e_model, env[n])
        assert e_model < 0.6, (n, e_model)
    print(f"bf16 st_gat_6 512 trees (tile kernels on {len(tiled)} launches): logits vs storage model {rel_err(logits, m_logits):.2e} "
          f"({rel_err(logits, m_logits) / ULP:.2f} ulp), loss {rel_err(loss, m_loss):.2e}; gradient closest to its envelope: {worst[0]} "
          f"{worst[1]:.2e} (envelope {worst[2]:.2e})")


def test_bf16_512_trees_properties():
    """BASELINE config 4 at its full size (512 trees): batching B trees == concatenating single-tree results (block
    diagonal graph: no cross-tree traffic) and bitwise run-to-run reproducibility."""
    cfg, model = _build("st_gat_6")
    model.eval()
    samples = synthetic.synthetic_trees(512, rank=0)
    g = synthetic.batch_from_samples(samples, "cuda", cfg.POS_ENC_DIM)
    with torch.no_grad():
        a = model(g)[0]
        b = model(g)[0]
        assert torch.equal(a, b)
        sub = synthetic.batch_from_samples(samples[100:103], "cuda", cfg.POS_ENC_DIM)
        n0 = sum(s["fvs"].shape[0] for s in samples[:100])
        c = model(sub)[0]
        assert torch.equal(a[n0:n0 + c.shape[0]], c)
