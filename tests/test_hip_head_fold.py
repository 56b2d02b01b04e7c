"""The output head with the classifier folded through it, against fp64: the linear-mean fold (spgnn_linear_mean_fold_fwd / _bwd in
spgnn_gemm.hip, ops.linear_mean_fold_buffers / linear_mean_fold_grads / _LinearMeanClassifierFn and its bf16 twin), the score fold
(spgnn_fold_scores_fwd / _bwd, ops.fold_scores) and the activation backward with the classifier's input and weight gradients
formed on the fly (spgnn_act_bwd_proj, spgnn_act_bwd_proj_wgrad).

Every reference is the UNFOLDED function in fp64, y = mean_h(Z_h W_fc,h^T + x W_res,h^T + b_h), logits = y Wc^T + bc, with its
gradients from fp64 autograd; the fold's own buffers are checked against their definitions (the comment above FoldFwd).  The
classifier widths J cover every template instance and both sides of each of its edges (tests/util.py FOLD_J and friends,
kept equal to the launchers by test_graph.test_head_fold_rule_covers_every_instance)."""
import math

import pytest
import torch

from spgnn_amd import _capi, ops, ops_bf16
from tests.util import ACT_BWD_PROJ_J, ACT_BWD_PROJ_WGRAD_J, FOLD_J, close_to_model, rel_err

pytestmark = pytest.mark.gpu
W_TOL, P_TOL, G_TOL = 1e-6, 2e-6, 1e-5       # W_comb / b_mean; P / c0 / logits / y; every gradient
DEV = "cuda"


def _pad16(k):
    return (k + 15) // 16 * 16


def _params(H, D, F_, J, res, bias, bcls, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)                     # noqa: E731
    return (r(H * D, F_) * F_ ** -0.5, r(H * D, F_) * F_ ** -0.5 if res else None, r(H * D) * 0.1 if bias else None,
            r(J, D) * D ** -0.5, r(J) * 0.1 if bcls else None)


def _fold64(w_fc, w_res, bias, w_cls, b_cls, H, D, x_block=True):
    """fp64 W_comb (D, Kc), b_mean (D,) or None, P (J, Kc), c0 (J,) by their definitions."""
    F_ = w_fc.shape[1]
    parts = [w_fc.view(H, D, F_).permute(1, 0, 2).reshape(D, H * F_)]
    if x_block:
        parts.append(w_res.view(H, D, F_).sum(0) if w_res is not None else w_fc.new_zeros((D, F_)))
    w_comb = torch.cat(parts, 1) / H
    b_mean = bias.view(H, D).mean(0) if bias is not None else None
    P = w_cls @ w_comb
    c0 = (w_cls @ b_mean if b_mean is not None else w_cls.new_zeros(w_cls.shape[0])) + (b_cls if b_cls is not None else 0.0)
    return w_comb, b_mean, P, c0


def _unfolded64(zx, w_fc, w_res, bias, w_cls, b_cls, H, D, x_block=True):
    """y = mean_h(Z_h W_fc,h^T + x W_res,h^T + b_h), logits = y Wc^T + bc."""
    F_ = w_fc.shape[1]
    x = zx[:, H * F_:] if x_block else None
    y = 0.0
    for h in range(H):
        t = zx[:, h * F_:(h + 1) * F_] @ w_fc[h * D:(h + 1) * D].t()
        if w_res is not None:
            t = t + x @ w_res[h * D:(h + 1) * D].t()
        if bias is not None:
            t = t + bias[h * D:(h + 1) * D]
        y = y + t
    y = y / H
    logits = y @ w_cls.t()
    return y, (logits + b_cls if b_cls is not None else logits)


def _d(t):
    return None if t is None else t.detach().double().requires_grad_(True)


def _tickets(H, F_):
    return ops._FOLD_WS[(str(torch.device(DEV, torch.cuda.current_device())), H, F_)][1]


# (H, D, F, residual, bias, classifier bias, x_block): H = 3 makes 1/H inexact; D = 8 leaves row quarters 1..3 empty, D = 200 a
# ragged last quarter, 1024 is the shipped width; F = 39 / 100 / 1063 put Kc = (H + x_block) F off multiples of 16 and 32
FOLD_SHAPES = [
    (1, 8, 39, True, True, True, True),
    (2, 200, 100, True, True, True, True),
    (3, 1024, 1063, True, True, True, True),
    (4, 200, 39, False, False, False, True),
    (3, 8, 1063, False, True, True, True),
    (2, 1024, 39, True, False, True, True),
    (4, 1024, 100, True, True, False, True),
    (1, 1024, 100, False, True, True, False),        # GraphConv's one-head route: W_comb = W_fc
    (1, 200, 1063, False, False, True, False),
]


@pytest.mark.parametrize("shape", FOLD_SHAPES, ids=lambda s: "H{}_D{}_F{}_r{:d}b{:d}c{:d}_x{:d}".format(*s))
@pytest.mark.parametrize("J", FOLD_J)
def test_linear_mean_fold_buffers_and_grads_against_fp64(J, shape):
    H, D, F_, res, bias, bcls, xb = shape
    w_fc, w_res, b, w_cls, b_cls = _params(H, D, F_, J, res, bias, bcls, seed=J * 131 + H * 17 + D + F_)
    Kc = (H + int(xb)) * F_
    Kp = _pad16(Kc)
    w_comb, blk, w_bf, b_mean, P, c0 = ops.linear_mean_fold_buffers(w_fc, w_res, b, w_cls, b_cls, H, D, x_block=xb)
    assert w_bf is None and w_comb.shape == (D, Kp) and P.shape == (J, Kp)
    r_w, r_b, r_P, r_c0 = _fold64(*(_d(t) for t in (w_fc, w_res, b, w_cls, b_cls)), H, D, x_block=xb)
    assert rel_err(w_comb[:, :Kc], r_w) < W_TOL
    assert rel_err(P[:, :Kc], r_P) < P_TOL and rel_err(c0, r_c0) < P_TOL
    assert (b_mean is None) == (not bias) and (b_mean is None or rel_err(b_mean, r_b) < W_TOL)
    assert torch.all(w_comb[:, Kc:] == 0) and torch.all(P[:, Kc:] == 0)                     # the zero padding Kc .. Kp
    assert ops.scale_value(blk) == ops.scale_value(ops.pow2_scale(w_comb))                  # absmax_out
    assert torch.all(_tickets(H, F_) == 0)                                                  # the tickets re-armed themselves
    again = ops.linear_mean_fold_buffers(w_fc, w_res, b, w_cls, b_cls, H, D, x_block=xb)
    for a_, b_ in zip((w_comb, b_mean, P, c0), (again[0], again[3], again[4], again[5])):
        assert a_ is None or torch.equal(a_, b_)                                              # bit-identical
    assert torch.all(_tickets(H, F_) == 0)

    # backward from given M1 = g_logits^T Zx and cs = colsum(g_logits): the gradients of <M1, P> + <cs, c0>
    gen = torch.Generator().manual_seed(J + 7 * D)
    M1, cs = torch.randn(J, Kc, generator=gen).to(DEV), torch.randn(J, generator=gen).to(DEV)
    g_fc, g_res, g_bias, g_wc = ops.linear_mean_fold_grads(M1, cs, w_cls, w_comb, b_mean, H, D, F_, res, bias, x_block=xb)
    leaves = [_d(t) for t in (w_fc, w_res, b, w_cls, b_cls)]
    _, _, q_P, q_c0 = _fold64(*leaves, H, D, x_block=xb)
    ((q_P * M1.double()).sum() + (q_c0 * cs.double()).sum()).backward()
    assert rel_err(g_fc, leaves[0].grad) < G_TOL and rel_err(g_wc, leaves[3].grad) < G_TOL
    assert (g_res is None) == (not res) and (g_res is None or rel_err(g_res, leaves[1].grad) < G_TOL)
    assert (g_bias is None) == (not bias) and (g_bias is None or rel_err(g_bias, leaves[2].grad) < G_TOL)
    again = ops.linear_mean_fold_grads(M1, cs, w_cls, w_comb, b_mean, H, D, F_, res, bias, x_block=xb)
    for a_, b_ in zip((g_fc, g_res, g_bias, g_wc), again):
        assert a_ is None or torch.equal(a_, b_)


# (H, D, F, residual, bias, classifier bias, x_block, w_fc as the transposed view of an (F, D) parameter)
E2E_SHAPES = [
    (3, 1024, 39, True, True, True, True, False),
    (2, 8, 1063, True, False, True, True, False),
    (4, 200, 100, False, True, False, True, False),
    (1, 200, 100, False, True, True, False, True),   # GraphConv: weight.t() of the (in, out) parameter, one head, no x block
]


@pytest.mark.parametrize("embedding_in_loss", [False, True], ids=["folded", "ordinary"])
@pytest.mark.parametrize("shape", E2E_SHAPES, ids=lambda s: "H{}_D{}_F{}_r{:d}b{:d}c{:d}_x{:d}_t{:d}".format(*s))
@pytest.mark.parametrize("J", FOLD_J)
def test_linear_mean_classifier_end_to_end_against_fp64(J, shape, embedding_in_loss):
    """_LinearMeanClassifierFn: logits (and y) and every gradient against fp64 autograd of the unfolded function, on the folded
    route (only the logits in the loss: linear_mean_fold_bwd) and the ordinary one (y in the loss too)."""
    H, D, F_, res, bias, bcls, xb, transposed = shape
    N = 600
    w_fc, w_res, b, w_cls, b_cls = _params(H, D, F_, J, res, bias, bcls, seed=J * 7 + D + F_)
    Kc = (H + int(xb)) * F_
    gen = torch.Generator().manual_seed(J + F_)
    zx = torch.randn(N, Kc, generator=gen).to(DEV)
    g_logits = torch.randn(N, J, generator=gen).to(DEV)
    g_y = torch.randn(N, D, generator=gen).to(DEV) * 0.1
    w_param = (w_fc.t().contiguous() if transposed else w_fc).requires_grad_(True)
    leaves = [zx.clone().requires_grad_(True), w_param] + [t.clone().requires_grad_(True) if t is not None else None
                                                           for t in (w_res, b, w_cls, b_cls)]
    w_arg = w_param.t() if transposed else w_param
    assert (w_arg.stride(1) != 1) == transposed
    y, logits = ops._LinearMeanClassifierFn.apply(leaves[0], w_arg, *leaves[2:], H, D, xb)
    loss = (logits * g_logits).sum() + ((y * g_y).sum() if embedding_in_loss else 0.0)
    loss.backward()
    ref = [_d(t) for t in leaves]
    r_w = ref[1].t() if transposed else ref[1]
    r_y, r_logits = _unfolded64(ref[0], r_w, *ref[2:], H, D, x_block=xb)
    ((r_logits * g_logits.double()).sum() + ((r_y * g_y.double()).sum() if embedding_in_loss else 0.0)).backward()
    # y and the logits are length-Kc fp32 dot products: their rounding grows as sqrt(Kc) (Kc = 3189: a sequential fp32 sum alone
    # is 1.1e-6 off on 64 of the rows)
    tol = P_TOL * max(1.0, math.sqrt(Kc / 1024))
    assert rel_err(logits, r_logits) < tol and rel_err(y, r_y) < tol
    names = ["zx", "w_fc", "w_res", "bias", "w_cls", "b_cls"]
    for n, a_, r_ in zip(names, leaves, ref):
        if a_ is not None:
            assert a_.grad is not None and rel_err(a_.grad, r_.grad) < G_TOL, (n, rel_err(a_.grad, r_.grad))
    assert torch.all(_tickets(H, F_) == 0)


def _rne32(t):
    return t.to(torch.bfloat16)


@pytest.mark.parametrize("H,D,F_,J", [(1, 64, 39, 1), (2, 200, 100, 22), (3, 8, 1063, 9), (4, 1024, 39, 32)])
def test_fold_bf16_image_is_the_rne_rounding_of_the_fp32_image(H, D, F_, J):
    """With bf16 = True, w_comb_bf16 is bit for bit the fp32 W_comb the kernel forms (W_fc / H in fp32; the x block sum_h W_res / H:
    summed in kernel order, so compared for H <= 2 only) rounded to nearest even; the fp32 image and P hold the rounded values."""
    w_fc, w_res, b, w_cls, b_cls = _params(H, D, F_, J, True, True, True, seed=H * D + F_)
    Kc, Kp = (H + 1) * F_, _pad16((H + 1) * F_)
    w_comb, blk, w_bf, b_mean, P, c0 = ops.linear_mean_fold_buffers(w_fc, w_res, b, w_cls, b_cls, H, D, bf16=True)
    assert blk is None and w_bf.dtype == torch.bfloat16 and w_bf.shape == (D, Kp)
    inv = torch.tensor(1.0 / H, dtype=torch.float32, device=DEV)
    fc32 = w_fc.view(H, D, F_).permute(1, 0, 2).reshape(D, H * F_) * inv
    assert torch.equal(w_bf[:, :H * F_].view(torch.int16), _rne32(fc32).view(torch.int16))
    if H <= 2:
        x32 = (w_res.view(H, D, F_)[0] + w_res.view(H, D, F_)[1] if H == 2 else w_res) * inv
        assert torch.equal(w_bf[:, H * F_:Kc].view(torch.int16), _rne32(x32).view(torch.int16))
    assert torch.equal(w_comb, w_bf.float()) and torch.all(w_bf[:, Kc:].float() == 0)
    assert rel_err(P[:, :Kc], w_cls.double() @ w_bf[:, :Kc].double()) < P_TOL and torch.all(P[:, Kc:] == 0)
    r_b = b.view(H, D).double().mean(0)
    assert rel_err(b_mean, r_b) < W_TOL and rel_err(c0, w_cls.double() @ r_b + b_cls.double()) < P_TOL
    assert torch.all(_tickets(H, F_) == 0)


def test_linear_mean_classifier_bf16_against_the_storage_model():
    """_LinearMeanClassifierBf16Fn on the folded route against fp64 with bf16 storage: Zx as bf16 rows, W_comb rounded to bf16
    (its gradient passes straight through the rounding), the input gradient stored as bf16 rows."""
    H, D, F_, J, N = 2, 64, 64, 22, 700
    w_fc, w_res, b, w_cls, b_cls = _params(H, D, F_, J, True, True, True, seed=3)
    Kc = (H + 1) * F_
    gen = torch.Generator().manual_seed(4)
    zb = ops_bf16.cast_rows(torch.randn(N, Kc, generator=gen).to(DEV))
    assert zb.shape == (N, Kc)
    g_logits = torch.randn(N, J, generator=gen).to(DEV)
    leaves = [zb.clone().requires_grad_(True)] + [t.clone().requires_grad_(True) for t in (w_fc, w_res, b, w_cls, b_cls)]
    y, logits = ops_bf16._LinearMeanClassifierBf16Fn.apply(*leaves, H, D)
    (logits * g_logits).sum().backward()
    ref = [_d(t) for t in leaves]
    w64, bm64, _, _ = _fold64(*ref[1:], H, D)
    wr = w64 + (w64.detach().float().bfloat16().double() - w64.detach())                 # bf16 image, straight-through gradient
    r_y = ref[0] @ wr.t() + bm64
    r_logits = r_y @ ref[4].t() + ref[5]
    (r_logits * g_logits.double()).sum().backward()
    close_to_model(y, r_y, "y")
    close_to_model(logits, r_logits, "logits")
    close_to_model(leaves[0].grad, ref[0].grad.float().bfloat16(), "g_zx")
    for n, a_, r_ in zip(["w_fc", "w_res", "bias", "w_cls", "b_cls"], leaves[1:], ref[1:]):
        close_to_model(a_.grad, r_.grad, n)


def _fold_fwd_raw(w_fc, w_res, w_cls, H, D, J, x_block, w_comb, ld_w, P, ld_p, c0):
    F_ = w_fc.shape[1]
    ws = ops._FOLD_WS.get((str(w_fc.device), H, F_))
    if ws is None:
        ops.linear_mean_fold_buffers(w_fc, w_res, None, w_cls[:1], None, H, D, x_block=x_block)  # valid call: creates the scratch
        ws = ops._FOLD_WS[(str(w_fc.device), H, F_)]
    return _capi.load().spgnn_linear_mean_fold_fwd(
        w_fc.data_ptr(), w_fc.stride(0), w_res.data_ptr() if w_res is not None else None, F_ if w_res is not None else 0, None,
        w_cls.data_ptr(), w_cls.stride(0), None, H, D, F_, J, w_comb.data_ptr(), ld_w, None, 0, None, P.data_ptr(), ld_p,
        c0.data_ptr(), None, ws[0].data_ptr(), ws[1].data_ptr(), int(x_block), torch.cuda.current_stream().cuda_stream)


def test_fold_refusals_launch_nothing():
    """J = 0 and J = 33, x_block = 0 with a residual, a too-short W_comb or P stride: refused through _capi.check, nothing
    written."""
    H, D, F_ = 2, 64, 39
    Kp = _pad16((H + 1) * F_)
    w_fc, w_res, _, w_cls, _ = _params(H, D, F_, 33, True, False, False, seed=5)
    bad = [(w_cls[:0], True, Kp, Kp, w_res), (w_cls, True, Kp, Kp, w_res), (w_cls[:4], False, Kp, Kp, w_res),
           (w_cls[:4], True, Kp - 16, Kp, w_res), (w_cls[:4], True, Kp, Kp - 16, w_res)]
    for wc, xb, ld_w, ld_p, wr in bad:
        w_comb = torch.full((D, Kp), float("nan"), device=DEV)
        P = torch.full((max(wc.shape[0], 1), Kp), float("nan"), device=DEV)
        c0 = torch.full((max(wc.shape[0], 1),), float("nan"), device=DEV)
        code = _fold_fwd_raw(w_fc, wr, wc, H, D, wc.shape[0], xb, w_comb, ld_w, P, ld_p, c0)
        with pytest.raises(RuntimeError, match="spgnn_linear_mean_fold_fwd"):
            _capi.check(code, "spgnn_linear_mean_fold_fwd")
        torch.cuda.synchronize()
        assert torch.isnan(w_comb).all() and torch.isnan(P).all() and torch.isnan(c0).all()
    for J in (0, 33):                                             # the same through the wrappers
        with pytest.raises(RuntimeError, match="spgnn_linear_mean_fold_fwd"):
            ops.linear_mean_fold_buffers(w_fc, w_res, None, torch.zeros(J, D, device=DEV), None, H, D)
        with pytest.raises(RuntimeError, match="spgnn_linear_mean_fold_bwd"):
            ops.linear_mean_fold_grads(torch.zeros(J, (H + 1) * F_, device=DEV), torch.zeros(J, device=DEV),
                                       torch.zeros(J, D, device=DEV), torch.zeros(D, Kp, device=DEV), None, H, D, F_, True, False)
    with pytest.raises(RuntimeError, match="spgnn_linear_mean_fold_bwd"):
        ops.linear_mean_fold_grads(torch.zeros(4, H * F_, device=DEV), torch.zeros(4, device=DEV), w_cls[:4],
                                   torch.zeros(D, Kp, device=DEV), None, H, D, F_, True, False, x_block=False)
    torch.cuda.synchronize()


def test_fold_ticket_buffer_covers_both_column_layouts(monkeypatch):
    """ops._FOLD_WS is keyed on (device, H, F); the kernel claims one ticket per 32 columns of the CURRENT call's Kp.  A first
    fold without the x block (GraphConv, Kp = pad16(F)) must leave tickets enough for a later fold with it (SAGEConv, same H = 1
    and F: Kp = pad16(2F)).  The size is checked BEFORE the wider fold is launched."""
    monkeypatch.setattr(ops, "_FOLD_WS", {})
    H, D, F_, J = 1, 64, 1024, 22
    w_fc, w_res, b, w_cls, b_cls = _params(H, D, F_, J, True, True, True, seed=6)
    w_comb, _, _, _, P, _ = ops.linear_mean_fold_buffers(w_fc, None, b, w_cls, b_cls, H, D, x_block=False)
    assert rel_err(P[:, :F_], _fold64(*(_d(t) for t in (w_fc, None, b, w_cls, b_cls)), H, D, x_block=False)[2]) < P_TOL
    tickets = _tickets(H, F_)
    assert tickets.numel() >= math.ceil(_pad16(2 * F_) / 32), tickets.numel()
    w_comb, _, _, b_mean, P, c0 = ops.linear_mean_fold_buffers(w_fc, w_res, b, w_cls, b_cls, H, D, x_block=True)
    r_w, r_b, r_P, r_c0 = _fold64(*(_d(t) for t in (w_fc, w_res, b, w_cls, b_cls)), H, D, x_block=True)
    assert rel_err(w_comb[:, :2 * F_], r_w) < W_TOL and rel_err(P[:, :2 * F_], r_P) < P_TOL and rel_err(c0, r_c0) < P_TOL
    assert torch.all(tickets == 0)


# ---------------------------------------------------------------------------------------------------------------------------
# score fold: w_lr[h] = sum_d attn_l[h, d] W[h D + d, :], w_lr[H + h] likewise with attn_r
# ---------------------------------------------------------------------------------------------------------------------------
def _fold_scores64(w, al, ar, H, D):
    K = w.shape[1]
    wv = w.view(H, D, K)
    return torch.cat([torch.einsum("hd,hdk->hk", al, wv), torch.einsum("hd,hdk->hk", ar, wv)], 0)


def _check_fold_scores(H, D, K, strided):
    gen = torch.Generator().manual_seed(H * 1000 + D + K)
    wb = (torch.randn(H * D, K + (13 if strided else 0), generator=gen) * D ** -0.5).to(DEV).requires_grad_(True)
    w = wb[:, :K] if strided else wb
    al = torch.randn(H, D, generator=gen).to(DEV).requires_grad_(True)
    ar = torch.randn(H, D, generator=gen).to(DEV).requires_grad_(True)
    assert w.stride(0) == (K + 13 if strided else K)
    w_lr = ops.fold_scores(w, al, ar)
    assert w_lr.shape == (2 * H, K) and w_lr._base is not None and w_lr._base.shape == (2 * H, _pad16(K))
    assert torch.all(w_lr._base[:, K:] == 0)                                            # padding K .. Kp
    w64, al64, ar64 = (t.detach().double().requires_grad_(True) for t in (w, al, ar))
    ref = _fold_scores64(w64, al64, ar64, H, D)
    assert rel_err(w_lr, ref) < W_TOL
    x = torch.randn(37, K, generator=gen).to(DEV).double()                               # functional: the per-head scores
    proj = (x @ w.detach().double().t()).view(37, H, D)
    s_ref = torch.cat([(proj * al.detach().double()).sum(-1), (proj * ar.detach().double()).sum(-1)], 1)
    assert rel_err(x @ w_lr.detach().double().t(), s_ref) < W_TOL
    gb = torch.randn(2 * H, K + (5 if strided else 0), generator=gen).to(DEV)
    g = gb[:, :K] if strided else gb
    g_w, g_al, g_ar = torch.autograd.grad(w_lr, (wb, al, ar), g)
    g_w = g_w[:, :K]
    r_w, r_al, r_ar = torch.autograd.grad(ref, (w64, al64, ar64), g.double())
    for n, a_, r_ in (("g_w", g_w, r_w), ("g_attn_l", g_al, r_al), ("g_attn_r", g_ar, r_ar)):
        assert rel_err(a_, r_) < G_TOL, (n, rel_err(a_, r_))


@pytest.mark.parametrize("K", [1, 39, 1024, 1063])
@pytest.mark.parametrize("D", [5, 64, 256, 1024])
@pytest.mark.parametrize("H", [1, 2, 4, 8])
def test_fold_scores_against_fp64(H, D, K):
    _check_fold_scores(H, D, K, strided=False)


@pytest.mark.parametrize("H,D,K", [(1, 5, 1), (2, 64, 39), (4, 256, 1063), (8, 1024, 1024)])
def test_fold_scores_strided_operands_against_fp64(H, D, K):
    """w with stride(0) > K and an incoming gradient with stride(0) > K."""
    _check_fold_scores(H, D, K, strided=True)


# ---------------------------------------------------------------------------------------------------------------------------
# activation backward with the classifier's gradients formed on the fly
# ---------------------------------------------------------------------------------------------------------------------------
ACTS = {"elu": ops.ACT_ELU, "tanh": ops.ACT_TANH, "relu": ops.ACT_RELU, "lrelu": ops.ACT_LRELU}
ABP_BIG_N = 32 * 512 + 3617            # above 32 x spgnn_act_bwd_proj_wgrad_blocks' cap: several row trips per block


def _act_out(pre, act):
    return {"elu": torch.nn.functional.elu, "tanh": torch.tanh, "relu": torch.relu,
            "lrelu": lambda t: torch.nn.functional.leaky_relu(t, 0.01)}[act](pre)


def _act_grad64(out, act):
    """The derivative as the kernels take it, from the stored output, in fp64."""
    o = out.double()
    return {"elu": torch.where(o > 0, torch.ones_like(o), o + 1), "tanh": 1 - o * o, "relu": (o > 0).double(),
            "lrelu": torch.where(o > 0, torch.ones_like(o), torch.full_like(o, float(torch.tensor(0.01, dtype=torch.float32))))}[act]


class _KeepJob:
    """A stand-in SumJobs queue: keeps the weight-gradient partials instead of summing them."""

    def add(self, job, *tensors):
        self.job, self.tensors = job, tensors


def _abp_case(N, H, D, J, act, seed):
    gen = torch.Generator().manual_seed(seed)
    g_s = torch.randn(N, J, generator=gen).to(DEV)
    w = (torch.randn(J, D, generator=gen) * D ** -0.5).to(DEV)
    out = _act_out(torch.randn(N, H * D, generator=gen).to(DEV), act)
    ref = ((g_s.double() @ w.double()) / H).repeat(1, H) * _act_grad64(out, act)
    return g_s, w, out, ref


def _absmax(part):
    return float(part[ops.SCALE_HEADER:].max())


@pytest.mark.parametrize("D", [36, 64, 1024])
@pytest.mark.parametrize("H", [1, 2, 3, 4])
@pytest.mark.parametrize("J", ACT_BWD_PROJ_J)
def test_act_bwd_proj_against_fp64(J, H, D):
    """g_pre = (g_s W / H) * act'(out) for every activation, N across the four-row trips and the block cap."""
    for i, act in enumerate(ACTS):
        for N in (1, 31, 32, 33, ABP_BIG_N if (J + H + i) % 4 == 0 else 257):
            g_s, w, out, ref = _abp_case(N, H, D, J, act, seed=N + 3 * J + 5 * H + D + i)
            g_pre, part = ops.act_bwd_proj(g_s, w, out, H, D, ACTS[act])
            assert rel_err(g_pre, ref) < P_TOL, (act, N, rel_err(g_pre, ref))
            assert _absmax(part) == float(g_pre.abs().max()), (act, N)


@pytest.mark.parametrize("D", [36, 64, 1024])
@pytest.mark.parametrize("H", [1, 2])
@pytest.mark.parametrize("J", ACT_BWD_PROJ_WGRAD_J)
def test_act_bwd_proj_wgrad_against_fp64(J, H, D):
    """spgnn_act_bwd_proj_wgrad: g_pre as spgnn_act_bwd_proj, and the per-block partials of the classifier's weight gradient,
    summed in block order, equal g_s^T mean_h(out)."""
    lib = _capi.load()
    for i, act in enumerate(ACTS):
        for N in (1, 31, 32, 33, ABP_BIG_N if (J + H + i) % 4 == 0 else 257):
            g_s, w, out, ref = _abp_case(N, H, D, J, act, seed=N + 3 * J + 5 * H + D + i)
            keep = _KeepJob()
            g_pre, part, g_w = ops.act_bwd_proj(g_s, w, out, H, D, ACTS[act], wgrad_jobs=keep)
            wpart = keep.tensors[0]
            assert wpart.shape == (int(lib.spgnn_act_bwd_proj_wgrad_blocks(N)), J, D)
            assert N != ABP_BIG_N or N > 32 * wpart.shape[0]                             # more than one row trip per block
            assert rel_err(g_pre, ref) < P_TOL, (act, N, rel_err(g_pre, ref))
            assert _absmax(part) == float(g_pre.abs().max()), (act, N)
            w_ref = g_s.double().t() @ out.double().view(N, H, D).mean(1)
            s = wpart[0].clone()
            for b in range(1, wpart.shape[0]):                                          # the ordered sum of the partials
                s += wpart[b]
            assert rel_err(s, w_ref) < G_TOL, (act, N, rel_err(s, w_ref))
            q = ops.SumJobs(g_s.device, local=True)
            q.add(keep.job, *keep.tensors)
            q.flush()
            assert rel_err(g_w, w_ref) < G_TOL, (act, N)
