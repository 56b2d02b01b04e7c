"""CPU side of the position-stream losses (spgnn_amd/posloss.py; reference job_runner.py:1827-1865): the host restatement
of the table kernel, the plain-torch restatement of the losses against their closed-form gradient, the label and
running-mean rules, the settings and the refusals of TrainStep(pos_losses=True)."""
import numpy as np
import pytest
import torch

from spgnn_amd import configs, models, posenc, posloss, synthetic
from spgnn_amd.train import TrainStep


def _trees(sizes, seed=0):
    rng = np.random.default_rng(seed)
    return [synthetic.random_tree_adj(n, rng) for n in sizes]


def test_hop_tables_match_bfs_distances_and_diameters():
    for adj in _trees([1, 2, 5, 21, 64, 150], seed=3):
        n = adj.shape[0]
        hops, diam = posloss.hop_tables_host(adj)
        assert np.array_equal(hops, posenc.bfs_distances(adj, list(range(n))))
        assert diam == (posenc._tree_diameter(adj) if n > 1 else 0)


def _closed_form(p, sizes, hops, B):
    """(d, dd/dp) from the formulas of the kernel: quadratic smooth-L1 branch, factor 2 from the symmetry of A."""
    g = np.zeros_like(p)
    d, off = 0.0, 0
    for n, h in zip(sizes, hops):
        pt = p[off:off + n]
        diff = pt[:, None, :] - pt[None, :, :]
        A = np.exp(-np.abs(diff).sum(2))
        diam = h.max()
        T = np.exp(-(h / diam).astype(np.float32).astype(np.float64)) if diam > 0 else np.ones_like(A)
        d += (0.5 * (A - T) ** 2).mean() / B
        g[off:off + n] = 2.0 / (B * n * n) * ((A - T) * -A)[:, :, None].__mul__(np.sign(diff)).sum(1)
        off += n
    return d, g


def test_torch_restatement_agrees_with_the_closed_form_gradient():
    sizes = [7, 21, 30]
    adjs = _trees(sizes, seed=5)
    hops = [posloss.hop_tables_host(a)[0] for a in adjs]
    N, D = sum(sizes), 6
    rng = np.random.default_rng(1)
    p_np = np.tanh(rng.standard_normal((N, D)))
    p_np[3, 2] = p_np[4, 2]                    # an exact tie: sign(0) = 0
    y = torch.zeros(N, dtype=torch.int64)
    p = torch.tensor(p_np, requires_grad=True)
    d, c, m = posloss.reference_pos_losses(p, sizes, hops, y, None, torch.zeros(3, posloss.NUM_LABELS, D))
    d.backward()
    d_ref, g_ref = _closed_form(p_np, sizes, hops, len(sizes))
    assert abs(d.item() - d_ref) <= 1e-12 * max(1.0, abs(d_ref))
    assert np.abs(p.grad.numpy() - g_ref).max() <= 1e-12
    assert c.item() == 0.0


def test_last_node_per_label_and_first_step_compactness_is_zero():
    sizes = [6, 5]
    hops = [posloss.hop_tables_host(a)[0] for a in _trees(sizes, seed=2)]
    D = 3
    y = torch.tensor([0, 2, 1, 2, 0, 1,   0, 0, 3, 0, 0], dtype=torch.int64)   # label 2 twice in tree 0: node 3 wins
    p = torch.arange(11 * D, dtype=torch.float64).reshape(11, D) / 40.0
    noise = torch.full((2, posloss.NUM_LABELS, D), 0.5, dtype=torch.float64)
    d, c, m = posloss.reference_pos_losses(p, sizes, hops, y, None, noise)
    assert c.item() == 0.0
    assert torch.equal(m[1], (p[3] + noise[1, 1]) / 2)                       # tree 0: node 3 (last label-2 node); tree 1: noise
    assert torch.equal(m[0], (p[5] + noise[1, 0]) / 2)                        # tree 1 has no label 1
    assert torch.equal(m[2], (noise[0, 2] + p[8]) / 2)
    # second step: c uses the first step's mean, only over the labels a tree has
    d2, c2, _ = posloss.reference_pos_losses(p, sizes, hops, y, m, noise)
    want = (((p[5] - m[0]) ** 2).sum() + ((p[3] - m[1]) ** 2).sum() + ((p[8] - m[2]) ** 2).sum()) / 2
    assert torch.allclose(c2, want, rtol=1e-14)


def test_running_mean_recurrence_over_three_steps():
    sizes = [9, 12]
    hops = [posloss.hop_tables_host(a)[0] for a in _trees(sizes, seed=7)]
    D, L = 4, posloss.NUM_LABELS
    y = torch.zeros(sum(sizes), dtype=torch.int64)
    y[2], y[10] = 1, 5
    rng = torch.Generator().manual_seed(0)
    m, means = None, []
    for step in range(3):
        p = torch.rand(sum(sizes), D, generator=rng, dtype=torch.float64)
        nz = torch.from_numpy(posloss.noise(99, step, 2, L, D)).double()
        stats = nz.clone()
        stats[0, 0] = p[2]
        stats[1, 4] = p[10]
        _, _, m_new = posloss.reference_pos_losses(p, sizes, hops, y, m, nz)
        want = stats.mean(0) if m is None else 0.15 * m + 0.85 * stats.mean(0)
        assert torch.allclose(m_new, want, rtol=1e-15, atol=0)
        m = m_new
        means.append(m)
    assert not torch.equal(means[1], means[2])


def test_noise_is_uniform_deterministic_and_step_dependent():
    a = posloss.noise(5, 0, 4, 21, 64)
    assert a.dtype == np.float32 and a.shape == (4, 21, 64)
    assert (a >= 0).all() and (a < 1).all() and abs(a.mean() - 0.5) < 0.02
    assert np.array_equal(a, posloss.noise(5, 0, 4, 21, 64))
    assert not np.array_equal(a, posloss.noise(5, 1, 4, 21, 64))


def test_settings_expose_use_dist_loss(tmp_path):
    for name in configs.CONFIGS:
        assert configs.get_config(name).USE_DIST_LOSS is False
    assert configs.get_config("st_pgat_spgnn_3").LAMBDA == 0.1
    f = tmp_path / "s.py"
    f.write_text("SAMPLING_RATE = 0.1\n")
    assert configs.load_settings(str(f)).USE_DIST_LOSS is False
    f.write_text("USE_DIST_LOSS = True\nLAMBDA = 1e-1\n")
    s = configs.load_settings(str(f))
    assert s.USE_DIST_LOSS is True and s.LAMBDA == 0.1


def _model(name):
    cfg = configs.get_config(name)
    m = models.build_model(cfg.MODEL)
    m.init(None)
    m.set_gcn_only()
    return cfg, m


def test_pos_losses_refuses_what_it_does_not_implement(monkeypatch):
    w = configs.class_weight_list(configs.CLASS_WEIGHTS)
    for name in ("st_gat_3", "st_pgat_spgnnnl_3"):
        _, m = _model(name)
        with pytest.raises(NotImplementedError):
            TrainStep(m, w, 0.15, 1e-3, pos_losses=True)
    _, m = _model("st_pgat_spgnn_3")
    with pytest.raises(NotImplementedError):
        TrainStep(m, w, 0.15, 1e-3, pos_losses=True, loss_rows_only=True)
    from spgnn_amd import train
    monkeypatch.setattr(train.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(train.dist, "get_world_size", lambda group=None: 2)
    with pytest.raises(NotImplementedError):
        TrainStep(m, w, 0.15, 1e-3, pos_losses=True)
    TrainStep(m, w, 0.15, 1e-3)                # off: unchanged
