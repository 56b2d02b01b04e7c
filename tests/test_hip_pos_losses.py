"""GPU side of the position-stream losses (spgnn_pos_loss_tables / spgnn_pos_losses, spgnn_amd/posloss.py): the kernels
against the plain-torch restatement of reference job_runner.py:1827-1865 in fp64, and TrainStep(pos_losses=True) against
a plain autograd step of the same model, eager and captured."""
import copy

import numpy as np
import pytest
import torch

from spgnn_amd import models, posenc, posloss, synthetic
from spgnn_amd.configs import class_weight_list, get_config
from spgnn_amd.train import TrainStep, masked_weighted_ce

pytestmark = pytest.mark.gpu


def _batch(sizes, seed=0, missing=()):
    rng = np.random.default_rng(seed)
    samples = [synthetic.synthetic_tree(n, rng, fv_dim=8) for n in sizes]
    for t in missing:                                   # labels absent from some trees: their statistics rows are noise
        lab = samples[t]["labels"]
        lab[lab % 3 == 0] = 0
    g = synthetic.batch_from_samples(samples, "cuda", pos_enc_dim=None)
    hops = [posenc.bfs_distances(s["adj"], list(range(s["adj"].shape[0]))) for s in samples]
    return g, hops


def _rel(a, b):
    a, b = torch.as_tensor(a).detach().double().cpu(), torch.as_tensor(b).detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def _check(sizes, D, missing=(), steps=2, seed=0):
    g, hops = _batch(sizes, seed, missing)
    N, B = g.number_of_nodes(), len(sizes)
    y = g.ndata["y"]
    tables = posloss.PosLossTables.of(g)
    for t in range(B):
        assert np.array_equal(tables.hops(t), hops[t])
    assert np.array_equal(tables.diam.cpu().numpy(), [h.max() for h in hops])
    st = posloss.PosLossState(D, "cuda", seed=3)
    gen = torch.Generator().manual_seed(seed)
    m_ref = None
    for step in range(steps):
        p = torch.tanh(torch.randn(N, D, generator=gen)).float()
        p[1] = p[0]                                     # identical rows: sign(0) = 0 everywhere on that pair
        d, c, g_p = posloss.pos_losses(g, p.cuda(), st)
        pr = p.double().cuda().requires_grad_(True)      # the fp64 restatement runs on the device too (512 trees: seconds)
        nz = torch.from_numpy(posloss.noise(st.seed, step, B, posloss.NUM_LABELS, D)).cuda()
        dr, cr, m_new = posloss.reference_pos_losses(pr, sizes, hops, y.cpu(), m_ref, nz)
        (dr + posloss.C_WEIGHT * cr).backward()
        assert _rel(d, dr) <= 1e-5, (step, float(d), float(dr))
        if step == 0:
            assert float(c) == 0.0
        else:
            assert _rel(c, cr) <= 1e-5
        assert _rel(g_p, pr.grad) <= 1e-5
        assert _rel(st.mean, m_new) <= 1e-5
        m_ref = st.mean.double()                        # continue from the device's state (fp32)
    return g, st


def test_kernel_matches_torch_on_small_and_large_trees_with_missing_labels():
    _check([21, 300, 64], 64, missing=(1,), steps=3)
    _check([21, 37, 5], 39, missing=(0, 2), steps=2, seed=1)


def test_kernel_matches_torch_on_64_trees_and_is_bit_identical():
    sizes = list(np.random.default_rng(4).integers(120, 181, 64))
    _check(sizes, 64, missing=(3, 17), steps=2)
    g, _ = _batch(sizes)
    p = torch.tanh(torch.randn(g.number_of_nodes(), 64, device="cuda"))
    outs = []
    for _ in range(2):
        st = posloss.PosLossState(64, "cuda", seed=1)
        w = torch.full((1,), 3.5, device="cuda")
        for _ in range(2):
            d, c, gp = posloss.pos_losses(g, p, st, weight_sum=w)
        outs.append(torch.cat([torch.stack([d, c]), gp.reshape(-1), st.mean.reshape(-1)]).cpu())
    assert torch.equal(outs[0], outs[1])


def test_kernel_matches_torch_on_512_trees():
    sizes = list(np.random.default_rng(5).integers(120, 181, 512))
    _check(sizes, 64, missing=(0, 511), steps=1)


def _spgnn(seed=0):
    cfg = get_config("st_pgat_spgnn_3")
    torch.manual_seed(seed)
    model = models.build_model(cfg.MODEL).cuda()
    model.init(None)
    model.set_gcn_only()
    return cfg, model


def test_train_step_with_pos_losses_matches_a_plain_autograd_step():
    """Three steps of TrainStep(pos_losses=True) == three torch SGD(momentum) steps on masked CE + d + 0.1 c formed with
    autograd through a copy of the same model, dropout ON: every dropout seed of a forward pass comes from torch's global
    generator (models.GATPSPGNN._seed_plan), so re-seeding it before each of the two forwards gives both the same masks."""
    cfg, model = _spgnn(1)
    model.train()
    samples = synthetic.synthetic_trees(64, rank=0)
    g = synthetic.batch_from_samples(samples, "cuda", 39)
    hops = [posenc.bfs_distances(s["adj"], list(range(s["adj"].shape[0]))) for s in samples]
    sizes = [s["adj"].shape[0] for s in samples]
    ref = copy.deepcopy(model)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    ts = TrainStep(model, w, cfg.SAMPLING_RATE, 1e-3, 0.9, pos_losses=True)
    params = [p for p in ref.parameters() if p.requires_grad]
    opt = torch.optim.SGD(params, lr=1e-3, momentum=0.9)
    y = g.ndata["y"]
    sp = torch.where(y != 0, 1.0, cfg.SAMPLING_RATE).float()
    gen = torch.Generator(device="cuda").manual_seed(5)
    m_ref = None
    for step in range(3):
        draws = torch.rand(y.shape[0], device="cuda", generator=gen)
        torch.manual_seed(100 + step)
        loss = ts.step(g, draws)
        d_dev, c_dev = ts.last_pos_losses
        opt.zero_grad()
        torch.manual_seed(100 + step)
        logits, _, p = ref(g)
        ce = masked_weighted_ce(logits, y, draws < sp, torch.tensor(w, device="cuda"))
        nz = torch.from_numpy(posloss.noise(ts._pos.seed, step, 64, posloss.NUM_LABELS, p.shape[1])).cuda()
        d, c, m_ref = posloss.reference_pos_losses(p, sizes, hops, y, m_ref, nz)
        total = ce + d + posloss.C_WEIGHT * c
        total.backward()
        opt.step()
        assert _rel(loss, total) < 1e-5, (step, float(loss), float(total))
        assert _rel(d_dev, d) < 1e-5 and (step == 0 and float(c_dev) == 0.0 or _rel(c_dev, c) < 1e-5)
    named = dict(ref.named_parameters())
    for k, v in model.named_parameters():
        if v.requires_grad:
            assert _rel(v, named[k]) < 1e-5, k
    assert _rel(ts._pos.mean, m_ref) < 1e-5
    with torch.no_grad():                       # the masks are live: another seed gives another position stream
        torch.manual_seed(1)
        p1 = ref(g)[2].clone()
        torch.manual_seed(2)
        assert not torch.equal(p1, ref(g)[2])
    sd = ts.state_dict()["spgnn"]["pos_losses"]
    assert sd["updates"] == 3 and torch.equal(sd["mean"], ts._pos.mean.cpu())


def _prime_for_replay(ts):
    """What TrainStep.capture sets up before its warm-up: device learning rate and seed counter, in-kernel mask draws."""
    ts._lr_dev = torch.full((1,), float(ts.lr), dtype=torch.float32, device="cuda")
    ts._seed_ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    ts._use_default_rng = True


def test_captured_steps_equal_eager_steps_bitwise_with_dropout():
    """run_batch on a batch arena (three eager warm-up steps, the capture, two replays), dropout ON == five eager steps on the
    arena under the same masks.  A replay's masks are the seed plan drawn at capture time (the generator state after the
    warm-up) plus the device counter each step advances; the eager side reproduces that by drawing its last two plans from
    that same generator state, with the same counter."""
    from spgnn_amd import ops as _ops
    cfg, m1 = _spgnn(2)
    m1.train()
    m2 = copy.deepcopy(m1)
    g = synthetic.make_batch(8, rank=1, device="cuda", pos_enc_dim=39)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    ta = TrainStep(m1, w, cfg.SAMPLING_RATE, 1e-3, 0.9, pos_losses=True, seed=4)
    tb = TrainStep(m2, w, cfg.SAMPLING_RATE, 1e-3, 0.9, pos_losses=True, seed=4)
    torch.manual_seed(7)
    la = ta.run_batch(g, 5)
    ag = tb.arena_graph(g)
    _prime_for_replay(tb)
    torch.manual_seed(7)
    for _ in range(3):
        tb.step(ag)
    state = torch.get_rng_state()
    for _ in range(2):
        torch.set_rng_state(state)
        lb = tb.step(ag)
    torch.cuda.synchronize()
    _ops.DROPOUT_SEED_OFFSET = None
    assert torch.isfinite(la) and torch.equal(la, lb)
    n = ta.bucket.numel
    assert torch.equal(ta.bucket.flat_param[:n], tb.bucket.flat_param[:n])
    assert torch.equal(ta._pos.mean, tb._pos.mean) and int(ta._pos.state[0]) == 5
    # a second batch of the same size class replays on the refreshed tables
    g2 = synthetic.make_batch(8, rank=3, device="cuda", pos_enc_dim=39)
    l2 = ta.run_batch(g2, 2)
    assert torch.isfinite(l2) and int(ta._pos.state[0]) == 7
    _ops.DROPOUT_SEED_OFFSET = None


def test_running_mean_round_trips_through_state_dict():
    """Save after two steps, load into a fresh step object (before its first step: the pending path) and into a used one;
    the third step is bit for bit the one the original object takes."""
    cfg, m1 = _spgnn(3)
    m1.eval()
    g = synthetic.make_batch(6, rank=2, device="cuda", pos_enc_dim=39)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    ta = TrainStep(m1, w, 1.0, 1e-3, 0.9, pos_losses=True, seed=9)
    ta.step(g); ta.step(g)
    sd = ta.state_dict()
    msd = {k: v.detach().clone() for k, v in m1.state_dict().items()}
    la = ta.step(g)
    for used in (False, True):
        _, m2 = _spgnn(0)
        m2.eval()
        m2.load_state_dict(msd)
        tb = TrainStep(m2, w, 1.0, 1e-3, 0.9, pos_losses=True, seed=1)
        if used:
            tb.step(g)                             # a running mean exists already: load_state_dict overwrites it
            m2.load_state_dict(msd)
        tb.load_state_dict(sd)
        lb = tb.step(g)
        assert torch.equal(la, lb), used
        assert torch.equal(ta._pos.mean, tb._pos.mean) and int(tb._pos.state[0]) == 3
        n = ta.bucket.numel
        assert torch.equal(ta.bucket.flat_param[:n], tb.bucket.flat_param[:n])


def _refusal_worker(rank, world, port, ret):
    import os
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    cfg, model = _spgnn(0)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    try:
        TrainStep(model, w, cfg.SAMPLING_RATE, 1e-3, 0.9, pos_losses=True)
        ret[rank] = "accepted"
    except NotImplementedError as e:
        ret[rank] = "refused: " + str(e)
    ts = TrainStep(model, w, cfg.SAMPLING_RATE, 1e-3, 0.9)     # the option off: the two-rank step is built as before
    ret[rank] += f" | world {ts.world}"
    dist.destroy_process_group()


def test_pos_losses_refuses_a_two_rank_process_group():
    import socket
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ret = mp.Manager().dict()
    mp.spawn(_refusal_worker, args=(2, port, ret), nprocs=2, join=True)
    for r in (0, 1):
        assert ret[r].startswith("refused: ") and "rank" in ret[r] and ret[r].endswith("| world 2"), ret[r]
