"""Cost of TrainStep(pos_losses=True) (USE_DIST_LOSS) on the 512-tree st_pgat_spgnn_3 step: captured-step replays with
and without the option in one process, and the spgnn_pos_losses launches alone, with the kernel's share of the fp32
vector-ALU roofline (pairs x D x 3 ops - sub, abs, add - plus one exp per pair, against 157.3 TFLOP/s).

    python tools/pos_loss_bench.py [--trees 512] [--steps 50]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from spgnn_amd import models, posloss, synthetic
from spgnn_amd.configs import class_weight_list, get_config
from spgnn_amd.train import TrainStep

PEAK_FP32_VECTOR = 157.3e12


def _time(fn, steps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    start.record()
    for _ in range(steps):
        fn()
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / steps * 1e3        # us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", type=int, default=512)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    cfg = get_config("st_pgat_spgnn_3")
    g = synthetic.make_batch(a.trees, rank=0, device="cuda", pos_enc_dim=cfg.POS_ENC_DIM)
    w = class_weight_list(cfg.CLASS_WEIGHTS)
    out = {"trees": a.trees, "nodes": g.number_of_nodes()}
    for flag in (False, True):
        torch.manual_seed(0)
        model = models.build_model(cfg.MODEL).cuda()
        model.init(None)
        model.set_gcn_only()
        model.train()
        ts = TrainStep(model, w, cfg.SAMPLING_RATE, 1e-4, 0.9, pos_losses=flag)
        ts.capture(g, warmup=3)
        out["step_us_pos_losses" if flag else "step_us"] = _time(ts.replay, a.steps)
    out["added_us"] = out["step_us_pos_losses"] - out["step_us"]
    # the kernel alone (both launches), on a p of the model's width
    D = 64
    sizes = np.asarray(posloss.tree_sizes(g))
    p = torch.tanh(torch.randn(g.number_of_nodes(), D, device="cuda"))
    st = posloss.PosLossState(D, "cuda")
    tab = posloss.PosLossTables.of(g)
    kern = _time(lambda: st.run(tab, p), a.steps * 4)
    pairs = int((sizes * sizes).sum())
    ops = pairs * (3.0 * D + 1.0)
    out.update(kernel_us=kern, pairs=pairs, D=D, valu_ops=ops, roofline_us=ops / PEAK_FP32_VECTOR * 1e6,
               roofline_fraction=ops / PEAK_FP32_VECTOR / (kern * 1e-6))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
