"""Times the Fast R-CNN head losses with their gradients at the training shapes N = 8 x 512 and N = 8 x 2048 rows, C = 81:

  fused   ONE call of dtc_fast_rcnn_loss (losses + both gradients) on the padded [B, R] layout with the compact targets;
  torch   the reference's formulation (train_fast.py:147-158: cross_entropy, lib/model/loss.py smooth_L1 and accuracy, backward)
          in torch ops on the same GPU, on the compacted rows with the expanded [n, 4C] targets and weights, which are built
          beforehand and not timed.

    python tools/loss_timing.py [--window 0.5] [--rounds 5] [--out FILE]

HIP events around windows of back-to-back calls; every window lasts at least --window seconds (the call count is set from a trial);
the two sides alternate, --rounds windows each, in one process, after a warm-up of both.  One JSON line per shape: the median time
per call of each side in microseconds, the spread (min .. max over the rounds), and torch / fused.  Both sides are checked against
each other before they are timed.  Needs the GPU: without one it fails."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from detectorch_amd import hip_loss  # noqa: E402


def inputs(B, R, C, seed, dev):
    """a padded batch as sample_rois_batched leaves it: a quarter foreground, an eighth of the rows padding (label -1)"""
    rs = np.random.RandomState(seed)
    N = B * R
    labels = np.zeros(N, np.int32)
    fg = rs.uniform(size=N) < 0.25
    labels[fg] = rs.randint(1, C, int(fg.sum()))
    labels[rs.uniform(size=N) < 0.125] = -1
    t5 = np.zeros((N, 5), np.float32)
    has = labels > 0
    t5[has, 0] = labels[has]
    t5[has, 1:] = (rs.standard_normal((int(has.sum()), 4)) * 0.7).astype(np.float32)
    d = lambda a: torch.from_numpy(a).to(dev)
    return (d((rs.standard_normal((N, C)) * 3.0).astype(np.float32)), d(labels),
            d((rs.standard_normal((N, 4 * C)) * 0.7).astype(np.float32)), d(t5))


def torch_side(cls_score, labels, bbox_pred, t5):
    """-> (step, leaves): step() runs forward + backward of the reference's formulation on the compacted rows"""
    keep = labels >= 0
    x = cls_score[keep].clone().requires_grad_()
    p = bbox_pred[keep].clone().requires_grad_()
    lab, t = labels[keep].long(), t5[keep]
    k = t[:, 0].long()
    cols = 4 * k[:, None] + torch.arange(4, device=p.device)[None, :]
    on = (k[:, None] > 0).float()
    bt = torch.zeros_like(p).scatter_(1, cols, t[:, 1:]) * on                # fast_rcnn_sample_rois.py:139-163
    bi = torch.zeros_like(p).scatter_(1, cols, 1.0) * on
    bo = (bi > 0).float()                                                    # :107
    beta = 1.0

    def step():
        x.grad = p.grad = None
        loss_cls = torch.nn.functional.cross_entropy(x, lab)                 # train_fast.py:147
        d = (p - bt) * bi                                                    # loss.py:14-20
        a = torch.abs(d)
        case1 = torch.le(a, beta).float()
        loss_bbox = torch.sum((0.5 * d ** 2 / beta * case1 + (a - 0.5 * beta) * (1 - case1)) * bo) / p.size(0)
        acc = torch.mean(torch.eq(torch.max(torch.nn.functional.softmax(x, dim=1), 1)[1], lab).float())   # loss.py:22-26
        (loss_cls + loss_bbox).backward()                                    # train_fast.py:154-158
        return loss_cls, loss_bbox, acc
    return step, (x, p, keep)


def window(fn, calls):
    """milliseconds of `calls` back-to-back calls, by HIP events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_timing needs the GPU: a CPU run gives no time")
    dev = torch.device("cuda", 0)
    lines = []
    for B, R in ((8, 512), (8, 2048)):
        C = 81
        cls_score, labels, bbox_pred, t5 = inputs(B, R, C, 40 + R, dev)
        out = hip_loss.loss_outputs(B * R, C, 4 * C, dev)
        fused = lambda: hip_loss.fast_rcnn_loss(cls_score, labels, bbox_pred, t5, out=out)
        step, (x, p, keep) = torch_side(cls_score, labels, bbox_pred, t5)
        # both sides compute the same thing
        fused()
        lc, lb, acc = step()
        torch.cuda.synchronize()
        L = out["losses"].cpu().numpy()
        assert abs(L[0] - float(lc)) <= 1e-5 * float(lc) and abs(L[1] - float(lb)) <= 1e-5 * float(lb) and abs(L[2] - float(acc)) < 1e-6
        assert float((out["grad_cls_score"][keep] - x.grad).abs().max()) <= 1e-6 / max(L[3], 1.0) * 16
        assert float((out["grad_bbox_pred"][keep] - p.grad).abs().max()) <= 1e-6
        sides = {"fused": fused, "torch": step}
        calls = {}
        for name, fn in sides.items():                                       # warm-up, then the call count of a window
            window(fn, 20)
            ms = window(fn, 50) / 50.0
            calls[name] = max(50, int(args.window * 1e3 / ms) + 1)
        us = {name: [] for name in sides}
        for _ in range(args.rounds):
            for name, fn in sides.items():                                   # alternating
                us[name].append(window(fn, calls[name]) / calls[name] * 1e3)
        med = {name: statistics.median(v) for name, v in us.items()}
        lines.append(json.dumps(dict(
            rows=B * R, classes=C, valid_rows=int(L[3]), window_s=args.window, rounds=args.rounds, calls_per_window=calls,
            fused_us=round(med["fused"], 2), fused_us_min_max=[round(min(us["fused"]), 2), round(max(us["fused"]), 2)],
            torch_us=round(med["torch"], 2), torch_us_min_max=[round(min(us["torch"]), 2), round(max(us["torch"]), 2)],
            torch_over_fused=round(med["torch"] / med["fused"], 2))))
        print(lines[-1], flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
