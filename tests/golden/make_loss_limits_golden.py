"""Generate tests/golden/loss_limits.npz from the REFERENCE ITSELF (needs the reference tree and `make -C oracle ref`): the
reference's own smooth_L1 and accuracy (lib/model/loss.py:13, :22) and torch.nn.functional.cross_entropy, imported in place through
make_loss_golden.load() (the stand-ins are described there), in FLOAT64 with autograd, on every case of tests/loss_limit_cases.py
that the reference can compute (loss_limit_cases.RECORDED, and every flat case of loss_limit_cases.FLAT).

    python tests/golden/make_loss_limits_golden.py

What the reference is given, where a case holds more than it can take:
  * the rows with label >= 0 only (train_fast.py:141-144), as make_loss_golden.py does;
  * cross_entropy and accuracy index with the label: they get the rows with label < C, and their means are rescaled by
    (rows given) / n_valid -- a row with label >= C stays in the divisor (include/detectorch_loss_hip.h);
  * _expand_bbox_targets (fast_rcnn_sample_rois.py:139) indexes [N, 8] with 4 * class: in the class-agnostic cases it gets the
    compact targets with every class > 0 set to 1, which is how the reference's roidb stores them for that form.
Not recorded (loss_limit_cases.UNRECORDED): the target-class values (no integer, or no index for _expand_bbox_targets) and the
magnitude cases (the float32 y1 * case1 of loss.py:20 is inf * 0 there, and float32 logits 2e38 apart leave the float32 chain
nothing to measure an e_ref with): the GPU tests compare those with the float64 restatement alone, e_ref = 0.

Stored per head case <c>: <c>_sha (SHA-256 of the seeded inputs, loss_limit_cases.head_digest), <c>_scalars float64 [6] =
(loss_cls, loss_bbox, accuracy, n_valid, e_ref_cls, e_ref_box), <c>_grad_cls [rows, C] and <c>_grad_box4 [rows, 4] (the four selected
columns; every other column is asserted zero here) on the rows loss_limit_cases.sample_rows names (all rows for a case of at most
70 rows and 17 classes).  Per flat case <f>: <f>_sha, <f>_scalars = (loss, e_ref), <f>_grad on loss_limit_cases.flat_sample.
The file is byte-reproducible (fixed member order and dates).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_loss_golden as mg  # noqa: E402
from make_train_limits_golden import save_deterministic  # noqa: E402
import loss_limit_cases as ll  # noqa: E402
import loss_ref as lr  # noqa: E402


def head_chain(ns, c, dtype):
    """-> (loss_cls, loss_bbox, grad_cls [N, C], grad_box [N, W] or None) as float64, in the entry's layout and scaling"""
    x, labels, pred, t5 = c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"]
    N, C = x.shape
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    idx = np.where(labels >= 0)[0]
    ok = np.where((labels >= 0) & (labels < C))[0]
    nv = len(idx)
    xs = t(x[ok]).requires_grad_()
    loss_cls = ns.loss.cross_entropy(xs, torch.from_numpy(labels[ok].astype(np.int64))) * (len(ok) / nv)
    total = loss_cls
    ps = None
    if pred is not None:
        W = pred.shape[1]
        compact = t5[idx].copy()
        if W == 8 and C != 2:
            compact[:, 0] = compact[:, 0] > 0
        bt, bi = ns.sample._expand_bbox_targets(compact, C, W == 8 and C != 2)
        bo = np.array(bi > 0, dtype=bi.dtype)                                # fast_rcnn_sample_rois.py:107
        assert bt.shape == (nv, W) and bt.dtype == np.float32
        ps = t(pred[idx]).requires_grad_()
        loss_bbox = ns.loss.smooth_L1(ps, t(bt), t(bi), t(bo), c["beta"])
        total = total + loss_bbox
    total.backward()
    grad_cls = np.zeros((N, C), np.float64)
    grad_cls[ok] = xs.grad.double().numpy()
    grad_box = None
    if pred is not None:
        grad_box = np.zeros(pred.shape, np.float64)
        grad_box[idx] = ps.grad.double().numpy()
    return float(loss_cls.detach()), float(loss_bbox.detach()) if pred is not None else 0.0, grad_cls, grad_box


def main():
    ns = mg.load()
    assert ns.loss.cross_entropy is torch.nn.functional.cross_entropy
    arrs = {}
    worst = dict(cls=(0.0, ""), box=(0.0, ""), flat=(0.0, ""))
    for name in ll.RECORDED:
        c = ll.case(name)
        x, labels = c["cls_score"], c["labels"]
        N, C = x.shape
        y, r = head_chain(ns, c, torch.float64), head_chain(ns, c, torch.float32)
        ok = np.where((labels >= 0) & (labels < C))[0]
        nv = int(np.sum(labels >= 0))
        acc = float(ns.loss.accuracy(torch.from_numpy(x[ok]), torch.from_numpy(labels[ok]))) * len(ok) / nv
        assert np.array_equal(lr.argmax_logits(x[ok]), lr.argmax_softmax(x[ok])), name     # no rounding tie in these cases
        rows = ll.sample_rows(name)
        rows = np.arange(N) if rows is None else rows
        arrs[name + "_sha"] = ll.head_digest(name)
        e_cls, e_box = abs(r[0] - y[0]), abs(r[1] - y[1])
        arrs[name + "_scalars"] = np.array([y[0], y[1], acc, nv, e_cls, e_box], np.float64)
        arrs[name + "_grad_cls"] = y[2][rows]
        if y[3] is not None:
            cols = ll.selected(c)[:, None] + np.arange(4)[None, :]
            rest = y[3].copy()
            np.put_along_axis(rest, cols, 0.0, 1)
            assert not rest.any() and not y[3][labels < 0].any()
            arrs[name + "_grad_box4"] = np.take_along_axis(y[3], cols, 1)[rows]
        b = lr.bounds(dict(loss_cls=y[0], loss_bbox=y[1], n_valid=nv), x[ok])
        u_cls, u_box = 32 * e_cls / b["loss_cls"], 32 * e_box / b["loss_bbox"] if b["loss_bbox"] else 0.0
        worst["cls"], worst["box"] = max(worst["cls"], (u_cls, name)), max(worst["box"], (u_box, name))
        print("%-7s N %5d valid %5d C %4d  loss_cls %.6f loss_bbox %.6f acc %.4f | float32 reference: loss_cls %.2f loss_bbox %.2f "
              "of the 32 eps scale" % (name, N, nv, C, y[0], y[1], acc, u_cls, u_box))
    for shape in ll.FLAT:
        c, name = ll.make_flat(shape), ll.flat_name(shape)
        res = {}
        for dt in (torch.float64, torch.float32):
            p = torch.tensor(c["pred"], dtype=dt).requires_grad_()
            loss = ns.loss.smooth_L1(p, *[torch.tensor(c[k], dtype=dt) for k in ("targets", "alpha_in", "alpha_out")], c["beta"])
            loss.backward()
            res[dt] = (float(loss.detach()), p.grad.double().numpy())
        y, r = res[torch.float64], res[torch.float32]
        e = abs(r[0] - y[0])
        arrs[name + "_sha"] = ll.flat_digest(c)
        arrs[name + "_scalars"] = np.array([y[0], e], np.float64)
        arrs[name + "_grad"] = y[1].reshape(-1)[ll.flat_sample(shape)]
        u = e / abs(y[0]) / lr.EPS if y[0] else 0.0
        worst["flat"] = max(worst["flat"], (u, name))
        print("%-12s loss %.6f | float32 reference: loss %.2f eps relative" % (name, y[0], u))
    path = os.path.join(HERE, "loss_limits.npz")
    save_deterministic(path, arrs)
    print("e_ref maxima: loss_cls %.2f (%s), loss_bbox %.2f (%s) of the 32 eps scale of their bound; flat loss %.2f eps relative (%s)" % (
        worst["cls"] + worst["box"] + worst["flat"]))
    print("%-28s %7.1f KB  %d arrays" % ("loss_limits", os.path.getsize(path) / 1024.0, len(arrs)))


if __name__ == "__main__":
    main()
