"""Generate tests/golden/loss.npz from the REFERENCE ITSELF (build container only; needs the reference tree +
`make -C oracle ref`), in the style of make_train_targets_golden.py.

    python tests/golden/make_loss_golden.py

On the seeded cases of tests/loss_ref.py, restricted to the rows with label >= 0 (the only rows the reference's training step ever
sees, train_fast.py:141-144), with the compact targets expanded by the reference's own _expand_bbox_targets
(lib/utils/fast_rcnn_sample_rois.py:139) and outside weights = inside > 0 (:107):
  * lib/model/loss.py smooth_L1 (:13) and accuracy (:22), imported in place;
  * torch.nn.functional.cross_entropy (what loss.py:11 imports) on the CPU;
  * gradients by autograd of loss_cls + loss_bbox (train_fast.py:154-158),
all in FLOAT64: the yardstick `y` of the tests.  The same chain in float32 gives e_ref, the float32 CPU reference's own distance
from y, per case and quantity.  accuracy is taken as the reference takes it, on the float32 logits.

Stand-ins, local to this script: empty `torchvision` / `torchvision.models` modules and a `model.roi_align` carrying a RoIAlign
attribute (loss.py:5-6 imports them; nothing here calls them); the names isnan, infbreak and printmax set to None on the
reference's utils.utils where it lacks them (loss.py:8 imports them from there, its commented-out module used them).

Stored per case <c>: <c>_digest (sha1 of the inputs' bytes: the seeded inputs are reproducible), <c>_loss_cls, <c>_loss_bbox,
<c>_accuracy, <c>_n_valid, <c>_e_ref_cls, <c>_e_ref_box, <c>_grad_cls [N, C] and <c>_grad_box4 [N, 4] (the four selected columns;
every other column is asserted zero), rows with label < 0 zero; for the cases of loss_ref.SAMPLED_CASES only the rows
loss_ref.sample_rows names.  Per general smooth_L1 case <s>: <s>_digest, <s>_loss, <s>_e_ref, <s>_grad [N, W].
"""
import hashlib
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402
import loss_ref as lr  # noqa: E402


def load():
    ns = rh.load_reference()
    for name in ("torchvision", "torchvision.models"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["torchvision"].models = sys.modules["torchvision.models"]
    stand_in = types.ModuleType("model.roi_align")
    stand_in.RoIAlign = object
    sys.modules.setdefault("model.roi_align", stand_in)
    utils = importlib.import_module("utils.utils")
    for name in ("isnan", "infbreak", "printmax"):
        if not hasattr(utils, name):
            setattr(utils, name, None)
    ns.loss = importlib.import_module("model.loss")
    ns.sample = importlib.import_module("utils.fast_rcnn_sample_rois")
    return ns


def digest(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return np.frombuffer(h.digest(), np.uint8)


def chain(ns, x, labels, pred, bt, bi, bo, beta, dtype):
    """train_fast.py:147-158 on valid rows -> (loss_cls, loss_bbox, grad_cls, grad_box) as float64 numpy"""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    xs, ps = t(x).requires_grad_(), t(pred).requires_grad_()
    loss_cls = ns.loss.cross_entropy(xs, torch.from_numpy(labels.astype(np.int64)))
    loss_bbox = ns.loss.smooth_L1(ps, t(bt), t(bi), t(bo), beta)
    (loss_cls + loss_bbox).backward()
    return (float(loss_cls.detach()), float(loss_bbox.detach()), xs.grad.double().numpy(), ps.grad.double().numpy())


def main():
    ns = load()
    assert ns.loss.cross_entropy is torch.nn.functional.cross_entropy
    arrs = {}
    for name in lr.GOLDEN_CASES:
        c = lr.make_case(name)
        x, labels, pred, t5, beta = c["cls_score"], c["labels"], c["bbox_pred"], c["targets5"], c["beta"]
        N, C = x.shape
        W = pred.shape[1]
        idx = np.where(labels >= 0)[0]
        bt, bi = ns.sample._expand_bbox_targets(t5[idx], C, W == 8 and C != 2)
        bo = np.array(bi > 0, dtype=bi.dtype)                                # fast_rcnn_sample_rois.py:107
        assert bt.shape == (len(idx), W) and bt.dtype == np.float32
        y = chain(ns, x[idx], labels[idx], pred[idx], bt, bi, bo, beta, torch.float64)
        r = chain(ns, x[idx], labels[idx], pred[idx], bt, bi, bo, beta, torch.float32)
        acc = float(ns.loss.accuracy(torch.from_numpy(x[idx]), torch.from_numpy(labels[idx])))
        assert np.array_equal(lr.argmax_logits(x[idx]), lr.argmax_softmax(x[idx])), name   # no rounding tie in the seeded cases
        grad_cls = np.zeros((N, C), np.float64)
        grad_cls[idx] = y[2]
        k = np.where(t5[:, 0] > 0, 1 if W == 8 else t5[:, 0], 0).astype(np.int64)
        cols = 4 * k[:, None] + np.arange(4)[None, :]
        full = np.zeros((N, W), np.float64)
        full[idx] = y[3]
        grad_box4 = np.where(k[:, None] > 0, np.take_along_axis(full, cols, 1), 0.0)
        rest = full.copy()
        np.put_along_axis(rest, cols, 0.0, 1)
        assert not rest.any() and not full[k == 0].any()
        if name in lr.SAMPLED_CASES:
            rows = lr.sample_rows(name, N)
            grad_cls, grad_box4 = grad_cls[rows], grad_box4[rows]
        e_cls, e_box = abs(r[0] - y[0]), abs(r[1] - y[1])
        nv = len(idx)
        e_gc = float(np.max(np.abs(r[2] - y[2]))) * nv / lr.EPS
        nz = y[3] != 0
        e_gb = float(np.max(np.abs(r[3][nz] - y[3][nz]) / np.abs(y[3][nz]))) / lr.EPS if nz.any() else 0.0
        arrs.update({name + "_digest": digest(x, labels, pred, t5), name + "_loss_cls": np.float64(y[0]),
                     name + "_loss_bbox": np.float64(y[1]), name + "_accuracy": np.float64(acc), name + "_n_valid": np.int64(nv),
                     name + "_e_ref_cls": np.float64(e_cls), name + "_e_ref_box": np.float64(e_box), name + "_grad_cls": grad_cls,
                     name + "_grad_box4": grad_box4})
        b = lr.bounds(dict(loss_cls=y[0], loss_bbox=y[1], n_valid=nv), x[idx])
        print("%-7s N %5d valid %5d C %4d  loss_cls %.6f loss_bbox %.6f acc %.4f | float32 reference: loss_cls %.2f loss_bbox %.2f "
              "of 32 eps scale, grad_cls %.2f of 16 eps / n, grad_box %.2f of 8 eps" % (
                  name, N, nv, C, y[0], y[1], acc, 32 * e_cls / b["loss_cls"] if b["loss_cls"] else 0.0,
                  32 * e_box / b["loss_bbox"] if b["loss_bbox"] else 0.0, e_gc, e_gb))
    for name in lr.SMOOTH_CASES:
        c = lr.make_smooth_case(name)
        res = {}
        for dt in (torch.float64, torch.float32):
            p = torch.tensor(c["pred"], dtype=dt).requires_grad_()
            loss = ns.loss.smooth_L1(p, *[torch.tensor(c[k], dtype=dt) for k in ("targets", "alpha_in", "alpha_out")], c["beta"])
            loss.backward()
            res[dt] = (float(loss.detach()), p.grad.double().numpy())
        y, r = res[torch.float64], res[torch.float32]
        arrs.update({name + "_digest": digest(c["pred"], c["targets"], c["alpha_in"], c["alpha_out"]), name + "_loss": np.float64(y[0]),
                     name + "_e_ref": np.float64(abs(r[0] - y[0])), name + "_grad": y[1]})
        nz = y[1] != 0
        print("%-7s shape %s loss %.6f | float32 reference: loss %.2f eps relative, grad %.2f eps relative" % (
            name, c["pred"].shape, y[0], abs(r[0] - y[0]) / abs(y[0]) / lr.EPS,
            float(np.max(np.abs(r[1][nz] - y[1][nz]) / np.abs(y[1][nz]))) / lr.EPS))
    path = os.path.join(HERE, "loss.npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %7.1f KB  %d arrays" % ("loss", os.path.getsize(path) / 1024.0, len(arrs)))


if __name__ == "__main__":
    main()
