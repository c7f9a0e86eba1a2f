"""Generate tests/golden/mask_train_limits.npz from the REFERENCE ITSELF (build container only; needs the reference tree and
`make -C oracle ref`), for the cases of tests/mask_train_limit_cases.py, in the way of make_mask_train_golden.py.

    python tests/golden/make_mask_train_limits_golden.py

Per targets case <c>: <c>_poly_boxes [E,4] (utils.segms.polys_to_boxes on the valid polygons of every eligible gt), <c>_overlaps
[rows,E] (cython_bbox.bbox_overlaps of the boxes of limit_cases.sample_rows(<c>), at most 64 mask rows, against those poly-boxes),
and the restatement's integers <c>_mask_gt and <c>_masks (int8).  The 56 calls of `all_m` share their image, so the poly-boxes, the
overlaps and mask_gt, which do not depend on M, are stored once as all_m_*, and all_m_masks holds the matched rows' masks of
M = 1 .. 56 one behind the other.  Per loss case <c> (and <c>_x: a multi-row case with the EXTREMES logits on its "ext" rows):
loss_<c> (float64, torch's binary_cross_entropy_with_logits), loss_<c>_e_ref and loss_<c>_e_grad (the float32 CPU run's distance
from it: absolute, and in units of the gradient bound), loss_<c>_grad (float64 at limit_cases.grad_sample(<c>), at most 64
elements).  Where pycocotools imports, segms.polys_to_mask_wrt_box itself is recorded on the sampled rows into
mask_train_limits_coco.npz.  Fixed zip timestamps: the same inputs give the same bytes.
"""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import mask_train_limit_cases as lc  # noqa: E402
import mask_train_ref as mr  # noqa: E402
from make_mask_train_golden import have_pycocotools, loss_chain, write_npz  # noqa: E402


def main():
    coco = have_pycocotools()
    import ref_harness as rh
    ns = rh.load_reference()
    segms = importlib.import_module("utils.segms")
    arrs, coco_arrs = {}, {}
    all_m_masks, all_m_coco = [], []
    for name in sorted(lc.TARGETS):
        img, M, k_min, k_max, Fm = lc.case(name)
        out = lc.want(name)
        elig = lc.eligible(img)
        flat = [[p.reshape(-1).tolist() for p in mr.valid_polys(img, g)] for g in elig]
        pb = segms.polys_to_boxes(flat) if flat else np.zeros((0, 4), np.float32)
        rows = lc.sample_rows(name)
        boxes = lc.row_boxes(name, rows)
        ov = ns.cython_bbox.bbox_overlaps(boxes, pb.astype(np.float32)) if rows and len(pb) else np.zeros((len(rows), len(pb)), np.float32)
        if coco:
            cw = np.stack([segms.polys_to_mask_wrt_box(flat[elig.index(int(out["mask_gt"][t]))], boxes[k], M).reshape(-1)
                           for k, t in enumerate(rows)]).astype(np.int8) if rows else np.zeros((0, M * M), np.int8)
        if name.startswith("all_m"):
            tag = "all_m"
            if tag + "_mask_gt" in arrs:
                assert np.array_equal(arrs[tag + "_mask_gt"], out["mask_gt"]) and np.array_equal(arrs[tag + "_overlaps"], ov)
            all_m_masks.append((M, out["masks"][rows].astype(np.int8).reshape(-1)))
            if coco:
                all_m_coco.append((M, cw.reshape(-1)))
        else:
            tag = name
            arrs[tag + "_masks"] = out["masks"].astype(np.int8)
            if coco:
                coco_arrs[tag + "_masks"] = cw
        arrs.update({tag + "_poly_boxes": pb.astype(np.float32), tag + "_overlaps": ov.astype(np.float32), tag + "_mask_gt": out["mask_gt"]})
        print("%-14s M %2d  rows %3d (overlaps of %2d)  eligible gt %3d  on %d" % (name, M, int(out["n_mask"]), len(rows), len(elig),
                                                                                int((out["masks"] == 1).sum())))
    arrs["all_m_masks"] = np.concatenate([m for _, m in sorted(all_m_masks)])
    if coco:
        coco_arrs["all_m_masks"] = np.concatenate([m for _, m in sorted(all_m_coco)])
    for name, extremes in [(n, False) for n in lc.LOSS] + [(n, True) for n in lc.MULTI_ROW]:
        tag = name + ("_x" if extremes else "")
        c = lc.loss_case(name, extremes)
        y, r = loss_chain(c, torch.float64), loss_chain(c, torch.float32)
        mine = lc.loss_want(name, extremes)
        b = mr.loss_bounds(mine)
        e_grad = float(np.max(np.abs(r[1] - y[1]))) / b["grad"]
        e_ref = abs(r[0] - y[0]) if np.isfinite(r[0]) else 0.0               # float32 torch overflows on a sum of 3e38 terms: not recorded
        arrs.update({"loss_" + tag: np.float64(y[0]), "loss_" + tag + "_e_ref": np.float64(e_ref),
                     "loss_" + tag + "_grad": y[1].ravel()[lc.grad_sample(name, extremes)], "loss_" + tag + "_e_grad": np.float64(e_grad)})
        print("%-13s loss %.6g | float32 reference: loss %.3f of 32 eps scale%s, gradient %.3f of its bound" % (
            tag, y[0], e_ref / (32 * mr.EPS * max(abs(mine["loss"]), mine["scale"], 1e-300)),
            "" if np.isfinite(r[0]) else " (its sum overflows: not recorded)", e_grad))
    path = os.path.join(HERE, "mask_train_limits.npz")
    write_npz(path, arrs)
    print("%-28s %7.1f KB  %d arrays" % ("mask_train_limits", os.path.getsize(path) / 1024.0, len(arrs)))
    if coco:
        write_npz(os.path.join(HERE, "mask_train_limits_coco.npz"), coco_arrs)
        print("mask_train_limits_coco: polys_to_mask_wrt_box recorded on %d arrays" % len(coco_arrs))
    else:
        print("pycocotools does not import: mask_train_limits_coco.npz not written (rasterisation parity stays unpinned)")


if __name__ == "__main__":
    main()
