"""Generate tests/golden/mask_train.npz from the REFERENCE ITSELF (build container only; needs the reference tree and
`make -C oracle ref`), in the style of make_rpn_train_golden.py.

    python tests/golden/make_mask_train_golden.py

The reference keeps add_mask_rcnn_blobs as a commented-out call; what the contract of include/detectorch_mask_hip.h is built from is
the reference's own and is run here, imported in place, on the cases of tests/mask_train_ref.py:
  * utils.segms.polys_to_boxes on the valid polygons of every eligible gt;
  * cython_bbox.bbox_overlaps of the mask rows' boxes against those poly-boxes;
  * torch.nn.functional.binary_cross_entropy_with_logits over the valid elements of the class channel, in float64 (the yardstick
    `y`) and in float32 (e_ref: the float32 CPU reference's own distance from y), gradients by autograd.

Stored per targets case <c>: <c>_poly_boxes [E,4], <c>_overlaps [rows,E] (rows: the mask rows with a usable box), and the
restatement's integers <c>_mask_gt and <c>_masks (int8).  Per loss case <c>: loss_<c> (float64), loss_<c>_e_ref, loss_<c>_grad (float64,
at most 2000 sampled elements), loss_<c>_e_grad (the float32 reference's largest gradient distance in units of the gradient bound);
<c>_x: the case with the extreme logits written over its first elements (where the float32 reference's own sum overflows -- terms of
3e38 -- its e_ref is stored as 0: not recorded, the case is compared with the float64 value alone).
Where pycocotools imports, segms.polys_to_mask_wrt_box itself is recorded on the same rows into mask_train_coco.npz (the test that
reads it skips while the file is absent: pin-when-available).  The archives are written with fixed zip timestamps: the same inputs
give the same bytes.
"""
import importlib
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mask_train_ref as mr  # noqa: E402

GOLDEN_LOSS_CASES = ("r1m1", "r3m14", "r65m7", "r64m28", "r257m14", "m3k81", "m28k81", "m5k2")


def have_pycocotools():
    try:
        importlib.import_module("pycocotools.mask")
        return True
    except ImportError:
        return False


def write_npz(path, arrs):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrs):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrs[k]), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def targets_cases():
    """name -> (image, M, k_min, k_max, Fm): the seeded images and the hand-made ones"""
    out = {n: mr.seeded_image(n) + (2, 5, 8) for n in mr.SEEDED}
    out.update(mr.hand_cases())
    return out


def loss_chain(c, dtype):
    Rm, K, M, _ = c["logits"].shape
    x = torch.tensor(c["logits"], dtype=dtype).requires_grad_()
    cls, masks = c["cls"], c["masks"]
    rows = np.where((cls >= 0) & (cls < K))[0]
    if len(rows) == 0:
        return 0.0, np.zeros(c["logits"].shape)
    sel = x.reshape(Rm, K, M * M)[torch.from_numpy(rows), torch.from_numpy(cls[rows].astype(np.int64))]
    t = torch.from_numpy(masks[rows])
    valid = (t == 0) | (t == 1)
    n = int(valid.sum())
    if n == 0:
        return 0.0, np.zeros(c["logits"].shape)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(sel[valid], t[valid].to(dtype), reduction="sum") / n
    loss.backward()
    return float(loss.detach()), x.grad.double().numpy()


def main():
    coco = have_pycocotools()
    import ref_harness as rh
    ns = rh.load_reference()
    segms = importlib.import_module("utils.segms")
    arrs, coco_arrs = {}, {}
    for name, (img, M, k_min, k_max, Fm) in sorted(targets_cases().items()):
        out = mr.targets(img, M, k_min, k_max, Fm)
        n_g = min(max(int(img["gt_count"]), 0), len(img["gt_boxes"]))
        elig = [g for g in range(n_g) if img["gt_classes"][g] > 0 and img["gt_is_crowd"][g] == 0 and mr.valid_polys(img, g)]
        flat = [[p.reshape(-1).tolist() for p in mr.valid_polys(img, g)] for g in elig]
        pb = segms.polys_to_boxes(flat) if flat else np.zeros((0, 4), np.float32)
        rows = [t for t in range(int(out["n_mask"])) if out["mask_gt"][t] >= 0]
        cand = np.concatenate([img["gt_boxes"][:n_g], img["proposals"]])
        fg = [r for r in range(min(max(int(img["n_rois"]), 0), len(img["labels"]))) if img["labels"][r] > 0][:Fm]
        boxes = np.stack([cand[img["keep_inds"][fg[t]]] for t in rows]).astype(np.float32) if rows else np.zeros((0, 4), np.float32)
        ov = ns.cython_bbox.bbox_overlaps(boxes, pb.astype(np.float32)) if rows and len(pb) else np.zeros((len(rows), len(pb)), np.float32)
        arrs.update({name + "_poly_boxes": pb.astype(np.float32), name + "_overlaps": ov.astype(np.float32),
                     name + "_mask_gt": out["mask_gt"], name + "_masks": out["masks"].astype(np.int8)})
        if coco:
            want = np.stack([segms.polys_to_mask_wrt_box(flat[elig.index(int(out["mask_gt"][t]))], boxes[k], M).reshape(-1)
                             for k, t in enumerate(rows)]) if rows else np.zeros((0, M * M))
            coco_arrs[name + "_masks"] = want.astype(np.int8)
        print("%-12s M %2d  rows %d  eligible gt %d  on %d" % (name, M, int(out["n_mask"]), len(elig), int((out["masks"] == 1).sum())))
    for name in GOLDEN_LOSS_CASES:
        for extremes in (False, True):
            tag = name + ("_x" if extremes else "")
            c = mr.make_loss_case(name, extremes=extremes)
            y, r = loss_chain(c, torch.float64), loss_chain(c, torch.float32)
            mine = mr.loss64(c["logits"], c["masks"], c["cls"])
            b = mr.loss_bounds(mine)
            keep = np.sort(np.random.RandomState(len(tag)).choice(y[1].size, min(2000, y[1].size), replace=False))
            e_grad = float(np.max(np.abs(r[1] - y[1]))) / b["grad"]
            e_ref = abs(r[0] - y[0]) if np.isfinite(r[0]) else 0.0      # float32 torch overflows on the sum of 3e38 terms: not recorded
            arrs.update({"loss_" + tag: np.float64(y[0]), "loss_" + tag + "_e_ref": np.float64(e_ref),
                         "loss_" + tag + "_grad": y[1].ravel()[keep], "loss_" + tag + "_e_grad": np.float64(e_grad)})
            print("%-10s loss %.6f | float32 reference: loss %.3f of 32 eps scale, gradient %.3f of its bound" % (
                tag, y[0], e_ref / (32 * mr.EPS * max(abs(mine["loss"]), mine["scale"], 1e-300)), e_grad))
    path = os.path.join(HERE, "mask_train.npz")
    write_npz(path, arrs)
    print("%-28s %7.1f KB  %d arrays" % ("mask_train", os.path.getsize(path) / 1024.0, len(arrs)))
    if coco:
        write_npz(os.path.join(HERE, "mask_train_coco.npz"), coco_arrs)
        print("mask_train_coco: polys_to_mask_wrt_box recorded on %d cases" % len(coco_arrs))
    else:
        print("pycocotools does not import: mask_train_coco.npz not written (rasterisation parity stays unpinned)")


if __name__ == "__main__":
    main()
