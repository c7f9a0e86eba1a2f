"""Generate tests/golden/train_targets.npz from the REFERENCE ITSELF (build container only; needs /root/reference +
`make -C oracle ref`), in the style of make_proposal_ingest_golden.py.

    python tests/golden/make_train_targets_golden.py [--time]

The reference's training-minibatch chain, imported in place and called on the seeded cases of tests/train_targets_ref.py:
lib/data/json_dataset.py _merge_proposal_boxes_into_roidb (:333), _filter_crowd_proposals (:397), _add_class_assignments (:417),
lib/data/roidb.py _compute_targets (:176), lib/utils/fast_rcnn_sample_rois.py fast_rcnn_sample_rois (:41) and, for the
class-agnostic case, _expand_bbox_targets (:139) with its own arguments (fast_rcnn_sample_rois calls it with the defaults).

Three stand-ins, all local to this script:
  * a `pycocotools.coco` module carrying a COCO attribute (json_dataset.py:37 imports it; nothing here calls it);
  * pycocotools.mask.iou := the float64 restatement of bbIou for iscrowd boxes (train_targets_ref.bb_iou_crowd) -- pycocotools is
    not installed, so the crowd filter's parity with the real package is UNPINNED (like the three legs of test_thirdparty_golden.py);
  * utils.fast_rcnn_sample_rois.npr := an object whose choice(a, size, replace) returns a[np.lexsort((a, keys[a]))][:size]: one of
    the samples numpy's generator may draw, chosen by the case's rand_keys.
The gt part of a roidb entry is built as _add_gt_annotations builds it (json_dataset.py:181-215).

Stored per case <c>: the inputs (gt_boxes, gt_classes, is_crowd, proposals, im_scale, rand_keys), max_overlaps, max_classes,
targets5 (the entry's bbox_targets), keep_inds, n_fg, labels, rois, and the expanded blobs except for the R = 512 case.
e_ref: the largest distance of the reference's own dw / dh from w * log(float64(ratio)), in float32 ulps of that value, over all
cases -- the yardstick of the device's tolerance (e_ref + 2).  --time also prints the chain's CPU time for eight images of case g.
"""
import importlib
import os
import sys
import time
import types

import numpy as np
import scipy.sparse

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_harness as rh  # noqa: E402
import train_targets_ref as tr  # noqa: E402


class KeyedChoice:
    """stands in for numpy.random inside utils.fast_rcnn_sample_rois; records what it hands out"""
    def __init__(self):
        self.keys, self.drawn = None, []

    def choice(self, a, size, replace=False):
        assert not replace
        out = a[np.lexsort((a, self.keys[a]))][:size]
        self.drawn.append(out)
        return out


def load():
    ns = rh.load_reference()
    coco = types.ModuleType("pycocotools.coco")
    coco.COCO = object
    sys.modules["pycocotools.coco"] = coco
    sys.modules["pycocotools.mask"].iou = lambda dt, gt, iscrowd: (
        tr.bb_iou_crowd(dt, gt) if all(iscrowd) else (_ for _ in ()).throw(NotImplementedError("iscrowd only")))
    ns.json_dataset = importlib.import_module("data.json_dataset")
    ns.roidb = importlib.import_module("data.roidb")
    ns.sample = importlib.import_module("utils.fast_rcnn_sample_rois")
    ns.npr = KeyedChoice()
    ns.sample.npr = ns.npr
    return ns


def gt_entry(case, num_classes):
    """json_dataset.py:181-215 for the case's gt"""
    gt, cls, crowd = case["gt_boxes"], case["gt_classes"], case["is_crowd"]
    G = len(gt)
    ov = np.zeros((G, num_classes), np.float32)
    for ix in range(G):
        if crowd[ix]:
            ov[ix, :] = -1.0                                                 # :213
        else:
            ov[ix, cls[ix]] = 1.0                                            # :215
    return dict(boxes=gt.astype(np.float32).reshape(G, 4), gt_classes=cls.astype(np.int32), is_crowd=crowd.astype(bool),
                seg_areas=np.zeros(G, np.float32), gt_overlaps=scipy.sparse.csr_matrix(ov),
                box_to_gt_ind_map=np.arange(G, dtype=np.int32))


def run_chain(ns, case, params):
    entry = gt_entry(case, params["num_classes"])
    ns.json_dataset._merge_proposal_boxes_into_roidb([entry], [case["proposals"]])
    if params["crowd_thresh"] > 0:                                           # json_dataset.py:328
        ns.json_dataset._filter_crowd_proposals([entry], params["crowd_thresh"])
    ns.json_dataset._add_class_assignments([entry])
    entry["bbox_targets"] = ns.roidb._compute_targets(entry, params["bbox_thresh"], params["cls_agnostic_bbox_reg"],
                                                      params["reg_weights"])
    ns.npr.keys, ns.npr.drawn = case["rand_keys"], []
    blobs = ns.sample.fast_rcnn_sample_rois(entry, case["im_scale"], 0, params["rois_per_image"], params["fg_fraction"],
                                            params["fg_thresh"], params["bg_thresh_hi"], params["bg_thresh_lo"])
    keep = np.concatenate(ns.npr.drawn).astype(np.int32) if ns.npr.drawn else np.zeros(0, np.int32)
    if params["cls_agnostic_bbox_reg"]:
        bt, bw = ns.sample._expand_bbox_targets(entry["bbox_targets"][keep, :], params["num_classes"], True)
        blobs.update(bbox_targets=bt, bbox_inside_weights=bw, bbox_outside_weights=np.array(bw > 0, dtype=bw.dtype))
    return entry, blobs, keep


def main():
    ns = load()
    arrs, e_ref = {}, 0.0
    for c in tr.GOLDEN_CASES:
        case, params = tr.make_case(c), tr.params_of(c)
        entry, blobs, keep = run_chain(ns, case, params)
        mo = np.asarray(entry["max_overlaps"])
        assert mo.dtype == np.float32 and entry["bbox_targets"].dtype == np.float32
        n_fg = min(int(np.round(params["fg_fraction"] * params["rois_per_image"])), int(np.sum(mo >= params["fg_thresh"])))
        for k in ("gt_boxes", "gt_classes", "is_crowd", "proposals", "rand_keys"):
            arrs[c + "_" + k] = case[k]
        arrs[c + "_im_scale"] = np.float64(case["im_scale"])
        arrs[c + "_max_overlaps"] = mo
        arrs[c + "_max_classes"] = np.asarray(entry["max_classes"], np.int32)
        arrs[c + "_targets5"] = entry["bbox_targets"]
        arrs[c + "_keep_inds"], arrs[c + "_n_fg"] = keep, np.int32(n_fg)
        arrs[c + "_labels"] = blobs["labels_int32"]
        arrs[c + "_rois"] = np.asarray(blobs["rois"], np.float32)
        assert blobs["rois"].dtype == np.float32 and len(blobs["rois"]) == len(keep)
        if c in tr.EXPANDED_CASES:
            for k in ("bbox_targets", "bbox_inside_weights", "bbox_outside_weights"):
                assert blobs[k].dtype == np.float32
                arrs[c + "_" + k] = blobs[k]
        # the reference's own distance from the float64 yardstick (the ratios are the restatement's, whose dx / dy and target
        # classes are bit-equal to the reference's: the same gt was assigned)
        mine = tr.minibatch(case, params)
        assert tr.same_bits(mine["targets5"][:, :3], entry["bbox_targets"][:, :3])
        u = tr.ulps_from(entry["bbox_targets"][:, 3:], mine["want64"])
        e_ref = max(e_ref, float(u.max()) if u.size else 0.0)
        crowd_filtered = int(np.sum(mo[len(case["gt_boxes"]):] == -1))
        print("%s: candidates %4d  fg %4d  bg %4d  crowd-filtered %3d  kept %3d (fg %3d)  max ulps of dw/dh %.2f" % (
            c, len(mo), int(np.sum(mo >= params["fg_thresh"])),
            int(np.sum((mo < params["bg_thresh_hi"]) & (mo >= params["bg_thresh_lo"]))), crowd_filtered, len(keep), n_fg,
            float(u.max()) if u.size else 0.0))
    assert np.isfinite(e_ref)
    arrs["e_ref"] = np.float64(e_ref)
    path = os.path.join(HERE, "train_targets.npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %7.1f KB  %d arrays  e_ref %.3f ulp" % ("train_targets", os.path.getsize(path) / 1024.0, len(arrs), e_ref))
    if "--time" in sys.argv:                                                 # the host chain on eight images of the default shape
        case, params = tr.make_case("g"), tr.params_of("g")
        best = float("inf")
        for _ in range(5):
            t0 = time.perf_counter()
            for _ in range(8):
                run_chain(ns, case, params)
            best = min(best, time.perf_counter() - t0)
        print("reference chain, 8 images of case g (G 16, P 2000, R 512): %.1f ms (best of 5, this machine's CPU)" % (best * 1e3))


if __name__ == "__main__":
    main()
