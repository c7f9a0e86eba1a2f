"""Pin-when-available golden for the mask evaluation: pycocotools' own maskUtils.iou / maskUtils.area and COCOeval(iouType='segm') on
the seeded cases of tests/segm_eval_cases.py whose run lists are plain COCO RLEs (random_masks and stream_case(3 .. 5)).  Run this ON
A HOST THAT HAS pycocotools:

    python tests/golden/make_segm_eval_golden.py             # writes tests/golden/segm_eval_pycocotools.npz

THIS SCRIPT HAS NOT BEEN RUN: pycocotools does not exist where the project is built and tested.  Until someone runs it and commits
the file, tests/test_segm_eval_pycocotools.py is skipped and parity of tests/segm_eval_ref.py (and so of libdetectorch_segm_hip.so)
with pycocotools itself stays unpinned (tests/README_segm_eval.md).  Nothing here imports the product."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))


def cases():
    import segm_eval_cases as sc
    return dict([("random_masks", sc.random_masks())] + [("stream_%d" % s, sc.stream_case(s)) for s in (3, 4, 5)])


def rows(case, n):
    """(detection rows, gt rows) of image n that take part"""
    nc = case["num_classes"]
    nd = min(max(int(case["det_count"][n]), 0), case["dets"].shape[1])
    ng = min(max(int(case["gt_counts"][n]), 0), case["gt_classes"].shape[1])
    return ([d for d in range(nd) if 1 <= case["dets"][n, d, 5] < nc], [g for g in range(ng) if 1 <= case["gt_classes"][n, g] < nc])


def record(case):
    from pycocotools import mask as mask_utils
    from pycocotools.coco import COCO
    from pycocotools.cocoeval import COCOeval
    N, max_out = case["dets"].shape[:2]
    G = case["gt_classes"].shape[1]
    rle = lambda runs, k, h, w: mask_utils.frPyObjects({'size': [h, w], 'counts': [int(v) for v in runs[:k]]}, h, w)
    iou = np.zeros((N, max_out, G))
    det_area, gt_mask_area = np.zeros((N, max_out), np.int64), np.zeros((N, G), np.int64)
    images, anns, results = [], [], []
    for n in range(N):
        h, w = int(case["im_size"][n, 0]), int(case["im_size"][n, 1])
        images.append(dict(id=n + 1, height=h, width=w))
        dr, gr = rows(case, n)
        dt = [rle(case["det_runs"][n, d], case["det_n_runs"][n, d], h, w) for d in dr]
        gt = [rle(case["gt_runs"][n, g], case["gt_n_runs"][n, g], h, w) for g in gr]
        if dt:
            det_area[n, dr] = mask_utils.area(dt)
        if gt:
            gt_mask_area[n, gr] = mask_utils.area(gt)
        if dt and gt:                                          # every pair, whatever the classes; the test reads the same-class ones
            iou[np.ix_([n], dr, gr)] = mask_utils.iou(dt, gt, [int(case["gt_is_crowd"][n, g]) for g in gr])[None]
        for g, r in zip(gr, gt):
            area = float(case["gt_area"][n, g]) if "gt_area" in case else float(gt_mask_area[n, g])
            anns.append(dict(id=len(anns) + 1, image_id=n + 1, category_id=int(case["gt_classes"][n, g]), segmentation=r, area=area,
                             iscrowd=int(case["gt_is_crowd"][n, g]), bbox=[float(v) for v in mask_utils.toBbox(r)]))
        for d, r in zip(dr, dt):
            results.append(dict(image_id=n + 1, category_id=int(case["dets"][n, d, 5]), segmentation=r, score=float(case["dets"][n, d, 4])))
    coco = COCO()
    coco.dataset = dict(images=images, annotations=anns, categories=[dict(id=k) for k in range(1, case["num_classes"])])
    coco.createIndex()
    out = dict(iou=iou, det_area=det_area, gt_mask_area=gt_mask_area)
    if results:
        ev = COCOeval(coco, coco.loadRes(results), 'segm')
        ev.params.iouThrs, ev.params.recThrs = case["iou_thrs"], case["rec_thrs"]
        ev.params.maxDets = list(case["max_dets"])
        ev.params.areaRng = [list(r) for r in case["area_rngs"]]
        ev.params.areaRngLbl = ['all', 'small', 'medium', 'large'][:len(case["area_rngs"])]
        ev.evaluate()
        ev.accumulate()
        ev.summarize()
        out.update(precision=ev.eval['precision'], recall=ev.eval['recall'], stats=np.asarray(ev.stats, np.float64))
    return out


def main():
    import pycocotools
    out = {"pycocotools_version": np.array(getattr(pycocotools, "__version__", "unknown"))}
    for name, case in cases().items():
        for k, v in record(case).items():
            out["%s_%s" % (name, k)] = v
    np.savez_compressed(os.path.join(HERE, "segm_eval_pycocotools.npz"), **out)
    print("wrote segm_eval_pycocotools.npz:", sorted(out))


if __name__ == "__main__":
    main()
