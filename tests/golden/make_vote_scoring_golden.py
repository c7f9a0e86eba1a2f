"""Generate tests/golden/postprocess_vote_scoring.npz from the REFERENCE ITSELF (build container only; needs the reference tree
+ `make -C oracle ref`), in the style of make_det_options_golden.py, which it leaves alone.

    python tests/golden/make_vote_scoring_golden.py

The reference's own box_results_with_nms_and_limit (lib/utils/result_utils.py:96-168) with do_bbox_vote and every scoring other
than 'ID' (bbox_vote_method; beta 1.0, as the function passes it) x {hard NMS, Soft-NMS linear, Soft-NMS gaussian} x
bbox_vote_thresh {0.8, 0.6}, on three inputs:
  pp     the postprocess.npz fixture's scores and clipped boxes (160 rois x 81 classes)
  crowd  make_det_options_golden.crowd_inputs (3 classes, 500 rois)
  dense  vote_scoring_ref.dense_inputs (3 classes, 2400 rois: clusters of 300 to 1200 overlapping boxes)
Stored per (case, nms, thresh, method): <case>_<nms>_<thresh*10>_<method>_{scores, boxes, cls_id} in the reference's order; the
'ID' results of the same runs (<case>_<nms>_<thresh*10>_ID_n, their row counts); the crowd and dense inputs.
Single-segment box_voting(top, all, thresh, method, beta) at beta 1.0 and 0.5: bv_top, bv_all (hundreds of voters per row),
bv_<thresh*10>_<method>_<beta*10>.
For the methods that are not bit-exact on the device (log / exp / pow: TEMP_AVG, GENERALIZED_AVG at beta != 1) the generator
asserts that no two distinct voted scores within 8 ulp straddle the max_det limit, so the device's row set stays exact there.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402
import vote_scoring_ref as vsr  # noqa: E402
from make_det_options_golden import crowd_inputs  # noqa: E402

NMS_KW = {"nms": {}, "linear": dict(do_soft_nms=True, soft_nms_method="linear"),
          "gaussian": dict(do_soft_nms=True, soft_nms_method="gaussian")}


def limit_margin_ok(ns, scores, boxes, ncls, kw, max_det=100):
    """the voted scores of every kept row (no limit): no distinct score within 8 ulp of the max_det-th largest"""
    sc, _, _ = ns.result_utils.box_results_with_nms_and_limit(scores, boxes.copy(), num_classes=ncls, max_detections_per_img=0, **kw)
    sc = np.asarray(sc, np.float32)
    if len(sc) <= max_det:
        return True
    th = np.sort(sc)[-max_det]
    near = sc[(sc != th) & (np.abs(sc - th) <= 8 * np.spacing(th))]
    return len(near) == 0


def main():
    ns = rh.load_reference()
    g = np.load(os.path.join(HERE, "postprocess.npz"))
    crowd_scores, crowd_boxes = crowd_inputs()
    dense_scores, dense_boxes = vsr.dense_inputs()
    cases = {"pp": (g["cls"], g["pred_clipped"], 81), "crowd": (crowd_scores, crowd_boxes, 3), "dense": (dense_scores, dense_boxes, 3)}
    arrs = dict(crowd_scores=crowd_scores, crowd_boxes=crowd_boxes, dense_scores=dense_scores, dense_boxes=dense_boxes)
    for case, (scores, boxes, ncls) in cases.items():
        for nm, nkw in NMS_KW.items():
            for th in vsr.THRESHOLDS:
                tag = "%s_%s_%d" % (case, nm, round(th * 10))
                for m in ("ID",) + vsr.METHODS:
                    kw = dict(nkw, do_bbox_vote=True, bbox_vote_thresh=th, bbox_vote_method=m)
                    sc, bx, cb = ns.result_utils.box_results_with_nms_and_limit(scores, boxes.copy(), num_classes=ncls, **kw)
                    if m == "ID":
                        arrs[tag + "_ID_n"] = np.int32(len(sc))
                        continue
                    if not vsr.exact(m):
                        assert limit_margin_ok(ns, scores, boxes, ncls, kw), (tag, m)
                    arrs["%s_%s_scores" % (tag, m)] = np.asarray(sc, np.float32)
                    arrs["%s_%s_boxes" % (tag, m)] = np.asarray(bx, np.float32)
                    arrs["%s_%s_cls_id" % (tag, m)] = np.concatenate([np.full(len(cb[j]), j, np.int32) for j in range(1, ncls)])
    # single segment: 64 rows of the dense case's class 1 against all 2400 candidates of that class
    alld = np.hstack([dense_boxes[:, 4:8], dense_scores[:, 1:2]]).astype(np.float32)
    top = alld[np.random.RandomState(7).choice(len(alld), 64, replace=False)]
    arrs.update(bv_top=top, bv_all=alld)
    for th in vsr.THRESHOLDS:
        for m in vsr.METHODS:
            for beta in (1.0, 0.5):
                out = ns.boxes.box_voting(top, alld, th, scoring_method=m, beta=beta)
                arrs["bv_%d_%s_%d" % (round(th * 10), m, round(beta * 10))] = np.asarray(out, np.float32)
    path = os.path.join(HERE, "postprocess_vote_scoring.npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %7.1f KB  %d arrays" % ("postprocess_vote_scoring", os.path.getsize(path) / 1024.0, len(arrs)))
    for case in cases:
        for nm in NMS_KW:
            for th in vsr.THRESHOLDS:
                tag = "%s_%s_%d" % (case, nm, round(th * 10))
                print(tag, "ID", int(arrs[tag + "_ID_n"]), {m: len(arrs["%s_%s_scores" % (tag, m)]) for m in vsr.METHODS})


if __name__ == "__main__":
    main()
