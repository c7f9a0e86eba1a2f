"""Generate tests/golden/postprocess_soft_vote.npz from the REFERENCE ITSELF (build container only; needs /root/reference +
`make -C oracle ref`), in the style of make_golden.py, which it leaves alone.

    python tests/golden/make_det_options_golden.py

The reference's own box_results_with_nms_and_limit (lib/utils/result_utils.py:96-168, imported in place, Cython NMS / Soft-NMS
built from lib/utils_cython) with its two test-time branches switched on, for the configurations in CONFIGS, on two inputs:
  pp     the postprocess.npz fixture's scores and clipped boxes (160 rois x 81 classes)
  crowd  a seeded synthetic case (3 classes): class 1 holds 150 separated cells of two heavily overlapping boxes each, the cells'
         scores on a 1/8 grid (exact ties at the 100th row of the limit), plus a pile of 200 boxes around one centre (a long
         Soft-NMS walk with many swap-with-last discards); class 2 a handful of boxes
Stored per (case, config): <case>_<config>_{scores, boxes, cls_id} in the reference's order; and the crowd case's inputs.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402

# name -> keyword arguments of box_results_with_nms_and_limit (sigma 0.5, Nt = overlap_thresh 0.5, 'ID' vote scoring)
CONFIGS = {
    "soft_linear": dict(do_soft_nms=True, soft_nms_method="linear"),
    "soft_gaussian": dict(do_soft_nms=True, soft_nms_method="gaussian"),
    "soft_hard": dict(do_soft_nms=True, soft_nms_method="hard"),
    "soft_linear_vote": dict(do_soft_nms=True, soft_nms_method="linear", do_bbox_vote=True, bbox_vote_thresh=0.8),
    "hard_vote06": dict(do_bbox_vote=True, bbox_vote_thresh=0.6),
}


def crowd_inputs():
    """Seeded crowded case: scores [500, 3], clipped boxes [500, 12] (class j in columns 4j..4j+3)."""
    rs = np.random.RandomState(20261016)
    im_h, im_w = 700.0, 1000.0
    gx, gy = np.meshgrid(np.arange(15), np.arange(10))
    ctr = np.stack([40.0 + 62.0 * gx.ravel(), 40.0 + 62.0 * gy.ravel()], 1)            # 150 cells, 40 px boxes, no overlap
    cell = np.repeat(ctr, 2, 0) + rs.uniform(-3, 3, (300, 2))
    pile = np.array([[500.0, 620.0]]) + rs.uniform(-12, 12, (200, 2))
    c = np.vstack([cell, pile])
    half = np.vstack([np.full((300, 2), 20.0), rs.uniform(30, 45, (200, 2))])
    b1 = np.hstack([c - half, c + half - 1])
    b1[:, 0::2] = np.clip(b1[:, 0::2], 0, im_w - 1)
    b1[:, 1::2] = np.clip(b1[:, 1::2], 0, im_h - 1)
    # exact ties only BETWEEN separated cells (the reference's hard NMS orders tied scores by an unstable argsort, cython_nms.pyx:55):
    # a cell's first box on the 1/8 grid, its second 1/64 below; the pile's scores distinct
    s_cell = np.repeat(rs.randint(2, 8, 150) / 8.0, 2) - np.tile([0.0, 1.0 / 64.0], 150)
    s1 = np.concatenate([s_cell, rs.permutation(200) / 256.0 + 0.1 + rs.uniform(0, 1.0 / 512.0, 200)])
    b2 = b1[rs.permutation(500)] + rs.uniform(-2, 2, (500, 4))
    b2 = np.clip(b2, 0, im_w - 1)
    s2 = np.zeros(500)
    s2[rs.choice(500, 12, replace=False)] = rs.uniform(0.1, 0.9, 12)
    boxes = np.hstack([np.zeros((500, 4)), b1, b2]).astype(np.float32)
    scores = np.stack([1.0 - np.maximum(s1, s2), s1, s2], 1).astype(np.float32)
    return scores, boxes


def main():
    ns = rh.load_reference()
    g = np.load(os.path.join(HERE, "postprocess.npz"))
    crowd_scores, crowd_boxes = crowd_inputs()
    cases = {"pp": (g["cls"], g["pred_clipped"], 81), "crowd": (crowd_scores, crowd_boxes, 3)}
    arrs = dict(crowd_scores=crowd_scores, crowd_boxes=crowd_boxes)
    for case, (scores, boxes, ncls) in cases.items():
        for name, kw in CONFIGS.items():
            sc, bx, cb = ns.result_utils.box_results_with_nms_and_limit(scores, boxes.copy(), num_classes=ncls, **kw)
            arrs["%s_%s_scores" % (case, name)] = np.asarray(sc, np.float32)
            arrs["%s_%s_boxes" % (case, name)] = np.asarray(bx, np.float32)
            arrs["%s_%s_cls_id" % (case, name)] = np.concatenate([np.full(len(cb[j]), j, np.int32) for j in range(1, ncls)])
    path = os.path.join(HERE, "postprocess_soft_vote.npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %7.1f KB  %d arrays" % ("postprocess_soft_vote", os.path.getsize(path) / 1024.0, len(arrs)))
    for case in cases:
        print(case, {n: len(arrs["%s_%s_scores" % (case, n)]) for n in CONFIGS})


if __name__ == "__main__":
    main()
