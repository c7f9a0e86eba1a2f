"""Generate tests/golden/decode_extremes.npz from the REFERENCE ITSELF (build container only; needs /root/reference +
`make -C oracle ref`), in the style of make_det_options_golden.py, which it leaves alone.

    python tests/golden/make_decode_extremes_golden.py

Box decoding on saturated and non-finite regression outputs.  Every other fixture draws its deltas from N(0, 0.2) / N(0, 0.1);
here seeded subsets of the deltas are overwritten by the values where a decode goes wrong:
  dw/dh  the float32 clamp log(1000/16), one ulp either side of it, 4.2, 30, 1e4, +inf (clamped); -20, -88 (subnormal exp),
         -104 (exp rounds to 0), -inf
  dx/dy  +-10, +-1e3, +-1e30, +-inf, alone and in pairs: centres past every border and the four corners, clipped to one-pixel
         lines and points at the edge
  NaN    in dx, dy, dw and dh, each in anchors of its own (RPN only)
Scores are tie-free throughout, so the reference's order is defined.

  rpn_<case>_*   lib/model/generate_proposals.py GenerateProposals.forward on one level, scaling factor 1.6:
                 c4 (A = 15), p3 and p6 (A = 3; p6 holds fewer anchors than pre_nms_top_n).  cls = the probabilities (the
                 correctly rounded sigmoid of lg, which the fused-logit path is handed), bbox = the deltas.  Runs
                 rpn_<case>_t<thr>_m<min_size>_{props,scores} for rpn_nms_thresh 0 (every filtered pre-NMS row) and 0.7, and
                 rpn_min_size 0 and 16 (p6 also 400: every row filtered).
  bt_*           lib/utils/boxes.py bbox_transform (weights 10, 10, 5, 5) and clip_tiled_boxes on the same value classes scaled
                 by the weights, +-inf but no NaN.
  pp_*           lib/utils/result_utils.py postprocess_output (+ box_results_with_nms_and_limit with linear Soft-NMS and 'ID'
                 voting at 0.8) on head deltas past the clamp and +-inf, RoIs that are one-pixel lines and points at the borders,
                 and classes collapsed onto identical border lines.  The Soft-NMS + vote run leaves out the (roi, class) pairs
                 of pp_soft_vote_drop (zero-area boxes, on which the reference's box_voting raises).  cls = softmax_rows(logits) (oracle/oracle.py), so the
                 same fixture pins the fused-logit path.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_harness as rh  # noqa: E402
import oracle as orc  # noqa: E402  (softmax_rows only: plain numpy, no library)

sys.path.insert(0, ROOT)
from detectorch_amd import synth  # noqa: E402

CLIP = np.float32(4.135166556742356)
F32 = np.float32
DWH = [CLIP, np.nextafter(CLIP, F32(0)), np.nextafter(CLIP, F32(10)), F32(4.2), F32(30), F32(1e4), F32(np.inf),
       F32(-20), F32(-88), F32(-104), F32(-np.inf)]
DXY = [F32(v) for v in (10, -10, 1e3, -1e3, 1e30, -1e30, np.inf, -np.inf)]
CORNERS = [(F32(sx * v), F32(sy * v)) for v in (1e3, np.inf) for sx in (1, -1) for sy in (1, -1)]

# case: (A, H, W, stride, anchor sizes, pre, post, im_h, im_w, copies of the extreme pattern, min sizes)
RPN_CASES = {
    "c4": (15, 8, 12, 16.0, (32, 64, 128, 256, 512), 600, 100, 120, 180, 3, (0, 16)),
    "p3": (3, 16, 24, 8.0, (64,), 800, 1000, 120, 180, 3, (0, 16)),
    "p6": (3, 6, 8, 64.0, (512,), 1000, 1000, 350, 500, 1, (0, 16, 400)),
}
RPN_THRESHOLDS = (0.0, 0.7)
SCALE = 1.6


def sigmoid_cr(x):
    """oracle.rpn_sigmoid: the correctly rounded float32 sigmoid (what the fused-logit RPN path computes)."""
    return (1.0 / (1.0 + np.exp(-np.asarray(x, np.float32).astype(np.float64)))).astype(np.float32)


def tie_free_logits(rs, shape, mu, sd):
    """logits whose correctly rounded sigmoids are pairwise distinct (re-drawn where two collide)."""
    lg = (rs.standard_normal(shape) * sd + mu).astype(np.float32)
    for _ in range(64):
        p = sigmoid_cr(lg).reshape(-1)
        _, idx = np.unique(p, return_index=True)
        if idx.size == p.size:
            return lg
        dup = np.ones(p.size, bool)
        dup[idx] = False
        lg.reshape(-1)[dup] = (rs.standard_normal(int(dup.sum())) * sd + mu).astype(np.float32)
    raise RuntimeError("could not draw tie-free logits")


def extreme_rows(copies, nan=True):
    """The extreme pattern as a list of (dx, dy, dw, dh) rows; None = keep the normal draw."""
    rows = []
    for _ in range(copies):
        rows += [(None, None, v, None) for v in DWH] + [(None, None, None, v) for v in DWH]
        rows += [(v, None, None, None) for v in DXY] + [(None, v, None, None) for v in DXY]
        rows += [(x, y, None, None) for (x, y) in CORNERS]
        rows += [(v, v, None, None) for v in DXY] + [(None, None, v, v) for v in DWH]
        if nan:
            rows += [(F32(np.nan), None, None, None), (None, F32(np.nan), None, None), (None, None, F32(np.nan), None),
                     (None, None, None, F32(np.nan))]
    return rows


def rpn_maps(rs, A, H, W, pre, copies, nan=True):
    """(lg [1,A,H,W], prob [1,A,H,W], deltas [1,4A,H,W]): the extreme rows land on anchors ranked inside the top pre_nms_top_n."""
    lg = tie_free_logits(rs, (1, A, H, W), -1.0, 2.0)
    p = sigmoid_cr(lg)
    d = (rs.standard_normal((1, 4 * A, H, W)) * 0.2).astype(np.float32)
    rows = extreme_rows(copies, nan)
    N = A * H * W
    K = min(N, pre)
    ranked = np.argsort(-p.reshape(-1), kind="stable")[:K]          # flat (a, h, w) indices of the top K
    assert len(rows) <= K, (len(rows), K)
    pick = rs.permutation(ranked)[:len(rows)]
    for flat, row in zip(pick, rows):
        a, hw = divmod(int(flat), H * W)
        h, w = divmod(hw, W)
        for c, v in enumerate(row):
            if v is not None:
                d[0, 4 * a + c, h, w] = v
    return lg, p, d


def rpn(ns, arrs):
    for k, (case, (A, H, W, stride, sizes, pre, post, im_h, im_w, copies, min_sizes)) in enumerate(RPN_CASES.items()):
        rs = synth.rng(17, k)
        lg, p, d = rpn_maps(rs, A, H, W, pre, copies)
        arrs["rpn_%s_cfg" % case] = np.array([A, H, W, stride, pre, post, im_h, im_w] + list(sizes), np.float64)
        arrs["rpn_%s_lg" % case], arrs["rpn_%s_cls" % case], arrs["rpn_%s_bbox" % case] = lg, p, d
        for thr in RPN_THRESHOLDS:
            for m in min_sizes:
                gp = ns.generate_proposals.GenerateProposals(spatial_scale=1.0 / stride, anchor_sizes=sizes,
                                                             rpn_pre_nms_top_n=pre, rpn_post_nms_top_n=post,
                                                             rpn_nms_thresh=thr, rpn_min_size=m)
                props, scores = gp(torch.from_numpy(p), torch.from_numpy(d), im_h, im_w, SCALE)
                tag = "rpn_%s_t%02d_m%d" % (case, int(thr * 10), m)
                arrs[tag + "_props"] = props.numpy().copy()
                arrs[tag + "_scores"] = scores.numpy().reshape(-1).copy()
                print("%-16s %4d rows" % (tag, arrs[tag + "_scores"].shape[0]))


def head_deltas(rs, R, n_cls, weights, nan=False):
    """N(0, 0.1) head deltas (quantised to 1/256, which keeps the fixture small) with the extreme pattern, scaled by the
    weights, written over seeded (roi, class) pairs."""
    d = (np.round(rs.standard_normal((R, 4 * n_cls)) * 0.1 * 256) / 256).astype(np.float32)
    rows = extreme_rows(1, nan)
    pairs = rs.permutation(R * n_cls)[:len(rows)]
    w = np.asarray(weights, np.float32)
    for pr, row in zip(pairs, rows):
        for c, v in enumerate(row):
            if v is not None:
                d.reshape(-1, 4)[pr, c] = np.float32(v * w[c]) if np.isfinite(v) else v
    return d


def bbox_transform(ns, arrs):
    rs = synth.rng(17, 10)
    n, K = 48, 4
    boxes = synth.make_rois(rs, n, im_h=300, im_w=400, min_side=1, max_side=300)
    boxes[:4] = [[0, 0, 0, 299], [399, 0, 399, 0], [0, 150, 399, 150], [200, 299, 200, 299]]   # lines and points
    deltas = head_deltas(rs, n, K, (10.0, 10.0, 5.0, 5.0))
    im_shape = np.array([300.0, 400.0], np.float32)
    pred = ns.boxes.bbox_transform(boxes, deltas, (10.0, 10.0, 5.0, 5.0))
    arrs.update(bt_boxes=boxes, bt_deltas=deltas, bt_im_shape=im_shape, bt_pred=pred,
                bt_pred_clipped=ns.boxes.clip_tiled_boxes(pred.copy(), im_shape))


def postprocess(ns, arrs):
    rs = synth.rng(17, 11)
    R, n_cls = 40, 81
    im_h, im_w, sf = 300.0, 400.0, np.float32(1.6)
    # original-image RoIs: ordinary boxes, and one-pixel lines / points on the four borders (+1 width convention: width 1)
    orig = synth.make_rois(rs, R, im_h=im_h, im_w=im_w, min_side=8, max_side=250)
    orig[:10] = [[0, 20, 0, 200], [399, 10, 399, 290], [30, 0, 350, 0], [5, 299, 395, 299], [0, 0, 0, 0],
                 [399, 299, 399, 299], [399, 0, 399, 0], [0, 299, 0, 299], [120, 0, 120, 0], [0, 140, 0, 140]]
    rois = (orig * sf).astype(np.float32)
    # ~12 confident classes per RoI, so > 100 detections survive NMS and the limit runs
    lg = (rs.standard_normal((R, n_cls)) * 0.3 - 3.0).astype(np.float32)
    for i in range(R):
        if i < 16:          # the RoIs collapsed below: classes 1..9 a little above the other confident ones, so they reach the limit
            lg[i, 1:10] += 7.0
            lg[i, 10 + rs.permutation(n_cls - 10)[:3]] += 6.0
        else:
            lg[i, 1 + rs.permutation(n_cls - 1)[:12]] += 6.0
    for _ in range(64):
        cls = orc.softmax_rows(lg)
        fg = cls[:, 1:]
        if all(np.unique(fg[:, j]).size == R for j in range(n_cls - 1)) and np.unique(fg[fg > 0.05]).size == (fg > 0.05).sum():
            break
        lg += (rs.standard_normal(lg.shape) * 1e-3).astype(np.float32)
    else:
        raise RuntimeError("could not draw tie-free class scores")
    deltas = head_deltas(rs, R, n_cls, (10.0, 10.0, 5.0, 5.0))
    # collapse: in classes 1..6 the first 16 RoIs get dx = dy = +inf (the bottom-right corner point, IoU 1 with each other),
    # in classes 7..9 dx = -inf with dh at the clamp (left-border lines)
    for j in range(1, 7):
        deltas[:16, 4 * j:4 * j + 2] = np.inf
    for j in range(7, 10):
        deltas[:16, 4 * j] = -np.inf
        deltas[:16, 4 * j + 3] = CLIP * F32(5)
    im_size = np.array([im_h, im_w, 3.0], np.float32)
    sc, bx, cb = ns.result_utils.postprocess_output(torch.from_numpy(rois), float(sf), torch.from_numpy(im_size),
                                                    torch.from_numpy(cls), torch.from_numpy(deltas))
    arrs.update(pp_rois=rois, pp_logits=lg, pp_cls=cls, pp_deltas=deltas, pp_im_size=im_size, pp_sf=np.array([sf], np.float32))
    arrs["pp_scores"], arrs["pp_boxes"] = np.asarray(sc, np.float32), np.asarray(bx, np.float32)
    arrs["pp_cls_id"] = np.concatenate([np.full(len(cb[j]), j, np.int32) for j in range(1, n_cls)])
    boxes = (torch.from_numpy(rois) / float(sf)).numpy()
    pred_c = ns.boxes.clip_tiled_boxes(ns.boxes.bbox_transform(boxes, deltas, (10.0, 10.0, 5.0, 5.0)), im_size)
    # the reference's box_voting has no result for a box of zero width or height (exp(dw) underflowed): it does not overlap
    # itself, nothing votes and np.average raises ZeroDivisionError.  Those (roi, class) pairs leave the Soft-NMS + vote run.
    wh = np.minimum(pred_c[:, 2::4] - pred_c[:, 0::4], pred_c[:, 3::4] - pred_c[:, 1::4]) + 1
    drop = np.flatnonzero((wh <= 0).reshape(-1)).astype(np.int32)
    arrs["pp_soft_vote_drop"] = drop
    cls = cls.copy()
    cls.reshape(-1)[drop] = 0.0
    sc, bx, cb = ns.result_utils.box_results_with_nms_and_limit(cls, pred_c.copy(), do_soft_nms=True, soft_nms_method="linear",
                                                                do_bbox_vote=True, bbox_vote_thresh=0.8)
    arrs["pp_soft_vote_scores"], arrs["pp_soft_vote_boxes"] = np.asarray(sc, np.float32), np.asarray(bx, np.float32)
    arrs["pp_soft_vote_cls_id"] = np.concatenate([np.full(len(cb[j]), j, np.int32) for j in range(1, n_cls)])
    print("postprocess: %d detections, %d soft-NMS + vote" % (arrs["pp_scores"].size, arrs["pp_soft_vote_scores"].size))


def main():
    ns = rh.load_reference()
    torch.manual_seed(0)
    arrs = {}
    rpn(ns, arrs)
    bbox_transform(ns, arrs)
    with np.errstate(invalid="ignore", over="ignore"):
        postprocess(ns, arrs)
    path = os.path.join(HERE, "decode_extremes.npz")
    np.savez_compressed(path, **arrs)
    print("%-28s %7.1f KB  %d arrays" % ("decode_extremes", os.path.getsize(path) / 1024.0, len(arrs)))


if __name__ == "__main__":
    main()
