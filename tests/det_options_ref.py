"""The checker of the detection post-processing options (test support, not a test module): box_results_with_nms_and_limit
(lib/utils/result_utils.py:96-168) composed per image from the oracle's pinned pieces -- oracle.nms / oracle.soft_nms per class,
then oracle.box_voting, then the max_det limit and the class-major vstack.  tests/test_det_options_host.py pins this composition
against the reference's own outputs (tests/golden/postprocess_soft_vote.npz); the GPU tests compare the device path with it."""
import numpy as np

# the configurations of make_det_options_golden.py: name -> (nms method, vote threshold or None)
CONFIGS = {
    "soft_linear": ("linear", None),
    "soft_gaussian": ("gaussian", None),
    "soft_hard": ("hard", None),
    "soft_linear_vote": ("linear", 0.8),
    "hard_vote06": ("nms", 0.6),
}


def kwargs_of(method, vote_thresh):
    """(method, vote threshold) -> the keyword arguments of box_results_with_nms_and_limit / hip.postprocess_detections"""
    kw = {}
    if method != "nms":
        kw.update(do_soft_nms=True, soft_nms_method=method, soft_nms_sigma=0.5)
    if vote_thresh is not None:
        kw.update(do_bbox_vote=True, bbox_vote_thresh=vote_thresh)
    return kw


def compose(orc, scores, boxes, method="nms", vote_thresh=None, score_thresh=0.05, nms_thresh=0.5, max_det=100, sigma=0.5):
    """scores [R, C], decoded + clipped boxes [R, 4C] of ONE image -> (dets [D, 6] = (x1, y1, x2, y2, score, class), roi [D])."""
    scores, boxes = np.asarray(scores, np.float32), np.asarray(boxes, np.float32)
    ncls = scores.shape[1]
    per_cls = []
    for j in range(1, ncls):
        inds = np.where(scores[:, j] > np.float32(score_thresh))[0]                           # :127
        dj = np.hstack((boxes[inds, j * 4:(j + 1) * 4], scores[inds, j][:, None])).astype(np.float32)
        if len(inds) == 0:
            nd, src = dj, inds
        elif method == "nms":
            keep = orc.nms(dj, nms_thresh)                                                      # :142
            nd, src = dj[keep], inds[keep]
        else:
            nd, k = orc.soft_nms(dj, sigma, nms_thresh, 0.0001, method)                         # :133-140
            src = inds[k]
        if vote_thresh is not None and len(nd):
            nd = orc.box_voting(nd, dj, vote_thresh)                                            # :145-151, 'ID'
        per_cls.append((nd, src))
    if max_det > 0:                                                                             # :154-163
        image_scores = np.concatenate([nd[:, 4] for nd, _ in per_cls])
        if len(image_scores) > max_det:
            th = np.sort(image_scores)[-max_det]
            per_cls = [(nd[nd[:, 4] >= th], src[nd[:, 4] >= th]) for nd, src in per_cls]
    dets = np.vstack([np.hstack([nd[:, :5], np.full((len(nd), 1), j + 1, np.float32)]) for j, (nd, _) in enumerate(per_cls)])
    roi = np.concatenate([src for _, src in per_cls]).astype(np.int32)
    return dets.astype(np.float32), roi


def decode(orc, rois, sf, im_size, deltas, weights=(10.0, 10.0, 5.0, 5.0)):
    """postprocess_output's decode (result_utils.py:76-84): rois [R, 4] at network scale -> clipped boxes [R, 4C]"""
    boxes = (np.asarray(rois, np.float32) / np.float32(sf)).astype(np.float32)
    return orc.clip_tiled_boxes(orc.bbox_transform(boxes, deltas, weights), im_size[0], im_size[1])
