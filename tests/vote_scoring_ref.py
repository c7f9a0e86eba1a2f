"""The checker of the bbox-vote scorings (test support, not a test module): box_voting(top, all, thresh, scoring_method, beta)
(lib/utils/boxes.py:280-329) from the oracle's pinned pieces -- oracle.box_voting for the boxes, oracle.bbox_overlaps for the
voter sets -- and the scorings in numpy float32 as the reference writes them; box_results_with_nms_and_limit with a scoring
(lib/utils/result_utils.py:96-168) is det_options_ref.compose with that vote: NMS / Soft-NMS per class, the vote, the max_det
limit on the VOTED scores, the class-major vstack.  tests/test_vote_scoring_host.py pins it against the reference's own outputs
(tests/golden/postprocess_vote_scoring.npz)."""
import numpy as np

import det_options_ref

METHODS = ("TEMP_AVG", "AVG", "IOU_AVG", "GENERALIZED_AVG", "QUASI_SUM")
NMS_METHODS = ("nms", "linear", "gaussian")
THRESHOLDS = (0.8, 0.6)
CASES = ("pp", "crowd", "dense")


def exact(method, beta=1.0):
    """True where the device score is bit-exact to the reference; else within 1e-6 relative (log / exp / pow)."""
    return method in ("ID", "AVG", "IOU_AVG", "QUASI_SUM") or (method == "GENERALIZED_AVG" and beta == 1.0)


def score(ws, iou, method, beta=1.0):
    """boxes.py:297-323 for one top det: ws the voters' scores, iou their overlaps with it (float32 arrays)."""
    if method == "TEMP_AVG":
        P = np.vstack((ws, 1.0 - ws))
        X = np.log(P / np.max(P, axis=0))
        X_exp = np.exp(X / beta)
        return (X_exp / np.sum(X_exp, axis=0))[0].mean()
    if method == "AVG":
        return ws.mean()
    if method == "IOU_AVG":
        return np.average(ws, weights=iou)
    if method == "GENERALIZED_AVG":
        return np.mean(ws ** beta) ** (1.0 / beta)
    if method == "QUASI_SUM":
        return ws.sum() / float(len(ws)) ** beta
    raise NotImplementedError("Unknown scoring method {}".format(method))


def box_voting(orc, top, alld, thresh, method="ID", beta=1.0):
    """[T,5], [A,5] -> [T,5]: the voted boxes (oracle.box_voting) and, for a scoring other than 'ID', the voted scores."""
    top, alld = np.asarray(top, np.float32), np.asarray(alld, np.float32)
    out = orc.box_voting(top, alld, thresh)
    if method == "ID":
        return out
    ov = orc.bbox_overlaps(top[:, :4], alld[:, :4])
    for k in range(len(top)):
        sel = np.where(ov[k] >= thresh)[0]
        out[k, 4] = score(alld[sel, 4], ov[k, sel], method, beta)
    return out


class _Scored:
    """the oracle with its box_voting replaced by the scored one (what det_options_ref.compose calls)"""

    def __init__(self, orc, method, beta):
        self._orc, self._method, self._beta = orc, method, beta

    def __getattr__(self, name):
        return getattr(self._orc, name)

    def box_voting(self, top, alld, thresh):
        return box_voting(self._orc, top, alld, thresh, self._method, self._beta)


def compose(orc, scores, boxes, method="nms", vote_thresh=0.8, vote_method="ID", beta=1.0, **kw):
    """box_results_with_nms_and_limit(do_bbox_vote=True, bbox_vote_method=vote_method) for ONE image -> (dets [D,6], roi [D])"""
    return det_options_ref.compose(_Scored(orc, vote_method, beta), scores, boxes, method, vote_thresh, **kw)


def kwargs_of(method, vote_thresh, vote_method):
    """keyword arguments of box_results_with_nms_and_limit / hip.postprocess_detections"""
    kw = det_options_ref.kwargs_of(method, vote_thresh)
    kw["bbox_vote_method"] = vote_method
    return kw


def dense_inputs():
    """Seeded dense case: scores [2400, 3], clipped boxes [2400, 12].  Class 1: clusters of 300, 700 and 1100 jittered copies of
    one box each; class 2: one cluster of 1200 plus scattered boxes -- voter counts across numpy's 8- and 128-element pairwise
    boundaries, up to over a thousand."""
    rs = np.random.RandomState(20261017)
    R, im_h, im_w = 2400, 800.0, 1200.0

    def cluster(n, cx, cy, half, jit):
        c = np.array([[cx, cy]]) + rs.uniform(-1, 1, (n, 2)) * rs.uniform(0.5, jit, (n, 1))
        h = np.maximum(half + rs.uniform(-jit, jit, (n, 2)), 8.0)
        return np.hstack([c - h, c + h - 1])

    b1 = np.vstack([cluster(300, 200, 200, 50, 6), cluster(700, 600, 300, 70, 10), cluster(1100, 900, 600, 90, 14),
                    cluster(300, 300, 600, 30, 30)])
    b2 = np.vstack([cluster(1200, 500, 450, 80, 12), cluster(1200, 600, 400, 120, 200)])
    for b in (b1, b2):
        b[:, 0::2] = np.clip(b[:, 0::2], 0, im_w - 1)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, im_h - 1)
    s1 = rs.uniform(0.06, 0.95, R)
    s2 = np.where(rs.uniform(0, 1, R) < 0.7, rs.uniform(0.06, 0.9, R), rs.uniform(0, 0.05, R))
    boxes = np.hstack([np.zeros((R, 4)), b1, b2[rs.permutation(R)]]).astype(np.float32)
    scores = np.stack([np.clip(1.0 - np.maximum(s1, s2), 0, 1), s1, s2], 1).astype(np.float32)
    return scores, boxes
