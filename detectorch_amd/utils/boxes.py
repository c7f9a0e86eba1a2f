"""Box utilities -- the subset of the reference's lib/utils/boxes.py that sits on the region-proposal hot path, with the
same names and numpy-in / numpy-out conventions, computed by the HIP kernels (detectorch_amd/csrc).

    nms              boxes.py:332-336   -> dtc_nms            (cython_nms.pyx:37-87)
    soft_nms         boxes.py:339-356   -> dtc_soft_nms       (cython_nms.pyx:98-203)
    bbox_transform   boxes.py:168-208   -> dtc_bbox_transform
    bbox_overlaps    boxes.py:53-69 (cython_bbox.pyx:32-72) -> dtc_bbox_overlaps
    box_voting       boxes.py:280-329   -> dtc_box_voting (+ host statistics for the non-'ID' scoring methods)
    clip_tiled_boxes boxes.py:150-165
    expand_boxes     boxes.py:245-261 ; boxes_area boxes.py:75-81  (trivial host numpy, identical arithmetic)
    flip_boxes       boxes.py:264-269   -> dtc_flip_boxes     (the side library of hip_flip.py)

There is no CPU fallback for the kernels: without the GPU library these raise.
"""
import numpy as np
import torch

from .. import hip, hip_flip

cfg_BBOX_XFORM_CLIP = 4.135166556742356   # boxes.py:73


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("detectorch_amd.utils.boxes needs the MI355X HIP path (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def nms(dets, thresh, tie_break='index_asc'):
    """Apply classic DPM-style greedy NMS (boxes.py:332).  dets: ndarray [N,5] -> ndarray int64 of kept indices.

    tie_break: visiting order of boxes with EQUAL scores.  The reference visits `scores.argsort()[::-1]`
    (cython_nms.pyx:45): the reverse of an ascending argsort, i.e. equal scores in DESCENDING index order whenever numpy's
    sort happens to be stable (it is unspecified for the default kind).  'index_asc' (default) is this library's canonical
    rule everywhere (score desc, index asc); 'index_desc' reproduces the stable-argsort reading of the reference -- done on
    the host by running the same kernel on the row-reversed array and mapping the kept indices back."""
    if dets.shape[0] == 0:
        return []                                              # boxes.py:334-335
    assert tie_break in ('index_asc', 'index_desc')
    a = np.ascontiguousarray(dets, dtype=np.float32)
    if tie_break == 'index_desc':
        a = np.ascontiguousarray(a[::-1])
    keep = hip.nms(torch.from_numpy(a).to(_dev()), thresh).cpu().numpy()
    if tie_break == 'index_desc':
        keep = np.sort(a.shape[0] - 1 - keep)
    return keep


def soft_nms(dets, sigma=0.5, overlap_thresh=0.3, score_thresh=0.001, method='linear'):
    """Apply the soft NMS algorithm (boxes.py:339-356) -> (dets', keep)."""
    if dets.shape[0] == 0:
        return dets, []
    methods = {'hard': 0, 'linear': 1, 'gaussian': 2}
    assert method in methods, 'Unknown soft_nms method: {}'.format(method)
    d = torch.from_numpy(np.ascontiguousarray(dets, dtype=np.float32)).to(_dev())
    out, keep = hip.soft_nms(d, np.float32(sigma), np.float32(overlap_thresh), np.float32(score_thresh), methods[method])
    return out.cpu().numpy(), keep.cpu().numpy()


def bbox_transform(boxes, deltas, weights=(1.0, 1.0, 1.0, 1.0)):
    """Forward transform boxes + regression deltas -> predicted boxes (boxes.py:168-208)."""
    if boxes.shape[0] == 0:
        return np.zeros((0, deltas.shape[1]), dtype=deltas.dtype)
    dev = _dev()
    b = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float32)).to(dev)
    d = torch.from_numpy(np.ascontiguousarray(deltas, dtype=np.float32)).to(dev)
    return hip.bbox_transform(b, d, weights).cpu().numpy()


def clip_tiled_boxes(boxes, im_shape):
    """Clip boxes to image boundaries (boxes.py:150-165); exact min/max, done in place on the host array like the reference."""
    assert boxes.shape[1] % 4 == 0
    boxes[:, 0::4] = np.maximum(np.minimum(boxes[:, 0::4], im_shape[1] - 1), 0)
    boxes[:, 1::4] = np.maximum(np.minimum(boxes[:, 1::4], im_shape[0] - 1), 0)
    boxes[:, 2::4] = np.maximum(np.minimum(boxes[:, 2::4], im_shape[1] - 1), 0)
    boxes[:, 3::4] = np.maximum(np.minimum(boxes[:, 3::4], im_shape[0] - 1), 0)
    return boxes


def boxes_area(boxes):
    w = (boxes[:, 2] - boxes[:, 0] + 1)
    h = (boxes[:, 3] - boxes[:, 1] + 1)
    areas = w * h
    assert np.all(areas >= 0), 'Negative areas founds'
    return areas


def expand_boxes(boxes, scale):
    w_half = (boxes[:, 2] - boxes[:, 0]) * .5
    h_half = (boxes[:, 3] - boxes[:, 1]) * .5
    x_c = (boxes[:, 2] + boxes[:, 0]) * .5
    y_c = (boxes[:, 3] + boxes[:, 1]) * .5
    w_half *= scale
    h_half *= scale
    boxes_exp = np.zeros(boxes.shape)
    boxes_exp[:, 0] = x_c - w_half
    boxes_exp[:, 2] = x_c + w_half
    boxes_exp[:, 1] = y_c - h_half
    boxes_exp[:, 3] = y_c + h_half
    return boxes_exp


def flip_boxes(boxes, im_width):
    """Flip boxes horizontally (boxes.py:264-269): boxes [n, 4k] -> float32 [n, 4k] with x1' = im_width - x2 - 1 and x2' = im_width -
    x1 - 1 in every group of four columns, in float32 as numpy evaluates it for float32 boxes."""
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    assert b.ndim == 2 and b.shape[1] % 4 == 0 and b.shape[1] > 0
    if b.shape[0] == 0:
        return b.copy()
    dev = _dev()
    out = hip_flip.flip_boxes(torch.from_numpy(b).to(dev).unsqueeze(0), torch.tensor([int(im_width)], dtype=torch.int32, device=dev), [1])
    return out[0].cpu().numpy()


def bbox_overlaps(boxes, query_boxes):
    """IoU matrix [N,K] float32 of boxes [N,4] vs query_boxes [K,4] (cython_bbox.bbox_overlaps, cython_bbox.pyx:32-72)."""
    b = np.ascontiguousarray(boxes, dtype=np.float32)
    q = np.ascontiguousarray(query_boxes, dtype=np.float32)
    if b.shape[0] == 0 or q.shape[0] == 0:
        return np.zeros((b.shape[0], q.shape[0]), dtype=np.float32)
    dev = _dev()
    return hip.bbox_overlaps(torch.from_numpy(b).to(dev), torch.from_numpy(q).to(dev)).cpu().numpy()


def box_voting(top_dets, all_dets, thresh, scoring_method='ID', beta=1.0):
    """Bounding-box voting (boxes.py:280-329): every row of top_dets [N,5] gets its box replaced by the score-weighted
    mean of the all_dets [M,5] that overlap it by IoU >= thresh; scoring_method other than 'ID' also rewrites the score
    column from the voters' scores.  One device call for every method (dtc_box_voting_scored, M <= 8192)."""
    hip.vote_scoring(scoring_method, beta)            # NotImplementedError for an unknown method (boxes.py:324-327)
    top = np.ascontiguousarray(top_dets, dtype=np.float32)
    alld = np.ascontiguousarray(all_dets, dtype=np.float32)
    if top.shape[0] == 0:
        return top.copy()
    dev = _dev()
    t_top, t_all = torch.from_numpy(top).to(dev), torch.from_numpy(alld).to(dev)
    voted, n_voters = hip.box_voting(t_top, t_all, np.float32(thresh), scoring_method, beta)
    if int(n_voters.min().item()) == 0:
        raise ZeroDivisionError("Weights sum to zero, can't be normalized")                 # what np.average raises at :295
    return voted.cpu().numpy()


def xyxy_to_xywh(xyxy):
    """lib/utils/boxes.py:110-123: [x1 y1 x2 y2] -> [x1 y1 w h] (w = x2 - x1 + 1)."""
    if isinstance(xyxy, (list, tuple)):
        assert len(xyxy) == 4
        x1, y1 = xyxy[0], xyxy[1]
        return (x1, y1, xyxy[2] - x1 + 1, xyxy[3] - y1 + 1)
    if isinstance(xyxy, np.ndarray):
        return np.hstack((xyxy[:, 0:2], xyxy[:, 2:4] - xyxy[:, 0:2] + 1))
    raise TypeError('Argument xyxy must be a list, tuple, or numpy array.')
