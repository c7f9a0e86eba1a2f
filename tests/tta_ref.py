"""Test-time augmentation restated in numpy (test support, not a test module; tests/README_tta.md): the merge of the views' box-head
outputs and the combination of their mask probabilities, as Detectron's core/test.py has them (im_detect_bbox_aug with
im_detect_bbox_hflip / im_detect_bbox_scale, im_detect_mask_aug with its flipped and scaled forms).  The reference has no test-time
augmentation, and Detectron is not on hand: this file IS the rule, written as Detectron writes it on float32 arrays; parity with
Detectron itself is unpinned.  What is pinned: the per-view decode equals oracle/'s (tests/test_tta_host.py), which is pinned to
the reference.

float32 throughout, one rounding per numpy operation, with the project's one convention on transcendental functions: exp and log
are evaluated in float64 and rounded once (oracle.py:rpn_sigmoid says why), where Detectron calls numpy's float32 routines.
combine_masks(..., exact=False) is LOGIT_AVG with numpy's own float32 log / exp, the form Detectron literally runs, and
combine_masks64 the same rule in float64 throughout: the GPU test takes its tolerance from the distance between those two."""
import numpy as np

f32 = np.float32
BBOX_XFORM_CLIP = np.log(1000. / 16.)
BOX_HEURS = ("UNION", "AVG", "ID")
MASK_HEURS = ("SOFT_AVG", "SOFT_MAX", "LOGIT_AVG")


def _exp(x):
    return np.exp(x.astype(np.float64)).astype(f32)


def bbox_transform(boxes, deltas, weights=(10.0, 10.0, 5.0, 5.0)):
    """box_utils.bbox_transform on float32 arrays: boxes [R,4], deltas [R,4C] -> [R,4C]"""
    boxes, deltas = np.asarray(boxes, f32), np.asarray(deltas, f32)
    if boxes.shape[0] == 0:
        return np.zeros((0, deltas.shape[1]), dtype=deltas.dtype)
    widths = boxes[:, 2] - boxes[:, 0] + f32(1.0)
    heights = boxes[:, 3] - boxes[:, 1] + f32(1.0)
    ctr_x = boxes[:, 0] + f32(0.5) * widths
    ctr_y = boxes[:, 1] + f32(0.5) * heights
    wx, wy, ww, wh = (f32(w) for w in weights)
    dx, dy = deltas[:, 0::4] / wx, deltas[:, 1::4] / wy
    dw, dh = deltas[:, 2::4] / ww, deltas[:, 3::4] / wh
    dw, dh = np.minimum(dw, f32(BBOX_XFORM_CLIP)), np.minimum(dh, f32(BBOX_XFORM_CLIP))
    pred_ctr_x = dx * widths[:, np.newaxis] + ctr_x[:, np.newaxis]
    pred_ctr_y = dy * heights[:, np.newaxis] + ctr_y[:, np.newaxis]
    pred_w = _exp(dw) * widths[:, np.newaxis]
    pred_h = _exp(dh) * heights[:, np.newaxis]
    out = np.zeros(deltas.shape, dtype=f32)
    out[:, 0::4] = pred_ctr_x - f32(0.5) * pred_w
    out[:, 1::4] = pred_ctr_y - f32(0.5) * pred_h
    out[:, 2::4] = pred_ctr_x + f32(0.5) * pred_w - f32(1)
    out[:, 3::4] = pred_ctr_y + f32(0.5) * pred_h - f32(1)
    return out


def clip_tiled_boxes(boxes, im_h, im_w):
    boxes = boxes.copy()
    boxes[:, 0::4] = np.maximum(np.minimum(boxes[:, 0::4], f32(im_w) - f32(1)), f32(0))
    boxes[:, 1::4] = np.maximum(np.minimum(boxes[:, 1::4], f32(im_h) - f32(1)), f32(0))
    boxes[:, 2::4] = np.maximum(np.minimum(boxes[:, 2::4], f32(im_w) - f32(1)), f32(0))
    boxes[:, 3::4] = np.maximum(np.minimum(boxes[:, 3::4], f32(im_h) - f32(1)), f32(0))
    return boxes


def flip_boxes(boxes, im_width):
    """box_utils.flip_boxes: x1' = w - x2 - 1, x2' = w - x1 - 1, on every class's box"""
    out = boxes.copy()
    out[:, 0::4] = f32(im_width) - boxes[:, 2::4] - f32(1)
    out[:, 2::4] = f32(im_width) - boxes[:, 0::4] - f32(1)
    return out


def softmax_rows(logits):
    """oracle.softmax_rows: exp and the sum in float64, the sum by slot j % 64 and a halving tree, one rounding"""
    l = np.asarray(logits, f32)
    m = l.max(axis=-1, keepdims=True).astype(np.float64)
    e = np.exp(l.astype(np.float64) - m)
    s = np.zeros(l.shape[:-1] + (64,), np.float64)
    for j in range(l.shape[-1]):
        s[..., j % 64] += e[..., j]
    for off in (32, 16, 8, 4, 2, 1):
        s = s[..., :off] + s[..., off:2 * off]
    return (e / s).astype(f32)


def view_boxes(rois, scale, im_size, deltas, flipped, weights=(10.0, 10.0, 5.0, 5.0)):
    """One view of one image (im_detect_bbox + im_detect_bbox_hflip's inversion): rois [n,4] in the view's coordinates -> decoded
    boxes [n,4C] in original-image coordinates"""
    boxes = (np.asarray(rois, f32) / f32(scale)).astype(f32)
    pred = clip_tiled_boxes(bbox_transform(boxes, deltas, weights), im_size[0], im_size[1])
    return flip_boxes(pred, im_size[1]) if flipped else pred


def merge_boxes(views, im_size, score_heur="UNION", coord_heur="UNION", logits=False, weights=(10.0, 10.0, 5.0, 5.0)):
    """views: dicts of rois5 [B,R,5], n_rois [B], cls_score [B,R,C], bbox_pred [B,R,4C], scale [B], flipped.  -> dict of out_scores
    [B,rows,C], out_boxes [B,rows,4C], out_n [B], out_src [B,rows] with rows = T R under UNION and R otherwise; padding rows zeros, -1."""
    assert score_heur in BOX_HEURS and coord_heur in BOX_HEURS
    assert (score_heur == "UNION") == (coord_heur == "UNION"), "Coord and score heuristics must both be UNION or neither"
    T = len(views)
    B, R, C = views[0]["cls_score"].shape
    rows = T * R if score_heur == "UNION" else R
    out = dict(out_scores=np.zeros((B, rows, C), f32), out_boxes=np.zeros((B, rows, 4 * C), f32), out_n=np.zeros(B, np.int32),
               out_src=np.full((B, rows), -1, np.int32))
    for b in range(B):
        scores_ts, boxes_ts, src_ts = [], [], []
        for t, v in enumerate(views):
            n = int(v["n_rois"][b])
            s = np.asarray(v["cls_score"][b, :n], f32)
            scores_ts.append(softmax_rows(s) if logits and n else s)
            boxes_ts.append(view_boxes(v["rois5"][b, :n, 1:], v["scale"][b], im_size[b], v["bbox_pred"][b, :n], v["flipped"], weights))
            src_ts.append(t * R + np.arange(n, dtype=np.int32))

        def one(heur, xs):
            if heur == "ID":
                return xs[-1]
            if heur == "AVG":
                return np.mean(xs, axis=0)                            # float32 in, float32 out: the sum in view order, one division
            return np.vstack(xs)
        sc, bx = one(score_heur, scores_ts), one(coord_heur, boxes_ts)
        assert sc.dtype == f32 and bx.dtype == f32
        src = np.concatenate(src_ts) if score_heur == "UNION" else src_ts[-1] if score_heur == "ID" else src_ts[0]
        n = sc.shape[0]
        assert bx.shape[0] == n
        out["out_scores"][b, :n], out["out_boxes"][b, :n], out["out_n"][b], out["out_src"][b, :n] = sc, bx, n, src
    return out


def logit(y, exact=True):
    """im_detect_mask_aug's logit: -1.0 * np.log((1.0 - y) / np.maximum(y, 1e-20)) on float32"""
    q = (f32(1.0) - y) / np.maximum(y, f32(1e-20))
    with np.errstate(divide="ignore"):
        return -(np.log(q.astype(np.float64)).astype(f32) if exact else np.log(q))


def combine_masks(masks, flipped, det_count, mask_class=None, heur="SOFT_AVG", exact=True):
    """masks: T arrays float32 [B*D,K,M,M]; flipped: T flags; det_count [B]; mask_class [B*D] or None.  -> [B*D,K,M,M]: rows past
    det_count zeros; with mask_class only that channel of a row is combined.  exact=False: numpy's float32 log and exp."""
    assert heur in MASK_HEURS
    ms = [np.asarray(m, f32)[:, :, :, ::-1] if f else np.asarray(m, f32) for m, f in zip(masks, flipped)]     # masks_hf[:, :, :, ::-1]
    if heur == "SOFT_AVG":
        c = np.mean(ms, axis=0)
    elif heur == "SOFT_MAX":
        c = np.amax(ms, axis=0)
    else:
        mean = np.mean([logit(y, exact) for y in ms], axis=0)
        e = np.exp((-mean).astype(np.float64)).astype(f32) if exact else np.exp(-mean)
        c = f32(1.0) / (f32(1.0) + e)
    assert c.dtype == f32
    return _live(c, det_count, mask_class)


def combine_masks64(masks, flipped, det_count, mask_class=None):
    """LOGIT_AVG in float64 throughout (the float32 inputs widened exactly)"""
    ms = [np.asarray(m, f32).astype(np.float64)[:, :, :, ::-1] if f else np.asarray(m, f32).astype(np.float64) for m, f in zip(masks, flipped)]
    with np.errstate(divide="ignore"):
        mean = np.mean([-1.0 * np.log((1.0 - y) / np.maximum(y, 1e-20)) for y in ms], axis=0)
    return _live(1.0 / (1.0 + np.exp(-mean)), det_count, mask_class)


def _live(c, det_count, mask_class):
    N, K = c.shape[:2]
    B = len(det_count)
    D = N // B
    keep = np.zeros((N, K), bool)
    for b in range(B):
        n = min(max(int(det_count[b]), 0), D)
        keep[b * D:b * D + n] = True
    if mask_class is not None:
        keep &= np.arange(K)[None, :] == np.asarray(mask_class)[:, None]
    return np.where(keep[:, :, None, None], c, c.dtype.type(0))
