"""The checker of the Fast R-CNN training minibatch (test support, not a test module): the reference's host chain restated in
numpy, one image at a time, with the seeded CASES both the golden generator and the tests use.

    merge     lib/data/json_dataset.py:333-394   _merge_proposal_boxes_into_roidb
    crowd     lib/data/json_dataset.py:397-414   _filter_crowd_proposals (pycocotools bbIou, restated from its published C:
                                                 common/maskApi.c -- pycocotools itself is not available: parity unpinned)
    assign    lib/data/json_dataset.py:417-435   _add_class_assignments
    targets   lib/data/roidb.py:176-206          _compute_targets, lib/utils/boxes.py:211-242 bbox_transform_inv
    sample    lib/utils/fast_rcnn_sample_rois.py:41-137, expansion :139-163

tests/test_train_targets_host.py pins it against the reference's own functions (tests/golden/train_targets.npz, made by
tests/golden/make_train_targets_golden.py); the GPU tests compare dtc_fast_rcnn_targets with it and with the golden.
The sampling order is explicit: npr.choice(a, size, replace=False) is a[np.lexsort((a, keys[a]))][:size].
"""
import numpy as np

DEFAULTS = dict(rois_per_image=512, fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0, bbox_thresh=0.5,
                crowd_thresh=0.7, reg_weights=(10.0, 10.0, 5.0, 5.0), num_classes=81, cls_agnostic_bbox_reg=False)

# name -> (seed, G, crowd gt among them, P, im_scale, parameter overrides); "d" and "e" are hand-made (make_case)
CASES = {
    "a": (0, 5, 1, 300, 1.6, dict(rois_per_image=64)),                       # basic
    "b": (1, 3, 0, 20, 800.0 / 427.0, dict(rois_per_image=64)),              # fewer fg than the quota, fewer bg than the rest
    "c": (2, 0, 0, 50, 1.25, dict(rois_per_image=32)),                       # no gt
    "d": (3, 1, 1, 30, 2.0, dict(rois_per_image=16)),                        # crowd gt only
    "e": (4, 3, 0, 14, 1.0, dict(rois_per_image=8)),                         # ties
    "f": (5, 6, 1, 300, 1333.0 / 1000.0, dict(rois_per_image=64, fg_thresh=0.6, bg_thresh_hi=0.4, bg_thresh_lo=0.1,
                                              bbox_thresh=0.3)),
    "g": (6, 16, 2, 2000, 1.6, dict()),                                      # the reference defaults
    "h": (7, 256, 4, 2048, 1.5, dict()),                                     # the entry's limits (restatement only)
    "i": (8, 5, 1, 120, 1.6, dict(rois_per_image=32, cls_agnostic_bbox_reg=True)),
}
GOLDEN_CASES = tuple(c for c in sorted(CASES) if c != "h")
EXPANDED_CASES = tuple(c for c in GOLDEN_CASES if c != "g")                  # the golden stores the 4K-wide blobs for small R only
IM_H, IM_W = 480, 640


def params_of(name):
    return dict(DEFAULTS, **CASES[name][5])


def _boxes(rs, n, min_size, max_w, max_h):
    x1 = rs.uniform(0, IM_W - min_size - 1, n)
    y1 = rs.uniform(0, IM_H - min_size - 1, n)
    w = rs.uniform(min_size, max_w, n)
    h = rs.uniform(min_size, max_h, n)
    return np.stack([x1, y1, np.minimum(x1 + w, IM_W - 1), np.minimum(y1 + h, IM_H - 1)], 1).astype(np.float32)


def make_case(name):
    """Seeded inputs of case `name`: dict(gt_boxes f32 [G,4], gt_classes i32 [G], is_crowd i32 [G], proposals f32 [P,4], im_scale
    (a Python float), rand_keys u32 [G+P]), original-image coordinates."""
    seed, G, n_crowd, P, im_scale, _ = CASES[name]
    rs = np.random.RandomState(20261018 + seed)
    keys = rs.randint(0, 2 ** 32, G + P, dtype=np.uint64).astype(np.uint32)
    if name == "d":            # one crowd gt inside a proposal of 5/3 its area: IoU = IoA = 0.6 -> fg label, not filtered, no targets
        gt = np.array([[100, 100, 299, 299]], np.float32)
        cls, crowd = np.array([17], np.int32), np.array([1], np.int32)
        prop = _boxes(rs, P, 8, 200, 200)
        prop[0] = [100, 100, 432, 299]
        prop[1] = [120, 120, 200, 180]                                       # inside the crowd region: filtered
        prop[2] = [90, 150, 250, 260]                                        # mostly inside: filtered
    elif name == "e":
        gt = np.array([[0, 0, 9, 9], [0, 0, 9, 9], [100, 100, 150, 160]], np.float32)
        cls, crowd = np.array([3, 7, 2], np.int32), np.zeros(3, np.int32)
        prop = _boxes(rs, P, 8, 100, 100) + np.float32(200)
        prop[0] = [0, 0, 9, 9]                                               # identical to two gt: the first one wins
        prop[1] = [0, 0, 9, 4]                                               # IoU exactly 0.5: on the >= / < boundary
        prop[2] = [0, 0, 4, 9]
        prop[3] = [100, 100, 150, 160]
        prop[4] = [0, 0, 9, 14]                                              # IoU 100 / 150 with both gt
        prop[5] = [0, 0, 9, 4]
        keys[:] = 7                                                          # equal keys: the index decides
        keys[-4:] = 3
    else:
        gt = _boxes(rs, G, 30, IM_W / 2.0, IM_H / 2.0)
        cls = rs.randint(1, 81, G).astype(np.int32)
        crowd = np.zeros(G, np.int32)
        if n_crowd:
            crowd[rs.choice(G, n_crowd, replace=False)] = 1
        prop = _boxes(rs, P, 4, IM_W / 2.0, IM_H / 2.0)
        if G:
            k = P // 2                                                       # jittered copies of gt: fg, near-fg and targets
            src = rs.randint(0, G, k)
            size = np.tile(gt[src, 2:] - gt[src, :2], 2)
            prop[:k] = gt[src] + (rs.uniform(-0.22, 0.22, (k, 4)) * size).astype(np.float32)
            prop[:k, 2:] = np.maximum(prop[:k, 2:], prop[:k, :2])
            if k > 8:
                prop[3] = gt[src[3]]                                         # exact copies of a gt
                prop[4] = gt[src[3]]
                keys[G + 5] = keys[G + 6] = keys[G + 7]                      # equal keys among likely-fg rows
            for j, ci in enumerate(np.where(crowd == 1)[0]):                 # small boxes inside each crowd region
                cb = gt[ci]
                for t in range(4):
                    fx, fy = rs.uniform(0.05, 0.5, 2)
                    w, h = (cb[2] - cb[0]) * 0.4, (cb[3] - cb[1]) * 0.4
                    x, y = cb[0] + fx * (cb[2] - cb[0]), cb[1] + fy * (cb[3] - cb[1])
                    prop[P - 1 - 4 * j - t] = [x, y, x + w, y + h]
    return dict(gt_boxes=np.ascontiguousarray(gt, np.float32), gt_classes=cls, is_crowd=crowd,
                proposals=np.ascontiguousarray(prop, np.float32), im_scale=float(im_scale), rand_keys=keys)


def bbox_overlaps(boxes, query):
    """cython_bbox.bbox_overlaps (lib/utils_cython/cython_bbox.pyx:32-74) in numpy: every `a - b + 1` is the float32 difference plus
    the C double 1.0, span products in double, rounded where the .pyx stores into a float32 variable (oracle/oracle.c has the
    derivation).  [N,4] x [K,4] -> [N,K] float32."""
    b = np.asarray(boxes, np.float32)[:, None, :]
    q = np.asarray(query, np.float32)[None, :, :]
    span = lambda hi, lo: (hi - lo).astype(np.float64) + 1.0
    box_area = (span(q[..., 2], q[..., 0]) * span(q[..., 3], q[..., 1])).astype(np.float32)                     # :54-57
    iw = span(np.minimum(b[..., 2], q[..., 2]), np.maximum(b[..., 0], q[..., 0])).astype(np.float32)           # :59-62
    ih = span(np.minimum(b[..., 3], q[..., 3]), np.maximum(b[..., 1], q[..., 1])).astype(np.float32)           # :64-67
    inter = iw * ih
    ua = (span(b[..., 2], b[..., 0]) * span(b[..., 3], b[..., 1]) + box_area.astype(np.float64) -
          inter.astype(np.float64)).astype(np.float32)                                                          # :69-73
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where((iw > 0) & (ih > 0), inter / ua, np.float32(0)).astype(np.float32)                      # :74


def xyxy_to_xywh(xyxy):
    """lib/utils/boxes.py:121 (float32 in, float32 out)"""
    return np.hstack((xyxy[:, 0:2], xyxy[:, 2:4] - xyxy[:, 0:2] + 1))


def bb_iou_crowd(dt, gt):
    """pycocotools' bbIou (common/maskApi.c) with every gt iscrowd, as COCOmask.iou(dt, gt, [1] * len(gt)) calls it: (x, y, w, h)
    boxes converted to double, intersection over the area of dt.  [m,4] x [n,4] -> [m,n] float64."""
    d = np.asarray(dt, np.float64)[:, None, :]
    g = np.asarray(gt, np.float64)[None, :, :]
    w = np.minimum(d[..., 2] + d[..., 0], g[..., 2] + g[..., 0]) - np.maximum(d[..., 0], g[..., 0])
    h = np.minimum(d[..., 3] + d[..., 1], g[..., 3] + g[..., 1]) - np.maximum(d[..., 1], g[..., 1])
    return np.where((w > 0) & (h > 0), (w * h) / (d[..., 2] * d[..., 3]), 0.0)


def choose(inds, size, keys):
    """the explicit npr.choice(inds, size, replace=False): ascending (key, index)"""
    return inds[np.lexsort((inds, keys[inds]))][:size]


def minibatch(case, params):
    """The whole chain for one image.  -> dict(max_overlaps f32 [n], max_classes i32 [n], targets5 f32 [n,5] (the roidb's
    bbox_targets of every candidate), want64 f64 [n,2] (w * log(float64(ratio)): the yardstick of dw, dh), keep_inds, n_fg, n_rois,
    labels, rois [n_rois,5] (batch index 0), bbox_targets5 [n_rois,5], bbox_targets / bbox_inside_weights / bbox_outside_weights)"""
    gt, gcls, crowd, prop = case["gt_boxes"], case["gt_classes"], case["is_crowd"], case["proposals"]
    G, P = len(gt), len(prop)
    n = G + P
    boxes = np.vstack([gt, prop]).astype(np.float32)
    gt_classes = np.r_[gcls, np.zeros(P, np.int32)]
    is_crowd = np.r_[crowd, np.zeros(P, np.int32)]
    # gt rows as _add_gt_annotations leaves them (json_dataset.py:210-215): 1.0 at the class, -1 across a crowd row
    max_overlaps = np.zeros(n, np.float32)
    max_classes = np.zeros(n, np.int64)
    max_overlaps[:G] = np.where(crowd == 1, -1.0, 1.0)
    max_classes[:G] = np.where(crowd == 1, 0, gcls)
    # json_dataset.py:350-367: proposals against ALL gt
    if G > 0 and P > 0:
        ov = bbox_overlaps(prop, gt)
        argmaxes, maxes = ov.argmax(axis=1), ov.max(axis=1)
        I = np.where(maxes > 0)[0]
        max_overlaps[G + I] = maxes[I]
        max_classes[G + I] = gcls[argmaxes[I]]
    # json_dataset.py:328, :404-413
    crowd_inds = np.where(is_crowd == 1)[0]
    non_gt_inds = np.where(gt_classes == 0)[0]
    if params["crowd_thresh"] > 0 and len(crowd_inds) > 0 and len(non_gt_inds) > 0:
        ious = bb_iou_crowd(xyxy_to_xywh(boxes[non_gt_inds]), xyxy_to_xywh(boxes[crowd_inds]))
        bad = np.where(ious.max(axis=1) > params["crowd_thresh"])[0]
        max_overlaps[non_gt_inds[bad]] = -1
        max_classes[non_gt_inds[bad]] = 0
    # roidb.py:182-205
    targets = np.zeros((n, 5), np.float32)
    want64 = np.zeros((n, 2), np.float64)
    gt_inds = np.where((gt_classes > 0) & (is_crowd == 0))[0]
    if len(gt_inds) > 0:
        ex_inds = np.where(max_overlaps >= params["bbox_thresh"])[0]
        gt_assignment = bbox_overlaps(boxes[ex_inds], boxes[gt_inds]).argmax(axis=1)
        ex, g = boxes[ex_inds], boxes[gt_inds[gt_assignment]]
        targets[ex_inds, 0] = 1 if params["cls_agnostic_bbox_reg"] else max_classes[ex_inds]
        # boxes.py:224-238
        wx, wy, ww, wh = [float(w) for w in params["reg_weights"]]
        ex_w, ex_h = ex[:, 2] - ex[:, 0] + 1.0, ex[:, 3] - ex[:, 1] + 1.0
        ex_cx, ex_cy = ex[:, 0] + 0.5 * ex_w, ex[:, 1] + 0.5 * ex_h
        g_w, g_h = g[:, 2] - g[:, 0] + 1.0, g[:, 3] - g[:, 1] + 1.0
        g_cx, g_cy = g[:, 0] + 0.5 * g_w, g[:, 1] + 0.5 * g_h
        assert ex_w.dtype == np.float32 and g_cx.dtype == np.float32
        targets[ex_inds, 1] = wx * (g_cx - ex_cx) / ex_w
        targets[ex_inds, 2] = wy * (g_cy - ex_cy) / ex_h
        targets[ex_inds, 3] = ww * np.log(g_w / ex_w)
        targets[ex_inds, 4] = wh * np.log(g_h / ex_h)
        want64[ex_inds, 0] = float(np.float32(ww)) * np.log((g_w / ex_w).astype(np.float64))
        want64[ex_inds, 1] = float(np.float32(wh)) * np.log((g_h / ex_h).astype(np.float64))
    # fast_rcnn_sample_rois.py:57-91
    R = int(params["rois_per_image"])
    fg_quota = int(np.round(params["fg_fraction"] * R))
    keys = case["rand_keys"]
    fg_inds = np.where(max_overlaps >= params["fg_thresh"])[0]
    n_fg = min(fg_quota, fg_inds.size)
    fg_inds = choose(fg_inds, n_fg, keys)
    bg_inds = np.where((max_overlaps < params["bg_thresh_hi"]) & (max_overlaps >= params["bg_thresh_lo"]))[0]
    bg_inds = choose(bg_inds, min(R - n_fg, bg_inds.size), keys)
    keep = np.append(fg_inds, bg_inds).astype(np.int64)
    labels = max_classes[keep].copy()
    labels[n_fg:] = 0
    # :139-163, :107
    t5 = targets[keep]
    n_reg = 2 if params["cls_agnostic_bbox_reg"] else int(params["num_classes"])
    bt = np.zeros((len(keep), 4 * n_reg), np.float32)
    bw = np.zeros_like(bt)
    for ind in np.where(t5[:, 0] > 0)[0]:
        c = int(t5[ind, 0])
        bt[ind, 4 * c:4 * c + 4] = t5[ind, 1:]
        bw[ind, 4 * c:4 * c + 4] = 1.0
    rois = np.hstack((np.zeros((len(keep), 1), np.float32), boxes[keep] * case["im_scale"]))                     # :112-114
    return dict(max_overlaps=max_overlaps, max_classes=max_classes.astype(np.int32), targets5=targets, want64=want64,
                keep_inds=keep.astype(np.int32), n_fg=n_fg, n_rois=len(keep), labels=labels.astype(np.int32), rois=rois,
                bbox_targets5=t5, bbox_targets=bt, bbox_inside_weights=bw, bbox_outside_weights=(bw > 0).astype(np.float32))


def ulps_from(got, want64):
    """distance of float32 `got` from the float64 yardstick, in float32 ulps of the yardstick (0 where both are exactly 0;
    inf where the yardstick is exactly 0 and got is not)"""
    got = np.asarray(got, np.float64)
    want64 = np.asarray(want64, np.float64)
    ulp = np.spacing(np.abs(want64).astype(np.float32)).astype(np.float64)
    d = np.abs(got - want64) / ulp
    return np.where(want64 == 0, np.where(got == 0, 0.0, np.inf), d)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
