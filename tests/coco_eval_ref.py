"""A plain numpy, loop-for-loop restatement of COCOeval for boxes (pycocotools/cocoeval.py: computeIoU, evaluateImg, accumulate,
summarize; common/maskApi.c: bbIou) on the fixed-shape tensors of include/detectorch_eval_hip.h -- the yardstick of the GPU tests.

pycocotools is not installed where the suite runs, so parity with pycocotools itself is unpinned (tests/README_eval.md); the
restatement is pinned on the host against cases whose answers are known without it (tests/test_eval_host.py).  Everything is float64
from the float32 inputs, one numpy operation per step, in the header's order.  TEST INFRASTRUCTURE: nothing in the product imports it.
"""
import numpy as np

PAD_KEY = np.int64(0x7fffffffffffffff)


def coco_params():
    iou_thrs = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
    rec_thrs = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
    area_rngs = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)
    return iou_thrs, rec_thrs, (1, 10, 100), area_rngs


def xywh(b):
    """the reference's xyxy_to_xywh in float64: (x, y, w, h)"""
    b = np.asarray(b, np.float32).astype(np.float64)
    return b[0], b[1], (b[2] - b[0]) + 1.0, (b[3] - b[1]) + 1.0


def bb_iou(d, g, crowd):
    dx, dy, dw, dh = d
    gx, gy, gw, gh = g
    da, ga = dw * dh, gw * gh
    iw = min(dx + dw, gx + gw) - max(dx, gx)
    if iw <= 0:
        return np.float64(0.0)
    ih = min(dy + dh, gy + gh) - max(dy, gy)
    if ih <= 0:
        return np.float64(0.0)
    i = iw * ih
    u = da if crowd else (da + ga) - i
    return i / u


def score_key(s):
    """the float32 score as an unsigned integer that decreases with it (-0 counts as +0)"""
    s = np.float32(s)
    if s == 0:
        s = np.float32(0.0)
    u = int(np.array(s, np.float32).view(np.uint32))
    u = (~u & 0xffffffff) if u & 0x80000000 else (u | 0x80000000)
    return ~u & 0xffffffff


def class_segment(sorted_keys, k):
    """dtc_eval_accumulate's segment of class k + 1 in the ascending keys: [first key >= (k + 1) << 53, first key >= the smaller of
    (k + 2) << 53 and the padding key), compared as unsigned 64-bit integers"""
    keys = [int(v) & 0xffffffffffffffff for v in sorted_keys]
    first = lambda bound: next((i for i, v in enumerate(keys) if v >= bound), len(keys))
    return first((k + 1) << 53), first(min((k + 2) << 53, int(PAD_KEY)))


def evaluate_img(dt_rows, dt_boxes, dt_scores, gt_rows, gt_boxes, gt_crowd, gt_area, iou_thrs, area_rng, max_det, tally=None):
    """COCOeval.evaluateImg for one image, one class and one area range.  dt_rows / gt_rows: the row numbers (the ids).
    -> dict(dt_rows (score order, cut at max_det), dt_scores, dt_m [T,D] gt row or -1, dt_ig [T,D], gt_rows, gt_m [T,G] dt row or -1,
    gt_ig [G]) with the gt back in row order, or None when the image has neither."""
    if len(dt_rows) == 0 and len(gt_rows) == 0:
        return None
    T = len(iou_thrs)
    g_ig_row = np.array([bool(gt_crowd[j]) or gt_area[j] < area_rng[0] or gt_area[j] > area_rng[1] for j in range(len(gt_rows))], bool)
    gtind = np.argsort(g_ig_row.astype(np.uint8), kind='mergesort')
    dtind = np.argsort(-np.asarray(dt_scores, np.float32), kind='mergesort')[:max_det]
    g_ig = g_ig_row[gtind]
    crowd = [bool(gt_crowd[j]) for j in gtind]
    D, G = len(dtind), len(gtind)
    dbox = [xywh(dt_boxes[i]) for i in dtind]
    gbox = [xywh(gt_boxes[j]) for j in gtind]
    gtm = -np.ones((T, G), np.int64)
    dtm = -np.ones((T, D), np.int64)
    dt_ig = np.zeros((T, D), bool)
    ious = {}
    for tind, t in enumerate(iou_thrs):
        for dind in range(D):
            iou = min([t, 1 - 1e-10])
            m = -1
            for gind in range(G):
                if gtm[tind, gind] >= 0 and not crowd[gind]:
                    continue
                if m > -1 and not g_ig[m] and g_ig[gind]:
                    if tally is not None:
                        tally["stop_at_ignored"] += 1
                    break
                if (dind, gind) not in ious:
                    ious[dind, gind] = bb_iou(dbox[dind], gbox[gind], crowd[gind])
                if ious[dind, gind] < iou:
                    continue
                if tally is not None and m > -1 and ious[dind, gind] == iou:
                    tally["equal_iou_later_gt"] += 1
                if tally is not None and ious[dind, gind] == t:
                    tally["iou_equals_threshold"] += 1
                iou = ious[dind, gind]
                m = gind
            if m == -1:
                continue
            if tally is not None and crowd[m] and gtm[tind, m] >= 0:
                tally["crowd_rematched"] += 1
            dt_ig[tind, dind] = g_ig[m]
            dtm[tind, dind] = gt_rows[gtind[m]]
            gtm[tind, m] = dt_rows[dtind[dind]]
    d_area = [b[2] * b[3] for b in dbox]
    a = np.array([ar < area_rng[0] or ar > area_rng[1] for ar in d_area], bool).reshape(1, D)
    if tally is not None:
        tally["matched_to_ignored"] += int((dt_ig & (dtm >= 0)).sum())
        tally["unmatched_out_of_range"] += int(((dtm < 0) & np.repeat(a, T, 0)).sum())
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm < 0, np.repeat(a, T, 0)))
    gt_m = -np.ones((T, G), np.int64)
    gt_m[:, gtind] = gtm
    return dict(dt_rows=[dt_rows[i] for i in dtind], dt_scores=[np.float32(dt_scores[i]) for i in dtind], dt_m=dtm, dt_ig=dt_ig,
                gt_rows=list(gt_rows), gt_m=gt_m, gt_ig=g_ig_row)


def evaluate(dets, det_count, gt_boxes, gt_classes, gt_is_crowd, gt_counts, gt_area, num_classes, iou_thrs, area_rngs, max_det,
             tally=None):
    """COCOeval.evaluate: evalImgs[k][a][n] for k in 0 .. K-1 (class k + 1)"""
    N, max_out = dets.shape[:2]
    G = gt_boxes.shape[1]
    out = [[[None] * N for _ in area_rngs] for _ in range(num_classes - 1)]
    for n in range(N):
        nd = min(max(int(det_count[n]), 0), max_out)
        ng = min(max(int(gt_counts[n]), 0), G)
        cls = [int(c) if 1 <= c < num_classes else 0 for c in dets[n, :nd, 5]]
        for k in range(1, num_classes):
            dr = [d for d in range(nd) if cls[d] == k]
            gr = [g for g in range(ng) if gt_classes[n, g] == k]
            gb = [gt_boxes[n, g] for g in gr]
            if gt_area is None:
                ga = [xywh(b)[2] * xywh(b)[3] for b in gb]
            else:
                ga = [np.float64(gt_area[n, g]) for g in gr]
            for a, rng in enumerate(area_rngs):
                out[k - 1][a][n] = evaluate_img(dr, [dets[n, d, :4] for d in dr], [dets[n, d, 4] for d in dr], gr, gb,
                                                [gt_is_crowd[n, g] for g in gr], ga, iou_thrs, rng, max_det, tally)
    return out


def records(eval_imgs, dets, det_count, G, num_classes, T, A, image_base=0):
    """the evalImgs in the layout of dtc_eval_match's outputs"""
    N, max_out = dets.shape[:2]
    K = num_classes - 1
    o = dict(dt_rank=-np.ones((N, max_out), np.int32), dt_match=np.zeros((N, max_out), np.uint64), dt_ignore=np.zeros((N, max_out), np.uint64),
             gt_ignore=np.zeros((N, G), np.int32), gt_match=-np.ones((N, G, A, T), np.int32), npig=np.zeros((N, K, A), np.int32),
             sort_key=np.full((N, max_out), PAD_KEY, np.int64))
    for k in range(K):
        for a in range(A):
            for n in range(N):
                e = eval_imgs[k][a][n]
                if e is None:
                    continue
                o["npig"][n, k, a] = int((~e["gt_ig"]).sum())
                for j, g in enumerate(e["gt_rows"]):
                    o["gt_ignore"][n, g] |= int(e["gt_ig"][j]) << a
                    o["gt_match"][n, g, a, :] = e["gt_m"][:, j]
                for r, d in enumerate(e["dt_rows"]):
                    o["dt_rank"][n, d] = r
                    o["sort_key"][n, d] = ((k + 1) << 53) | (score_key(e["dt_scores"][r]) << 21) | (image_base + n)
                    for t in range(T):
                        o["dt_match"][n, d] |= np.uint64(int(e["dt_m"][t, r] >= 0) << (a * T + t))
                        o["dt_ignore"][n, d] |= np.uint64(int(e["dt_ig"][t, r]) << (a * T + t))
    return o


def accumulate(eval_imgs, num_classes, iou_thrs, rec_thrs, max_dets, n_areas):
    """COCOeval.accumulate -> precision [T,R,K,A,M], recall [T,K,A,M], counts [K,A] (npig)"""
    T, R, K, A, M = len(iou_thrs), len(rec_thrs), num_classes - 1, n_areas, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    counts = np.zeros((K, A), np.int32)
    for k in range(K):
        for a in range(A):
            for m, max_det in enumerate(max_dets):
                E = [e for e in eval_imgs[k][a] if e is not None]
                if len(E) == 0:
                    continue
                dt_scores = np.concatenate([np.asarray(e["dt_scores"][0:max_det], np.float32) for e in E])
                inds = np.argsort(-dt_scores, kind='mergesort')
                dtm = np.concatenate([e["dt_m"][:, 0:max_det] for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ig"][:, 0:max_det] for e in E], axis=1)[:, inds]
                gt_ig = np.concatenate([e["gt_ig"] for e in E])
                npig = np.count_nonzero(gt_ig == 0)
                counts[k, a] = npig
                if npig == 0:
                    continue
                tps = np.logical_and(dtm >= 0, np.logical_not(dt_ig))
                fps = np.logical_and(dtm < 0, np.logical_not(dt_ig))
                tp_sum = np.cumsum(tps, axis=1).astype(dtype=np.float64)
                fp_sum = np.cumsum(fps, axis=1).astype(dtype=np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    tp = np.array(tp)
                    fp = np.array(fp)
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    pr = pr.tolist()
                    q = q.tolist()
                    for i in range(nd - 1, 0, -1):
                        if pr[i] > pr[i - 1]:
                            pr[i - 1] = pr[i]
                    inds_r = np.searchsorted(rc, rec_thrs, side='left')
                    try:
                        for ri, pi in enumerate(inds_r):
                            q[ri] = pr[pi]
                    except IndexError:
                        pass
                    precision[t, :, k, a, m] = np.array(q)
    return precision, recall, counts


def summarize(precision, recall, iou_thrs):
    """COCOeval.summarize for 'bbox' (the twelve stats); -1 everywhere when the shape is not COCO's"""
    stats = np.full(12, -1.0)
    if precision.shape[3] != 4 or precision.shape[4] != 3 or len(iou_thrs) != 10:
        return stats

    def _summarize(ap=1, iouThr=None, aind=0, mind=2):
        if ap == 1:
            s = precision
            if iouThr is not None:
                t = np.where(iouThr == iou_thrs)[0]
                s = s[t]
            s = s[:, :, :, [aind], [mind]]
        else:
            s = recall
            if iouThr is not None:
                t = np.where(iouThr == iou_thrs)[0]
                s = s[t]
            s = s[:, :, [aind], [mind]]
        if len(s[s > -1]) == 0:
            return -1
        return np.mean(s[s > -1])

    stats[0] = _summarize(1)
    stats[1] = _summarize(1, iouThr=.5)
    stats[2] = _summarize(1, iouThr=.75)
    stats[3] = _summarize(1, aind=1)
    stats[4] = _summarize(1, aind=2)
    stats[5] = _summarize(1, aind=3)
    stats[6] = _summarize(0, mind=0)
    stats[7] = _summarize(0, mind=1)
    stats[8] = _summarize(0, mind=2)
    stats[9] = _summarize(0, aind=1)
    stats[10] = _summarize(0, aind=2)
    stats[11] = _summarize(0, aind=3)
    return stats


def run(case, tally=None):
    """a case dict (tests/eval_cases.py) through evaluate, records, accumulate and summarize"""
    iou_thrs, rec_thrs, max_dets, area_rngs = case["iou_thrs"], case["rec_thrs"], case["max_dets"], case["area_rngs"]
    ev = evaluate(case["dets"], case["det_count"], case["gt_boxes"], case["gt_classes"], case["gt_is_crowd"], case["gt_counts"],
                  case.get("gt_area"), case["num_classes"], iou_thrs, area_rngs, max_dets[-1], tally)
    rec = records(ev, case["dets"], case["det_count"], case["gt_boxes"].shape[1], case["num_classes"], len(iou_thrs), len(area_rngs))
    precision, recall, counts = accumulate(ev, case["num_classes"], iou_thrs, rec_thrs, max_dets, len(area_rngs))
    return dict(rec, precision=precision, recall=recall, counts=counts, stats=summarize(precision, recall, iou_thrs))
