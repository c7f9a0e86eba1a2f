"""A plain numpy restatement of COCOeval for iouType 'segm' on the fixed-shape tensors of include/detectorch_segm_hip.h -- the yardstick
of the GPU tests of libdetectorch_segm_hip.so.

COCOeval's segm branch differs from its box branch in two things: the IoU is maskApi.c:rleIou, and a detection's area is its mask's
pixel count.  Here the run lists are DECODED to numpy bitmaps under the header's rules (column-major, zeros first, zero-length runs
anywhere, run ends as 64-bit prefix sums clipped to h * w, zeros past the last run, n_runs <= 0 empty, n_runs clamped to the stride),
the counts are np.count_nonzero and the IoU is one float64 division.  evaluate_img is coco_eval_ref.evaluate_img with the IoU matrix
and the detection areas as arguments; the records, accumulate and summarize are coco_eval_ref's own.

pycocotools is not installed where the suite runs, so parity with pycocotools itself is unpinned (tests/README_segm_eval.md); the
restatement is pinned on the host against known answers and, on filled rectangles, against coco_eval_ref on the boxes
(tests/test_segm_eval_host.py).  TEST INFRASTRUCTURE: nothing in the product imports it.
"""
import numpy as np

import coco_eval_ref as cr

MAX_PIXELS = 1 << 30


def pixels(im_size):
    """h * w of one image as the header takes it from float32 (h, w)"""
    side = lambda v: 0 if not v >= 1 else min(int(v), MAX_PIXELS)
    return min(side(np.float32(im_size[0])) * side(np.float32(im_size[1])), MAX_PIXELS)


def run_ends(runs, n_runs, hw):
    """the clipped run ends of one list, as Python ints"""
    n = min(max(int(n_runs), 0), len(runs))
    ends, pos = [], 0
    for j in range(n):
        pos += int(np.uint32(runs[j]))                        # Python ints: no wrap, whatever the runs hold
        ends.append(min(pos, hw))
    return ends


def decode(runs, n_runs, hw):
    """one run list -> its bitmap as a flat bool array of h * w positions (position x * h + y)"""
    m = np.zeros(hw, bool)
    ends = run_ends(runs, n_runs, hw)
    for j in range(1, len(ends), 2):
        m[ends[j - 1]:ends[j]] = True
    return m


def mask_iou(d, g, crowd):
    """rleIou of two bitmaps -> (iou, i, da, ga)"""
    i, da, ga = int(np.count_nonzero(d & g)), int(np.count_nonzero(d)), int(np.count_nonzero(g))
    u = da if crowd else da + ga - i
    return (np.float64(0.0) if i == 0 else np.float64(i) / np.float64(u)), i, da, ga


def interval_counts(runs_d, n_d, runs_g, n_g, hw):
    """(i, da, ga) without a bitmap, by intersecting the one-runs as intervals in Python integers: for images too large to decode;
    pinned against decode() on every small case (test_segm_eval_host.py)"""
    ed, eg = run_ends(runs_d, n_d, hw), run_ends(runs_g, n_g, hw)
    iv = lambda e: [(e[j - 1], e[j]) for j in range(1, len(e), 2) if e[j] > e[j - 1]]
    a, b = iv(ed), iv(eg)
    i = p = q = 0
    while p < len(a) and q < len(b):
        i += max(0, min(a[p][1], b[q][1]) - max(a[p][0], b[q][0]))
        if a[p][1] <= b[q][1]:
            p += 1
        else:
            q += 1
    return i, sum(e - s for s, e in a), sum(e - s for s, e in b)


def valid_class(c, num_classes):
    return int(c) if 1 <= c < num_classes else 0


def iou_matrix(case, counts=None):
    """dtc_segm_iou: dict(iou f64 [N,max_out,G], det_area i32 [N,max_out], gt_mask_area i32 [N,G], n_bad i32 [N]).
    counts: a function (runs_d, n_d, runs_g, n_g, hw) -> (i, da, ga) to use instead of the bitmaps (interval_counts)."""
    dets, G = case["dets"], case["gt_runs"].shape[1]
    N, max_out = dets.shape[:2]
    nc = case["num_classes"]
    out = dict(iou=np.zeros((N, max_out, G)), det_area=np.zeros((N, max_out), np.int32), gt_mask_area=np.zeros((N, G), np.int32),
               n_bad=np.zeros(N, np.int32))
    for n in range(N):
        hw = pixels(case["im_size"][n])
        nd = min(max(int(case["det_count"][n]), 0), max_out)
        ng = min(max(int(case["gt_counts"][n]), 0), G)
        out["n_bad"][n] = sum(1 for d in range(nd) if case["det_n_runs"][n, d] < 0)
        dcls = [valid_class(dets[n, d, 5], nc) for d in range(nd)]
        gcls = [valid_class(case["gt_classes"][n, g], nc) for g in range(ng)]
        if counts is None:
            dm = {d: decode(case["det_runs"][n, d], case["det_n_runs"][n, d], hw) for d in range(nd) if dcls[d]}
            gm = {g: decode(case["gt_runs"][n, g], case["gt_n_runs"][n, g], hw) for g in range(ng) if gcls[g]}
            for d, m in dm.items():
                out["det_area"][n, d] = np.count_nonzero(m)
            for g, m in gm.items():
                out["gt_mask_area"][n, g] = np.count_nonzero(m)
        else:
            empty = (np.zeros(0, np.uint32), 0)
            for d in range(nd):
                if dcls[d]:
                    out["det_area"][n, d] = counts(case["det_runs"][n, d], case["det_n_runs"][n, d], *empty, hw)[1]
            for g in range(ng):
                if gcls[g]:
                    out["gt_mask_area"][n, g] = counts(*empty, case["gt_runs"][n, g], case["gt_n_runs"][n, g], hw)[2]
        for d in range(nd):
            for g in range(ng):
                if not dcls[d] or dcls[d] != gcls[g]:
                    continue
                crowd = bool(case["gt_is_crowd"][n, g])
                if counts is None:
                    out["iou"][n, d, g] = mask_iou(dm[d], gm[g], crowd)[0]
                else:
                    i, da, ga = counts(case["det_runs"][n, d], case["det_n_runs"][n, d], case["gt_runs"][n, g], case["gt_n_runs"][n, g], hw)
                    out["iou"][n, d, g] = 0.0 if i == 0 else np.float64(i) / np.float64(da if crowd else da + ga - i)
    return out


def evaluate_img(dt_rows, dt_scores, dt_area, gt_rows, gt_crowd, gt_area, iou, iou_thrs, area_rng, max_det, tally=None):
    """COCOeval.evaluateImg for one image, one class and one area range, on given IoUs: iou[d][g] for the positions d of dt_rows and
    g of gt_rows; dt_area: the detections' own areas.  -> the dict of coco_eval_ref.evaluate_img, or None when the image has neither."""
    if len(dt_rows) == 0 and len(gt_rows) == 0:
        return None
    T = len(iou_thrs)
    g_ig_row = np.array([bool(gt_crowd[j]) or gt_area[j] < area_rng[0] or gt_area[j] > area_rng[1] for j in range(len(gt_rows))], bool)
    gtind = np.argsort(g_ig_row.astype(np.uint8), kind='mergesort')
    dtind = np.argsort(-np.asarray(dt_scores, np.float32), kind='mergesort')[:max_det]
    g_ig = g_ig_row[gtind]
    crowd = [bool(gt_crowd[j]) for j in gtind]
    D, G = len(dtind), len(gtind)
    gtm = -np.ones((T, G), np.int64)
    dtm = -np.ones((T, D), np.int64)
    dt_ig = np.zeros((T, D), bool)
    for tind, t in enumerate(iou_thrs):
        for dind in range(D):
            best = min([t, 1 - 1e-10])
            m = -1
            for gind in range(G):
                if gtm[tind, gind] >= 0 and not crowd[gind]:
                    continue
                if m > -1 and not g_ig[m] and g_ig[gind]:
                    if tally is not None:
                        tally["stop_at_ignored"] += 1
                    break
                v = np.float64(iou[dtind[dind]][gtind[gind]])
                if v < best:
                    continue
                if tally is not None and m > -1 and v == best:
                    tally["equal_iou_later_gt"] += 1
                if tally is not None and v == t:
                    tally["iou_equals_threshold"] += 1
                best = v
                m = gind
            if m == -1:
                continue
            if tally is not None and crowd[m] and gtm[tind, m] >= 0:
                tally["crowd_rematched"] += 1
            dt_ig[tind, dind] = g_ig[m]
            dtm[tind, dind] = gt_rows[gtind[m]]
            gtm[tind, m] = dt_rows[dtind[dind]]
    a = np.array([np.float64(dt_area[i]) < area_rng[0] or np.float64(dt_area[i]) > area_rng[1] for i in dtind], bool).reshape(1, D)
    if tally is not None:
        tally["matched_to_ignored"] += int((dt_ig & (dtm >= 0)).sum())
        tally["unmatched_out_of_range"] += int(((dtm < 0) & np.repeat(a, T, 0)).sum())
    dt_ig = np.logical_or(dt_ig, np.logical_and(dtm < 0, np.repeat(a, T, 0)))
    gt_m = -np.ones((T, G), np.int64)
    gt_m[:, gtind] = gtm
    return dict(dt_rows=[dt_rows[i] for i in dtind], dt_scores=[np.float32(dt_scores[i]) for i in dtind], dt_m=dtm, dt_ig=dt_ig,
                gt_rows=list(gt_rows), gt_m=gt_m, gt_ig=g_ig_row)


def evaluate(dets, det_count, iou, det_area, gt_classes, gt_is_crowd, gt_counts, gt_area, gt_mask_area, num_classes, iou_thrs, area_rngs,
             max_det, tally=None):
    """dtc_segm_match as COCOeval.evaluate: evalImgs[k][a][n] for k in 0 .. K-1 (class k + 1)"""
    N, max_out = dets.shape[:2]
    G = gt_classes.shape[1]
    out = [[[None] * N for _ in area_rngs] for _ in range(num_classes - 1)]
    for n in range(N):
        nd = min(max(int(det_count[n]), 0), max_out)
        ng = min(max(int(gt_counts[n]), 0), G)
        cls = [valid_class(c, num_classes) for c in dets[n, :nd, 5]]
        for k in range(1, num_classes):
            dr = [d for d in range(nd) if cls[d] == k]
            gr = [g for g in range(ng) if gt_classes[n, g] == k]
            ga = [np.float64(gt_mask_area[n, g]) if gt_area is None else np.float64(gt_area[n, g]) for g in gr]
            sub = [[iou[n, d, g] for g in gr] for d in dr]
            for a, rng in enumerate(area_rngs):
                out[k - 1][a][n] = evaluate_img(dr, [dets[n, d, 4] for d in dr], [det_area[n, d] for d in dr], gr,
                                                [gt_is_crowd[n, g] for g in gr], ga, sub, iou_thrs, rng, max_det, tally)
    return out


def match_records(case, iou, det_area, gt_mask_area, tally=None, image_base=0):
    """dtc_segm_match's outputs (coco_eval_ref.records' layout) and the evalImgs they came from"""
    iou_thrs, area_rngs = case["iou_thrs"], case["area_rngs"]
    ev = evaluate(case["dets"], case["det_count"], iou, det_area, case["gt_classes"], case["gt_is_crowd"], case["gt_counts"],
                  case.get("gt_area"), gt_mask_area, case["num_classes"], iou_thrs, area_rngs, case["max_dets"][-1], tally)
    rec = cr.records(ev, case["dets"], case["det_count"], case["gt_classes"].shape[1], case["num_classes"], len(iou_thrs), len(area_rngs),
                     image_base)
    return rec, ev


def run(case, tally=None, counts=None):
    """a case dict (tests/segm_eval_cases.py) through iou_matrix, evaluate, records, accumulate and summarize"""
    pairs = iou_matrix(case, counts)
    rec, ev = match_records(case, pairs["iou"], pairs["det_area"], pairs["gt_mask_area"], tally)
    precision, recall, counts_ = cr.accumulate(ev, case["num_classes"], case["iou_thrs"], case["rec_thrs"], case["max_dets"],
                                               len(case["area_rngs"]))
    return dict(rec, **pairs, precision=precision, recall=recall, counts=counts_, stats=cr.summarize(precision, recall, case["iou_thrs"]))
