"""A plain numpy restatement of the mask post-processing block of the reference's lib/utils/segms.py -- rle_masks_to_boxes, the
mask_util.iou under rle_mask_nms / rle_mask_voting, rle_mask_nms' walk and rle_mask_voting -- on the fixed-shape tensors of
include/detectorch_mpost_hip.h: the yardstick of the GPU tests of libdetectorch_mpost_hip.so.

The run lists are DECODED to numpy bitmaps (segm_eval_ref.decode, under the header's rules), and then the code is what the reference
writes on bitmaps: sums over rows and columns for the boxes, np.count_nonzero and one float64 division for the overlaps (maskApi.c:
rleIou), a stable np.argsort(-scores) and np.where(ovr <= thresh) for the walk, weight planes filled by real numpy slicing, an
explicit voter-order loop in float64 for the average (== np.average bit for bit: avg_numpy, asserted on every case by the host
test), np.diff on the column-major flattening for the encoding.  The kernels build no bitmap, so the two sides share no method.
The cast of a voter's box coordinates is stated (trunc_box: toward zero, NaN -> 0, as the header has it), not left to numpy's
platform-defined astype; vote_sparse is the vote on position windows from run ends, for images too large to decode, pinned
against vote on every case that can be decoded (tests/test_mask_post_limits_host.py).

pycocotools is not installed where the suite runs, so parity with pycocotools itself (mask_util.iou / decode / encode) is UNPINNED
(tests/README_mask_post.md); the restatement is pinned on the host against known answers and, on filled rectangles, against
coco_eval_ref's box IoU.  TEST INFRASTRUCTURE: nothing in the product imports it.

`variant` arguments restate a MUTANT of the contract (tests/README_mask_post.md): the host test uses them to show that the cases
can tell the mutant from the contract; the default is the contract.
"""
import numpy as np

import segm_eval_ref as sr

FLOOR = 1e-5


def sides(im_size):
    """(h, w) of one image as the header takes them from float32"""
    side = lambda v: 0 if not v >= 1 else min(int(v), sr.MAX_PIXELS)
    return side(np.float32(im_size[0])), side(np.float32(im_size[1]))


def bitmap(runs, n_runs, h, w):
    """one run list -> its [h, w] bool bitmap (column-major: position x * h + y)"""
    return sr.decode(runs, n_runs, h * w).reshape(w, h).T


def encode(mask):
    """rleEncode: a [h, w] bitmap -> the canonical COCO run lengths (zeros first; only the first run may have length 0)"""
    flat = np.asarray(mask, bool).reshape(-1, order='F')
    change = np.flatnonzero(np.diff(flat.astype(np.int8))) + 1
    runs = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return [0] + runs if flat.size and flat[0] else runs


def clamp(count, R):
    return min(max(int(count), 0), R)


# ---- rle_masks_to_boxes ------------------------------------------------------------------------------------------------------------------
def mask_box(mask):
    """segms.py:252-266 on one decoded mask -> ((x0, y0, x1, y1), keep)"""
    mask = np.array(mask, dtype=np.float32)
    if mask.sum() == 0:
        return (0, 0, 0, 0), False
    get_bounds = lambda flat: (np.where(flat > 0)[0].min(), np.where(flat > 0)[0].max())
    x0, x1 = get_bounds(mask.sum(axis=0))
    y0, y1 = get_bounds(mask.sum(axis=1))
    return (int(x0), int(y0), int(x1), int(y1)), True


def masks_to_boxes(runs, n_runs, counts, im_size, fill=-1):
    """dtc_mpost_boxes: dict(boxes i32 [N,R,4], area i32 [N,R], nonempty i32 [N,R]); rows past the counts hold `fill`"""
    N, R = n_runs.shape
    out = dict(boxes=np.full((N, R, 4), fill, np.int32), area=np.full((N, R), fill, np.int32), nonempty=np.full((N, R), fill, np.int32))
    for n in range(N):
        h, w = sides(im_size[n])
        for r in range(R if counts is None else clamp(counts[n], R)):
            m = bitmap(runs[n, r], n_runs[n, r], h, w)
            out["boxes"][n, r], keep = mask_box(m)
            out["area"][n, r], out["nonempty"][n, r] = np.count_nonzero(m), int(keep)
    return out


def interval_box(runs, n_runs, h, w):
    """((x0, y0, x1, y1), area) without a bitmap, on the one-runs as intervals in Python integers: for images too large to decode;
    pinned against mask_box on every small case (test_mask_post_host.py)"""
    e = sr.run_ends(runs, n_runs, h * w)
    iv = [(e[j - 1], e[j]) for j in range(1, len(e), 2) if e[j] > e[j - 1]]
    if not iv:
        return (0, 0, 0, 0), 0
    ys = [y for s, t in iv for y in ((0, h - 1) if s // h != (t - 1) // h else (s % h, (t - 1) % h))]
    return (iv[0][0] // h, min(ys), (iv[-1][1] - 1) // h, max(ys)), sum(t - s for s, t in iv)


# ---- maskUtils.iou ---------------------------------------------------------------------------------------------------------------------------
def overlaps(a_runs, a_n_runs, a_count, b_runs, b_n_runs, b_count, im_size, crowd, counts=None):
    """dtc_mpost_overlaps: dict(ovr f64 [N,Ra,Rb], a_area i32 [N,Ra], b_area i32 [N,Rb]).  counts: a function (runs_a, n_a, runs_b,
    n_b, hw) -> (i, aa, ab) to use instead of the bitmaps (segm_eval_ref.interval_counts)"""
    N, Ra = a_n_runs.shape
    Rb = b_n_runs.shape[1]
    out = dict(ovr=np.zeros((N, Ra, Rb)), a_area=np.zeros((N, Ra), np.int32), b_area=np.zeros((N, Rb), np.int32))
    for n in range(N):
        h, w = sides(im_size[n])
        hw = sr.pixels(im_size[n])
        na, nb = clamp(a_count[n], Ra), clamp(b_count[n], Rb)
        if counts is None:
            am = [sr.decode(a_runs[n, r], a_n_runs[n, r], hw) for r in range(na)]
            bm = [sr.decode(b_runs[n, r], b_n_runs[n, r], hw) for r in range(nb)]
            out["a_area"][n, :na] = [np.count_nonzero(m) for m in am]
            out["b_area"][n, :nb] = [np.count_nonzero(m) for m in bm]
            for i in range(na):
                for j in range(nb):
                    out["ovr"][n, i, j] = sr.mask_iou(am[i], bm[j], crowd)[0]
        else:
            empty = (np.zeros(0, np.uint32), 0)
            out["a_area"][n, :na] = [counts(a_runs[n, r], a_n_runs[n, r], *empty, hw)[1] for r in range(na)]
            out["b_area"][n, :nb] = [counts(*empty, b_runs[n, r], b_n_runs[n, r], hw)[2] for r in range(nb)]
            for i in range(na):
                for j in range(nb):
                    k, aa, ab = counts(a_runs[n, i], a_n_runs[n, i], b_runs[n, j], b_n_runs[n, j], hw)
                    out["ovr"][n, i, j] = 0.0 if k == 0 else np.float64(k) / np.float64(aa if crowd else aa + ab - k)
    return out


# ---- rle_mask_nms -------------------------------------------------------------------------------------------------------------------------------
def nms_walk(scores, classes, ious, thresh, mode, variant=None):
    """segms.py:209-240 on a given matrix for the rows of one image; rows suppress rows of their own class only.  variant: 'lt' (<
    at thresh), 'swap' (CONTAINMENT reads ovr[j, i]), 'reverse_ties' (equal scores in reverse row order), 'nan_class_equal'"""
    ious = np.array(ious, np.float64)
    if mode == 'IOMA':
        ious = np.maximum(ious, ious.transpose())
    elif mode == 'CONTAINMENT' and variant == 'swap':
        ious = ious.transpose()
    elif mode not in ('IOU', 'CONTAINMENT'):
        raise NotImplementedError('Mode {} is unknown'.format(mode))
    scores, classes = np.asarray(scores, np.float32), np.asarray(classes, np.float32)
    order = np.argsort(-scores, kind='stable')
    if variant == 'reverse_ties':
        order = (len(scores) - 1 - np.argsort(-scores[::-1], kind='stable'))
    keep = []
    while order.size > 0:
        i = order[0]
        keep.append(int(i))
        ovr = ious[i, order[1:]]
        with np.errstate(invalid='ignore'):
            stays = (ovr < thresh) if variant == 'lt' else (ovr <= thresh)
        other = classes[order[1:]] != classes[i]
        if variant == 'nan_class_equal':                         # (the mutant: two NaN classes are the same class)
            other &= ~(np.isnan(classes[order[1:]]) & np.isnan(classes[i]))
        inds_to_keep = np.where(stays | other)[0]
        order = order[inds_to_keep + 1]
    return keep


def nms(dets, count, ovr, thresh, mode, variant=None):
    """dtc_mpost_nms: dict(keep i32 [N,R] (then -1), keep_count i32 [N])"""
    N, R = dets.shape[:2]
    out = dict(keep=np.full((N, R), -1, np.int32), keep_count=np.zeros(N, np.int32))
    for n in range(N):
        c = clamp(count[n], R)
        keep = nms_walk(dets[n, :c, 4], dets[n, :c, 5], ovr[n, :c, :c], thresh, mode, variant) if c else []
        out["keep"][n, :len(keep)], out["keep_count"][n] = keep, len(keep)
    return out


# ---- rle_mask_voting ----------------------------------------------------------------------------------------------------------------------------
def trunc_box(coords, nan_to=0):
    """the header's cast of box coordinates to int32, stated explicitly: truncated toward zero, NaN: 0.  (The reference writes
    astype(np.int32), which C leaves undefined for a NaN and numpy leaves to the platform: on x86 it gives -2^31.  nan_to=-2**31
    restates that as a MUTANT of the contract.)  Magnitudes up to 2^30 are exact; anything above, +/-inf included, is the caller's to
    avoid and is not stated here"""
    c = np.asarray(coords, np.float32)
    nan = np.isnan(c)
    with np.errstate(invalid='ignore'):
        out = np.trunc(np.where(nan, np.float32(0), c)).astype(np.int64)
    out[nan] = nan_to
    return out.astype(np.int32)


def weight_planes(all_dets, h, w, variant=None):
    """segms.py:153-166: the weight of every voter at every pixel, float64 [A, h, w].  variant: 'floor' (coordinates floored, not
    truncated), 'clamp_neg' (a negative slice end clamped to 0), 'no_floor' (without the np.maximum), 'nan_int_min' (a NaN
    coordinate cast to -2^31, as numpy's own astype does on x86)"""
    with np.errstate(invalid='ignore'):
        all_boxes = trunc_box(np.floor(all_dets[:, :4]) if variant == 'floor' else all_dets[:, :4],
                              nan_to=-2 ** 31 if variant == 'nan_int_min' else 0)
    all_scores = all_dets[:, 4]
    mask_weights = np.zeros((len(all_dets), h, w))
    for k in range(len(all_dets)):
        ref_box = all_boxes[k]
        ref_box = [int(v) for v in ref_box]                       # (Python integers: INT_MIN + 1 and 2^30 + 1 without a warning)
        x_0 = max(ref_box[0], 0)
        x_1 = min(ref_box[2] + 1, w)
        y_0 = max(ref_box[1], 0)
        y_1 = min(ref_box[3] + 1, h)
        if variant == 'clamp_neg':
            x_1, y_1 = max(x_1, 0), max(y_1, 0)
        mask_weights[k, y_0:y_1, x_0:x_1] = all_scores[k]
    return mask_weights if variant == 'no_floor' else np.maximum(mask_weights, FLOOR)


def avg_loop(masks, ws, order=None):
    """sum_k w_k m_k / sum_k w_k with both sums added sequentially in voter order from 0.0, float64"""
    num, den = np.zeros(masks[0].shape), np.zeros(masks[0].shape)
    for k in (range(len(masks)) if order is None else order):
        with np.errstate(invalid='ignore'):                      # (an infinite weight times 0.0 is NaN, as in np.average)
            num = num + ws[k] * masks[k].astype(np.float64)
        den = den + ws[k]
    with np.errstate(invalid='ignore', divide='ignore'):
        return num / den


def avg_numpy(masks, ws):
    """what the reference calls (segms.py:184)"""
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.average([np.array(m, dtype=np.float32) for m in masks], axis=0, weights=ws)


def vote_image(top_lists, all_lists, all_dets, ovr, h, w, iou_thresh, binarize_thresh, method, variant=None, average=avg_loop):
    """segms.py:168-195 for one image.  top_lists / all_lists: [(runs, n_runs)] of the rows below the counts; ovr [T, A].  -> per top
    the voted run list, or None for "copied as it is".  variant: 'reverse' (voters summed in reverse order), 'gt' (> at iou_thresh),
    'skip_chunks' (AVG: a 256-pixel chunk, counted from position 0, that no voter has a pixel in is off whatever the threshold), and
    weight_planes'"""
    if method not in ('AVG', 'UNION'):
        raise NotImplementedError('Method {} is unknown'.format(method))
    decoded_all = [bitmap(r, k, h, w) for r, k in all_lists]
    mask_weights = weight_planes(np.asarray(all_dets, np.float32)[:len(all_lists)], h, w, variant)
    out = []
    for t, (r, k) in enumerate(top_lists):
        if bitmap(r, k, h, w).sum() == 0:
            out.append(None)
            continue
        with np.errstate(invalid='ignore'):
            row = np.asarray(ovr[t][:len(all_lists)], np.float64)
            inds_to_vote = np.where(row > iou_thresh if variant == 'gt' else row >= iou_thresh)[0]
        if len(inds_to_vote) < 2:
            out.append(None)
            continue
        masks_to_vote = [decoded_all[i] for i in inds_to_vote]
        if method == 'AVG':
            ws = mask_weights[inds_to_vote]
            soft_mask = average(masks_to_vote, ws, range(len(ws) - 1, -1, -1)) if variant == 'reverse' else average(masks_to_vote, ws)
            with np.errstate(invalid='ignore'):
                mask = soft_mask > binarize_thresh
            if variant == 'skip_chunks':                         # (the mutant: a 256-pixel chunk no voter has a pixel in is off)
                flat = mask.reshape(-1, order='F').copy()
                any_on = np.any(masks_to_vote, axis=0).reshape(-1, order='F')
                for base in range(0, flat.size, 256):
                    if not any_on[base:base + 256].any():
                        flat[base:base + 256] = False
                mask = flat.reshape(w, h).T
        else:
            mask = np.sum([np.array(m, dtype=np.float32) for m in masks_to_vote], axis=0) > 1e-5
        out.append(encode(mask))
    return out


def vote(case, ovr, method, variant=None, average=avg_loop):
    """dtc_mpost_vote on a case dict (tests/mask_post_cases.py): dict(lists [N][T]: the voted (or copied) run list of a row or None
    where out_n_runs < 0 or the row is past the count; out_n_runs i32 [N,T], need i32 [N,T]; copied bool [N,T]).  Rows past top_count
    hold -1 in out_n_runs and need: they are not written."""
    return _vote_rows(case, ovr, lambda tops, alls, dets, rows, h, w, n: vote_image(
        tops, alls, dets, rows, h, w, case["iou_thresh"], case["binarize_thresh"], method, variant, average))


def _vote_rows(case, ovr, image):
    """the rows of dtc_mpost_vote around a per-image vote `image(tops, alls, dets, ovr rows, h, w, n)`"""
    N, T = case["top_n_runs"].shape
    A = case["all_n_runs"].shape[1]
    stride, out_stride = case["top_runs"].shape[2], case["out_stride"]
    lists = [[None] * T for _ in range(N)]
    out_n, need, copied = np.full((N, T), -1, np.int32), np.full((N, T), -1, np.int32), np.zeros((N, T), bool)
    for n in range(N):
        h, w = sides(case["im_size"][n])
        nt, na = clamp(case["top_count"][n], T), clamp(case["all_count"][n], A)
        fits = h * w <= sr.MAX_PIXELS                            # h w > 2^30 before clipping: every row -1, need 0
        ok = [t for t in range(nt) if 0 <= case["top_n_runs"][n, t] <= stride and fits]
        tops = [(case["top_runs"][n, t], case["top_n_runs"][n, t]) for t in ok]
        alls = [(case["all_runs"][n, k], case["all_n_runs"][n, k]) for k in range(na)]
        voted = image(tops, alls, case["all_dets"][n], [ovr[n, t] for t in ok], h, w, n) if ok else []
        for t in range(nt):
            if t not in ok:
                out_n[n, t], need[n, t] = -1, 0
                continue
            runs = voted[ok.index(t)]
            if runs is None:
                copied[n, t] = True
                runs = [int(v) for v in case["top_runs"][n, t, :case["top_n_runs"][n, t]]]
            need[n, t] = len(runs)
            if len(runs) <= out_stride:
                out_n[n, t], lists[n][t] = len(runs), runs
    return dict(lists=lists, out_n_runs=out_n, need=need, copied=copied)


# ---- the vote on position windows, without a bitmap ---------------------------------------------------------------------------------------------
def clipped_ends(runs, n_runs, hw):
    """segm_eval_ref.run_ends as an int64 array (the sum of at most 2^20 uint32 runs is below 2^52: exact in uint64)"""
    n = min(max(int(n_runs), 0), len(runs))
    return np.minimum(np.cumsum(np.asarray(runs[:n], np.uint32).astype(np.uint64)), np.uint64(hw)).astype(np.int64)


def one_runs(ends):
    """the one-runs [s, e) of a list of clipped ends that hold a pixel -> (starts, stops)"""
    e = np.concatenate([[0], ends])
    s, t = e[1:-1:2], e[2::2]
    return s[t > s], t[t > s]


def on_at(ends, pos):
    """is the pixel at each position of pos set: the first run whose end lies above it is a one-run"""
    r = np.searchsorted(ends, pos, side='right')
    return (r < len(ends)) & (r % 2 == 1)


def vote_sparse(case, ovr, method, windows, variant=None):
    """vote() evaluated on position windows only, for UNION and for AVG with binarize_thresh >= 0, where a pixel no voter has is off:
    windows[n] is a list of [start, stop) position ranges of image n that together hold every one-run of every row of the pool below
    the count (asserted); the pixels outside them are off.  Works from the run ends: no bitmap, no h x w plane -- what a 2^30-pixel
    image needs.  The supports are numpy slices still: slice(y_0, y_1).indices(h) is the rule numpy applies to mask_weights[k,
    y_0:y_1, x_0:x_1].  Pinned against vote() on every case small enough to decode (test_mask_post_limits_host.py)"""
    if method not in ('AVG', 'UNION'):
        raise NotImplementedError('Method {} is unknown'.format(method))
    bt, iou_thresh = case["binarize_thresh"], case["iou_thresh"]
    assert method == 'UNION' or bt >= 0, "a negative threshold turns pixels on that no voter has"

    def image(tops, alls, dets, rows, h, w, n):
        hw = h * w
        wins = []
        for s, t in sorted((max(int(s), 0), min(int(t), hw)) for s, t in windows[n]):
            if wins and s <= wins[-1][1]:
                wins[-1][1] = max(wins[-1][1], t)
            elif t > s:
                wins.append([s, t])
        w_lo, w_hi = np.array([s for s, _ in wins], np.int64), np.array([t for _, t in wins], np.int64)
        ends = [clipped_ends(r, k, hw) for r, k in alls]
        for e in ends:
            s, t = one_runs(e)
            at = np.searchsorted(w_lo, s, side='right') - 1
            assert (at >= 0).all() and (t <= w_hi[at]).all(), "a one-run of the pool outside the windows"
        dets = np.asarray(dets, np.float32)[:len(alls)]
        boxes = trunc_box(dets[:, :4], nan_to=-2 ** 31 if variant == 'nan_int_min' else 0)
        out = []
        for t, (r, k) in enumerate(tops):
            if len(one_runs(clipped_ends(r, k, hw))[0]) == 0:
                out.append(None)
                continue
            with np.errstate(invalid='ignore'):
                voters = np.where(np.asarray(rows[t][:len(alls)], np.float64) >= iou_thresh)[0]
            if len(voters) < 2:
                out.append(None)
                continue
            starts, prev_on, prev_stop = [], False, 0
            for s, stop in wins:
                pos = np.arange(s, stop, dtype=np.int64)
                x, y = pos // h, pos % h
                num, den, any_on = np.zeros(len(pos)), np.zeros(len(pos)), np.zeros(len(pos), bool)
                for v in voters:
                    on = on_at(ends[v], pos)
                    any_on |= on
                    b = [int(c) for c in boxes[v]]
                    x0, x1, _ = slice(max(b[0], 0), min(b[2] + 1, w)).indices(w)
                    y0, y1, _ = slice(max(b[1], 0), min(b[3] + 1, h)).indices(h)
                    inside = (x >= x0) & (x < x1) & (y >= y0) & (y < y1)
                    wt = np.maximum(np.where(inside, np.float64(dets[v, 4]), 0.0), FLOOR)
                    with np.errstate(invalid='ignore'):
                        num, den = num + wt * on.astype(np.float64), den + wt
                with np.errstate(invalid='ignore', divide='ignore'):
                    val = (num / den > bt) if method == 'AVG' else any_on
                if prev_on and s > prev_stop:                     # the pixels between two windows are off
                    starts.append(prev_stop)
                    prev_on = False
                change = np.flatnonzero(np.diff(np.concatenate([[prev_on], val]).astype(np.int8))) + s
                starts += change.tolist()
                prev_on, prev_stop = bool(val[-1]), stop
            if prev_on and prev_stop < hw:
                starts.append(prev_stop)
            out.append(np.diff([0] + starts + [hw]).tolist())
        return out
    return _vote_rows(case, ovr, image)
