"""numpy restatement of include/detectorch_kps_hip.h (tests/README_keypoints.md): Detectron's utils/keypoints.py:heatmaps_to_keypoints
with OpenCV's cv2.resize(INTER_CUBIC), restated from their published sources with every cast written out.  Neither Detectron nor
OpenCV is on hand: parity with them is unpinned.  float32 arrays stay float32 under numpy's rules (a float32 array with a float32
scalar), so every operation below rounds once, in the order it is written."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
MAX_SIDE = 4096                    # DTC_KPS_MAX_SIDE
A = f32(-0.75)                     # OpenCV's INTER_CUBIC


def axis_taps(n_dst, S):
    """Destination indices 0 .. n_dst-1 of an axis resized from S -> (tap indices int64 [n_dst, 4], clamped; weights f32 [n_dst, 4])"""
    d = np.arange(n_dst, dtype=f64)
    f = ((d + f64(0.5)) * (f64(S) / f64(n_dst)) - f64(0.5)).astype(f32)        # in double, cast once
    fl = np.floor(f)
    s = fl.astype(np.int64)
    t = f - fl                                                                  # f32; not reset at a border
    one = f32(1)
    t1, u = t + one, one - t
    c0 = ((A * t1 - f32(5) * A) * t1 + f32(8) * A) * t1 - f32(4) * A
    c1 = ((A + f32(2)) * t - (A + f32(3))) * t * t + one
    c2 = ((A + f32(2)) * u - (A + f32(3))) * u * u + one
    c3 = one - c0 - c1 - c2
    w = np.stack([c0, c1, c2, c3], 1)
    assert w.dtype == f32
    return np.clip(s[:, None] + np.arange(-1, 3)[None, :], 0, S - 1), w


def resize_cubic(m, Hr, Wr):
    """m f32 [S, S] -> f32 [Hr, Wr]: horizontal first, then vertical over the horizontal results, left to right"""
    m = np.asarray(m, f32)
    S = m.shape[0]
    ix, cx = axis_taps(Wr, S)
    iy, cy = axis_taps(Hr, S)
    with np.errstate(invalid="ignore", over="ignore"):
        H = ((m[:, ix[:, 0]] * cx[:, 0] + m[:, ix[:, 1]] * cx[:, 1]) + m[:, ix[:, 2]] * cx[:, 2]) + m[:, ix[:, 3]] * cx[:, 3]    # [S, Wr]
        V = ((H[iy[:, 0]] * cy[:, 0, None] + H[iy[:, 1]] * cy[:, 1, None]) + H[iy[:, 2]] * cy[:, 2, None]) + H[iy[:, 3]] * cy[:, 3, None]
    assert V.dtype == f32 and V.shape == (Hr, Wr)
    return V


def row_size(box, min_size=0):
    """(x1, y1, x2, y2) f32 -> None for a refused row, or (Wr, Hr, wc, hc)"""
    x1, y1, x2, y2 = (f32(v) for v in box)
    if not all(np.isfinite(v) for v in (x1, y1, x2, y2)):
        return None
    with np.errstate(over="ignore"):
        w, h = np.maximum(x2 - x1, f32(1)), np.maximum(y2 - y1, f32(1))
    cw, ch = np.ceil(w), np.ceil(h)
    if min_size > 0:
        cw, ch = np.maximum(cw, f32(min_size)), np.maximum(ch, f32(min_size))
    if not (cw <= MAX_SIDE and ch <= MAX_SIDE):
        return None
    Wr, Hr = int(cw), int(ch)
    return Wr, Hr, f32(w / f32(Wr)), f32(h / f32(Hr))


def keypoint_xy(pos, Wr, wc, hc, x1, y1):
    """the explicit-cast form: in double, rounded once"""
    x_int, y_int = pos % Wr, pos // Wr
    return f32((f64(x_int) + f64(0.5)) * f64(wc) + f64(x1)), f32((f64(y_int) + f64(0.5)) * f64(hc) + f64(y1))


def prob_terms(v, m):
    """the float32 terms of the spatial softmax's denominator against the maximum m"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.exp((v - f32(m)).astype(f32).astype(f64)).astype(f32)


def prob_of(v, m):
    with np.errstate(invalid="ignore", divide="ignore"):
        return f32(f64(1.0) / prob_terms(v, m).astype(f64).sum(dtype=f64))


def prob_fsum(v, m):
    t = prob_terms(v, m).reshape(-1)
    if not np.all(np.isfinite(t)):
        return f32(np.nan)
    with np.errstate(divide="ignore"):
        return f32(f64(1.0) / f64(math.fsum(float(e) for e in t)))


def prob_literal_f32(v, m):
    """what numpy's own float32 exp and sum give (the form Detectron runs): for the record, not a reference"""
    with np.errstate(invalid="ignore", over="ignore", under="ignore", divide="ignore"):
        e = np.exp(v - f32(m))
        return f32(f32(1) / np.sum(e, dtype=f32))


def map_to_keypoint(m, box, min_size=0):
    """one map and one accepted box -> (x, y, logit, prob) f32, and pos"""
    Wr, Hr, wc, hc = row_size(box, min_size)
    v = resize_cubic(m, Hr, Wr)
    pos = int(np.argmax(v))                       # the first index of the maximum; a NaN counts as the maximum, the first NaN wins
    logit = v.reshape(-1)[pos]
    x, y = keypoint_xy(pos, Wr, wc, hc, f32(box[0]), f32(box[1]))
    return (x, y, logit, prob_of(v, logit)), pos


def heatmaps_to_keypoints(heatmaps, dets, det_count, person_class=-1, min_size=0):
    """heatmaps f32 [B*max_out, K, S, S], dets f32 [B, max_out, 6], det_count [B] -> keyps f32 [B, max_out, 4, K], kp_status i32
    [B, max_out]"""
    heatmaps, dets = np.asarray(heatmaps, f32), np.asarray(dets, f32)
    B, max_out = dets.shape[:2]
    K = heatmaps.shape[1]
    keyps, status = np.zeros((B, max_out, 4, K), f32), np.zeros((B, max_out), np.int32)
    for b in range(B):
        for d in range(min(max(int(det_count[b]), 0), max_out)):
            if person_class >= 0 and dets[b, d, 5] != f32(person_class):
                continue
            if row_size(dets[b, d, :4], min_size) is None:
                status[b, d] = -1
                continue
            status[b, d] = 1
            for k in range(K):
                keyps[b, d, :, k] = map_to_keypoint(heatmaps[b * max_out + d, k], dets[b, d, :4], min_size)[0]
    return keyps, status
