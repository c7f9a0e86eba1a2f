"""The cases of tests/test_kps_host.py and tests/test_hip_kps.py (tests/README_keypoints.md): B = 2 images of max_out = 6 rows with
det_count (0, 5) or (6, 3), so that an empty image, a partly filled one and a full one all occur, and boxes whose resized maps cover
every path of the kernel split.  The split (csrc/kps/kps_heatmaps.hip): a map is cut into BANDS of max(ceil(Hr / 8), 32) resized
rows, one workgroup each, and a band into STRIPS of 64 columns, one wavefront each in turns of four."""
import numpy as np

f32 = np.float32
B, MAX_OUT = 2, 6
COUNTS = [(0, 5), (6, 3)]
MAPS = [(17, 56), (1, 4), (3, 4), (1, 7), (3, 7), (1, 64), (3, 64)]                    # (K, S)
CLASSES = [1, 2, 1, 1, 3, 1, 1, 2, 1, 1, 1, 2]                                         # the class column of the rows, mixed


def box(x1, y1, w, h):
    return [x1, y1, x1 + w, y1 + h]


def boxes_of(S, n):
    """n = 5 or 9 live boxes (x1, y1, x2, y2); w x h in the comments"""
    if n == 5:
        return [box(3.25, 7.5, 257.0, 130.0),        # 257 x 130: five strips (a second turn of wavefront 0) and five bands of 32 rows
                box(-7.5, 2.0, 4096.0, 1.0),         # 4096 x 1: the side limit, 64 strips, one band of one row
                box(10.0, 20.0, 0.4, 0.7),           # below 1 in both: raised to 1 x 1
                box(-30.5, -12.25, 13.3, 20.6),      # fractional size, negative fractional offset
                box(0.0, 0.0, float(S), float(S))]   # identity
    return [box(5.0, 6.0, 12.0, 9.0),                # exactly integral
            box(1.5, 2.5, 5.0, 9.0),                 # below S for S >= 7 (shrinking), fractional offset
            box(100.0, 50.0, 1.0, 1.0),              # 1 x 1
            box(17.0, 3.0, 2.0, 300.0),              # 2 x 300: eight bands of 38 rows (the last of 34), two live lanes
            box(-4.0, 9.75, 300.0, 2.0),             # 300 x 2: five strips, one band
            box(40.0, 40.0, float(S), float(S)),     # identity
            box(0.125, 0.375, 33.7, 64.2),           # fractional: 34 x 65, three bands
            box(2.0, 2.0, 0.5, 40.0),                # width below 1 alone: 1 x 40
            box(7.0, -3.0, 70.0, 31.01)]             # 70 x 32: a strip boundary and exactly one band


def case(K, S, counts, seed=0):
    """-> heatmaps f32 [B*MAX_OUT, K, S, S], dets f32 [B, MAX_OUT, 6], det_count i32 [B].  The rows past a count hold NaN boxes and NaN
    maps: they must never matter."""
    rs = np.random.RandomState(1000 * seed + 64 * K + S)
    heat = (rs.randn(B * MAX_OUT, K, S, S) * 3.0).astype(f32)
    dets = np.full((B, MAX_OUT, 6), np.nan, f32)
    bx = boxes_of(S, sum(counts))
    i = 0
    for b in range(B):
        for d in range(counts[b]):
            dets[b, d, :4] = bx[i]
            dets[b, d, 4] = 0.9 - 0.05 * d
            dets[b, d, 5] = CLASSES[i]
            i += 1
        heat[b * MAX_OUT + counts[b]:(b + 1) * MAX_OUT] = np.nan
    return heat, dets, np.asarray(counts, np.int32)


def special_case():
    """K = 3, S = 7, det_count (0, 5).  Row (1, 0), identity size: map 0 has two equal maxima (the first, at (2, 3), wins), map 1 a NaN
    at (3, 2) -- a zero weight does not stop a NaN (0 * NaN), so it reaches the resized values whose taps touch it and the first of
    them, (1, 0), wins --, map 2 is all zeros (pos 0).  Row (1, 1), a general upscale (14 x 21): map 0 has a NaN at source (4, 5) -- the first
    resized value it reaches wins.  Row (1, 2), identity size: map 0 two NaNs (the first resized NaN, (0, 4), wins), map 1 a NaN at (0, 0), which is the
    first value it reaches: it picks its own position."""
    K, S = 3, 7
    heat, dets, cnt = case(K, S, (0, 5), seed=7)
    r = 1 * MAX_OUT
    dets[1, 0, :4] = box(2.5, -1.25, 7.0, 7.0)
    heat[r, 0] = np.minimum(heat[r, 0], 5.0)
    heat[r, 0, 2, 3] = heat[r, 0, 4, 1] = 9.0
    heat[r, 1, 3, 2] = np.nan
    heat[r, 2] = 0.0
    dets[1, 1, :4] = box(-30.5, -12.25, 13.3, 20.6)
    heat[r + 1, 0, 4, 5] = np.nan
    dets[1, 2, :4] = box(0.0, 0.0, 7.0, 7.0)
    heat[r + 2, 0, 5, 1] = heat[r + 2, 0, 1, 6] = np.nan
    heat[r + 2, 1, 0, 0] = np.nan
    return heat, dets, cnt


def refused_case():
    """K = 3, S = 7, det_count (6, 3): rows (0, 1) a NaN coordinate, (0, 3) an inf coordinate, (0, 4) a side of 4097, (1, 1) a side of
    4096.5 (ceil 4097), (1, 2) finite corners whose difference overflows; the rows beside them stay as they are."""
    heat, dets, cnt = case(3, 7, (6, 3), seed=3)
    dets[0, 1, 2] = np.nan
    dets[0, 3, 1] = -np.inf
    dets[0, 4, :4] = box(0.0, 0.0, 4097.0, 5.0)
    dets[1, 1, :4] = box(1.0, 1.0, 3.0, 4096.5)
    dets[1, 2, :4] = [-3e38, 0.0, 3e38, 4.0]
    want = np.array([[1, -1, 1, -1, -1, 1], [1, -1, -1, 0, 0, 0]], np.int32)
    return heat, dets, cnt, want
