"""dtc_poly_rle past where tests/test_hip_poly_rle.py stops (test support, not a test module): the "Limits" section of
tests/README_poly_rle.md lists the cases.  Every builder is seeded, runs once (lru_cache), returns the INPUTS only -- a case of
poly_rle_ref.make_case -- and its arrays are read-only.  tests/test_poly_rle_limits_host.py pins on the CPU the condition every case is
named for; tests/test_hip_poly_rle_limits.py launches them.

The kernel arithmetic the conditions speak of (detectorch_amd/csrc/poly_rle/poly_rle.hip): the first sort's key is polygon << 32 |
position, sorted by the 8-bit digits in use only -- digit 3 is position bits 24 .. 31, digit 4 polygon bits 0 .. 7, digit 5 polygon bits
8 .. 15; the second sort's key is position << 1 | end.  The sorting node runs 256, 512 or 1024 threads for events_stride up to 2048,
4096 or 8192, thread t owns the events [t per, (t + 1) per) with per = ceil(events / threads) <= 8.
"""
import functools

import numpy as np

import poly_rle_ref as pr

BASE_SEED = 20261020 + 5000
KEYS_PER_THREAD = 8                                           # csrc/poly_rle: kPolyKeysPerThread
SORT_CAPACITIES = (2048, 4096, 8192)
DENSE_PIXELS = 1 << 22                                        # cases up to this size are also decoded (poly_rle_ref.run)


def _freeze(case):
    for v in case.values():
        v.setflags(write=False)
    return case


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], np.float64)


# ---- 1. many_polygons -----------------------------------------------------------------------------------------------------------------------
MANY_HW = (70, 100)


@functools.lru_cache(maxsize=None)
def many_polygons():
    """one 70 x 100 image: row 0 holds 300 small triangles, row 1 the three polygons behind them (numbers 300 .. 302 of the image, 0 .. 2
    of the row).  Triangle 256 + j of row 0 is triangle j moved by (1.3, 0.7): their events interleave by position, so a sort that
    takes the two for one polygon pairs them wrongly (every polygon has an even number of events: merely putting one polygon's
    block of events behind another's keeps every parity)"""
    rs = np.random.RandomState(BASE_SEED + 1)
    h, w = MANY_HW
    tris = []
    for _ in range(303):
        c = rs.uniform([2, 2], [w - 2, h - 2])
        tris.append(c + rs.uniform(-4.5, 4.5, (3, 2)))
    for j in range(300 - 256):
        tris[256 + j] = tris[j] + np.array([1.3, 0.7])
    return _freeze(pr.make_case([[tris[:300], tris[300:]]], [MANY_HW]))


# ---- 2. full_strides ------------------------------------------------------------------------------------------------------------------------
FULL_HW = (40, 1100)
FULL_COLUMNS = (256, 512, 1024)


@functools.lru_cache(maxsize=None)
def full_strides():
    """three 40 x 1100 images; image k: a small row, a row of four rectangles from x0 = 10.3 over FULL_COLUMNS[k] pixel columns (2
    events per rectangle and column: 2048, 4096, 8192), a small row"""
    per = []
    for k in FULL_COLUMNS:
        big = [rect(10.3, 2.5 + 9 * j, 10.3 + k, 7.5 + 9 * j) for j in range(4)]
        per.append([[rect(3, 3, 9, 9)], big, [rect(20.5, 30.5, 31.5, 38.5)]])
    return _freeze(pr.make_case(per, [FULL_HW] * 3))


# ---- 3. stacked_positions -------------------------------------------------------------------------------------------------------------------
STACK_HW = (40, 60)
STACK_N = 50
STACK_RECT = (10.3, 5.5, 30.3, 30.5)


@functools.lru_cache(maxsize=None)
def stacked_positions():
    """one 40 x 60 image: row 0 the same rectangle STACK_N times; row 1 STACK_N rectangles of 1 .. STACK_N pixel columns from the same
    left edge and between the same rows (they share the two events of their first column only); rows 2 and 3: the rectangle once, the
    widest one once"""
    x0, y0, x1, y1 = STACK_RECT
    fan = [rect(x0, y0, x0 + k, y1) for k in range(1, STACK_N + 1)]
    return _freeze(pr.make_case([[[rect(*STACK_RECT)] * STACK_N, fan, [rect(*STACK_RECT)], [fan[-1]]]], [STACK_HW]))


# ---- 4. big_image / 5. mid_image ------------------------------------------------------------------------------------------------------------
BIG_HW = (32768, 32768)


@functools.lru_cache(maxsize=None)
def big_image():
    """2^30 pixels: a quadrilateral in the far corner that reaches past the right and the bottom border and, BEHIND it in the same row,
    a rectangle in columns 2774 .. 2779 (by polygon the far one sorts first, by position last; and the low 24 bits of position << 1
    alone would leave the two mixed); in row 1 a small polygon at the origin"""
    corner = np.array([[32690.2, 32600.4], [32768.5, 32611.3], [32768.5, 32768.5], [32701.7, 32768.5]], np.float64)
    return _freeze(pr.make_case([[[corner, rect(2774.3, 100.2, 2780.4, 140.7)], [rect(-1, -1, 3.4, 2.6)]]], [BIG_HW]))


MID_HW = (3000, 3000)


@functools.lru_cache(maxsize=None)
def mid_image():
    """9e6 pixels, at least 2^23: a polygon in the last columns and, BEHIND it in the same row, one in columns 2000 .. 2019 (by polygon
    the far one sorts first, by position last; the low 24 bits of position << 1 alone would keep that order)"""
    far = np.array([[2950.3, 100.2], [2998.6, 140.7], [2990.1, 2990.4], [2960.8, 2900.9]], np.float64)
    return _freeze(pr.make_case([[[far, rect(2000.3, 50.2, 2020.4, 90.7)]]], [MID_HW]))


# ---- 6. far_vertices ------------------------------------------------------------------------------------------------------------------------
FAR_HW = (120, 160)


@functools.lru_cache(maxsize=None)
def far_vertices():
    """120 x 160: a quadrilateral with every vertex about a million pixels away -- two shallow and two steep edges across the image --
    and a row whose coordinates are all negative.  (A row with a vertex at 2^26 - 1 is left out: its point-by-point trace takes
    arrays of 3.4e8 elements on the host, tests/README_poly_rle.md.)"""
    far = np.array([[-1e6, 10.3], [1e6, 90.7], [50.2, 1e6], [40.1, -1e6]], np.float64)
    return _freeze(pr.make_case([[[far], [rect(-90.5, -70.25, -3.5, -2.75), np.array([[-1.0, -1.0], [-200.0, -3.0], [-7.0, -900.0]])]]], [FAR_HW]))


# ---- 7. im_sizes ----------------------------------------------------------------------------------------------------------------------------
IM_SIZES = ((7.9, 5.2), (0.5, 9), (np.nan, 9), (1, 1), (2.0 ** 30, 1), (65536, 32768))


@functools.lru_cache(maxsize=None)
def im_sizes():
    """six images of one row each: a fraction, below 1, NaN, one pixel, 2^30 x 1 with the polygon at its top, and 65536 x 32768 whose
    product is clipped to 2^30 (the polygon lies across column 16384, the first one past the clipped image)"""
    small = rect(1, 2, 3, 5)
    per = [[[small]], [[small]], [[small]], [[rect(-1, -1, 3, 3)]], [[rect(-1, 2.4, 3, 9.6)]], [[rect(16380.3, 100.2, 16390.4, 220.7)]]]
    return _freeze(pr.make_case(per, IM_SIZES))


# ---- 8. max_shapes --------------------------------------------------------------------------------------------------------------------------
MAX_HW = (20, 30)
MAX_G, MAX_NP = 256, 4096
MAX_COUNTS = (256, 255, 300, -4)


@functools.lru_cache(maxsize=None)
def max_shapes():
    """G = 256, NP = 4096, gt_counts (256, 255, 300, -4): image 0 has 16 small triangles in every row, 4096 polygons in all, the last
    one owned by row 255; the others one small rectangle per row, placed by the row's number"""
    rs = np.random.RandomState(BASE_SEED + 8)
    h, w = MAX_HW
    im0 = [[rs.uniform([1, 1], [w - 1, h - 1]) + rs.uniform(-2.5, 2.5, (3, 2)) for _ in range(16)] for g in range(MAX_G)]
    tiny = [[rect(g % 27 + 0.3, g // 27 + 0.4, g % 27 + 2.6, g // 27 + 3.7)] for g in range(MAX_G)]
    return _freeze(pr.make_case([im0, tiny, tiny, tiny], [MAX_HW] * 4, gt_counts=MAX_COUNTS))


# ---- the cases and the capacities they run at: name -> (builder, [(runs_stride, events_stride)]) ---------------------------------------------
CASES = {
    "many_polygons": (many_polygons, [(4096, 8192)]),
    "full_strides": (full_strides, [(8200, e) for e in (2048, 2047, 4096, 4095, 8192, 8191)] + [(2049, 8192), (2048, 8192)]),
    "stacked_positions": (stacked_positions, [(256, 4096)]),
    "big_image": (big_image, [(512, 2048)]),
    "mid_image": (mid_image, [(512, 2048)]),
    "far_vertices": (far_vertices, [(1024, 2048)]),
    "im_sizes": (im_sizes, [(512, 2048)]),
    "max_shapes": (max_shapes, [(256, 2048)]),
}


def decodable(case):
    return max(pr.side(h) * pr.side(w) for h, w in case["im_size"]) <= DENSE_PIXELS


@functools.lru_cache(maxsize=None)
def expected(name, runs_stride, events_stride):
    """the sparse restatement's answer, computed once for the host and the GPU tests"""
    return pr.run_sparse(CASES[name][0](), runs_stride, events_stride)
