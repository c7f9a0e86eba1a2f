"""The cases of the mask post-processing tests (tests/README_mask_post.md), shared by the host and the GPU tests.  A case is a dict of
numpy arrays in the layout of include/detectorch_mpost_hip.h; run lists are uint32.  The rows past every count hold garbage runs, the
run counts -2^31 / 2^30 / 2^31 - 1 and NaN scores.  Everything is seeded."""
import itertools

import numpy as np

import mask_post_ref as mr
import segm_eval_cases as sc

GARBAGE_COUNTS = [-(1 << 31), 1 << 30, (1 << 31) - 1]


def pack_lists(images, R, stride, seed):
    """images: per image a list of run lists -- a list of lengths, or (array-like, n_runs) to give a count of its own -> (runs uint32
    [N,R,stride], n_runs i32 [N,R]); what no list covers is garbage"""
    rs = np.random.RandomState(seed)
    N = len(images)
    runs = rs.randint(0, 1 << 32, (N, R, stride), dtype=np.uint64).astype(np.uint32)
    n_runs = rs.choice(GARBAGE_COUNTS, (N, R)).astype(np.int32)
    for n, rows in enumerate(images):
        assert len(rows) <= R
        for j, row in enumerate(rows):
            lst, k = row if isinstance(row, tuple) else (row, len(row))
            lst = np.asarray(lst, np.uint32)
            assert len(lst) <= stride, (len(lst), stride)
            runs[n, j, :len(lst)], n_runs[n, j] = lst, k
    return runs, n_runs


def vote_case(images, T, A, top_stride, all_stride, out_stride, iou_thresh, binarize_thresh, seed, dets_stride=5):
    """images: [((h, w), tops [run list], pool [(run list, (x1, y1, x2, y2), score)])]"""
    rs = np.random.RandomState(seed + 1000)
    N = len(images)
    top_runs, top_n_runs = pack_lists([tops for _, tops, _ in images], T, top_stride, seed)
    all_runs, all_n_runs = pack_lists([[v[0] for v in pool] for _, _, pool in images], A, all_stride, seed + 1)
    all_dets = (rs.rand(N, A, dets_stride) * 40 - 10).astype(np.float32)
    all_dets[:, :, 4] = np.nan
    for n, (_, _, pool) in enumerate(images):
        for k, (_, box, score) in enumerate(pool):
            all_dets[n, k, :4], all_dets[n, k, 4] = box, score
    return dict(top_runs=top_runs, top_n_runs=top_n_runs, top_count=np.array([len(t) for _, t, _ in images], np.int32),
                all_runs=all_runs, all_n_runs=all_n_runs, all_dets=all_dets, all_count=np.array([len(p) for _, _, p in images], np.int32),
                im_size=np.array([s for s, _, _ in images], np.float32), out_stride=out_stride, iou_thresh=iou_thresh,
                binarize_thresh=binarize_thresh)


def real_ovr(case):
    """entry 2 on (top, all) without crowd, by the restatement"""
    return mr.overlaps(case["top_runs"], case["top_n_runs"], case["top_count"], case["all_runs"], case["all_n_runs"], case["all_count"],
                       case["im_size"], False)["ovr"]


# ---- tiny ------------------------------------------------------------------------------------------------------------------------------------------
def tiny():
    """7 x 5 and 5 x 7 images in one batch: the fourteen list shapes of segm_eval_cases.tiny, each as top and as voter; supports that
    cover the image, are empty, end at a negative slice index, come from negative and fractional coordinates; a negative score; tops
    of area 0, with one voter, with no voter"""
    src = sc.tiny()
    images = []
    for n, (h, w) in enumerate(((7, 5), (5, 7))):
        shapes = [(src["det_runs"][n, j].copy(), int(src["det_n_runs"][n, j])) for j in range(14)]
        boxes = [
            ((0, 0, w - 1, h - 1), 0.9),                         # the whole image
            ((3, 3, 1, 1), 0.8),                                 # x_0 = 3 > x_1 = 2: an empty support
            ((2, 0, -5, h - 1), 0.7),                            # b2 = -5: x_1 = -4 counts from the far edge: columns 2 .. w - 5
            ((-0.5, -0.9, 2.7, 3.9), 0.6),                       # truncation: (0, 0, 2, 3)
            ((0, 0, -0.5, -0.3), 0.95),                          # truncated: the pixel (0, 0); floored: b2 = b3 = -1: no support
            ((1, 1, 3, 3), -0.4),                                # a negative score: 1e-5 everywhere
            ((-3, 2, 1.9, h + 4), 0.3), ((1, -2, w + 3, 2), 0.55),
        ]
        pool = [(shapes[j], boxes[j % len(boxes)][0], boxes[j % len(boxes)][1]) for j in range(14)]
        # four more voters that make the supports matter: near copies of shapes with other boxes
        extra = [([0, h * w], boxes[4][0], boxes[4][1]), ([h + 2, 3 * h - 1, h * w - 4 * h - 1], boxes[2][0], 0.2),
                 ([1] * (h * w), boxes[0][0], 0.45), ([0, h * w], boxes[1][0], 0.5)]
        pool += extra
        lone = [17, 1, h * w - 18]                               # a top no voter overlaps
        images.append(((h, w), shapes + [lone], pool))
    return vote_case(images, T=16, A=20, top_stride=36, all_stride=40, out_stride=36, iou_thresh=0.2, binarize_thresh=0.5, seed=11)


# ---- threshold -------------------------------------------------------------------------------------------------------------------------------------
def threshold_vote():
    """a crafted ovr: values one float64 ulp below, at and above iou_thresh, NaN; a 3-voter pixel with num / den exactly
    binarize_thresh (weights 0.25 / 0.25 / 0.5, threshold 0.5).  -> (case, ovr); run it at binarize_thresh 0.5 and at the float64
    below it, where the pixels at equality are one ulp above the threshold"""
    h = w = 4
    px = lambda on: sc.runs_of(np.isin(np.arange(16), on).reshape(w, h).T)
    whole = (0, 0, 3, 3)
    pool = [(px([0, 1, 2, 3]), whole, 0.25), (px([2, 3, 4, 5]), whole, 0.25), (px([3, 5, 6, 7]), whole, 0.5),
            (px([8, 9, 10, 11]), whole, 1.0), (px(list(range(16))), whole, 0.3)]
    tops = [px([0, 1, 2, 3])] * 4
    case = vote_case([((h, w), tops, pool)], T=5, A=6, top_stride=6, all_stride=6, out_stride=8, iou_thresh=0.3, binarize_thresh=0.5, seed=12)
    t = 0.3
    lo, hi, nan = np.nextafter(t, 0), np.nextafter(t, 1), np.nan
    ovr = np.full((1, 5, 6), 0.9)                               # the rows and columns past the counts would vote
    ovr[0, :4, :5] = [[t, t, t, lo, nan],                       # voters 0, 1, 2: pixels 2, 6, 7 sit at num / den = 0.5
                      [hi, lo, lo, hi, nan],                    # voters 0, 3
                      [t, lo, nan, lo, lo],                     # one voter: copied
                      [lo, nan, lo, lo, lo]]                    # none: copied
    return case, ovr


def threshold_nms(seed=0):
    """a crafted, asymmetric "crowd" matrix and a symmetric one: values one float64 ulp below, at and above thresh, NaN; equal scores
    (row order decides), a NaN score, two classes.  -> dict(dets, count, crowd, iou, thresh)"""
    rs = np.random.RandomState(seed)
    R, t = 12, 0.5
    values = [0.1, np.nextafter(t, 0), t, np.nextafter(t, 1), 0.9, np.nan, 0.3, 0.45]
    crowd = rs.choice(values, (1, R, R), p=[0.2, 0.15, 0.15, 0.15, 0.1, 0.05, 0.1, 0.1])
    iou = np.minimum(crowd, crowd.transpose(0, 2, 1))           # symmetric, as a real IoU matrix is
    dets = np.full((1, R, 6), np.nan, np.float32)
    dets[0, :, 5] = 1.0
    dets[0, :10, 4] = [0.9, 0.8, 0.8, 0.7, np.nan, 0.6, 0.6, 0.6, 0.95, 0.5]
    dets[0, :10, 5] = [1, 1, 1, 1, 1, 1, 1, 1, 2, 2]
    return dict(dets=dets, count=np.array([10], np.int32), crowd=crowd, iou=iou, thresh=t)


# ---- order -----------------------------------------------------------------------------------------------------------------------------------------
ORDER_SCORES = [np.float32(1.0), np.float32(0.1), np.float32(0.2), np.float32(0.3)]


def order_weights():
    """the voters' weights of the order case: 1e-5 (a voter without support) and the float32 scores"""
    return [mr.FLOOR] + [float(s) for s in ORDER_SCORES]


def order_search():
    """-> (subset of voters that have the pixel, binarize_thresh): the first subset for which num / den added in voter order and in
    reverse order differ; the threshold is the smaller of the two, so exactly one order turns the pixel on"""
    ws = order_weights()
    for r in range(1, len(ws)):
        for on in itertools.combinations(range(len(ws)), r):
            ratio = []
            for order in (range(len(ws)), range(len(ws) - 1, -1, -1)):
                num = den = 0.0
                for k in order:
                    num, den = num + ws[k] * (1.0 if k in on else 0.0), den + ws[k]
                ratio.append(num / den)
            if ratio[0] != ratio[1]:
                return on, min(ratio)
    raise AssertionError("no subset tells the orders apart")


def order():
    """five voters of weights 1e-5, 1.0, 0.1f, 0.2f, 0.3f on a 4 x 8 image whose pixel p is set in the voters of the bits of p: every
    subset of voters is a pixel.  iou_thresh 0: every row below the count votes"""
    h, w = 4, 8
    _, bt = order_search()
    whole = (0, 0, w - 1, h - 1)
    bits = lambda k: sc.runs_of(np.array([(p >> k) & 1 for p in range(32)], bool).reshape(w, h).T)
    pool = [(bits(0), (5, 5, 2, 2), 0.5)] + [(bits(k + 1), whole, float(s)) for k, s in enumerate(ORDER_SCORES)]
    return vote_case([((h, w), [bits(0), bits(3)], pool)], T=3, A=6, top_stride=33, all_stride=33, out_stride=33, iou_thresh=0.0,
                     binarize_thresh=bt, seed=13)


# ---- chunks ----------------------------------------------------------------------------------------------------------------------------------------
def _list_of(n_runs, hw, rs, ends_at=()):
    """a run list of exactly n_runs runs that sums to hw, some run ends on the given positions"""
    cuts = set(ends_at)
    while len(cuts) < n_runs - 1:
        cuts.add(int(rs.randint(1, hw)))
    cuts = sorted(cuts)
    return np.diff([0] + cuts + [hw]).tolist()


def chunks():
    """32 x 40 = 5 chunks of 256 pixels.  Pool: 130 near copies of one blob (the 130 voters of top 0), then lists of 64, 65, 128 and
    129 runs with run ends on the chunk borders, then combs; T = A = 200, counts 180.  out_stride is the second largest need: the
    longest voted list does not fit, another fits exactly."""
    rs = np.random.RandomState(14)
    h, w = 32, 40
    hw = h * w
    yy, xx = np.mgrid[0:h, 0:w]
    blob = ((yy - 15) / 11.0) ** 2 + ((xx - 18) / 14.0) ** 2 <= 1.0
    blob[0, 0] = True                                           # the walk starts at position 0: chunks end at multiples of 256
    pool = []
    box = lambda: (int(rs.randint(-4, 20)), int(rs.randint(-4, 16)), int(rs.randint(15, 44)), int(rs.randint(12, 36)))
    for k in range(130):
        m = blob.copy()
        m[rs.randint(0, h, 6), rs.randint(0, w, 6)] ^= True
        m[0, 0] = True
        pool.append((sc.runs_of(m), box(), float(np.float32(rs.rand()))))
    for n_runs in (64, 65, 128, 129):
        for rep in range(5):
            lst = [0] + _list_of(n_runs - 1, hw, rs, ends_at=(256, 512, 768, 1024)[:2 + rep % 3])     # position 0 is set
            pool.append((lst, box(), float(np.float32(rs.rand()))))
    while len(pool) < 180:                                      # combs of different phase: their vote is longer than any of them
        phase = len(pool) % 4
        pool.append(([phase] + [2, 3] * 64, box(), float(np.float32(rs.rand()))))
    tops = [p[0] for p in pool]
    case = vote_case([((h, w), tops, pool)], T=200, A=200, top_stride=300, all_stride=280, out_stride=300, iou_thresh=0.25,
                     binarize_thresh=0.4, seed=14)
    need = np.unique(mr.vote(case, real_ovr(case), 'AVG')["need"][0, :180])
    case["out_stride"] = int(need[-2])
    return case


# ---- large -----------------------------------------------------------------------------------------------------------------------------------------
def large():
    """one 800 x 1333 image with six blob masks and boxes past 2^16 positions"""
    rs = np.random.RandomState(15)
    h, w = 800, 1333
    yy, xx = np.mgrid[0:h, 0:w]
    pool = []
    for k in range(6):
        cy, cx, ry, rx = 400 + 30 * k, 900 + 25 * (k % 3), 120 + 10 * k, 150 - 8 * k
        m = ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0
        m[cy - 20:cy + 20, cx - 5 * k:cx + 9] &= rs.rand(40, 9 + 5 * k) < 0.7
        pool.append((sc.runs_of(m), (cx - rx + 10 * k, cy - ry - 7, cx + rx - 30, cy + ry // 2), 0.9 - 0.13 * k))
    tops = [p[0] for p in pool]
    stride = max(len(t) for t in tops) + 3
    return vote_case([((h, w), tops, pool)], T=7, A=8, top_stride=stride, all_stride=stride + 5, out_stride=stride + 200, iou_thresh=0.5,
                     binarize_thresh=0.5, seed=15)


def huge():
    """one 30000 x 30000 pair, for dtc_mpost_boxes and dtc_mpost_overlaps only: too large to decode, the answers come from
    segm_eval_ref.interval_counts and mask_post_ref.interval_box"""
    hw = 30000 * 30000
    a = [[1000, hw - 1000], [12345, hw - 12345]]
    b = [[hw - 7, 7], [29999 * 30000 + 5, 3, 29992], [0, 30000, hw - 30000]]
    a_runs, a_n = pack_lists([a], 3, 4, 16)
    b_runs, b_n = pack_lists([b], 4, 3, 17)
    return dict(a_runs=a_runs, a_n_runs=a_n, a_count=np.array([2], np.int32), b_runs=b_runs, b_n_runs=b_n, b_count=np.array([3], np.int32),
                im_size=np.array([[30000, 30000]], np.float32))


# ---- boxes -----------------------------------------------------------------------------------------------------------------------------------------
def boxes():
    """5 x 4 and 3 x 6: a single pixel in each corner, a full column, a run that wraps a column boundary (y-bounds 0 and h - 1), a full
    image, an empty mask, zero-length runs in front, a list short of the image, one past it.  -> (runs, n_runs, counts, im_size, names)"""
    images, names = [], None
    for h, w in ((5, 4), (3, 6)):
        hw = h * w
        rows = {
            "corner_00": [0, 1, hw - 1], "corner_h0": [h - 1, 1, hw - h], "corner_0w": [hw - h, 1, h - 1], "corner_hw": [hw - 1, 1],
            "full_column": [h, h, hw - 2 * h], "wraps": [2 * h - 1, 2, hw - 2 * h - 1], "full": [0, hw], "empty": [hw], "no_runs": [],
            "zero_runs_in_front": [0, 0, 0, 0, h + 1, 1, hw - h - 2], "two_columns_inside": [h + 1, 1, h, 1, hw - 2 * h - 3],
            "short": [1, 2], "past": [hw - 2, 7, 3, 4], "count_negative": ([0, hw], -1),
        }
        names = sorted(rows)
        images.append([rows[k] for k in names])
    runs, n_runs = pack_lists(images, 16, 8, 18)
    return runs, n_runs, np.array([14, 14], np.int32), np.array([(5, 4), (3, 6)], np.float32), names


# ---- the bridge: filled integer rectangles ---------------------------------------------------------------------------------------------------------
def rects(seed=19, R=30, thresh=0.301):
    """30 filled integer rectangles in a 40 x 50 image, clustered so that box NMS at `thresh` suppresses many.  -> dict(boxes f32
    [R,4], scores f32 [R], runs, n_runs, count, im_size, thresh)"""
    rs = np.random.RandomState(seed)
    h, w = 40, 50
    b = np.zeros((R, 4), np.float32)
    for k in range(R):
        cx, cy = (12, 10) if k % 3 == 0 else ((30, 25) if k % 3 == 1 else (20, 30))
        x1, y1 = cx + rs.randint(-4, 5), cy + rs.randint(-4, 5)
        b[k] = (x1, y1, x1 + rs.randint(6, 14), min(y1 + rs.randint(5, 9), h - 1))
    scores = rs.permutation(R).astype(np.float32) / R
    runs, n_runs = pack_lists([[sc.rect_runs(h, *[int(v) for v in box]) for box in b]], R + 2, 2 * 14 + 2, seed)
    return dict(boxes=b, scores=scores, runs=runs, n_runs=n_runs, count=np.array([R], np.int32), im_size=np.array([[h, w]], np.float32),
                thresh=thresh)


VOTE_CASES = {"tiny": tiny, "order": order, "chunks": chunks, "large": large}
