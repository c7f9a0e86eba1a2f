"""The cases of the mask-evaluation tests (tests/README_segm_eval.md), shared by the host and the GPU tests.  A case is a dict of numpy
arrays in the layout of include/detectorch_segm_hip.h; run lists are uint32.  The rows past the counts hold garbage runs, run counts
that are huge or negative, and classes that would count if they were read."""
import numpy as np

import coco_eval_ref as cr
import eval_cases as ec


def pack(images, num_classes=3, max_out=8, G=6, det_stride=None, gt_stride=None, params=None, seed=0):
    """images: [((h, w), dets [(runs, score, cls)], gts [(runs, cls, crowd, area or None)], det_count or None)]; runs: a list of run
    lengths, or (runs, n_runs) to give a count of its own (negative, zero, past the list)"""
    rs = np.random.RandomState(seed)
    N = len(images)
    own = lambda r: r if isinstance(r, tuple) else (r, len(r))
    longest = lambda rows: max([1] + [len(own(r[0])[0]) for _, d, g, _ in images for r in rows(d, g)])
    det_stride = det_stride or longest(lambda d, g: d)
    gt_stride = gt_stride or longest(lambda d, g: g)
    dets = np.full((N, max_out, 6), np.nan, np.float32)
    dets[:, :, 5] = 1.0                                        # a padding row of class 1: must not count
    det_runs = rs.randint(0, 1 << 32, (N, max_out, det_stride), dtype=np.uint64).astype(np.uint32)
    det_n_runs = rs.choice([-(1 << 31), -7, 5, 1 << 30, (1 << 31) - 1], (N, max_out)).astype(np.int32)
    gt_runs = rs.randint(0, 1 << 32, (N, G, gt_stride), dtype=np.uint64).astype(np.uint32)
    gt_n_runs = rs.choice([-(1 << 31), -7, 5, 1 << 30, (1 << 31) - 1], (N, G)).astype(np.int32)
    gt_classes, gt_is_crowd = np.ones((N, G), np.int32), np.zeros((N, G), np.int32)
    gt_area = np.full((N, G), np.nan, np.float32)
    det_count, gt_counts, im_size = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros((N, 2), np.float32)
    any_area = False
    for n, (size, d, g, count) in enumerate(images):
        im_size[n] = size
        det_count[n] = len(d) if count is None else count
        gt_counts[n] = len(g)
        for j, (runs, score, c) in enumerate(d[:max_out]):
            runs, k = own(runs)
            det_runs[n, j, :len(runs)], det_n_runs[n, j] = np.asarray(runs, np.uint32), k
            dets[n, j, 4:] = (score, c)
        for j, (runs, c, crowd, area) in enumerate(g):
            runs, k = own(runs)
            gt_runs[n, j, :len(runs)], gt_n_runs[n, j] = np.asarray(runs, np.uint32), k
            gt_classes[n, j], gt_is_crowd[n, j] = c, crowd
            if area is not None:
                gt_area[n, j], any_area = area, True
    iou_thrs, rec_thrs, max_dets, area_rngs = params or cr.coco_params()
    case = dict(dets=dets, det_count=det_count, det_runs=det_runs, det_n_runs=det_n_runs, im_size=im_size, gt_runs=gt_runs,
                gt_n_runs=gt_n_runs, gt_classes=gt_classes, gt_is_crowd=gt_is_crowd, gt_counts=gt_counts, num_classes=num_classes,
                iou_thrs=np.asarray(iou_thrs, np.float64), rec_thrs=np.asarray(rec_thrs, np.float64), max_dets=tuple(max_dets),
                area_rngs=np.asarray(area_rngs, np.float64))
    if any_area:
        case["gt_area"] = gt_area
    return case


def runs_of(mask):
    """a [h, w] bitmap -> COCO's run lengths (column-major, zeros first)"""
    flat = np.asarray(mask, bool).reshape(-1, order='F')
    change = np.flatnonzero(flat[1:] != flat[:-1]) + 1
    runs = np.diff(np.concatenate([[0], change, [flat.size]])).tolist()
    return [0] + runs if flat.size and flat[0] else runs


# area ranges that tell tiny masks apart: all, up to 5 pixels, 6 .. 20, above 20
TINY_PARAMS = (cr.coco_params()[0], cr.coco_params()[1], (1, 10, 100), np.array([[0, 1e10], [0, 5], [5, 20], [20, 1e10]]))


def tiny():
    """7 x 5 and 5 x 7 images in one batch: the shapes of a run list, each both as a detection and as a gt"""
    def shapes(h, w):
        hw = h * w
        return {
            "no_runs": [], "one_run_of_zeros": [hw], "full": [0, hw], "first_pixel": [0, 1, hw - 1], "last_pixel": [hw - 1, 1],
            "alternating": [1] * hw,                             # n_runs = h * w
            "zero_first_alternating": [0] + [1] * (hw - 1) + [0],     # hw + 1 runs: the first and the last of length zero
            "across_columns": [h + 2, 3 * h - 1, hw - 4 * h - 1],        # one run of ones through four columns
            "zero_runs_inside": [3, 4, 0, 2, 5, 0, 0, 6, 1],         # 3 zeros, 4 + 2 ones joined by an empty run of zeros, ...
            "short_of_the_image": [2, 5, 3, 4],                       # ends at 14: the rest is zeros
            "past_the_image": [hw - 6, 4, 1, 100, 7, 9],               # the fourth run is cut at h * w, the rest is nothing
            "past_in_64_bits": [10, 0xffffffff, 0xffffffff, 5],       # the prefix sum leaves 32 bits
            "count_zero": ([0, hw], 0), "count_negative": ([0, hw], -3),    # a full mask whose count says: empty
        }
    images = []
    for size in ((7, 5), (5, 7)):
        s = shapes(*size)
        names = sorted(s)
        stride = size[0] * size[1] + 1
        # class 1: every shape against every shape; class 2: a few, with a crowd gt; the rows past the counts are pack()'s garbage
        d = [(s[k], 0.9 - 0.05 * j, 1) for j, k in enumerate(names)]
        g = [(s[k], 1, int(k == "full"), None) for k in names]
        d += [(s["across_columns"], 0.5, 2), (s["full"], 0.4, 2), (s["alternating"], 0.3, 7), (s["alternating"], 0.3, 0)]
        g += [(s["alternating"], 2, 1, None), (s["across_columns"], 2, 0, None), (s["full"], 3, 0, None), (s["full"], 0, 0, None)]
        images.append((size, d, g, None))
        assert len(s["zero_first_alternating"]) == stride
    # det stride 36 = the longest list exactly (n_runs == runs_stride); gt stride larger: the strides differ
    return pack(images, num_classes=4, max_out=20, G=20, det_stride=36, gt_stride=40, params=TINY_PARAMS, seed=1)


def random_masks(seed=5):
    """37 x 53 random masks at densities 0.1 / 0.5 / 0.9: hundreds to about 1000 runs; detection and gt strides differ"""
    rs = np.random.RandomState(seed)
    h, w = 37, 53
    images = []
    for n in range(2):
        gm = [rs.rand(h, w) < p for p in (0.1, 0.5, 0.9, 0.5)]
        g = [(runs_of(m), 1 + j % 2, int(j == 3), None) for j, m in enumerate(gm)]
        d = []
        for j, p in enumerate((0.1, 0.5, 0.9, 0.5, 0.9, 0.1)):
            m = rs.rand(h, w) < p
            if j % 2:
                m |= gm[j % 4] & (rs.rand(h, w) < 0.8)           # overlaps a gt well
            d.append((runs_of(m), round(float(rs.rand()), 2), 1 + j % 2))
        images.append(((h, w), d, g, None))
    return pack(images, num_classes=3, max_out=8, G=5, det_stride=1200, gt_stride=1100, seed=2)


def _rect_minus_line(h, w, x1, y1, x2, y2, line_x):
    m = np.zeros((h, w), bool)
    m[y1:y2 + 1, x1:x2 + 1] = True
    m[:, line_x] = False
    return runs_of(m)


def large():
    """one 800 x 1333 pair of rectangles minus a line: positions and areas past 2^16, few runs per column"""
    h, w = 800, 1333
    d = [(_rect_minus_line(h, w, 100, 50, 900, 700, 400), 0.9, 1)]
    g = [(_rect_minus_line(h, w, 300, 100, 1200, 799, 650), 1, 0, None)]
    return pack([((h, w), d, g, None)], num_classes=2, max_out=2, G=2, seed=3)


def huge():
    """one 30000 x 30000 pair of two-run masks: an intersection near 9e8 (32-bit integer sums, not floats).  Too large to decode:
    its answer comes from segm_eval_ref.interval_counts"""
    hw = 30000 * 30000
    d = [([1000, hw - 1000], 0.9, 1)]
    g = [([12345, hw - 12345], 1, 0, None), ([hw - 7, 7], 1, 1, None)]
    return pack([((30000, 30000), d, g, None)], num_classes=2, max_out=2, G=3, seed=4)


def counts_case():
    """class mismatches, an image with gt_counts = 0 and one with det_count = 0, det_count above max_out, and masks that did not fit
    (negative det_n_runs): counted in n_bad, scored as empty"""
    h, w = 9, 6
    full, half, dot = [0, 54], [0, 27, 27], [20, 1, 33]
    im0 = ((h, w), [(full, 0.9, 1), ((half, -40), 0.8, 1), (half, 0.7, 2), ((full, -1), 0.6, 2), (dot, 0.5, 3)],
           [(half, 1, 0, 2000.0), (full, 2, 0, 54.0), (dot, 1, 0, 2.0)], None)          # gt_area: COCO's annotation area, given
    im1 = ((h, w), [(full, 0.9, 1), (half, 0.8, 2)], [], None)                              # gt_counts 0
    im2 = ((h, w), [], [(half, 1, 0, 27.0), (full, 2, 1, 54.0)], None)                      # det_count 0
    im3 = ((h, w), [(half, 0.9 - 0.1 * j, 1 + j % 2) for j in range(6)], [(half, 1, 0, 27.0), (dot, 2, 0, 1.0)], 9)    # det_count 9 > 6
    im4 = ((h, w), [((full, -2), 0.9, 1)] * 3, [(full, 1, 0, 54.0)], -5)                   # a negative det_count: no row, none bad
    return pack([im0, im1, im2, im3, im4], num_classes=4, max_out=6, G=3, seed=5)


def stream_case(seed, N=6):
    """N images of 24 x 17 with noisy blobs, three classes, some crowd gt, gt_area given: a whole small evaluation, for the evaluator
    (chunks, graph replay, the result lists).  The strides are fixed so that cases of different seeds share their shapes."""
    rs = np.random.RandomState(seed)
    h, w = 24, 17
    yy, xx = np.mgrid[0:h, 0:w]

    def blob():
        cy, cx, ry, rx = rs.randint(3, h - 3), rs.randint(3, w - 3), rs.randint(2, 9), rs.randint(2, 7)
        return ((((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2) <= 1.0) & (rs.rand(h, w) < 0.9)

    images = []
    for n in range(N):
        gm = [blob() for _ in range(rs.randint(0, 6))]
        g = [(runs_of(m), int(rs.randint(1, 4)), int(rs.rand() < 0.2), float(m.sum() * rs.choice([1.0, 40.0, 400.0]))) for m in gm]
        d = []
        for j in range(rs.randint(0, 11)):
            if gm and rs.rand() < 0.75:
                k = rs.randint(len(gm))
                m = (gm[k] & (rs.rand(h, w) < 0.9)) | (blob() & (rs.rand(h, w) < 0.2))
                c = g[k][1] if rs.rand() < 0.85 else int(rs.randint(1, 4))
            else:
                m, c = blob(), int(rs.randint(1, 4))
            d.append((runs_of(m), round(float(rs.rand()), 1), c))
        d.sort(key=lambda r: r[2])                               # class-major rows, as the detection stage writes them
        images.append(((h, w), d, g, None))
    case = pack(images, num_classes=4, max_out=10, G=5, det_stride=160, gt_stride=150, params=STREAM_PARAMS, seed=seed)
    case["dets"][:, :, :4] = 0.0                                  # boxes are not read; zeros so that the result lists can carry them
    if "gt_area" not in case:
        case["gt_area"] = np.full((N, 5), np.nan, np.float32)
    return case


# area ranges in which the pixel counts of stream_case's blobs (and their multiples) spread
STREAM_PARAMS = (cr.coco_params()[0], cr.coco_params()[1], (1, 10, 100), np.array([[0, 1e10], [0, 60], [60, 2000], [2000, 1e10]]))

IOU_CASES = {"tiny": tiny, "random_masks": random_masks, "large": large, "counts": counts_case}


# ---- the bridge: filled integer rectangles, on which the segm protocol must equal the box protocol bit for bit -------------------------------
def exact_rects():
    """gt 10 x 10 / 10 x 20 / 10 x 20 with a detection of 10 x 5 / 10 x 15 / 10 x 19 inside: IoU exactly 1/2, 3/4, 19/20; and one pixel
    row less / more in classes 2 and 3: below and above"""
    images = []
    for gh, dh in ((10, 5), (20, 15), (20, 19)):
        d, g = [], []
        for c, dy in ((1, 0), (2, -1), (3, 1)):
            ox = 30.0 * c
            d.append((ox, 0, ox + 9, dh - 1.0 + dy, 0.9, c))
            g.append((ox, 0, ox + 9, gh - 1.0, c, 0, None))
        images.append((d, g, None))
    return ec.build(images)


# crowd, out-of-range areas, ties (basic); det_count above max_out (overflow); the max_det cut (many_dets); T = 3, A = 2 (nondefault)
BOX_CASES = {"exact_rects": exact_rects, "basic": ec.basic, "overflow": ec.overflow, "random": lambda: ec.random_case(7),
             "many_dets": ec.many_dets, "nondefault": ec.nondefault}


def rect_runs(h, x1, y1, x2, y2):
    """the run list of the filled rectangle [x1..x2] x [y1..y2] in an image of height h; a column-high rectangle gives zero-length
    runs of zeros between its columns"""
    runs = [x1 * h + y1]
    for x in range(x1, x2 + 1):
        runs += [y2 - y1 + 1, h - (y2 - y1 + 1)]
    return runs[:-1]


def from_boxes(box_case, shift=8, with_gt_area=True):
    """a box case whose boxes are integers -> (the box case moved by `shift` into the image, the segm case of the filled rectangles).
    with_gt_area False: neither has gt_area: the box area there, the mask's pixel count here."""
    b = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in box_case.items()}
    N, max_out = b["dets"].shape[:2]
    G = b["gt_boxes"].shape[1]
    b["dets"][:, :, :4] += shift
    b["gt_boxes"] += shift
    if not with_gt_area:
        b.pop("gt_area", None)
    size = 0
    rows = []
    for n in range(N):
        nd, ng = min(max(int(b["det_count"][n]), 0), max_out), min(max(int(b["gt_counts"][n]), 0), G)
        boxes = [b["dets"][n, d, :4] for d in range(nd)] + [b["gt_boxes"][n, g] for g in range(ng)]
        for box in boxes:
            assert np.all(box == np.round(box)) and box[0] >= 0 and box[1] >= 0 and box[2] >= box[0] and box[3] >= box[1], box
            size = max(size, int(box[2]) + 2, int(box[3]) + 2)
        rows.append((nd, ng))
    h = w = size
    images = []
    for n, (nd, ng) in enumerate(rows):
        d = [(rect_runs(h, *[int(v) for v in b["dets"][n, j, :4]]), float(b["dets"][n, j, 4]), float(b["dets"][n, j, 5])) for j in range(nd)]
        g = [(rect_runs(h, *[int(v) for v in b["gt_boxes"][n, j]]), int(b["gt_classes"][n, j]), int(b["gt_is_crowd"][n, j]),
              float(b["gt_area"][n, j]) if "gt_area" in b else None) for j in range(ng)]
        images.append(((h, w), d, g, int(b["det_count"][n])))
    s = pack(images, num_classes=b["num_classes"], max_out=max_out, G=G,
             params=(b["iou_thrs"], b["rec_thrs"], b["max_dets"], b["area_rngs"]), seed=6)
    for n, (nd, _) in enumerate(rows):
        s["dets"][n, :nd, :4] = b["dets"][n, :nd, :4]           # unused by the mask evaluation; the scores and classes are pack()'s
        assert np.array_equal(s["dets"][n, :nd, 4:], b["dets"][n, :nd, 4:])
    return b, s


# ---- crafted IoU matrices for dtc_segm_match -----------------------------------------------------------------------------------------------
def crafted(params=None, with_gt_area=False):
    """IoU matrices that no pair of masks need give: one float64 ulp below, at and above a threshold; equal IoU on two gt; the stop at
    an ignored gt; a crowd gt met again.  One class per condition, image 0; image 1: the same matrix with other areas."""
    iou_thrs, rec_thrs, max_dets, area_rngs = params or cr.coco_params()
    iou_thrs = np.asarray(iou_thrs, np.float64)
    N, max_out, G, num_classes = 2, 8, 8, 5
    t = float(iou_thrs[min(1, len(iou_thrs) - 1)])
    dets = np.full((N, max_out, 6), np.nan, np.float32)
    dets[:, :, 5] = 1.0
    iou = np.full((N, max_out, G), np.nan)                      # never read where the classes differ or past the counts
    det_area = np.full((N, max_out), 1 << 30, np.int32)
    gt_classes, gt_is_crowd = np.ones((N, G), np.int32), np.zeros((N, G), np.int32)
    gt_mask_area = np.full((N, G), -1, np.int32)
    for n in range(N):
        # class 1: three detections, three gt: below, at, above the threshold
        dets[n, 0:3, 4], dets[n, 0:3, 5] = (0.9, 0.8, 0.7), 1
        gt_classes[n, 0:3] = 1
        iou[n, 0:3, 0:3] = 0.0
        iou[n, 0, 0], iou[n, 1, 1], iou[n, 2, 2] = np.nextafter(t, 0), t, np.nextafter(t, 1)
        # class 2: one detection with the same IoU on two gt (the later one wins), a second that takes the one left
        dets[n, 3:5, 4], dets[n, 3:5, 5] = (0.9, 0.8), 2
        gt_classes[n, 3:5] = 2
        iou[n, 3:5, 3:5] = [[0.8, 0.8], [0.8, 0.6]]
        # class 3: a plain gt (IoU 0.6) in front of an ignored (crowd) one with IoU 1.0: the walk stops at the crowd gt above 0.6
        dets[n, 5:7, 4], dets[n, 5:7, 5] = (0.9, 0.5), 3
        gt_classes[n, 5:7], gt_is_crowd[n, 6] = 3, 1
        iou[n, 5:7, 5:7] = [[0.6, 1.0], [0.1, 0.9]]           # the second detection meets the crowd gt again
        # class 4: a detection without a gt, by area in one range or another
        dets[n, 7, 4:] = (0.5, 4)
        gt_classes[n, 7] = 1                                   # past gt_counts: would count in class 1
        det_area[n, :8] = (100, 100, 100, 2000, 2000, 20000, 20000, 500 if n == 0 else 5000)
        gt_mask_area[n, :7] = (100, 100, 100, 2000, 2000, 20000, 20000) if n == 0 else (100, 2000, 20000, 100, 2000, 100, 20000)
    case = dict(dets=dets, det_count=np.array([8, 8], np.int32), gt_classes=gt_classes, gt_is_crowd=gt_is_crowd,
                gt_counts=np.array([7, 7], np.int32), num_classes=num_classes, iou_thrs=iou_thrs, rec_thrs=np.asarray(rec_thrs, np.float64),
                max_dets=tuple(max_dets), area_rngs=np.asarray(area_rngs, np.float64))
    if with_gt_area:                                           # another area than the mask's: the ranges follow gt_area
        case["gt_area"] = np.where(gt_mask_area > 0, gt_mask_area * 12.5, np.nan).astype(np.float32)
    return case, iou, det_area, gt_mask_area


NONDEFAULT_PARAMS = (np.array([0.3, 0.5, 0.85]), np.linspace(0, 1, 11), (2, 5), np.array([[0, 1e10], [900.0, 40000.0]]))
