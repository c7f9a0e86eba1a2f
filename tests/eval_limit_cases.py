"""dtc_eval_match / dtc_segm_match, dtc_eval_accumulate, dtc_eval_proposal_recall and dtc_segm_iou at the limits of their contracts
(test support, not a test module): the "limits" sections of tests/README_eval.md and tests/README_segm_eval.md list the cases.  Built
from eval_cases.build / segm_eval_cases.pack, deterministic from fixed seeds, made once and never modified.
tests/test_eval_limits_host.py pins on the CPU the condition every case is there for, tests/test_hip_eval_limits.py launches them,
tests/golden/make_eval_limits_golden.py records the reference's evaluate_box_proposals on the proposal cases
(tests/golden/eval_limits.npz).

The launch arithmetic the conditions speak of: the match kernels run one 64-lane wave per (image, class), lane a * T + t, the
matched-gt mask of a lane is four 64-bit words over the class's gt POSITIONS (row order), the visiting order is a byte list; the
accumulate kernel stages a class's segment of the sorted rows in tiles of 256; the proposal kernel and the pair kernel of
dtc_segm_iou give gt row g to thread g of four waves and compact across them; the prepare kernel of dtc_segm_iou scans a run list
in chunks of 64 runs.
"""
import functools

import numpy as np

import coco_eval_ref as cr
import eval_cases as ec
import segm_eval_cases as sc

f32 = np.float32
BASE_SEED = 20261020 + 3000
TILE = 256                                                    # csrc/eval/eval_accumulate.hip: kAccTile
REC11 = np.linspace(0, 1, 11)
EDGE_POS = (0, 63, 64, 127, 128, 191, 192, 255)               # the ends of the four words of the matched-gt mask


def _params(iou=(0.5, 0.75), rec=REC11, max_dets=(1, 10, 100), areas=((0, 1e10), (20.0, 1e10))):
    return np.asarray(iou, np.float64), np.asarray(rec, np.float64), tuple(max_dets), np.asarray(areas, np.float64)


def _freeze(case):
    for v in case.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return case


def up(v, dtype=f32):
    return dtype(np.nextafter(dtype(v), dtype(np.inf)))


def down(v, dtype=f32):
    return dtype(np.nextafter(dtype(v), dtype(-np.inf)))


# ---- 1. full_gt ------------------------------------------------------------------------------------------------------------------------------
def _grid_gt(j, cls=1):
    """gt j of a 16 x 16 grid: 5 x 5 pixels, every third 4 x 4 (out of the second area range), one in seventeen crowd"""
    x, y, s = 7.0 * (j % 16), 7.0 * (j // 16), 4 if j % 3 == 1 else 5
    return (x, y, x + s - 1, y + s - 1, cls, int(j % 17 == 6), None)


@functools.lru_cache(maxsize=None)
def full_gt():
    """G = 256.  Image 0: all 256 rows of class 1, a detection equal to the gt at each of EDGE_POS and 40 jittered ones; image 1:
    gt_counts = 300, classes alternating; image 2: gt_counts = -4 over 256 rows that would count"""
    rs = np.random.RandomState(BASE_SEED + 1)

    def jittered(g, n, classes):
        out = []
        for _ in range(n):
            x1, y1, x2, y2, c = g[rs.randint(len(g))][:5]
            out.append((x1 + rs.randint(-1, 2), y1, x2, y2 + rs.randint(-1, 2), round(float(rs.rand()), 2),
                        c if classes is None else int(rs.choice(classes))))
        return out

    g0 = [_grid_gt(j) for j in range(256)]
    d0 = [g0[j][:4] + (0.99 - 0.01 * i, 1) for i, j in enumerate(EDGE_POS)] + jittered(g0, 40, None) + jittered(g0, 5, [2])
    g1 = [_grid_gt(j, 1 + j % 2) for j in range(256)]
    d1 = jittered(g1, 20, None)
    d2 = jittered(g0, 6, [1, 2])
    case = ec.build([(d0, g0, None), (d1, g1, None), (d2, g0, None)], num_classes=3, max_out=64, G=256, params=_params())
    case["gt_counts"][1], case["gt_counts"][2] = 300, -4
    return _freeze(case)


# ---- 2. full_dets ----------------------------------------------------------------------------------------------------------------------------
SCORE_VALUES = (0.05, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)
FULL_DETS = {"one_1": (False, 1), "one_100": (False, 100), "one_512": (False, 512), "one_600": (False, 600), "two_512": (True, 512)}


@functools.lru_cache(maxsize=None)
def full_dets(name):
    """max_out = det_count = 512 in image 0: one class, or a second class on every third row (the compaction ballots are partial at
    every 64-row border); scores from ten values; max_det = 1, 100, 512 and 600"""
    two, max_det = FULL_DETS[name]
    rs = np.random.RandomState(BASE_SEED + 2)
    g = [(12.0 * j, 0, 12.0 * j + 9, 9 + j % 3, 1 + (j % 2 if two else 0), int(j == 5), None) for j in range(12)]
    d = []
    for j in range(512 + 30):
        c = 2 if two and j % 3 == 0 else 1
        k = rs.choice([i for i in range(12) if g[i][4] == c])
        d.append((12.0 * k + rs.randint(-2, 3), 0, 12.0 * k + 9, 9 + rs.randint(-2, 3), SCORE_VALUES[rs.randint(10)], c))
    max_dets = {1: (1,), 100: (1, 10, 100), 512: (1, 100, 512), 600: (1, 100, 600)}[max_det]
    return _freeze(ec.build([(d[:512], g, None), (d[512:], g, None)], num_classes=3, max_out=512, G=12,
                            params=_params(max_dets=max_dets, areas=((0, 1e10), (0, 105.0)))))


# ---- 3. all_lanes ----------------------------------------------------------------------------------------------------------------------------
ALL_LANES = ((4, 16), (16, 4), (64, 1), (1, 1))


@functools.lru_cache(maxsize=None)
def all_lanes(T, A):
    """a small random case at T * A = 64 (lane 63 and bit 63 in use), A = 16 (bit 15 of gt_ignore) and T = A = 1"""
    iou = np.linspace(0.3, 0.95, T) if T > 1 else [0.5]
    areas = [((6.0 * a) ** 2, (40.0 + 25.0 * a) ** 2) for a in range(A - 1)] + [(900.0, 40000.0)]
    return _freeze(ec.random_case(BASE_SEED % 1000 + 3, params=_params(iou=iou, areas=areas)))


# ---- 4. score_bits ---------------------------------------------------------------------------------------------------------------------------
TINY, FMAX = f32(np.nextafter(f32(0), f32(1))), np.finfo(f32).max
SCORES = (f32(0.0), f32(-0.0), TINY, -TINY, f32(-0.0), f32(0.0), FMAX, -FMAX, f32(-1.5), f32(-0.25), f32(0.5), up(0.5), down(0.5),
          f32(1.0), up(1.0), -TINY, TINY, down(-1.5), up(FMAX * f32(0.5)), f32(1e-38), f32(-1e-38))


@functools.lru_cache(maxsize=None)
def score_bits():
    """class 1 of four images holds SCORES, rotated from image to image (equal keys within and across images): +0 and -0 in both row
    orders, the smallest subnormals of either sign, +-FLT_MAX, negative scores, neighbours one float32 ulp apart"""
    rs = np.random.RandomState(BASE_SEED + 4)
    g = [(30.0 * j, 0, 30.0 * j + 19, 19, 1 + (j == 5), 0, None) for j in range(6)]
    images = []
    for n in range(4):
        s = SCORES[3 * n:] + SCORES[:3 * n]
        d = [(30.0 * (i % 5) + rs.randint(-3, 4), 0, 30.0 * (i % 5) + 19, 19 + rs.randint(-3, 4), s[i], 1) for i in range(len(s))]
        d += [(150.0, 0, 169.0, 19, f32(-0.0), 2), (150.0, 0, 169.0, 18, f32(0.0), 2)]
        images.append((d, g, None))
    case = ec.build(images, num_classes=3, max_out=24, G=8, params=_params(max_dets=(1, 10, 100), areas=((0, 1e10), (0, 390.0))))
    assert np.array_equal(case["dets"][0, :len(SCORES), 4].view(np.uint32), np.asarray(SCORES, f32).view(np.uint32))
    return _freeze(case)


def run_at(case, image_base):
    """coco_eval_ref.run with the image_base of the call"""
    out = cr.run(case)
    ev = cr.evaluate(case["dets"], case["det_count"], case["gt_boxes"], case["gt_classes"], case["gt_is_crowd"], case["gt_counts"],
                     case.get("gt_area"), case["num_classes"], case["iou_thrs"], case["area_rngs"], case["max_dets"][-1])
    out["sort_key"] = cr.records(ev, case["dets"], case["det_count"], case["gt_boxes"].shape[1], case["num_classes"], len(case["iou_thrs"]),
                                 len(case["area_rngs"]), image_base)["sort_key"]
    return out


# ---- 5. threshold_edges ----------------------------------------------------------------------------------------------------------------------
THRESHOLDS = {"sorted": (0.0, 0.5, 1.0, 1.5), "unsorted": (0.5, 0.0, 1.5, 0.5, 1.0)}
EDGE_AREAS = ((0, 1e10), (400.0, 400.0), (400.0, 900.0), (900.0, 400.0))
UNMATCHED_SIDES = ((21, 19), (20, 20), (401, 1), (29, 31), (30, 30), (17, 53))          # areas 399, 400, 401, 899, 900, 901


@functools.lru_cache(maxsize=None)
def threshold_edges(name):
    """thresholds 0 (a disjoint gt matches), >= 1 (an identical box matches); area ranges lo = hi = a gt's exact area, gt_area on lo,
    on hi and one float32 ulp outside each, unmatched detections of area 399 .. 901, a range with lo > hi"""
    box = lambda x, y, w, h: (float(x), float(y), float(x + w - 1), float(y + h - 1))
    gt_area = (None, 900.0, down(400.0), up(400.0), down(900.0), up(900.0))
    g = [box(50 * j, 0, 20 if j in (0, 2, 3) else 30, 20 if j in (0, 2, 3) else 30) + (1, 0, gt_area[j]) for j in range(6)]
    d = [g[0][:4] + (0.95, 1), box(50, 0, 30, 15) + (0.9, 1)] + [g[j][:4] + (0.9 - 0.05 * j, 1) for j in range(2, 6)]
    d += [box(0, 100 + 60 * i, w, h) + (0.5 - 0.05 * i, 1) for i, (w, h) in enumerate(UNMATCHED_SIDES)]       # disjoint from every gt
    g.append(box(0, 50, 10, 10) + (2, 0, None))
    d.append(box(300, 50, 10, 10) + (0.5, 2))                                         # class 2: one gt, one disjoint detection
    d1 = [box(0, 60 * i, w, h) + (0.3, 1) for i, (w, h) in enumerate(UNMATCHED_SIDES[:3])]     # image 1: no gt at all
    return _freeze(ec.build([(d, g, None), (d1, [], None)], num_classes=3, max_out=16, G=8,
                            params=_params(iou=THRESHOLDS[name], areas=EDGE_AREAS)))


@functools.lru_cache(maxsize=None)
def area_fraction():
    """boxes only: unmatched detections whose float64 box area is 400 / 900 exactly, and with y2 one float32 ulp above / below: just
    outside lo = hi = 400 and the ends of [400, 900]"""
    d = [(0, 0, 19, y2, 0.9 - 0.1 * i, 1) for i, y2 in enumerate((19.0, up(19.0), down(19.0)))]
    d += [(0, 0, 29, y2, 0.5 - 0.1 * i, 1) for i, y2 in enumerate((29.0, up(29.0), down(29.0)))]
    return _freeze(ec.build([(d, [(500, 500, 519, 519, 1, 0, None)], None)], num_classes=2, max_out=8, G=2,
                            params=_params(iou=(0.5,), areas=EDGE_AREAS)))


# ---- 6. degenerate_boxes (boxes only) ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def degenerate_boxes():
    """w = 0 (x2 = x1 - 1) and w = -4 (x2 = x1 - 5), likewise h, on detections and on gt, each overlapping an ordinary box in the
    other axis; thresholds 0 and 0.5; an area range [-100, 0] that holds their areas"""
    g = [(10, 10, 29, 29, 1, 0, None),
         (50, 10, 49, 29, 2, 0, None), (60, 10, 55, 29, 2, 0, None), (50, 40, 69, 39, 2, 0, None), (80, 40, 99, 35, 2, 1, None),
         (120, 10, 139, 29, 2, 0, None)]
    d = [(15, 10, 14, 29, 0.9, 1), (15, 10, 10, 29, 0.8, 1), (10, 15, 29, 14, 0.7, 1), (10, 15, 29, 10, 0.6, 1), (15, 15, 11, 11, 0.5, 1),
         (10, 10, 29, 28, 0.4, 1),
         (45, 10, 64, 29, 0.9, 2), (50, 35, 99, 44, 0.8, 2), (50, 10, 49, 29, 0.7, 2), (60, 10, 55, 29, 0.6, 2), (120, 10, 139, 29, 0.5, 2)]
    return _freeze(ec.build([(d, g, None)], num_classes=3, max_out=12, G=8,
                            params=_params(iou=(0.0, 0.5), areas=((0, 1e10), (-100.0, 0.0), (1.0, 1e10)))))


# ---- 7. class_column -------------------------------------------------------------------------------------------------------------------------
DET_CLASSES = (0.99, 1.0, 2.7, 3.5, 4.0, -1.0, 1e30, np.nan, 2.0, 3.0, 1.0)           # num_classes = 4: K = 3, K + 0.5, num_classes
GT_CLASSES = (1, 0, 2, -3, 3, 4, -(1 << 31), 1)


@functools.lru_cache(maxsize=None)
def class_column():
    """class values inside the counts that belong to no class, on boxes that would match if they were read; 2.7 and 3.5 truncate"""
    g = [(0, 0, 19, 19, 1, 0, None) for j in range(len(GT_CLASSES))]
    d = [(0, 0, 19, 18 + i % 2, 0.9 - 0.05 * i, 1.0) for i in range(len(DET_CLASSES))]
    case = ec.build([(d, g, None)], num_classes=4, max_out=12, G=8, params=_params(areas=((0, 1e10), (0, 390.0))))
    case["dets"][0, :len(DET_CLASSES), 5] = np.asarray(DET_CLASSES, f32)
    case["gt_classes"][0, :len(GT_CLASSES)] = np.asarray(GT_CLASSES, np.int64).astype(np.int32)
    return _freeze(case)


def crafted_from_boxes(case):
    """-> (iou, det_area, gt_mask_area) for dtc_segm_match from the box protocol's own IoU, where the boxes cannot be rectangles of
    pixels: every pair inside the counts, NaN past them; the detections' areas are integers here"""
    N, max_out = case["dets"].shape[:2]
    G = case["gt_boxes"].shape[1]
    iou = np.full((N, max_out, G), np.nan)
    det_area, gt_mask_area = np.full((N, max_out), 1 << 30, np.int32), np.full((N, G), -1, np.int32)
    for n in range(N):
        nd, ng = min(max(int(case["det_count"][n]), 0), max_out), min(max(int(case["gt_counts"][n]), 0), G)
        for d in range(nd):
            b = cr.xywh(case["dets"][n, d, :4])
            assert b[2] * b[3] == int(b[2] * b[3])
            det_area[n, d] = int(b[2] * b[3])
            for g in range(ng):
                iou[n, d, g] = cr.bb_iou(b, cr.xywh(case["gt_boxes"][n, g]), bool(case["gt_is_crowd"][n, g]))
    return iou, det_area, gt_mask_area


def bridge(case):
    """segm_eval_cases.from_boxes with the case's own gt_counts (above G, negative) kept"""
    b, s = sc.from_boxes(case)
    s["gt_counts"][:] = b["gt_counts"]
    return b, s


# ---- 8. segment_lengths (accumulate) ----------------------------------------------------------------------------------------------------------
SEG_LENGTHS = (0, 1, 255, 256, 257, 512, 513)                 # classes 1 .. 7; class 8: detections and npig = 0 (its only gt is crowd)


@functools.lru_cache(maxsize=None)
def segment_lengths():
    """52 images; class c <= 7 has exactly SEG_LENGTHS[c - 1] detections left by the max_det = 10 cut (every other full image has two
    more, cut); the rows of an image are shuffled over the classes; max_dets = (100, 1, 10)"""
    rs = np.random.RandomState(BASE_SEED + 8)
    left = dict(zip(range(1, 8), SEG_LENGTHS))
    images = []
    for n in range(52):
        g = [(40.0 * c, 0, 40.0 * c + 29, 29, c, int(c == 8), None) for c in range(1, 9)]
        rows = []
        for c in range(2, 8):
            keep = min(10, left[c])
            left[c] -= keep
            rows += [c] * (keep + (2 if keep == 10 and n % 2 == 0 else 0))
        rows += [8] * (3 if n % 5 == 0 else 0)
        rs.shuffle(rows)
        d = [(40.0 * c + rs.randint(-4, 5), rs.randint(0, 4), 40.0 * c + 29, 29 + rs.randint(-4, 5), round(float(rs.rand()), 2), c) for c in rows]
        images.append((d, g, None))
    assert not any(left.values())
    return _freeze(ec.build(images, num_classes=9, max_out=64, G=12, params=_params(max_dets=(100, 1, 10), areas=((0, 1e10), (0, 1000.0)))))


@functools.lru_cache(maxsize=None)
def all_padding():
    """two images with gt and det_count = 0: every row of the run is padding"""
    g = [(0, 0, 19, 19, 1, 0, None), (30, 0, 49, 19, 2, 0, None)]
    return _freeze(ec.build([([], g, None), ([], g, None)], num_classes=3, max_out=4, G=4, params=_params()))


@functools.lru_cache(maxsize=None)
def one_row():
    """rows = 1: one image with max_out = 1"""
    return _freeze(ec.build([([(0, 0, 19, 18, 0.5, 1)], [(0, 0, 19, 19, 1, 0, None)], None)], num_classes=2, max_out=1, G=1, params=_params()))


# ---- 9. recall_edges (accumulate) ------------------------------------------------------------------------------------------------------------
def edge_thresholds():
    """j / 10.0 for j = 0 .. 10 with the float64 neighbours of each, 0.5 twice, and two values above 1; non-decreasing"""
    v = [f(j / 10.0) for j in range(11) for f in (lambda x: down(x, np.float64), np.float64, lambda x: up(x, np.float64))]
    return np.sort(np.asarray(v + [0.5, 1.5, 2.0], np.float64))


RECALL_EDGES = ("r1", "r1024", "m16")


@functools.lru_cache(maxsize=None)
def recall_edges(name):
    """class 1: exactly 10 gt that count (and a crowd one) over two images, every gt found, false positives in between: every recall
    j / 10 is attained; class 2: a segment whose detections are all ignored (inside a crowd gt) next to a gt that counts"""
    rs = np.random.RandomState(BASE_SEED + 9)
    images = []
    for n in range(2):
        g = [(30.0 * j, 0, 30.0 * j + 19, 19, 1, 0, None) for j in range(5)] + [(0, 100, 99, 199, 1, 1, None)]
        g += [(0, 300, 99, 399, 2, 1, None), (300, 300, 319, 319, 2, 0, None)]
        d = [(30.0 * j, 0, 30.0 * j + 19, 19 - (j + n) % 2, round(0.95 - 0.09 * j - 0.04 * n, 2), 1) for j in range(5)]
        d += [(30.0 * j + 200, 200, 30.0 * j + 219, 219, round(0.9 - 0.13 * j - 0.02 * n, 2), 1) for j in range(5)]      # false positives
        d += [(10 + 5 * j, 310, 60 + 5 * j, 360, 0.5 + 0.1 * j, 2) for j in range(3)]
        order = rs.permutation(len(d))
        images.append(([d[i] for i in order], g, None))
    edges = edge_thresholds()
    fill = np.linspace(0, 1.2, 1024 - len(edges))
    rec, max_dets = {"r1": ([3 / 10.0], (1, 10, 100)), "r1024": (np.sort(np.concatenate([edges, fill])), (1, 10, 100)),
                     "m16": (edges, tuple(range(1, 17)))}[name]
    return _freeze(ec.build(images, num_classes=3, max_out=16, G=8, params=_params(rec=rec, max_dets=max_dets, areas=((0, 1e10), (390.0, 1e10)))))


MATCH_CASES = {"full_gt": full_gt, **{"full_dets_" + k: functools.partial(full_dets, k) for k in FULL_DETS},
               **{"all_lanes_%dx%d" % ta: functools.partial(all_lanes, *ta) for ta in ALL_LANES}, "score_bits": score_bits,
               **{"threshold_edges_" + k: functools.partial(threshold_edges, k) for k in THRESHOLDS},
               "area_fraction": area_fraction, "degenerate_boxes": degenerate_boxes, "class_column": class_column, "segment_lengths": segment_lengths,
               "all_padding": all_padding, "one_row": one_row, **{"recall_edges_" + k: functools.partial(recall_edges, k) for k in RECALL_EDGES}}
NOT_RECTANGLES = ("degenerate_boxes", "class_column")        # dtc_segm_match gets crafted_from_boxes there, bridge() elsewhere
BOX_ONLY = ("area_fraction",)                                # a fractional area: dtc_segm_match's det_area is an integer


# ---- 10. proposal recall ---------------------------------------------------------------------------------------------------------------------
PROPOSAL_AREAS = ("all", "medium")                            # [0, 1e10] and [32^2, 96^2]
SPLIT_ROWS = (63, 64, 127, 128, 191, 192)                     # the first and last threads of the wavefronts inside


def _jitter_props(rs, gt, n):
    out = np.zeros((n, 4), f32)
    for i in range(n):
        out[i] = np.asarray(gt[rs.randint(len(gt))][:4]) + rs.randint(-12, 13, 4)
    return out


def _noise_props(rs, n, span=3000, lo=10, hi=40):
    xy = rs.randint(0, span, (n, 2)).astype(f32)
    return np.concatenate([xy, xy + rs.randint(lo, hi, (n, 2))], 1).astype(f32)


def _grid_rows(rs, n=256):
    """n gt on a 16-wide grid, sides around 20, 50 and 110: 'medium' takes about a third"""
    out = []
    for j in range(n):
        s = (20, 50, 110)[j % 3] + rs.randint(-4, 5, 2)
        x, y = 130.0 * (j % 16), 130.0 * (j // 16)
        out.append((x, y, x + s[0], y + s[1], int(rs.randint(1, 5)), 0, float(s[0] * s[1] * rs.uniform(0.7, 1.0))))
    return out


def _leave_out(rs, rows, keep):
    """all but `keep` rows stop taking part -- crowd, class 0 (a proposal to the reference) or an area above every range -- SPLIT_ROWS
    first"""
    out = [r for r in SPLIT_ROWS] + [int(r) for r in rs.permutation(len(rows)) if r not in SPLIT_ROWS]
    rows = list(rows)
    for i, r in enumerate(out[:len(rows) - keep]):
        x1, y1, x2, y2, c, crowd, area = rows[r]
        rows[r] = [(x1, y1, x2, y2, c, 1, area), (x1, y1, x2, y2, 0, 0, area), (x1, y1, x2, y2, c, 0, 2e10)][i % 3]
    return rows


@functools.lru_cache(maxsize=None)
def proposal_cases():
    """name -> dict(roidb: what the reference is given (the proposals that count), n_gt: the gt rows of each entry, limit, and
    optionally device = (proposals [N, P, 4], prop_counts [N]) where the kernel's inputs are not the roidb's own, no_area)"""
    rs = np.random.RandomState(BASE_SEED + 10)
    cases = {}
    entry = lambda gt, props: ec.roidb_entry(gt, np.asarray(props, f32).reshape(-1, 4))

    # G = 256: G' = 256, 65, 128, 129, 255
    roidb = []
    for keep in (256, 65, 128, 129, 255):
        g = _grid_rows(rs)
        if keep == 256:
            # rows 10 and 200 tie on their best proposal (the smaller gt takes it); rows 11 and 201 are identical;
            # areas exactly on the ends of 'medium' and one float32 ulp outside
            g[10], g[200] = (3000, 3000, 3099, 3099, 1, 0, 5000.0), (3020, 3000, 3119, 3099, 1, 0, 5000.0)
            g[201] = g[11]
            for r, area in ((1, 1024.0), (2, 9216.0), (3, float(down(1024.0))), (4, float(up(9216.0)))):
                g[r] = g[r][:6] + (area,)
            p = np.concatenate([_jitter_props(rs, g[:10] + g[11:200], 296), np.asarray([(3010, 3000, 3109, 3099), (3000, 3000, 3099, 3149),
                                                                       (3020, 3000, 3119, 3129), g[11][:4]], f32)])
        elif keep == 255:
            g[64] = g[64][:5] + (1, g[64][6])
            p = _jitter_props(rs, g, 300)
        else:
            g = _leave_out(rs, g, keep)
            p = _jitter_props(rs, g, 300)
        roidb.append(entry(g, p))
    cases["g256"] = dict(roidb=roidb, n_gt=[256] * 5, limit=None)

    # P = 65536: six gt far apart whose best proposals sit at 0, 255, 256 and 65535 (and 70, 40000)
    g = [(400.0 * j, 3200.0, 400.0 * j + 99, 3299.0, 1 + j % 3, 0, 7000.0 + 500 * j) for j in range(6)]
    p = _noise_props(rs, 65536)
    for j, q in enumerate((0, 255, 256, 65535, 70, 40000)):
        p[q] = np.asarray(g[j][:4], f32) + (1 + j % 2, 0, 1, -1)
    cases["p65536"] = dict(roidb=[entry(g, p)], n_gt=[6], limit=None)

    # equal overlaps: gt A_i with a proposal 10 to its left at q and one 10 to its right at q + 1 / q + 64 / q + 256; the right one
    # is the better one for the gt B_i that overlaps A_i's right half, so the choice shows in B_i's round; and gt C_i with two
    # identical best proposals at the same distances
    g, p = [], _noise_props(rs, 1024)
    for i, (q, dq) in enumerate(((10, 1), (30, 64), (120, 256))):
        y = 400.0 * i
        g += [(100, y, 199, y + 99, 1, 0, 6000.0), (160, y, 259, y + 99, 2, 0, 6000.0), (600, y, 699, y + 99, 3, 0, 6000.0)]
        p[q], p[q + dq] = (90, y, 189, y + 99), (110, y, 209, y + 99)
        p[600 + q], p[600 + q + dq] = (600, y + 2, 699, y + 97), (600, y + 2, 699, y + 97)
    cases["ties"] = dict(roidb=[entry(g, p)], n_gt=[len(g)], limit=None)

    # G' = 200 with P' = 7
    g = _leave_out(rs, _grid_rows(rs), 200)
    g = [r if r[4] != 0 else r[:4] + (1, 1, r[6]) for r in g]                   # no class-0 row: they would be proposals
    cases["p7_g200"] = dict(roidb=[entry(g, _jitter_props(rs, [r for r in g if not r[5] and r[6] < 1e10], 7))], n_gt=[256], limit=None)

    # limit = 1 and limit = P
    g40 = ec._rand_gt(rs, 40)
    for name, limit in (("limit_1", 1), ("limit_p", 300)):
        cases[name] = dict(roidb=[entry(g40, ec._rand_props(rs, g40, 300)), entry(g40[:9], ec._rand_props(rs, g40, 300))], n_gt=[40, 9],
                           limit=limit)

    # prop_counts above P and negative: all P rows count; none does (the reference's entry has no proposal)
    p = np.asarray(ec._rand_props(rs, g40, 50), f32)
    cases["counts"] = dict(roidb=[entry(g40, p), entry(g40[:12], [])], n_gt=[40, 12], limit=None,
                           device=(np.stack([p, p]), np.asarray([50 + 1000, -5], np.int32)))

    # 100 gt around one box share their best proposal: every round retires it and every column left is scanned again
    base = np.asarray((500, 500, 699, 699))
    g = [tuple(float(v) for v in base + rs.randint(-6, 7, 4)) + (1, 0, 6000.0) for _ in range(100)]
    p = np.concatenate([[base], base + rs.randint(-60, 61, (299, 4)), _noise_props(rs, 724, span=1500, lo=50, hi=300)]).astype(f32)
    cases["shared_best"] = dict(roidb=[entry(g, p)], n_gt=[100], limit=None)

    # gt_area NULL: integer boxes whose float64 box area is the seg_area, 32 x 32 and 96 x 96 on the ends of 'medium'
    sides = ((32, 32), (96, 96), (32, 33), (31, 33), (96, 97), (95, 97), (50, 50), (10, 10))
    g = [(150.0 * j, 0.0, 150.0 * j + w - 1, h - 1.0, 1, int(j == 6), float(w * h)) for j, (w, h) in enumerate(sides)]
    cases["no_area"] = dict(roidb=[entry(g, _jitter_props(rs, g, 40))], n_gt=[len(g)], limit=None, no_area=True)
    for c in cases.values():
        for e in c["roidb"]:
            _freeze(e)
    return cases


# ---- 11. dtc_segm_iou ------------------------------------------------------------------------------------------------------------------------
SEGM_PARAMS = _params(areas=((0, 1e10), (0, 20.0)))
H, W = 16, 12
HW = H * W


def _blob_runs(rs):
    m = np.zeros((H, W), bool)
    y, x = rs.randint(0, H - 3), rs.randint(0, W - 3)
    m[y:y + rs.randint(2, 9), x:x + rs.randint(2, 7)] = True
    return sc.runs_of(m & (rs.rand(H, W) < 0.9))


@functools.lru_cache(maxsize=None)
def segm_full_gt():
    """G = 256 on a 16 x 12 image: 199 gt of class 1 among 57 of class 2 (pairs from all four wavefronts, neither list a multiple of
    4 long); max_out = 200, det_count = 180, det_n_runs negative at rows 63, 64, 130 and at row 185, past the count"""
    rs = np.random.RandomState(BASE_SEED + 11)
    g = [(_blob_runs(rs), 2 if j % 9 in (3, 7) else 1, int(j % 31 == 4), None) for j in range(256)]
    d = []
    for j in range(180):
        runs = _blob_runs(rs) if rs.rand() < 0.5 else g[rs.randint(256)][0]
        d.append(((runs, -1 - j % 3) if j in (63, 64, 130) else runs, round(float(rs.rand()), 2), 2 if j % 7 == 2 else 1))
    case = sc.pack([((H, W), d, g, None)], num_classes=3, max_out=200, G=256, params=SEGM_PARAMS, seed=BASE_SEED % 1000 + 11)
    case["det_n_runs"][0, 185] = -3
    return _freeze(case)


def one_runs(k):
    """k one-runs of one pixel, zero-length runs of zeros between them: 2 k runs"""
    return [3] + [1, 0] * (k - 1) + [1]


def reach(n, r, exact=False):
    """n runs whose prefix sum first reaches h * w at run r (exactly, or passing it); the runs behind lie outside the image"""
    return [1] * r + [HW - r + (0 if exact else 5)] + [2] * (n - r - 1)


def chunk_lists():
    lists = {"ones_%d" % k: one_runs(k) for k in (64, 65, 128)}
    for n, r in ((64, 63), (65, 63), (65, 64), (128, 63), (128, 64), (128, 127), (129, 64), (129, 127), (129, 128)):
        lists["reach_%d_%d" % (n, r)] = reach(n, r)
    lists["reach_exact_128_63"], lists["reach_exact_129_64"] = reach(128, 63, True), reach(129, 64, True)
    big = 0xffffffff
    for r in (63, 64):                                           # the prefix sum leaves 32 bits at run r: a wrapped sum would come back
        lists["past_2_32_at_%d" % r] = [1] * r + [big, 7, 9, 11]
        lists["past_2_32_summed_%d" % r] = [0] * (r - 3) + [1 << 30] * 4 + [5, 9, 20]
    lists["gt_zero_runs"] = [5, 3, 0, 0, 0, 4, 10, 6]            # ends 5 8 8 8 8 12 22 28: the end 8 four times
    lists["on_the_ends"] = [8, 4, 10, 6]                          # ones [8, 12) and [22, 28): start and end on the ends above
    lists["on_the_ends_2"] = [5, 3, 4, 10]                        # ones [5, 8) and [12, 22)
    return lists


@functools.lru_cache(maxsize=None)
def segm_chunks():
    """every list of chunk_lists() as a detection and as a gt of class 1; both strides 256 = the runs of ones_128"""
    lists = chunk_lists()
    names = sorted(lists)
    d = [(lists[k], round(0.95 - 0.03 * i, 2), 1) for i, k in enumerate(names)]
    g = [(lists[k], 1, int(k == "reach_65_64"), None) for k in names]
    assert max(len(v) for v in lists.values()) == 256
    return _freeze(sc.pack([((H, W), d, g, None)], num_classes=2, max_out=32, G=32, det_stride=256, gt_stride=256, params=SEGM_PARAMS,
                           seed=BASE_SEED % 1000 + 12))


IM_SIZES = ((7.9, 5.2), (0.5, 9), (np.nan, 9), (float(1 << 30), 1), (65536, 32768), (3e9, 1.5))


@functools.lru_cache(maxsize=None)
def segm_im_sizes():
    """im_size with fractions, below 1, NaN, h = 2^30, a product of 2^31 (clipped to 2^30) and a side above 2^30; masks of a few runs,
    some ending past the image.  Too large to decode: the answer comes from segm_eval_ref.interval_counts"""
    d = [([3, 9, 4, 1 << 29, 100, 1 << 29, 5, 1 << 30], 0.9, 1), ([0, 20, 1 << 28, 7], 0.8, 1)]
    g = [([5, 12, 1 << 29, 3000, 1 << 29, 1 << 29], 1, 0, None), ([0, 35], 1, 1, None), ([2, 1 << 31, 5], 1, 0, None)]
    return _freeze(sc.pack([(size, d, g, None) for size in IM_SIZES], num_classes=2, max_out=3, G=4, params=SEGM_PARAMS,
                           seed=BASE_SEED % 1000 + 13))


SEGM_CASES = {"segm_full_gt": (segm_full_gt, None), "segm_chunks": (segm_chunks, None), "segm_im_sizes": (segm_im_sizes, "interval")}
