"""The cases of the evaluation tests (tests/README_eval.md), shared by the host tests, the GPU tests and the golden generator.
Match / accumulate cases are dicts of numpy arrays in the layout of include/detectorch_eval_hip.h; the rows past the counts hold
NaN boxes and scores, and classes that would count if they were read."""
import numpy as np

import coco_eval_ref as cr


def build(images, num_classes=4, max_out=16, G=12, params=None):
    """images: [(dets [(x1,y1,x2,y2,score,cls)], gts [(x1,y1,x2,y2,cls,crowd,area or None)], det_count or None)]"""
    N = len(images)
    dets = np.full((N, max_out, 6), np.nan, np.float32)
    dets[:, :, 5] = 1.0                                        # a padding row of class 1: must not count
    gt_boxes = np.full((N, max(G, 1), 4), np.nan, np.float32)[:, :G]
    gt_area = np.full((N, G), np.nan, np.float32)
    gt_classes, gt_is_crowd = np.ones((N, G), np.int32), np.zeros((N, G), np.int32)
    det_count, gt_counts = np.zeros(N, np.int32), np.zeros(N, np.int32)
    for n, (d, g, count) in enumerate(images):
        d = np.asarray(d, np.float32).reshape(-1, 6)[:max_out]
        dets[n, :len(d)] = d
        det_count[n] = len(d) if count is None else count
        gt_counts[n] = len(g)
        for j, (x1, y1, x2, y2, c, crowd, area) in enumerate(g):
            gt_boxes[n, j] = (x1, y1, x2, y2)
            gt_classes[n, j], gt_is_crowd[n, j] = c, crowd
            w, h = np.float32(x2).astype(np.float64) - np.float32(x1).astype(np.float64) + 1.0, \
                np.float32(y2).astype(np.float64) - np.float32(y1).astype(np.float64) + 1.0
            gt_area[n, j] = w * h if area is None else area
    iou_thrs, rec_thrs, max_dets, area_rngs = params or cr.coco_params()
    return dict(dets=dets, det_count=det_count, gt_boxes=np.ascontiguousarray(gt_boxes), gt_classes=gt_classes, gt_is_crowd=gt_is_crowd,
                gt_counts=gt_counts, gt_area=gt_area, num_classes=num_classes, iou_thrs=np.asarray(iou_thrs, np.float64),
                rec_thrs=np.asarray(rec_thrs, np.float64), max_dets=tuple(max_dets), area_rngs=np.asarray(area_rngs, np.float64))


def ulp(v, up):
    return float(np.nextafter(np.float32(v), np.float32(np.inf if up else -np.inf)))


def exact_iou():
    """gt 10 x 10 / 10 x 20 / 10 x 20 with a detection of 10 x 5 / 10 x 15 / 10 x 19 inside: IoU exactly 1/2, 3/4, 19/20 (class 1), and
    the detection's y2 one float32 ulp below (class 2) and above (class 3)"""
    images = []
    for gh, dh in ((10, 5), (20, 15), (20, 19)):
        d, g = [], []
        for c, y2 in ((1, dh - 1.0), (2, ulp(dh - 1.0, False)), (3, ulp(dh - 1.0, True))):
            ox = 100.0 * c
            d.append((ox, 0, ox + 9, y2, 0.9, c))
            g.append((ox, 0, ox + 9, gh - 1.0, c, 0, None))
        images.append((d, g, None))
    return build(images)


def basic():
    """the engineered conditions, one per class and image"""
    im0_d = [
        (0, 0, 19, 19, 0.9, 1),                                # two identical gt: the later one wins
        (100, 100, 139, 139, 0.8, 2), (105, 105, 134, 134, 0.7, 2), (110, 110, 129, 129, 0.7, 2),   # three inside one crowd gt
        (300, 0, 309, 9, 0.6, 3),                              # matched to a small gt: ignored at medium and large
        (400, 400, 404, 404, 0.5, 3),                          # unmatched and small
        (0, 300, 299, 599, 0.5, 3),                            # unmatched and large; equal score
    ]
    im0_g = [(0, 0, 19, 19, 1, 0, None), (0, 0, 19, 19, 1, 0, None), (90, 90, 149, 149, 2, 1, None), (300, 0, 309, 9, 3, 0, None)]
    im1_d = [
        (0, 0, 59, 99, 0.9, 1),                                # IoU 0.6 with the plain gt, 1.0 with the crowd one behind it: stays
        (200, 200, 239, 239, 0.9, 2),                          # gt_area 900 against a 40 x 40 box: small, not medium
        (300, 300, 389, 389, 0.5, 2),                          # gt_area 10000 against a 90 x 90 box: large, not medium
        (500, 500, 520, 520, 0.5, 3),                          # class 3: detections and no gt
    ]
    im1_g = [(0, 0, 99, 99, 1, 0, None), (0, 0, 59, 99, 1, 1, None), (200, 200, 239, 239, 2, 0, 900.0), (300, 300, 389, 389, 2, 0, 10000.0)]
    im2_d = []                                                 # det_count 0; class 1: gt and no detection
    im2_g = [(10, 10, 50, 50, 1, 0, None)]
    im3_d = [(0, 0, 30, 30, 0.9, 1), (0, 0, 31, 31, 0.9, 1), (5, 5, 60, 60, 0.5, 2)]      # gt_counts 0; scores equal across images
    return build([(im0_d, im0_g, None), (im1_d, im1_g, None), (im2_d, im2_g, None), (im3_d, [], None)])


def overflow():
    """det_count above max_out: the first max_out rows count"""
    rs = np.random.RandomState(3)
    g = [(20.0 * j, 0, 20.0 * j + 15, 15, 1 + j % 3, 0, None) for j in range(6)]
    d = [(20.0 * (j % 6) + rs.randint(0, 4), 0, 20.0 * (j % 6) + 15, 15, round(float(rs.rand()), 2), 1 + j % 3) for j in range(16)]
    return build([(d, g, 21), (d[:5], g, 5), (d[::-1], g[:3], 16)])


def random_case(seed, N=6, num_classes=4, max_out=16, G=12, n_det=14, params=None, classes=None):
    rs = np.random.RandomState(seed)
    images = []
    for n in range(N):
        g = []
        for j in range(rs.randint(0, min(G, 9) + 1)):
            s = float(rs.choice([12, 28, 31, 33, 60, 95, 97, 200]))
            x, y = float(rs.randint(0, 400)), float(rs.randint(0, 400))
            w, h = s + rs.randint(-2, 3), s + rs.randint(-2, 3)
            c = int(rs.randint(1, num_classes)) if classes is None else int(rs.choice(classes))
            g.append((x, y, x + w - 1, y + h - 1, c, int(rs.rand() < 0.15), None if rs.rand() < 0.6 else float(w * h * rs.uniform(0.5, 1.1))))
        d = []
        for j in range(rs.randint(0, n_det + 1)):
            if g and rs.rand() < 0.75:
                x1, y1, x2, y2, c = g[rs.randint(len(g))][:5]
                j4 = rs.randint(-6, 7, 4) * (rs.rand() < 0.8)
                box = (x1 + j4[0], y1 + j4[1], x2 + j4[2], y2 + j4[3])
                c = c if rs.rand() < 0.85 else int(rs.randint(1, num_classes))
            else:
                x, y = float(rs.randint(0, 400)), float(rs.randint(0, 400))
                box, c = (x, y, x + rs.randint(5, 150), y + rs.randint(5, 150)), int(rs.randint(1, num_classes))
            d.append(box + (round(float(rs.rand()), 1), c))
        images.append((d, g, None))
    return build(images, num_classes, max_out, G, params)


def many_gt():
    """33 gt of class 1 and 65 of class 2 in one image: across the words of the matched-gt bitmask"""
    rs = np.random.RandomState(11)
    g = [(12.0 * (j % 33), 40.0 * (j // 33), 12.0 * (j % 33) + 10, 40.0 * (j // 33) + 30, 1 if j < 33 else 2, int(j % 17 == 5), None)
         for j in range(98)]
    d = []
    for j in range(60):
        x1, y1, x2, y2, c = g[rs.randint(98)][:5]
        d.append((x1 + rs.randint(-1, 2), y1, x2, y2 + rs.randint(-3, 4), round(float(rs.rand()), 2), c))
    d += [g[32][:4] + (0.99, 1), g[97][:4] + (0.99, 2)]         # the last gt of either class is matched
    return build([(d, g, None), (d[:7], g[:40], None), ([], g[30:], None)], num_classes=3, max_out=64, G=100)


def many_dets():
    """130 detections of one class in one image with max_out = 160: past the max_det cut at 100"""
    rs = np.random.RandomState(12)
    g = [(30.0 * j, 0, 30.0 * j + 25, 25, 1, 0, None) for j in range(10)]
    d = [(30.0 * (j % 10) + rs.randint(-3, 4), rs.randint(0, 5), 30.0 * (j % 10) + 25, 25, round(float(rs.rand()), 2), 1) for j in range(130)]
    d += [(5, 5, 40, 40, 0.5, 2)] * 20
    return build([(d, g, None), (d[:9], g, None)], num_classes=3, max_out=160, G=12)


def long_segment():
    """one class with 3000 detections over 30 images: past one tile of the accumulate scan"""
    return random_case(21, N=30, num_classes=3, max_out=100, G=12, n_det=0, classes=[1]) | _dense_dets(21)


def _dense_dets(seed):
    base = random_case(seed, N=30, num_classes=3, max_out=100, G=12, n_det=0, classes=[1])
    rs = np.random.RandomState(seed + 1)
    dets = np.zeros((30, 100, 6), np.float32)
    for n in range(30):
        ng = int(base["gt_counts"][n])
        for j in range(100):
            if ng and rs.rand() < 0.6:
                b = base["gt_boxes"][n, rs.randint(ng)] + rs.randint(-4, 5, 4)
            else:
                x, y = rs.randint(0, 400, 2)
                b = (x, y, x + rs.randint(5, 120), y + rs.randint(5, 120))
            dets[n, j] = tuple(b) + (round(float(rs.rand()), 3), 1)
    return dict(dets=dets, det_count=np.full(30, 100, np.int32))


def nondefault():
    """T = 3, A = 2, max_dets = (2, 5)"""
    params = (np.array([0.3, 0.5, 0.85]), np.linspace(0, 1, 11), (2, 5), np.array([[0, 1e10], [900.0, 40000.0]]))
    return random_case(31, params=params)


def box_area_case():
    """gt_area absent: the area of a gt is its box area"""
    c = random_case(7)
    del c["gt_area"]
    return c


def max_classes():
    """num_classes = 1024, the limit: the last class's segment of the sorted keys ends at the padding keys, which sort right behind it;
    seven detections of class 1023 in one image, two of them cut by max_det = 5"""
    params = (np.array([0.3, 0.5, 0.85]), np.linspace(0, 1, 11), (2, 5), np.array([[0, 1e10], [900.0, 40000.0]]))
    g = [(10, 10, 59, 59, 1023, 0, None), (100, 10, 139, 49, 1023, 0, None), (200, 200, 260, 260, 1, 0, None), (300, 0, 340, 40, 512, 0, None)]
    d = [(10 + j, 10, 59, 59 + j, 0.9 - 0.1 * j, 1023) for j in range(5)] + [(100, 10, 139, 49, 0.35, 1023), (400, 400, 450, 450, 0.95, 1023),
                                                                         (200, 200, 260, 258, 0.5, 1), (300, 0, 340, 41, 0.5, 512), (0, 0, 5, 5, 0.1, 1022)]
    return build([(d, g, None), (d[5:], g[:2], None), ([], g, None)], num_classes=1024, params=params)


MATCH_CASES = {"max_classes": max_classes, "box_area": box_area_case, "exact_iou": exact_iou, "basic": basic, "overflow": overflow, "random": lambda: random_case(7), "many_gt": many_gt,
               "many_dets": many_dets, "long_segment": long_segment, "nondefault": nondefault}


# ---- proposal recall ---------------------------------------------------------------------------------------------------------------------
AREAS = ('all', 'small', 'medium', 'large', '96-128', '128-256', '256-512', '512-inf')


def roidb_entry(gt, props):
    """gt: [(x1,y1,x2,y2,cls,crowd,seg_area)], props: [(x1,y1,x2,y2)] -> the roidb dict: gt rows first, then the proposals (class 0)"""
    gt, props = list(gt), np.asarray(props, np.float32).reshape(-1, 4)
    boxes = np.concatenate([np.asarray([g[:4] for g in gt], np.float32).reshape(-1, 4), props])
    z = np.zeros(len(props))
    return dict(boxes=boxes, gt_classes=np.concatenate([[g[4] for g in gt], z]).astype(np.int32),
                is_crowd=np.concatenate([[g[5] for g in gt], z]).astype(bool),
                seg_areas=np.concatenate([[g[6] for g in gt], z]).astype(np.float32))


def _rand_gt(rs, n, sizes=(20, 50, 110, 120, 200, 300, 600)):
    out = []
    for _ in range(n):
        s = float(rs.choice(sizes))
        x, y = float(rs.randint(0, 500)), float(rs.randint(0, 500))
        w, h = s + rs.randint(-5, 6), s + rs.randint(-5, 6)
        out.append((x, y, x + w, y + h, int(rs.randint(1, 5)), 0, float(w * h * rs.uniform(0.6, 1.0))))
    return out


def _rand_props(rs, gt, n):
    out = []
    for _ in range(n):
        if gt and rs.rand() < 0.7:
            b = np.asarray(gt[rs.randint(len(gt))][:4]) + rs.randint(-15, 16, 4)
        else:
            x, y = rs.randint(0, 600, 2)
            b = np.array([x, y, x + rs.randint(10, 400), y + rs.randint(10, 400)])
        out.append(tuple(float(v) for v in b))
    return out


def proposal_cases():
    """name -> (roidb, limit)"""
    rs = np.random.RandomState(5)
    cases = {}
    g = _rand_gt(rs, 7)
    cases["fewer_proposals"] = ([roidb_entry(g, _rand_props(rs, g, 3)), roidb_entry(g[:5], _rand_props(rs, g, 2))], None)
    cases["more_proposals"] = ([roidb_entry(g, _rand_props(rs, g, 40)), roidb_entry(g[:2], _rand_props(rs, g, 9))], None)
    cases["no_proposals"] = ([roidb_entry(g, []), roidb_entry(g[:3], _rand_props(rs, g, 5))], None)
    cases["no_gt"] = ([roidb_entry([], _rand_props(rs, [], 6)), roidb_entry(g[:3], _rand_props(rs, g, 5))], None)
    p = _rand_props(rs, g, 6)
    cases["duplicates"] = ([roidb_entry(g[:3] + g[:3] + [g[1]], p + p + [g[1][:4], g[1][:4]])], None)
    far = [(900.0, 900.0, 950.0, 950.0, 1, 0, 2000.0)]
    cases["zero_overlap_late"] = ([roidb_entry(g[:3] + far, _rand_props(rs, g[:3], 12))], None)
    cases["limit_below"] = ([roidb_entry(g, _rand_props(rs, g, 30))], 4)
    cases["limit_above"] = ([roidb_entry(g, _rand_props(rs, g, 30))], 1000)
    mixed = [g[0], g[1][:4] + (0, 0, g[1][6]), g[2][:5] + (1, g[2][6]), g[3], g[4][:5] + (1, g[4][6]), g[5]]
    # a gt_classes == 0 row among the gt is a proposal to the reference: roidb_entry keeps the row order, so it leads the proposals
    cases["crowd_and_class0"] = ([roidb_entry(mixed, _rand_props(rs, g, 20))], None)
    g40 = _rand_gt(rs, 40)
    cases["p600_g40"] = ([roidb_entry(g40, _rand_props(rs, g40, 600)), roidb_entry(g40[:11], _rand_props(rs, g40, 300))], None)
    # limit = 0 keeps no proposal (boxes[:0]): an image with proposals still records a zero per gt, one without records nothing
    cases["limit_zero"] = ([roidb_entry(g, _rand_props(rs, g, 8)), roidb_entry(g[:4], [])], 0)
    return cases
