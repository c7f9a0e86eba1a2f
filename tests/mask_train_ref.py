"""The checker of mask training (test support, not a test module): the contract of include/detectorch_mask_hip.h restated serially in
numpy, one image at a time, with the seeded and hand-made CASES the golden generator and the tests use.

    raster        the RASTERISATION RULE of the header, the trace loop literally as written there (COCO's polygon-to-RLE and decode,
                  from the published algorithm; pycocotools is not available: parity unpinned)
    normalise     lib/utils/segms.py:99-110 (polys_to_mask_wrt_box) in float32
    poly_boxes    lib/utils/segms.py:120-131 (polys_to_boxes)
    targets       Detectron's add_mask_rcnn_blobs on the compact minibatch: rows, fallback, matching (bbox_overlaps of
                  tests/train_targets_ref.py), rasterisation, OR over the polygons
    even_odd      an independent check: the even-odd rule at pixel centres, written without the trace
    loss64        float64 yardsticks of dtc_mask_loss and its gradient

tests/test_mask_train_host.py pins the building blocks against the reference's own functions (tests/golden/mask_train.npz, made by
tests/golden/make_mask_train_golden.py); the GPU tests compare dtc_mask_targets and dtc_mask_loss with this module.
"""
import math

import numpy as np

from train_targets_ref import bbox_overlaps

EPS = 2.0 ** -24
BLOCK = 256                                    # csrc/mask_train: kMaskThreads
COORD_LIMIT = np.float32(2.0 ** 26)
MAX_M, MAX_GT, MAX_ROWS = 56, 256, 512
f32 = np.float32


# ---- rasterisation -------------------------------------------------------------------------------------------------------------------
def trace_events(xy, M):
    """xy: [n, 2] normalised points (float32 or float64).  -> the list of toggled column-major positions (those < M * M), in trace
    order.  The loop is the header's text, one trace point at a time."""
    h = w = M
    X = [int(5.0 * float(x) + 0.5) for x in xy[:, 0]]                            # int(): C's (int), toward zero
    Y = [int(5.0 * float(y) + 0.5) for y in xy[:, 1]]
    n, out = len(X), []
    for k in range(n):
        xs, ys, xe, ye = X[k], Y[k], X[(k + 1) % n], Y[(k + 1) % n]
        dx, dy = abs(xe - xs), abs(ye - ys)
        if dx == 0 and dy == 0:
            continue
        if dx >= dy:
            if xs > xe:
                xs, ys, xe, ye = xe, ye, xs, ys
            s = float(ye - ys) / dx
            pts = [(xs + t, int(ys + s * t + 0.5)) for t in range(dx + 1)]
        else:
            if ys > ye:
                xs, ys, xe, ye = xe, ye, xs, ys
            s = float(xe - xs) / dy
            pts = [(int(xs + s * t + 0.5), ys + t) for t in range(dy + 1)]
        for (u0, v0), (u1, v1) in zip(pts[:-1], pts[1:]):
            if u0 == u1:
                continue
            us, vs = min(u0, u1), min(v0, v1)
            if (us - 2) % 5 != 0:
                continue
            i = (us - 2) // 5
            if i < 0 or i > w - 1:
                continue
            j = int(math.ceil(min(max((vs + 0.5) / 5.0 - 0.5, 0.0), float(h))))
            if i * h + j < h * w:
                out.append(i * h + j)
    return out


def kernel_events(xy, M):
    """The events as csrc/mask_train/mask_targets.hip produces them (mask_edge_events restated line for line): closed form per pixel
    column when dx >= dy, a bisection on the monotone trace per column when dx < dy.  The same multiset as trace_events."""
    X = [int(5.0 * float(x) + 0.5) for x in xy[:, 0]]
    Y = [int(5.0 * float(y) + 0.5) for y in xy[:, 1]]
    n, out = len(X), []

    def toggle(i, vs):
        pos = i * M + int(math.ceil(min(max((vs + 0.5) / 5.0 - 0.5, 0.0), float(M))))
        if pos < M * M:
            out.append(pos)
    for k in range(n):
        xs, ys, xe, ye = X[k], Y[k], X[(k + 1) % n], Y[(k + 1) % n]
        dx, dy = abs(xe - xs), abs(ye - ys)
        if dx == 0 and dy == 0:
            continue
        if dx >= dy:
            if xs > xe:
                xs, ys, xe, ye = xe, ye, xs, ys
            s = float(ye - ys) / dx
            for i in range(max(0, (xs - 2 + 4) // 5), min(M - 1, (xe - 1 - 2) // 5) + 1):
                t = 5 * i + 2 - xs
                toggle(i, min(int(ys + s * t + 0.5), int(ys + s * (t + 1) + 0.5)))
        else:
            if ys > ye:
                xs, ys, xe, ye = xe, ye, xs, ys
            s = float(xe - xs) / dy
            u = lambda t: int(xs + s * t + 0.5)
            u0, u1 = u(0), u(dy)
            lo, hi, rising = min(u0, u1), max(u0, u1), u0 < u1
            for i in range(max(0, (lo - 2 + 4) // 5), min(M - 1, (hi - 1 - 2) // 5) + 1):
                c, a, z = 5 * i + 2, 0, dy
                while z - a > 1:
                    m = a + ((z - a) >> 1)
                    if (u(m) <= c) if rising else (u(m) > c):
                        a = m
                    else:
                        z = m
                if (u(a) if rising else u(z)) == c:
                    toggle(i, ys + a)
    return out


def raster(xy, M):
    """one polygon -> [M, M] uint8, row-major [y][x]"""
    tog = np.zeros(M * M, np.int64)
    for pos in trace_events(xy, M):
        tog[pos] ^= 1
    return (np.cumsum(tog) % 2).astype(np.uint8).reshape(M, M).T.copy()          # position x * h + y


def normalise(xy, box, M):
    """segms.py:99-110 in float32, one rounding per operation; xy [n, 2] float32, box [4] float32"""
    box = np.asarray(box, f32)
    w, h = np.maximum(box[2] - box[0], f32(1)), np.maximum(box[3] - box[1], f32(1))
    out = np.empty_like(xy, dtype=f32)
    with np.errstate(all="ignore"):
        out[:, 0] = ((xy[:, 0] - box[0]) * f32(M)) / w
        out[:, 1] = ((xy[:, 1] - box[1]) * f32(M)) / h
    return out


def even_odd(xy, M):
    """The even-odd rule at the pixel centres (x + 0.5, y + 0.5) on the float64 polygon: for each centre, the number of edges that
    cross the horizontal ray to its right.  Written without the trace."""
    p = np.asarray(xy, np.float64)
    q = np.roll(p, -1, axis=0)
    c = np.arange(M) + 0.5
    cx, cy = c[None, :, None], c[:, None, None]
    x0, y0, x1, y1 = p[:, 0], p[:, 1], q[:, 0], q[:, 1]
    straddle = (y0 <= cy) != (y1 <= cy)
    with np.errstate(all="ignore"):
        xi = x0 + (cy - y0) * (x1 - x0) / (y1 - y0)
    return ((straddle & (xi > cx)).sum(axis=2) % 2).astype(np.uint8)


# ---- the entry's contract for one image ----------------------------------------------------------------------------------------------
def poly_range(img, q):
    ps, pe = int(img["poly_ptr"][q]), int(img["poly_ptr"][q + 1])
    return (ps, pe) if ps >= 0 and pe <= len(img["poly_xy"]) and ps <= pe - 3 else None


def valid_polys(img, g):
    """the valid polygons of gt g as [n, 2] float32 arrays (None: the gt's own range is malformed)"""
    NP = len(img["poly_ptr"]) - 1
    q0, q1 = int(img["gt_poly_ptr"][g]), int(img["gt_poly_ptr"][g + 1])
    if not (q0 >= 0 and q1 <= NP and q0 <= q1):
        return None
    out = []
    for q in range(q0, q1):
        r = poly_range(img, q)
        if r is not None and np.isfinite(img["poly_xy"][r[0]:r[1]]).all():
            out.append(img["poly_xy"][r[0]:r[1]])
    return out


def poly_boxes(polys_per_gt):
    """segms.py:120-131 on lists of [n, 2] float32 arrays"""
    out = np.zeros((len(polys_per_gt), 4), f32)
    for i, polys in enumerate(polys_per_gt):
        out[i] = [min(p[:, 0].min() for p in polys), min(p[:, 1].min() for p in polys), max(p[:, 0].max() for p in polys),
                  max(p[:, 1].max() for p in polys)]
    return out


def fpn_level(box, k_min, k_max):
    """csrc/fpn_map.h (multilevel_rois.py:47-52) in float32, the logarithm in double rounded once"""
    with np.errstate(all="ignore"):
        area = (box[2] - box[0] + f32(1)) * (box[3] - box[1] + f32(1))
        s = np.sqrt(area)
        t = np.floor(f32(4) + f32(np.log2(np.float64(f32(s / f32(224)) + f32(1e-6)))))
    return int(min(max(t, f32(k_min)), f32(k_max))) if not np.isnan(t) else k_min


_raster_cache = {}


def row_mask(img, g, box, M):
    """the OR over the valid polygons of gt g, normalised to box -> [M * M] int32 in {0, 1}"""
    acc = np.zeros((M, M), np.uint8)
    for p in valid_polys(img, g):
        nv = normalise(p, box, M)
        if not (np.isfinite(nv).all() and (np.abs(nv) < COORD_LIMIT).all()):
            continue
        key = (nv.tobytes(), M)
        if key not in _raster_cache:
            _raster_cache[key] = raster(nv, M)
        acc |= _raster_cache[key]
    return acc.reshape(-1).astype(np.int32)


def targets(img, M, k_min, k_max, Fm, b=0):
    """img: dict(labels [R], keep_inds [R], n_rois, gt_boxes [G,4], gt_classes [G], gt_is_crowd [G], gt_count, proposals [P,4],
    im_scale, poly_xy [PTS,2], poly_ptr [NP+1], gt_poly_ptr [G+1]) -> the outputs of dtc_mask_targets for that image"""
    R, G, P = len(img["labels"]), len(img["gt_boxes"]), len(img["proposals"])
    n_r = min(max(int(img["n_rois"]), 0), R)
    n_g = min(max(int(img["gt_count"]), 0), G)
    labels = img["labels"]
    fg = [r for r in range(n_r) if labels[r] > 0]
    bg = [r for r in range(n_r) if labels[r] == 0]
    fallback = not fg and bool(bg)
    rows = [bg[0]] if fallback else fg[:Fm]
    out = dict(mask_rois=np.zeros((Fm, 5), f32), masks=np.full((Fm, M * M), -1, np.int32), mask_class=np.zeros(Fm, np.int32),
               mask_roi_levels=np.zeros(Fm, np.int32), roi_has_mask=np.zeros(R, np.int32), n_mask=np.int32(len(rows)),
               mask_gt=np.full(Fm, -1, np.int32))
    out["roi_has_mask"][rows] = 1
    has_polys = G > 0 and len(img["poly_ptr"]) > 1 and len(img["poly_xy"]) > 0
    elig = []
    for g in range(n_g):
        if has_polys and img["gt_classes"][g] > 0 and img["gt_is_crowd"][g] == 0 and valid_polys(img, g):
            elig.append(g)
    pboxes = poly_boxes([valid_polys(img, g) for g in elig]) if elig else np.zeros((0, 4), f32)
    scale = f32(img["im_scale"])
    for t, r in enumerate(rows):
        c = int(img["keep_inds"][r])
        box, have = np.zeros(4, f32), True
        if 0 <= c < n_g:
            box = img["gt_boxes"][c].astype(f32)
        elif c >= n_g and c - n_g < P:
            box = img["proposals"][c - n_g].astype(f32)
        else:
            have = False
        with np.errstate(all="ignore"):
            sb = (box * scale).astype(f32)
        out["mask_rois"][t] = [f32(b), sb[0], sb[1], sb[2], sb[3]]
        out["mask_class"][t] = 0 if fallback else labels[r]
        out["mask_roi_levels"][t] = 0 if k_min == k_max else fpn_level(sb, k_min, k_max) - k_min
        if have and not fallback and np.isfinite(box).all() and elig:
            ov = bbox_overlaps(box[None], pboxes)[0]
            g = elig[int(np.argmax(ov))]
            out["mask_gt"][t] = g
            out["masks"][t] = row_mask(img, g, box, M)
    return out


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
def pack(polys_per_gt, G=None, PTS=None, NP=None):
    """per gt a list of [n, 2] arrays -> (poly_xy [PTS,2] f32, poly_ptr [NP+1] i32, gt_poly_ptr [G+1] i32) of one image"""
    xy, ptr, gptr = [], [0], [0]
    for polys in polys_per_gt:
        for p in polys:
            p = np.asarray(p, f32).reshape(-1, 2)
            xy.append(p)
            ptr.append(ptr[-1] + len(p))
        gptr.append(len(ptr) - 1)
    G = len(polys_per_gt) if G is None else G
    xy = np.concatenate(xy, 0) if xy else np.zeros((0, 2), f32)
    PTS, NP = max(len(xy), 1) if PTS is None else PTS, max(len(ptr) - 1, 1) if NP is None else NP
    poly_xy = np.zeros((PTS, 2), f32)
    poly_xy[:len(xy)] = xy
    poly_ptr = np.full(NP + 1, ptr[-1], np.int32)
    poly_ptr[:len(ptr)] = ptr
    gt_poly_ptr = np.full(G + 1, gptr[-1], np.int32)
    gt_poly_ptr[:len(gptr)] = gptr
    return poly_xy, poly_ptr, gt_poly_ptr


def image(labels, keep_inds, gt_boxes, gt_classes, polys_per_gt, proposals, gt_is_crowd=None, im_scale=1.0, n_rois=None, gt_count=None):
    G = len(gt_boxes)
    poly_xy, poly_ptr, gt_poly_ptr = pack(polys_per_gt, G)
    return dict(labels=np.asarray(labels, np.int32), keep_inds=np.asarray(keep_inds, np.int32),
                n_rois=len(labels) if n_rois is None else n_rois, gt_boxes=np.asarray(gt_boxes, f32).reshape(G, 4),
                gt_classes=np.asarray(gt_classes, np.int32), gt_is_crowd=np.zeros(G, np.int32) if gt_is_crowd is None else
                np.asarray(gt_is_crowd, np.int32), gt_count=G if gt_count is None else gt_count,
                proposals=np.asarray(proposals, f32).reshape(-1, 4), im_scale=float(im_scale), poly_xy=poly_xy, poly_ptr=poly_ptr,
                gt_poly_ptr=gt_poly_ptr)


def rect(x0, y0, x1, y1):
    return np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]], f32)


def random_polygon(rs, cx, cy, r, n, star=False):
    """n points around (cx, cy); star: the angles are not sorted, so the polygon intersects itself"""
    a = rs.uniform(0, 2 * np.pi, n)
    if not star:
        a = np.sort(a)
    rad = r * rs.uniform(0.35, 1.0, n)
    return np.stack([cx + rad * np.cos(a), cy + rad * np.sin(a)], 1).astype(f32)


SEEDED = {"s1": (1, 1), "s2": (2, 2), "s7": (3, 7), "s14": (4, 14), "s28": (5, 28), "s56": (6, 56)}       # name -> (seed, M)
IM_W, IM_H = 200.0, 150.0


def seeded_image(name):
    """A random image: 4 gt (one crowd, one of class 0 among them on the larger seeds) of 1-3 polygons each, a third of the polygons
    self-intersecting and some reaching outside their RoIs; 12 minibatch rows: gt rows, jittered proposals, bg and padding."""
    seed, M = SEEDED[name]
    rs = np.random.RandomState(20261020 + seed)
    G, P = 4, 10
    polys, boxes = [], []
    for g in range(G):
        cx, cy, r = rs.uniform(40, IM_W - 40), rs.uniform(40, IM_H - 40), rs.uniform(12, 45)
        ps = [random_polygon(rs, cx + rs.uniform(-r, r) * (k > 0), cy + rs.uniform(-r, r) * (k > 0), r * (1.0 if k == 0 else 0.5),
                             rs.randint(3, 12), star=rs.rand() < 1 / 3.0) for k in range(rs.randint(1, 4))]
        polys.append(ps)
        allp = np.concatenate(ps)
        boxes.append([allp[:, 0].min(), allp[:, 1].min(), allp[:, 0].max(), allp[:, 1].max()])
    boxes = np.asarray(boxes, f32)
    cls = rs.randint(1, 81, G).astype(np.int32)
    crowd = np.zeros(G, np.int32)
    if seed >= 3:
        crowd[3] = 1
    if seed >= 5:
        cls[2] = 0
    src = rs.randint(0, G, P)
    jit = rs.uniform(-0.25, 0.25, (P, 4)) * np.stack([boxes[src, 2] - boxes[src, 0], boxes[src, 3] - boxes[src, 1]] * 2, 1)
    props = (boxes[src] + jit).astype(f32)
    labels = np.array([cls[0], cls[1], 5, 9, 13, 2, 77, 0, 0, 0, -1, -1], np.int32)
    keep = np.array([0, 1, G + 0, G + 1, G + 2, G + 3, G + 4, G + 5, G + 6, G + 7, -1, -1], np.int32)
    return image(labels, keep, boxes, cls, polys, props, gt_is_crowd=crowd, im_scale=1.5 if seed % 2 else 4.0, n_rois=10), M


def seeded_polygons(M, n=40, seed=0):
    """normalised polygons of the kind the seeded images hold, for the independent check: around the M x M grid, a third
    self-intersecting, many reaching outside it"""
    rs = np.random.RandomState(20261021 + seed + M)
    return [random_polygon(rs, rs.uniform(0, M), rs.uniform(0, M), rs.uniform(0.3 * M, 0.9 * M) + 1, rs.randint(3, 12),
                           star=rs.rand() < 1 / 3.0) for _ in range(n)]


# hand-made images: name -> (image, M, k_min, k_max, Fm)
def hand_cases():
    c = {}
    box = [10, 20, 38, 48]                                                       # w = h = 28: at M = 28 one pixel per unit
    one = lambda polys, M=28, bx=box, **kw: (image([3], [0], [bx], [3], [polys], np.zeros((0, 4)), **kw), M, 0, 0, 4)
    c["triangle"] = one([np.array([[12, 22], [36, 30], [20, 46]], f32)])
    # corners on the 1/5 grid: x in {2.4, 9.8} + 10, y in {3.2, 20.6} + 20
    c["rect_fifth"] = one([rect(12.4, 23.2, 19.8, 40.6)])
    c["rect_whole"] = one([rect(10, 20, 38, 48)])                                # covers the RoI: all one
    c["cover"] = one([rect(-100, -100, 300, 300)])
    c["outside"] = one([rect(100, 100, 130, 140)])                               # wholly outside: all zero
    c["negative"] = one([np.array([[7.3, 17.1], [30.2, 12.6], [44.9, 33.3], [21.7, 55.5], [3.1, 40.9]], f32)])   # around the RoI
    c["degenerate"] = one([np.array([[12, 22], [12, 22], [20, 30], [20, 40], [20, 40], [30, 40], [34, 36], [12, 22.0]], f32)])
    c["three_polys"] = one([rect(12, 22, 30, 40), rect(16, 26, 24, 34), np.array([[28, 38], [37, 40], [31, 47]], f32)])   # OR, not XOR
    c["two_points"] = (image([3, 4], [0, 1], [box, box], [3, 4], [[np.array([[12, 22], [30, 40]], f32)],
                                                                  [np.array([[12, 22], [30, 40]], f32), rect(12, 22, 30, 40)]],
                             np.zeros((0, 4))), 14, 0, 0, 4)
    c["zero_width"] = one([rect(9, 20, 11, 48)], bx=[10, 20, 10, 48])            # w -> 1
    # two gt tie the overlap: the first wins; crowd and class-0 gt (better overlaps) skipped
    tie = image([7, 7], [4, 5], [[0, 0, 9, 9]] * 4, [0, 5, 6, 7], [[rect(20, 20, 40, 40)], [rect(20, 20, 40, 40)], [rect(22, 20, 42, 40)],
                [rect(22, 20, 42, 40)]], [[21, 20, 41, 40], [20, 20, 40, 40]], gt_is_crowd=[0, 1, 0, 0])
    c["tie"] = (tie, 7, 2, 5, 4)
    c["no_fg"] = (image([0, 0, -1], [2, 1, -1], [box], [3], [[rect(12, 22, 30, 40)]], [[1, 2, 30, 40], [5, 5, 20, 20]], n_rois=2), 7, 2, 5, 2)
    c["nothing"] = (image([-1, -1], [-1, -1], [box], [3], [[rect(12, 22, 30, 40)]], [[1, 2, 30, 40]], n_rois=0), 7, 0, 0, 2)
    c["above_fm"] = (image([3] * 6 + [0], list(range(7)), [box], [3], [[rect(12, 22, 30, 40)]], [[11, 21, 37, 47]] * 6), 7, 0, 0, 4)
    # garbage: offsets out of range and non-monotone, NaN points past the counts, keep_inds out of range, a NaN box
    nanbox = [np.nan] * 4
    g = image([3, 3, 3, 3, 3], [3, 1, 2, 99, 5], [box, box, box, nanbox], [3, 3, 3, 3], [[rect(12, 22, 30, 40)], [rect(14, 24, 32, 42)],
              [rect(12, 22, 30, 40)], [rect(0, 0, 5, 5)]], [[11, 21, 37, 47], [11, 21, np.nan, 47], nanbox], gt_count=3)
    g["poly_xy"] = np.concatenate([g["poly_xy"][:12], np.full((5, 2), np.nan, f32)])           # 12 good points, then NaN
    # polygons: 0, 1, 2 good; 3 = the NaN points; 4 ends past PTS; 5 runs backwards; 6 starts below 0
    g["poly_ptr"] = np.array([0, 4, 8, 12, 17, 40, 3, -5], np.int32)
    # gt 0: polygon 0; gt 1: polygons 1 .. 6, two of them good; gt 2: a range past NP; the row past gt_count: backwards
    g["gt_poly_ptr"] = np.array([0, 1, 7, 9, -3], np.int32)
    c["garbage"] = (g, 14, 0, 0, 8)
    n1 = image([3], [0], [[0, 0, 99, 99]], [3], [[np.array([[1, 1], [98, 1], [98, 98], [np.nan, 50]], f32), rect(10, 10, 60, 60)]],
               np.zeros((0, 4)))
    c["nan_point"] = (n1, 14, 0, 0, 2)
    for name, n in (("edges300", 300), ("edges1100", 1100)):                     # more edges than one and than four rounds of the block
        a = np.linspace(0, 2 * np.pi, n, endpoint=False)
        rad = 12 + 2 * np.cos(7 * a)
        c[name] = one([np.stack([24 + rad * np.cos(a), 34 + rad * np.sin(a)], 1).astype(f32)], M=14)
    c["far"] = one([rect(-3000, -2000, 24, 34)], M=14)                            # long edges: the bisection's range
    for M in (1, 2, 7, 14, 28, 56):
        c["m%d" % M] = one([np.array([[11, 21], [37, 26], [30, 47], [14, 44]], f32)], M=M)
    return c


def stack(images, Fm):
    """images of one M -> batch arrays padded to common strides (padding: label / keep -1, zero boxes, empty polygon ranges), and the
    padded per-image dicts the restatement takes"""
    R, G, P = (max(len(i[k]) for i in images) for k in ("labels", "gt_boxes", "proposals"))
    PTS, NP = max(len(i["poly_xy"]) for i in images), max(len(i["poly_ptr"]) - 1 for i in images)
    P = max(P, 1)
    padded = []
    for i in images:
        pad = lambda a, n, v=0: np.concatenate([a, np.full((n - len(a),) + a.shape[1:], v, a.dtype)])
        padded.append(dict(i, labels=pad(i["labels"], R, -1), keep_inds=pad(i["keep_inds"], R, -1), gt_boxes=pad(i["gt_boxes"], G),
                           gt_classes=pad(i["gt_classes"], G), gt_is_crowd=pad(i["gt_is_crowd"], G), proposals=pad(i["proposals"], P),
                           poly_xy=pad(i["poly_xy"], PTS), poly_ptr=pad(i["poly_ptr"], NP + 1, i["poly_ptr"][-1]),
                           gt_poly_ptr=pad(i["gt_poly_ptr"], G + 1, i["gt_poly_ptr"][-1])))
    batch = {k: np.stack([p[k] for p in padded]) for k in ("labels", "keep_inds", "gt_boxes", "gt_classes", "gt_is_crowd", "proposals",
                                                             "poly_xy", "poly_ptr", "gt_poly_ptr")}
    batch["n_rois"] = np.array([p["n_rois"] for p in padded], np.int32)
    batch["gt_counts"] = np.array([p["gt_count"] for p in padded], np.int32)
    batch["im_scale"] = np.array([p["im_scale"] for p in padded], f32)
    return batch, padded


# ---- loss ----------------------------------------------------------------------------------------------------------------------------
def loss64(logits, masks, cls, upstream=1.0):
    """float64 yardstick of dtc_mask_loss: logits [Rm,K,M,M] float32, masks [Rm,M*M] int32, cls [Rm] int32
    -> dict(loss, n_valid, grad [Rm,K,M,M] float64, valid [Rm,K,M,M] bool: the elements the gradient formula covers -- every other
    one is a promised +0.0 --, scale = max |x| over the valid elements)"""
    Rm, K, M, _ = logits.shape
    x = logits.astype(np.float64).reshape(Rm, K, M * M)
    grad, covered = np.zeros_like(x), np.zeros(x.shape, bool)
    row_ok = (cls >= 0) & (cls < K)
    valid = ((masks == 0) | (masks == 1)) & row_ok[:, None]
    n = int(valid.sum())
    total, scale = 0.0, 0.0
    for r in np.where(row_ok)[0]:
        v = valid[r]
        xr, t = x[r, cls[r]][v], masks[r][v].astype(np.float64)
        total += float(np.sum(np.maximum(xr, 0) - xr * t + np.log1p(np.exp(-np.abs(xr)))))
        e = np.exp(-np.abs(xr))
        sig = np.where(xr >= 0, 1 / (1 + e), e / (1 + e))
        grad[r, cls[r], v] = (sig - t) * float(upstream) / max(n, 1)
        covered[r, cls[r], v] = True
        scale = max(scale, float(np.abs(xr).max(initial=0.0)))
    return dict(loss=total / n if n else 0.0, n_valid=n, grad=grad.reshape(logits.shape), valid=covered.reshape(logits.shape),
                scale=scale)


def loss_bounds(y, e_ref=0.0, upstream=1.0):
    """tests/README_loss.md's rule: loss max(4 e_ref, 32 eps max(|y|, max |x|)); gradient absolute 16 eps |upstream| / n_valid"""
    return dict(loss=max(4 * e_ref, 32 * EPS * max(abs(y["loss"]), y["scale"])), grad=16 * EPS * abs(upstream) / max(y["n_valid"], 1))


EXTREMES = np.array([0.0, 1e-40, -1e-40, 16.7, -16.7, 88.0, -88.0, 104.0, -104.0, 1e4, -1e4, 3e38, -3e38], f32)
LOSS_ROWS = (1, 2, 3, 63, 64, 65, 255, 256, 257)
LOSS_MS = (1, 7, 14, 28)
# name -> (Rm, M, K): every Rm at every M; K = 81 where the case stays small, 1 and 2 in turn elsewhere
LOSS_CASES = {"r%dm%d" % (r, m): (r, m, 81 if r <= 65 and m <= 14 else 1 + (i + j) % 2) for i, r in enumerate(LOSS_ROWS)
              for j, m in enumerate(LOSS_MS)}
LOSS_CASES.update(m3k81=(5, 3, 81), m28k81=(4, 28, 81), m5k2=(70, 5, 2))           # K = 81 at M = 28; odd M * M with K * M * M odd too


def make_loss_case(name, extremes=False, seed=0):
    """-> dict(logits f32 [Rm,K,M,M], masks i32 [Rm,M*M] with a fifth of the targets -1, some 2 and INT_MIN, cls i32 [Rm] with classes
    -1 and K on some rows)"""
    Rm, M, K = LOSS_CASES[name]
    rs = np.random.RandomState(20261022 + seed + 13 * sorted(LOSS_CASES).index(name))
    logits = (rs.standard_normal((Rm, K, M, M)) * 3).astype(f32)
    masks = rs.randint(0, 2, (Rm, M * M)).astype(np.int32)
    u = rs.rand(Rm, M * M)
    masks[u < 0.2] = -1
    masks[u < 0.04] = 2
    masks[u < 0.02] = np.iinfo(np.int32).min
    cls = rs.randint(0, K, Rm).astype(np.int32)
    if Rm >= 3:
        cls[rs.randint(0, Rm)] = -1
        cls[rs.randint(0, Rm)] = K
        masks[rs.randint(0, Rm)] = -1                                            # a row of padding
    if extremes:
        flat = logits.reshape(Rm, K, M * M)
        for r in range(Rm):
            if 0 <= cls[r] < K:
                n = min(len(EXTREMES), M * M)
                flat[r, cls[r], :n] = EXTREMES[:n]
                masks[r, :n] = (np.arange(n) + r) % 2
    return dict(logits=logits, masks=masks, cls=cls)
