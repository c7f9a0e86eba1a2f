"""dtc_mask_targets and dtc_mask_loss past the sizes of tests/mask_train_ref.py's cases (test support, not a test module): images
with more rows than one round of the 256-thread workgroup, more gt than wavefronts, polygons around the lane and workgroup widths,
every M from 1 to 56; loss shapes above the 1024 workgroups of the dense pass, above M = 28 and at K = 1024.  Built from
mask_train_ref.image / pack / random_polygon / rect, deterministic from fixed seeds, made once and never modified.
tests/golden/make_mask_train_limits_golden.py records them (tests/golden/mask_train_limits.npz), tests/test_mask_train_limits_host.py
pins on the CPU the condition every case is there for, tests/test_hip_mask_train_limits.py launches them.

The launch arithmetic of csrc/mask_train/*.hip that the conditions speak of: mask_rows_kernel walks the R rows in rounds of BLOCK =
256, wavefront w of a round holds rows base + 64 w .. base + 64 w + 63; wavefront w takes gt w, w + 4, ...; the polygon's points go
over the 64 lanes; mask_loss_* run min(Rm, LOSS_BLOCKS) workgroups, workgroup x takes rows x, x + nb, ....
"""
import functools

import numpy as np

import mask_train_ref as mr

f32 = np.float32
BASE_SEED = 20261020 + 2000
BLOCK, WAVE, WAVES = mr.BLOCK, 64, mr.BLOCK // 64
LOSS_BLOCKS = 1024                                                           # csrc/mask_train/mask_loss.hip: kMaskLossMaxBlocks


def _freeze(img):
    for v in img.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return img


def _bbox(polys):
    p = np.concatenate([q for q in polys if len(q) >= 3 and np.isfinite(q).all()])
    return [p[:, 0].min(), p[:, 1].min(), p[:, 0].max(), p[:, 1].max()]


def _scene(rs, G, P, W, H, r_lo, r_hi):
    """G gt of one or two random polygons (a quarter self-intersecting), their boxes, P proposals jittered from them"""
    polys = []
    for _ in range(G):
        cx, cy, r = rs.uniform(r_hi, W - r_hi), rs.uniform(r_hi, H - r_hi), rs.uniform(r_lo, r_hi)
        polys.append([mr.random_polygon(rs, cx + rs.uniform(-r, r) * (k > 0), cy + rs.uniform(-r, r) * (k > 0), r * (1.0, 0.5)[k > 0],
                                        rs.randint(3, 12), star=rs.rand() < 0.25) for k in range(rs.randint(1, 3))])
    boxes = np.asarray([_bbox(p) for p in polys], f32)
    src = rs.randint(0, G, P)
    jit = rs.uniform(-0.2, 0.2, (P, 4)) * np.stack([boxes[src, 2] - boxes[src, 0], boxes[src, 3] - boxes[src, 1]] * 2, 1)
    return polys, boxes, (boxes[src] + jit).astype(f32)


# ---- the rows: sections 1, 2 and 4 of mask_rows_kernel ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rows700():
    """R = 700, n_rois = 650, G = 37, P = 300: about 85 % of the labels > 0, rows 650 .. 699 among them; keep_inds random over gt and
    proposals; a crowd gt and a class-0 gt"""
    rs = np.random.RandomState(BASE_SEED + 1)
    G, P, R = 37, 300, 700
    polys, boxes, props = _scene(rs, G, P, 640.0, 480.0, 15.0, 60.0)
    cls = rs.randint(1, 81, G).astype(np.int32)
    crowd = np.zeros(G, np.int32)
    crowd[5], cls[11] = 1, 0
    u = rs.rand(R)
    labels = np.where(u < 0.85, rs.randint(1, 81, R), np.where(u < 0.93, 0, -1)).astype(np.int32)
    keep = rs.randint(0, G + P, R).astype(np.int32)
    return _freeze(mr.image(labels, keep, boxes, cls, polys, props, gt_is_crowd=crowd, im_scale=1.5, n_rois=650))


@functools.lru_cache(maxsize=None)
def rows4096():
    """R = n_rois = 4096, the limit: about 3 % foreground, most of the rest background"""
    rs = np.random.RandomState(BASE_SEED + 2)
    G, P, R = 6, 64, 4096
    polys, boxes, props = _scene(rs, G, P, 640.0, 480.0, 20.0, 80.0)
    cls = rs.randint(1, 81, G).astype(np.int32)
    u = rs.rand(R)
    labels = np.where(u < 0.03, rs.randint(1, 81, R), np.where(u < 0.9, 0, -1)).astype(np.int32)
    keep = rs.randint(0, G + P, R).astype(np.int32)
    return _freeze(mr.image(labels, keep, boxes, cls, polys, props, im_scale=1.5))


LATE_BG_ROWS = (403, 590)


@functools.lru_cache(maxsize=None)
def late_bg(n_rois):
    """R = 600, every label -1 but 0 at rows 403 and 590"""
    R = 600
    labels = np.full(R, -1, np.int32)
    labels[list(LATE_BG_ROWS)] = 0
    keep = np.full(R, -1, np.int32)
    keep[403], keep[590] = 3, 0
    boxes = [[10, 20, 60, 90], [100, 40, 180, 120]]
    return _freeze(mr.image(labels, keep, boxes, [3, 4], [[mr.rect(*b)] for b in boxes],
                            [[5, 6, 70, 80], [1, 2, 30, 40], [90, 30, 170, 110], [20, 20, 50, 50]], im_scale=2.0, n_rois=n_rois))


# ---- the gt: section 3 ------------------------------------------------------------------------------------------------------------------
GT256_TIES = ((71, 74), (131, 134))                                          # duplicate gt on different wavefronts, indices above 64
GT256_TIE_ROWS = {0: 71, 1: 71, 2: 131, 3: 131}                              # mask row -> the gt it must match (keep_inds 71, 74, 134, 131)
GT256_STALE_ROWS = (4, 5, 6, 7, 8, 9)                                        # mask rows on proposals 0 .. 5, whose copies are gt 250 .. 255
GT256_COUNT = 250


@functools.lru_cache(maxsize=None)
def gt256():
    """G = 256 (the limit), gt_counts = 250, R = 300 rows, all foreground.  One gt per 40 px cell of a 16 x 16 grid; every 7th is
    crowd, every 11th of class 0, every g = 5 mod 13 has only a 2-point polygon; gt 74 and 134 are copies of gt 71 and 131; the gt
    rows 250 .. 255, past gt_counts, are exact copies of proposals 0 .. 5 with a rectangle polygon each, class > 0, no crowd."""
    rs = np.random.RandomState(BASE_SEED + 3)
    G, P, R = 256, 64, 300
    polys = []
    for g in range(G):
        cx, cy = 20.0 + 40.0 * (g % 16), 20.0 + 40.0 * (g // 16)
        if g % 13 == 5:
            polys.append([np.array([[cx - 5, cy - 5], [cx + 5, cy + 5]], f32)])
            rs.uniform(8, 18)
        else:
            polys.append([mr.random_polygon(rs, cx, cy, rs.uniform(8, 18), rs.randint(3, 12))])
    for a, b in GT256_TIES:
        polys[b] = [polys[a][0].copy()]
    boxes = np.asarray([_bbox(p) if len(p[0]) >= 3 else [p[0][0, 0], p[0][0, 1], p[0][1, 0], p[0][1, 1]] for p in polys], f32)
    cls = rs.randint(1, 81, G).astype(np.int32)
    cls[np.arange(G) % 11 == 0] = 0
    crowd = (np.arange(G) % 7 == 0).astype(np.int32)
    src = rs.randint(0, GT256_COUNT, P)
    src[:6] = [1, 2, 3, 4, 6, 8]                                                 # eligible gt: the rows on proposals 0 .. 5 have a match
    jit = rs.uniform(-0.2, 0.2, (P, 4)) * np.stack([boxes[src, 2] - boxes[src, 0], boxes[src, 3] - boxes[src, 1]] * 2, 1)
    props = (boxes[src] + jit).astype(f32)
    for k in range(GT256_COUNT, G):                                          # the stale rows: what a larger minibatch left behind
        boxes[k] = props[k - GT256_COUNT]
        polys[k] = [mr.rect(*props[k - GT256_COUNT])]
        cls[k], crowd[k] = 7 + k - GT256_COUNT, 0
    labels = rs.randint(1, 81, R).astype(np.int32)
    keep = rs.randint(0, GT256_COUNT + P, R).astype(np.int32)
    keep[:4] = [71, 74, 134, 131]
    keep[4:10] = GT256_COUNT + np.arange(6)
    return _freeze(mr.image(labels, keep, boxes, cls, polys, props, gt_is_crowd=crowd, im_scale=1.5, gt_count=GT256_COUNT))


POINT_COUNTS = (3, 63, 64, 65, 128, 129, 255, 256, 257, 513)


def points_polygon(k):
    """n - 1 points around (60, 60) at radius about 20, then the LAST point at (60 + d, 60 + d), d = 40 + 6 k: it alone carries the
    largest x and y"""
    n = POINT_COUNTS[k]
    a = np.linspace(0, 2 * np.pi, n - 1, endpoint=False) + 0.1 * k
    rad = 20.0 * (1 + 0.1 * np.cos(5 * a))
    d = 40.0 + 6.0 * k
    return np.concatenate([np.stack([60 + rad * np.cos(a), 60 + rad * np.sin(a)], 1), [[60 + d, 60 + d]]]).astype(f32)


@functools.lru_cache(maxsize=None)
def points_edges(drop_last_of=-1):
    """10 gt of one polygon each, the RoIs are the gt boxes; two background rows.  drop_last_of = k: polygon k without its last point
    (the host test's picture of a lane loop that loses its last trip), the RoIs unchanged"""
    polys = [[points_polygon(k)] for k in range(len(POINT_COUNTS))]
    boxes = np.asarray([_bbox(p) for p in polys], f32)
    if drop_last_of >= 0:
        polys[drop_last_of] = [polys[drop_last_of][0][:-1]]
    G = len(polys)
    labels = list(range(1, G + 1)) + [0, 0]
    keep = list(range(G)) + [G, G]
    return _freeze(mr.image(labels, keep, boxes, list(range(1, G + 1)), polys, [[30, 30, 90, 90]], im_scale=1.5))


MANY_POLYS, MANY_TWO_POINT, MANY_NAN = 40, 13, 27


@functools.lru_cache(maxsize=None)
def many_polys(only_gt1=False):
    """gt 0: 40 polygons, 38 overlapping rectangles with a 2-point polygon (number 13) and a polygon with a NaN point (number 27) among
    them; gt 1: one triangle"""
    rs = np.random.RandomState(BASE_SEED + 4)
    ps = []
    for q in range(MANY_POLYS):
        x0, y0, w, h = rs.uniform(10, 100), rs.uniform(10, 100), rs.uniform(10, 50), rs.uniform(10, 50)
        p = mr.rect(x0, y0, x0 + w, y0 + h)
        if q == MANY_TWO_POINT:
            p = p[[0, 2]]
        if q == MANY_NAN:
            p[2, 1] = np.nan
        ps.append(p)
    tri = np.array([[160, 20], [200, 30], [175, 70]], f32)
    b0, b1 = [10, 10, 150, 150], [160, 20, 200, 70]
    if only_gt1:
        return _freeze(mr.image([4], [0], [b1], [4], [[tri]], np.zeros((0, 4))))
    return _freeze(mr.image([3, 4], [0, 1], [b0, b1], [3, 4], [ps, [tri]], np.zeros((0, 4))))


ALL_M = tuple(range(1, 57))


@functools.lru_cache(maxsize=None)
def all_m():
    """the quadrilateral of mask_train_ref.hand_cases()'s m* cases, and a gt of three polygons (one inside another)"""
    b0, b1 = [10, 20, 38, 48], [50, 20, 78, 48]
    quad = np.array([[11, 21], [37, 26], [30, 47], [14, 44]], f32)
    three = [mr.rect(52, 22, 70, 40), mr.rect(56, 26, 64, 34), np.array([[68, 38], [77, 40], [71, 47]], f32)]
    return _freeze(mr.image([3, 4], [0, 1], [b0, b1], [3, 4], [[quad], three], np.zeros((0, 4))))


LEVEL_SIZES = (2.0 / 256, 2.0, 20.0, 100.0, 700.0, 2000.0, 3000.0, 4000.0)   # x im_scale 256: 2 px .. 1 024 000 px


@functools.lru_cache(maxsize=None)
def levels():
    """8 foreground rows on square proposals of LEVEL_SIZES at im_scale 256: the unclamped FPN level runs from -3 to 16"""
    props = [[8, 8, 8 + s, 8 + s] for s in LEVEL_SIZES]
    return _freeze(mr.image([5] * 8, list(range(1, 9)), [[0, 0, 4100, 4100]], [5], [[mr.rect(4, 4, 4090, 4090)]], props, im_scale=256.0))


# name -> (image, M, k_min, k_max, Fm); "all_m" stands for one call per M of ALL_M
TARGETS = {
    "rows700_fm512": (rows700, 7, 2, 5, 512), "rows700_fm300": (rows700, 7, 2, 5, 300), "rows700_fm5": (rows700, 7, 2, 5, 5),
    "rows4096": (rows4096, 7, 2, 5, 512),
    "late_bg": (functools.partial(late_bg, 600), 7, 2, 5, 4), "late_bg_past": (functools.partial(late_bg, 403), 7, 2, 5, 4),
    "gt256": (gt256, 14, 2, 5, 300), "points_edges": (points_edges, 14, 2, 5, 16), "many_polys": (many_polys, 28, 2, 5, 4),
    "levels": (levels, 7, 0, 15, 8), "levels_single": (levels, 7, 3, 3, 8),
}
TARGETS.update({"all_m%d" % M: (all_m, M, 2, 5, 4) for M in ALL_M})
BATCH2 = ("rows700_fm512", "rows4096")
OVERLAP_ROWS, OVERLAP_FIRST = 64, 16


def case(name):
    fn, M, k_min, k_max, Fm = TARGETS[name]
    return fn(), M, k_min, k_max, Fm


@functools.lru_cache(maxsize=None)
def want(name):
    """the restatement's outputs of a case, computed once and shared"""
    out = mr.targets(*case(name))
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def fg_rows(img, Fm=None):
    n_r = min(max(int(img["n_rois"]), 0), len(img["labels"]))
    return [r for r in range(n_r) if img["labels"][r] > 0][:Fm]


def eligible(img):
    n_g = min(max(int(img["gt_count"]), 0), len(img["gt_boxes"]))
    return [g for g in range(n_g) if img["gt_classes"][g] > 0 and img["gt_is_crowd"][g] == 0 and mr.valid_polys(img, g)]


def sample_rows(name):
    """the matched mask rows whose overlaps the fixture keeps: all of at most 64; else the first 16 and a seeded sample of 48"""
    o = want(name)
    rows = [t for t in range(int(o["n_mask"])) if o["mask_gt"][t] >= 0]
    if len(rows) <= OVERLAP_ROWS:
        return rows
    rs = np.random.RandomState(BASE_SEED + 100 + sorted(TARGETS).index(name))
    rest = rs.choice(len(rows) - OVERLAP_FIRST, OVERLAP_ROWS - OVERLAP_FIRST, replace=False) + OVERLAP_FIRST
    return rows[:OVERLAP_FIRST] + [rows[i] for i in np.sort(rest)]


def row_boxes(name, rows):
    """the boxes (original coordinates) of mask rows of a case without the fallback"""
    img, _, _, _, Fm = case(name)
    n_g = min(max(int(img["gt_count"]), 0), len(img["gt_boxes"]))
    cand = np.concatenate([img["gt_boxes"][:n_g], img["proposals"]])
    fg = fg_rows(img, Fm)
    return np.stack([cand[img["keep_inds"][fg[t]]] for t in rows]).astype(f32) if rows else np.zeros((0, 4), f32)


def wave_groups(img):
    """the foreground rows below n_rois per 64-row group (one wavefront of one round of section 2)"""
    n_r = min(max(int(img["n_rois"]), 0), len(img["labels"]))
    return [[r for r in range(b, min(b + WAVE, n_r)) if img["labels"][r] > 0] for b in range(0, n_r, WAVE)]


# ---- the loss ---------------------------------------------------------------------------------------------------------------------------
# name -> (Rm, M, K)
LOSS = {"r1025m7k2": (1025, 7, 2), "r2047": (2047, 7, 2), "r2048": (2048, 7, 2), "r2049": (2049, 7, 2), "r3077m7k3": (3077, 7, 3),
        "r1025m28k3": (1025, 28, 3), "r3m56k2": (3, 56, 2), "r5m55k3": (5, 55, 3), "r3m2k1024": (3, 2, 1024), "r4m1k1024": (4, 1, 1024)}
MULTI_ROW = tuple(n for n, (r, _, _) in LOSS.items() if r > LOSS_BLOCKS)
# what is planted on the row pair (x, x + 1024) of workgroup x: (first, second), in every multi-row case with at least 8 shared
# workgroups; "valid": an ordinary row, "neg" / "K": class -1 / K, "pad": every target -1, "ext": the EXTREMES logits on a valid row
PLANTED = {10: ("valid", "neg"), 20: ("neg", "valid"), 30: ("valid", "K"), 40: ("K", "valid"), 50: ("valid", "pad"), 60: ("pad", "valid"),
           70: ("ext", "neg"), 80: ("K", "ext"), 90: ("ext", "pad"), 100: ("pad", "ext")}
# the cases whose only shared workgroup is workgroup 0, rows 0 and 1024
PLANTED_SINGLE = {"r1025m7k2": ("ext", "neg"), "r1025m28k3": ("pad", "ext")}
FIXED_CLASSES = {"r3m2k1024": (1023, 0, 1024), "r4m1k1024": (0, 1023, -1, 512)}    # the class channel as the last and as the first


def _plant(kind, r, logits, masks, cls, rs, extremes):
    K, MM = logits.shape[1], masks.shape[1]
    if kind == "neg":
        cls[r] = -1
    elif kind == "K":
        cls[r] = K
    else:
        cls[r] = rs.randint(0, K)
        if kind == "pad":
            masks[r] = -1
        else:
            masks[r] = rs.randint(0, 2, MM)
            masks[r, rs.rand(MM) < 0.2] = -1
            if kind == "ext" and extremes:
                n = min(len(mr.EXTREMES), MM)
                logits.reshape(len(cls), K, MM)[r, cls[r], :n] = mr.EXTREMES[:n]
                masks[r, :n] = (np.arange(n) + r) % 2


@functools.lru_cache(maxsize=None)
def loss_case(name, extremes=False):
    """as mask_train_ref.make_loss_case: logits N(0, 3), a fifth of the targets -1, some 2 and INT_MIN, random classes; then the
    planted rows.  extremes: the "ext" rows carry the EXTREMES logits (max |x| = 3e38 then widens the loss bound to 32 eps 3e38, so
    the loss is pinned by the plain form of the case, where an "ext" row is an ordinary valid row, and the gradient by both)"""
    Rm, M, K = LOSS[name]
    rs = np.random.RandomState(BASE_SEED + 200 + 13 * sorted(LOSS).index(name))
    logits = (rs.standard_normal((Rm, K, M, M)) * 3).astype(f32)
    masks = rs.randint(0, 2, (Rm, M * M)).astype(np.int32)
    u = rs.rand(Rm, M * M)
    masks[u < 0.2] = -1
    masks[u < 0.04] = 2
    masks[u < 0.02] = np.iinfo(np.int32).min
    cls = rs.randint(0, K, Rm).astype(np.int32)
    if name in FIXED_CLASSES:
        cls[:] = FIXED_CLASSES[name]
    elif name in PLANTED_SINGLE:
        for r, kind in zip((0, LOSS_BLOCKS), PLANTED_SINGLE[name]):
            _plant(kind, r, logits, masks, cls, rs, extremes)
    elif name in MULTI_ROW:
        for x, kinds in sorted(PLANTED.items()):
            for r, kind in zip((x, x + LOSS_BLOCKS), kinds):
                _plant(kind, r, logits, masks, cls, rs, extremes)
    c = dict(logits=logits, masks=masks, cls=cls)
    for v in c.values():
        v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def loss_want(name, extremes=False, upstream=1.0):
    c = loss_case(name, extremes)
    return mr.loss64(c["logits"], c["masks"], c["cls"], upstream=upstream)


def row_kind(c, r):
    """what row r of a loss case is, in PLANTED's words"""
    K = c["logits"].shape[1]
    k, m = int(c["cls"][r]), c["masks"][r]
    if k < 0:
        return "neg"
    if k >= K:
        return "K"
    if not ((m == 0) | (m == 1)).any():
        return "pad"
    n = min(len(mr.EXTREMES), m.size)
    x = c["logits"].reshape(len(c["cls"]), K, -1)[r, k, :n]
    return "ext" if x.tobytes() == mr.EXTREMES[:n].tobytes() else "valid"


def shared_pairs(c):
    """(kind of row x, kind of row x + nb) over the workgroups that take a second row"""
    Rm = len(c["cls"])
    nb = min(Rm, LOSS_BLOCKS)
    return {(row_kind(c, x), row_kind(c, x + nb)) for x in range(nb) if x + nb < Rm}


def rows_per_workgroup(Rm):
    nb = min(Rm, LOSS_BLOCKS)
    return [len(range(x, Rm, nb)) for x in range(nb)]


def grad_sample(name, extremes=False):
    """the flat gradient elements the fixture keeps: 48 of the elements the formula covers and 16 of all, seeded"""
    y = loss_want(name, extremes)
    rs = np.random.RandomState(BASE_SEED + 300 + sorted(LOSS).index(name))
    cov = np.flatnonzero(y["valid"].ravel())
    a = rs.choice(cov, min(48, len(cov)), replace=False)
    b = rs.choice(y["valid"].size, min(16, y["valid"].size), replace=False)
    return np.unique(np.concatenate([a, b]))
