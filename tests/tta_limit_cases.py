"""The cases that take the test-time-augmentation library past where tests/tta_cases.py stops (test support, not a test module; the
"Limits" section of tests/README_tta.md), shared by tests/test_tta_limits_host.py and tests/test_hip_tta_limits.py: class counts past
one wave, eight views, the row, batch and mask-size limits, NaN under SOFT_MAX.  Seeded numpy only; the builders are cached and what
they return is READ-ONLY."""
import functools

import numpy as np

import tta_cases as tc
import tta_ref as tr

f32 = np.float32


def frozen(x):
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            frozen(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            frozen(v)
    return x


# ---- the merge -------------------------------------------------------------------------------------------------------------------------------------
IM_SIZE = np.array([[37.0, 1.0], [600.0, 4097.0]], f32)       # tta_cases.IM_SIZE


@functools.lru_cache(maxsize=None)
def merge_case(T, R, n_cls, counts, logits, seed=0):
    """tta_cases.merge_case with the shape free: T views of 2 x R rows of n_cls classes; counts: per view the n_rois of the two
    images, cycled over the views.  Rois cross the image border, one delta in eight is saturated, the rows past n_rois hold NaN.
    -> (views, im_size)"""
    rs = np.random.RandomState(3000 + 17 * seed + 131 * T + n_cls)
    B, views = 2, []
    for t in range(T):
        n_rois = np.array(counts[t % len(counts)], np.int32)
        scale = (f32(tc.SCALES[t]) * np.array([1.0, 1.03125], f32)).astype(f32)
        rois5 = np.zeros((B, R, 5), f32)
        for b in range(B):
            h, w = IM_SIZE[b] * scale[b]
            x = np.sort(rs.uniform(-20, w + 20, (R, 2)), axis=1)
            y = np.sort(rs.uniform(-20, h + 20, (R, 2)), axis=1)
            rois5[b] = np.stack([np.full(R, b), x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1)
            rois5[b, 0, 1:] = [0, 0, w - 1, h - 1]
        deltas = (rs.randn(B, R, 4 * n_cls) * 0.5).astype(f32)
        sat = rs.rand(B, R, n_cls) < 0.125
        big = np.stack([rs.choice([-1e4, 1e4], sat.shape), rs.choice([-1e4, 1e4], sat.shape), rs.choice([50.0, -50.0], sat.shape),
                        rs.choice([50.0, -50.0], sat.shape)], axis=-1).astype(f32)
        deltas = np.where(np.repeat(sat, 4, axis=2), big.reshape(B, R, 4 * n_cls), deltas)
        lg = (rs.randn(B, R, n_cls) * 3.0).astype(f32)
        cls = lg if logits else tr.softmax_rows(lg)
        for b in range(B):
            deltas[b, n_rois[b]:] = np.nan
            cls[b, n_rois[b]:] = np.nan
            rois5[b, n_rois[b]:, 1:] = np.nan
        views.append(dict(rois5=rois5, n_rois=n_rois, cls_score=cls, bbox_pred=deltas, scale=scale, flipped=bool(tc.FLIPS[t])))
    return frozen((views, IM_SIZE.copy()))


# (T, heuristics, n_cls, R, counts, logits): the class loop runs 2 and 5 times per lane, the softmax fold adds 2 and 5 terms by slot
WIDE = [(T, heurs, n_cls, 5, counts, logits)
        for n_cls in (81, 257) for logits in (False, True)
        for T, heurs, counts in ((2, ("UNION", "UNION"), ((3, 5), (5, 0))), (3, ("AVG", "AVG"), ((4, 5),)))]
# eight views: the whole register table of the aligned heuristics, flips mixed as in tta_cases.FLIPS
EIGHT = [(8, heurs, 81, 3, ((3, 2),), True) for heurs in (("AVG", "AVG"), ("ID", "ID"), ("AVG", "ID"), ("ID", "AVG"))]
MERGES = WIDE + EIGHT
ROWS_COUNTS = (4096, 4001, 0, 4096, 13, 4095, 2222, 4096)     # R = 4096, T = 8: 32768 output rows; one view has none; the sum is odd


@functools.lru_cache(maxsize=None)
def merge_rows_limit():
    """B = 1, T = 8, R = 4096, n_cls = 2 under UNION with probabilities: out_rows = 32768.  -> (views, im_size)"""
    rs = np.random.RandomState(3100)
    R, views = 4096, []
    im = np.array([[480.0, 641.0]], f32)
    for t in range(8):
        scale = np.array([tc.SCALES[t]], f32)
        x = np.sort(rs.uniform(-20, 660 * scale[0], (R, 2)), axis=1)
        y = np.sort(rs.uniform(-20, 500 * scale[0], (R, 2)), axis=1)
        rois5 = np.stack([np.zeros(R), x[:, 0], y[:, 0], x[:, 1], y[:, 1]], axis=1).astype(f32)[None]
        p = rs.rand(1, R, 1).astype(f32)
        n = ROWS_COUNTS[t]
        deltas = (rs.randn(1, R, 8) * 0.5).astype(f32)
        cls = np.concatenate([p, f32(1) - p], axis=2)
        deltas[0, n:], cls[0, n:], rois5[0, n:, 1:] = np.nan, np.nan, np.nan
        views.append(dict(rois5=rois5, n_rois=np.array([n], np.int32), cls_score=cls, bbox_pred=deltas, scale=scale, flipped=bool(tc.FLIPS[t])))
    return frozen((views, im))


NB = 65535


@functools.lru_cache(maxsize=None)
def merge_batch_limit(logits):
    """B = 65535, T = 1, R = 1, n_cls = 2, one flipped view at scale 1.5 of 300 x 400 images: image b's roi starts at (b % 397, b % 293)
    and its count is b % 3 != 0.  -> (views, im_size, expected) with the expectation from ONE call of tta_ref.view_boxes over all
    rows (the restatement is row by row, and scale and size are the same in every image)"""
    rs = np.random.RandomState(3200)
    b = np.arange(NB)
    n_rois = (b % 3 != 0).astype(np.int32)
    x1, y1 = (b % 397).astype(f32), (b % 293).astype(f32)
    rois5 = (np.stack([b.astype(f32), x1, y1, x1 + 30 + b % 11, y1 + 20 + b % 7], axis=1) * f32(1.5)).astype(f32)[:, None, :]
    deltas = (rs.randn(NB, 1, 8) * 0.5).astype(f32)
    lg = (rs.randn(NB, 1, 2) * 3.0).astype(f32)
    cls = lg if logits else tr.softmax_rows(lg)
    view = dict(rois5=rois5, n_rois=n_rois, cls_score=cls, bbox_pred=deltas, scale=np.full(NB, 1.5, f32), flipped=True)
    im = np.tile(np.array([[300.0, 400.0]], f32), (NB, 1))
    live = n_rois == 1
    boxes = tr.view_boxes(rois5[:, 0, 1:], 1.5, im[0], deltas[:, 0], True)
    scores = tr.softmax_rows(lg[:, 0]) if logits else cls[:, 0]
    want = dict(out_scores=np.where(live[:, None], scores, f32(0))[:, None, :], out_boxes=np.where(live[:, None], boxes, f32(0))[:, None, :],
                out_n=n_rois.copy(), out_src=np.where(live, 0, -1).astype(np.int32)[:, None])
    return frozen(([view], im, want))


# ---- the combination -------------------------------------------------------------------------------------------------------------------------------
MASK_B, MAX_OUT = 3, 4
DET_COUNT = np.array([0, 3, MAX_OUT], np.int32)
SIZES = (1, 2, 3, 4, 8, 63, 64)                               # 4: the mirrored group of four is the group itself; 64: the limit
MASK_FLIPS = {2: (0, 1), 3: (0, 1, 1), 8: tc.FLIPS}
COMBINES = [(M, T) for M in SIZES for T in (2, 8)]


def channels(M):
    return 2 if M == 64 else 3


@functools.lru_cache(maxsize=None)
def combine_case(M, T, special=False):
    """tta_cases.combine_case with M, T and K free: T maps float32 [12, K, M, M] in [0, 1); special scatters tta_cases.SPECIAL.
    -> (masks, flipped, det_count, mask_class)"""
    rs = np.random.RandomState(4000 + 7 * M + T + (100 if special else 0))
    K, N = channels(M), MASK_B * MAX_OUT
    masks = []
    for t in range(T):
        m = np.minimum(rs.uniform(0, 1, (N, K, M, M)).astype(f32), np.nextafter(f32(1), f32(0)))
        if special:
            at = rs.randint(0, m.size, max(m.size // 6, 4))
            m.reshape(-1)[at] = tc.SPECIAL[rs.randint(0, len(tc.SPECIAL), len(at))]
        masks.append(m)
    mask_class = rs.randint(0, K, N).astype(np.int32)
    mask_class[MAX_OUT + 1], mask_class[2 * MAX_OUT + 2] = -1, K
    return frozen((masks, MASK_FLIPS[T], DET_COUNT.copy(), mask_class))


NAN_PLACES = ("first_view", "last_view", "flipped_view")


@functools.lru_cache(maxsize=None)
def nan_case(M, where):
    """three views (the last two flipped) with NaN in row 5, channel 1, map row 0: in view 0 at column 1; in the last view at
    column M - 2, which the flip brings to column 1; in view 1 (flipped, in the middle) at column M - 1 -> column 0.  -> (masks,
    flipped, det_count, place of the NaN in the output)"""
    masks, flipped, det_count, _ = combine_case(M, 3)
    masks = [np.array(m) for m in masks]
    view, col, out_col = {"first_view": (0, 1, 1), "last_view": (2, M - 2, 1), "flipped_view": (1, M - 1, 0)}[where]
    masks[view][5, 1, 0, col] = np.nan
    return frozen((masks, flipped, det_count, (5, 1, 0, out_col)))


def soft_max_without_the_nan_arm(masks, flipped):
    """the MUTANT of SOFT_MAX that folds with a plain `v > a`: a NaN in view 0 stays, a NaN in a later view is lost"""
    ms = [np.asarray(m)[..., ::-1] if f else np.asarray(m) for m, f in zip(masks, flipped)]
    a = ms[0].copy()
    for v in ms[1:]:
        with np.errstate(invalid="ignore"):
            a = np.where(v > a, v, a)
    return a


ROWS_B, ROWS_MAX_OUT = 33000, 2                               # 66000 mask rows: more than 65535


@functools.lru_cache(maxsize=None)
def combine_rows_limit():
    """B = 33000, max_out = 2, K = 1, M = 4, T = 2 (the second view flipped); det_count alternates 0, 1, 2.  -> (masks, flipped,
    det_count, mask_class)"""
    rs = np.random.RandomState(4100)
    N = ROWS_B * ROWS_MAX_OUT
    masks = [np.minimum(rs.uniform(0, 1, (N, 1, 4, 4)).astype(f32), np.nextafter(f32(1), f32(0))) for _ in range(2)]
    mask_class = np.where(np.arange(N) % 5 == 4, 1, 0).astype(np.int32)      # one row in five names a class outside [0, K)
    return frozen((masks, (0, 1), (np.arange(ROWS_B) % 3).astype(np.int32), mask_class))
