"""The cases that take the mask post-processing library past where tests/mask_post_cases.py stops (the "Limits" section of
tests/README_mask_post.md), shared by tests/test_mask_post_limits_host.py and tests/test_hip_mask_post_limits.py.  Every case is the
smallest shape at which the situation it is named for still occurs; the host test asserts that situation.  Seeded; the builders are
cached and what they return is READ-ONLY (the arrays are frozen)."""
import functools

import numpy as np

import mask_post_cases as mc
import mask_post_ref as mr
import segm_eval_cases as sc
import segm_eval_ref as sr

U32 = 0xFFFFFFFF
P30 = 1 << 30


def frozen(x):
    """a case with every array read-only"""
    if isinstance(x, np.ndarray):
        x.setflags(write=False)
    elif isinstance(x, dict):
        for v in x.values():
            frozen(v)
    elif isinstance(x, (list, tuple)):
        for v in x:
            frozen(v)
    return x


def cached(fn):
    return functools.lru_cache(maxsize=None)(lambda: frozen(fn()))


def px(h, w, on):
    """the run list of the [h, w] mask whose set POSITIONS (x * h + y) are `on`"""
    return sc.runs_of(np.isin(np.arange(h * w), list(on)).reshape(w, h).T)


def full_windows(case):
    """vote_sparse windows that cover every image whole"""
    return [[(0, sr.pixels(s))] for s in case["im_size"]]


# ---- many_voters -----------------------------------------------------------------------------------------------------------------------------------
MANY_TOP1 = list(range(255)) + [300, 511]                     # the 257 voters of top 1: list places 255 and 256 are voters 300 and 511


@cached
def many_voters():
    """16 x 48 = 3 chunks, T = 2, A = 512 = all_count.  Top 0 has all 512 voters, top 1 exactly 257 (MANY_TOP1).  Every voter has
    pixels in chunk 0 (voter 0 has position 0, so the chunks are [0, 256), [256, 512), [512, 768)); in chunk 1 only voters >= 256 --
    every fourth one from 260 on except 300, and 511 --; in chunk 2 only voters 300 and 511.  -> (case, ovr)"""
    rs = np.random.RandomState(31)
    h, w, A = 16, 48, 512
    pool = []
    for k in range(A):
        on = set(rs.randint(0, 256, 5).tolist())
        if k == 0:
            on.add(0)
        if k >= 256 and ((k % 4 == 0 and k != 300 and k >= 260) or k == 511):
            on |= set(rs.randint(256, 512, 4).tolist())
        if k == 300:
            on |= {520, 521, 600, 601, 602, 767}
        if k == 511:
            on |= {530, 531, 532, 601, 700, 701}
        if k < 256:                                             # a small support over the left of the image, a score of its own
            x0, y0 = int(rs.randint(0, 14)), int(rs.randint(0, 10))
            box, score = (x0, y0, x0 + int(rs.randint(1, 6)), y0 + int(rs.randint(2, 7))), float(np.float32(rs.rand()))
        else:
            box, score = (0, 0, w - 1, h - 1), 40.0 if k in (300, 511) else float(np.float32(0.05 + rs.rand()))
        pool.append((px(h, w, on), box, score))
    tops = [pool[0][0], pool[511][0]]
    case = mc.vote_case([((h, w), tops, pool)], T=2, A=A, top_stride=40, all_stride=40, out_stride=400, iou_thresh=0.5, binarize_thresh=0.02,
                        seed=31)
    ovr = np.full((1, 2, A), 0.9)
    ovr[0, 1] = 0.1
    ovr[0, 1, MANY_TOP1] = 0.5                                  # at the threshold: a voter
    ovr[0, 1, 400] = np.nan
    return case, ovr


# ---- negative_threshold_chunks ---------------------------------------------------------------------------------------------------------------------
@cached
def negative_threshold_chunks():
    """the 32 x 40 image of mask_post_cases.chunks (5 chunks) with 12 voters and 6 tops of 5 to 10 voters: voters 0 .. 5 are near
    copies of the blob cut to the columns below 24, so tops 0 and 1, which only they vote on, have no voter in chunks 3 and 4;
    voters 6 .. 11 are run lists with ends on the chunk borders.  Voter 1 has a NaN score, voter 2 +inf.  -> (case, ovr); run it at
    binarize_thresh -0.25, -0.0 and 0.0"""
    rs = np.random.RandomState(32)
    h, w = 32, 40
    yy, xx = np.mgrid[0:h, 0:w]
    blob = (((yy - 15) / 11.0) ** 2 + ((xx - 12) / 10.0) ** 2 <= 1.0) & (xx < 24)
    pool = []
    box = lambda: (int(rs.randint(-4, 12)), int(rs.randint(-4, 12)), int(rs.randint(14, 30)), int(rs.randint(14, 36)))
    for k in range(6):
        m = blob.copy()
        m[rs.randint(0, h, 6), rs.randint(0, 24, 6)] ^= True
        m[0, 0] = True
        pool.append((sc.runs_of(m), box(), [0.7, np.nan, np.inf, 0.4, 0.9, 0.2][k]))
    for n_runs in (64, 65, 128, 129, 33, 7):
        pool.append(([0] + mc._list_of(n_runs - 1, h * w, rs, ends_at=(256, 512, 768)), box(), float(np.float32(rs.rand()))))
    tops = [pool[k][0] for k in (0, 3, 6, 7, 8, 9)]
    case = mc.vote_case([((h, w), tops, pool)], T=7, A=13, top_stride=140, all_stride=132, out_stride=700, iou_thresh=0.3,
                        binarize_thresh=-0.25, seed=32)
    ovr = np.full((1, 7, 13), 0.9)                              # the rows and columns past the counts would vote
    voters = [[0, 1, 2, 3, 4, 5], [0, 1, 3, 4, 5], [0, 2, 4, 6, 7, 8, 9, 10, 11], list(range(2, 12)), [1, 6, 7, 9, 11], [0, 3, 5, 8, 10, 11, 6]]
    for t, vs in enumerate(voters):
        ovr[0, t, :12] = 0.1
        ovr[0, t, vs] = 0.6
    return case, ovr


NEG_VOTERS = (6, 5, 9, 10, 5, 7)


# ---- encoder_edges ---------------------------------------------------------------------------------------------------------------------------------
@cached
def encoder_edges():
    """16 x 64 = 4 chunks.  Voter 0 is WEAK (score 0.01): it has positions 0 and 1023, so every walk starts at 0 and ends at h w,
    and its pixels alone lose the vote; every top t < 5 is voted by voter 0 and a pair of identical strong voters (score 1):
      0  the even positions of chunk 0: all 256 pixels of the chunk start a run; 257 runs = out_stride: fits exactly
      1  the same and [1000, 1024): one more start, the closing run is ones: need 258, -1
      2  all of chunk 1, nobody in chunk 2: the run ends at 512, at thread 0 of a chunk no voter touches
      3  [1020, 1024): the last pixel on, the closing run is ones
      4  [0, 5): pixel 0 on, the first run is 0
      5  a top of 300 runs with one voter: copied, need 300 > out_stride: -1
    -> (case, ovr)"""
    h, w = 16, 64
    hw = h * w
    whole = (0, 0, w - 1, h - 1)
    shapes = [set(range(0, 256, 2)), set(range(0, 256, 2)) | set(range(1000, 1024)), set(range(256, 512)), set(range(1020, 1024)),
              set(range(5))]
    pool = [(px(h, w, {0, 1023}), whole, 0.01)]
    for s in shapes:
        pool += [(px(h, w, s), whole, 1.0)] * 2
    tops = [px(h, w, s) for s in shapes] + [[1] * 299 + [hw - 299]]
    case = mc.vote_case([((h, w), tops, pool)], T=7, A=12, top_stride=300, all_stride=260, out_stride=257, iou_thresh=0.5, binarize_thresh=0.5,
                        seed=33)
    ovr = np.full((1, 7, 12), 0.9)
    ovr[0, :, :11] = 0.0
    for t in range(5):
        ovr[0, t, [0, 2 * t + 1, 2 * t + 2]] = 1.0
    ovr[0, 5, 0] = 1.0
    return case, ovr


# ---- jumps -----------------------------------------------------------------------------------------------------------------------------------------
JH = 32768
CA = 15259 * JH                                               # the column boundary inside cluster A, near 5e8
P0 = CA - 1000                                                # where the wrapped voter's only ones start
SB = P30 - 3000                                               # the first one of cluster B
JUMP_WINDOWS = [[(CA - 2048, CA + 2048), (P30 - 4096, P30)]]


def _scatter(rs, lo, hi, n):
    """about n / 2 disjoint one-runs [s, e) inside [lo, hi), apart from each other, from n seeded cuts"""
    cuts = sorted(set(rs.randint(lo, hi + 1, n + n % 2).tolist()))
    cuts = cuts[:len(cuts) - len(cuts) % 2]
    return [(cuts[i], cuts[i + 1]) for i in range(0, len(cuts), 2)]


def _runs(intervals, tail=None):
    """disjoint, increasing one-runs [s, e) (touching ones and empty ones allowed: they give zero-length runs) -> the run list; tail:
    where the closing zero-run ends, or None for a list that ends on its last one-run"""
    runs, pos = [], 0
    for s, e in intervals:
        runs += [s - pos, e - s]
        pos = e
    return runs if tail is None else runs + [tail - pos]


@cached
def jumps():
    """one 32768 x 32768 image, h w = 2^30, four voters whose ones lie in cluster A = [CA - 1500, CA + 1500) across the column boundary
    CA, outside the hole [P0 + 8, P0 + 300), and in cluster B = [SB, 2^30):
      0  scattered runs in A and in B: B starts with a one-run at SB, the last one-run ends on pixel 2^30 - 1
      1  scattered runs in A; its list ENDS at CA + 1200, short of the image, on a one-run
      2  128 runs: ones [P0, P0 + 7), sixty zero-length runs, 0xFFFFFFFF twice -- the sum passes 2^32 at the end of the first 64 runs
         and is clipped to h w --, then 64 more runs (10, 3, 1, 3, 1, ...) that lie past the image: no pixel.  Carried in 32 bits the
         sum wraps to P0 + 5 and those runs land in the hole, where no voter has a pixel
      3  scattered runs in A; then zeros up to SB, two one-runs of length 0 there, 90 zeros, and scattered runs in B: the jump over
         the gap lands on SB, on its zero-length one-runs (and on voter 0's first one)
    Supports are column and row ranges around the clusters; one is +/-2^30.  Tops: the voters' own lists.  -> (case, ovr)"""
    rs = np.random.RandomState(34)
    in_a = lambda n: _scatter(rs, CA - 1500, P0 + 8, n) + _scatter(rs, P0 + 300, CA + 1500, n)
    b0 = _scatter(rs, SB + 1, P30 - 1, 24)
    v0 = _runs(in_a(10) + [(SB, b0[0][0] - 1)] + b0[1:-1] + [(b0[-1][0], P30)])
    a1 = in_a(8)
    v1 = _runs([iv for iv in a1 if iv[1] < CA + 1100] + [(CA + 1150, CA + 1200)])
    v2 = [P0, 7] + [0] * 60 + [U32, U32] + [10] + [3, 1] * 31 + [3]
    v3 = _runs(in_a(9) + [(SB, SB), (SB, SB)] + _scatter(rs, SB + 90, P30 - 40, 14), tail=P30)
    col = CA // JH                                              # 15259: cluster A is the bottom of column 15258 and the top of 15259
    boxes = [(col - 1, JH - 1200, col, JH - 1), (col - 1, 0, col + 3, 900), (-P30, -P30, P30, P30), (JH - 1, JH - 2000, JH - 1, JH - 100)]
    pool = [(v, b, s) for v, b, s in zip((v0, v1, v2, v3), boxes, (0.8, 0.6, 0.9, 0.5))]
    tops = [v0, v1, v3, v2]
    case = mc.vote_case([((JH, JH), tops, pool)], T=5, A=5, top_stride=130, all_stride=130, out_stride=260, iou_thresh=0.5, binarize_thresh=0.3,
                        seed=34)
    ovr = np.full((1, 5, 5), 0.9)
    ovr[0, :, :4] = [[.9, .9, .9, .9], [.9, .9, .1, np.nan], [.1, .9, .9, .9], [.1, .1, .9, .1], [.9] * 4]
    return case, ovr


# ---- max_stride ------------------------------------------------------------------------------------------------------------------------------------
S20 = 1 << 20


@cached
def max_stride():
    """one 1024 x 1024 image, every stride 2^20.  Pool: A = [1] * 2^20 (the odd positions), B = [0] + [1] * (2^20 - 1) (the even
    positions; its last pixel is off), B again with another score, C = [3, 5].  Tops (the list of each is C's, or A for the copy):
      0  voters A (0.6) and B (0.3) at 0.5: AVG gives A's pixels, 2^20 runs: fits out_stride = 2^20 exactly; UNION all ones, [0, 2^20]
      1  voters A (0.6) and B (0.9): AVG gives B's pixels, [0] + [1] * 2^20: need 2^20 + 1, -1
      2  the top A with one voter: copied, 2^20 runs
    -> (case, ovr)"""
    h = w = 1024
    whole = (0, 0, w - 1, h - 1)
    A, B, Cl = np.ones(S20, np.uint32), np.ones(S20, np.uint32), [3, 5]
    B[0] = 0
    pool = [((A, S20), whole, 0.6), ((B, S20), whole, 0.3), ((B, S20), whole, 0.9), (Cl, whole, 0.5)]
    tops = [Cl, Cl, (A, S20)]
    case = mc.vote_case([((h, w), tops, pool)], T=3, A=4, top_stride=S20, all_stride=S20, out_stride=S20, iou_thresh=0.5, binarize_thresh=0.5,
                        seed=35)
    ovr = np.zeros((1, 3, 4))
    ovr[0, 0, [0, 1]], ovr[0, 1, [0, 2]], ovr[0, 2, 0] = 0.5, 0.5, 0.5
    return case, ovr


def max_stride_pairs(crowd):
    """the overlaps of the pool with itself by hand: |A| = |B| = 2^19, A and B share nothing, C = positions 3 .. 7 has 3 odd and 2 even"""
    area = np.array([S20 // 2, S20 // 2, S20 // 2, 5], np.int64)
    inter = np.array([[S20 // 2, 0, 0, 3], [0, S20 // 2, S20 // 2, 2], [0, S20 // 2, S20 // 2, 2], [3, 2, 2, 5]], np.int64)
    union = np.broadcast_to(area[:, None], (4, 4)) if crowd else area[:, None] + area[None, :] - inter
    ovr = np.where(inter == 0, 0.0, inter.astype(np.float64) / union.astype(np.float64))
    return dict(ovr=ovr[None], a_area=area.astype(np.int32)[None], b_area=area.astype(np.int32)[None])


MAX_STRIDE_BOXES = [((0, 1, 1023, 1023), S20 // 2), ((0, 0, 1023, 1022), S20 // 2), ((0, 0, 1023, 1022), S20 // 2), ((0, 3, 0, 7), 5)]


# ---- nan_box ---------------------------------------------------------------------------------------------------------------------------------------
@cached
def nan_box():
    """a 6 x 8 image; voters with NaN in each of the four box columns in turn (score 2), with +/-2^30 in them, and two plain ones.
    With NaN -> 0 a NaN in column 2 (3) leaves column (row) 0 in the support; with NaN -> -2^31 the slice is empty.  -> (case, ovr)"""
    rs = np.random.RandomState(36)
    h, w = 6, 8
    nan = np.nan
    boxes = [((nan, 0, 7, 5), 2.0), ((0, nan, 7, 5), 2.0), ((0, 0, nan, 5), 2.0), ((0, 0, 7, nan), 2.0), ((-P30, -P30, P30, P30), 0.5),
             ((P30, 0, P30, 5), 2.0), ((0, 0, -P30, 5), 2.0), ((0, 0, 7, 5), 0.3), ((2, 1, 5, 4), 0.4)]
    pool = []
    for k, (box, score) in enumerate(boxes):
        m = rs.rand(h, w) < 0.4
        if k == 2:
            m[:, 0] = True                                      # pixels in column 0 (row 0 for voter 3), where the two rules part
        if k == 3:
            m[0, :] = True
        pool.append((sc.runs_of(m), box, score))
    tops = [p[0] for p in pool[:4]]
    case = mc.vote_case([((h, w), tops, pool)], T=5, A=10, top_stride=40, all_stride=40, out_stride=49, iou_thresh=0.5, binarize_thresh=0.3,
                        seed=36)
    ovr = np.full((1, 5, 10), 0.9)
    ovr[0, 3, :9] = [0, 0, 1, 1, 0, 1, 1, 0, 0]                 # top 3: only the voters whose support a rule decides
    return case, ovr


# ---- im_size_rules ---------------------------------------------------------------------------------------------------------------------------------
IM_SIZES = [(7.9, 5.2), (0.99, 5), (np.nan, 5), (3e9, 1.5), (65536, 32768), (1, 1), (1, 300)]
IM_WINDOWS = [[(0, 35)], [], [], [(0, 2048), (P30 // 2 - 1024, P30 // 2 + 1024), (P30 - 2048, P30)], [], [(0, 1)], [(0, 300)]]


@cached
def im_size_rules():
    """seven images whose sides are fractional, below 1, NaN, above 2^30, of a product 2^31, and 1: four lists each, the same lists as
    tops and as voters, every voter on every top (ovr 0.9).  -> (case, ovr)"""
    small = [[3, 4, 28], [0, 35], [10, 1, 3, 9, 12], [33, 2]]
    tall = [[100, 50, P30 - 150], [P30 - 5, 5], [120, 100], [P30 // 2, 10, 5, 10]]
    row = [[10, 20, 270], [0, 300], [15, 10, 100, 50], [299, 1]]
    one = [[0, 1], [1], [0, 1], [0, 5]]
    lists = [small, small, small, tall, tall, one, row]
    dets = [[(0, 0, 4, 6), (1, 1, 3, 5), (-2, 2, 2.5, 9), (0, 0, 0, 0)]] * 3 + \
           [[(0, 0, 0, P30), (0, 110, 0, 1000), (0, 90, 0, 130), (0, P30 // 2, 0, P30 // 2 + 12)]] * 2 + \
           [[(0, 0, 0, 0), (0, 0, 5, 5), (-1, -1, 0, 0), (1, 0, 1, 0)], [(0, 0, 299, 0), (12, 0, 40, 0), (0, 0, -270, 0), (100, 0, 130, 2)]]
    scores = (0.9, 0.5, 0.7, 0.3)
    images = [(size, ls, [(l, b, s) for l, b, s in zip(ls, bs, scores)]) for size, ls, bs in zip(IM_SIZES, lists, dets)]
    case = mc.vote_case(images, T=5, A=5, top_stride=6, all_stride=5, out_stride=12, iou_thresh=0.5, binarize_thresh=0.3, seed=37)
    ovr = np.full((7, 5, 5), 0.9)
    return case, ovr


def interval_boxes(runs, n_runs, counts, im_size, fill=-1):
    """mask_post_ref.masks_to_boxes by mask_post_ref.interval_box: h w clipped to 2^30 with h kept"""
    N, R = n_runs.shape
    out = dict(boxes=np.full((N, R, 4), fill, np.int32), area=np.full((N, R), fill, np.int32), nonempty=np.full((N, R), fill, np.int32))
    for n in range(N):
        h, hw = mr.sides(im_size[n])[0], sr.pixels(im_size[n])
        for r in range(R if counts is None else mr.clamp(counts[n], R)):
            if hw == 0:
                box, area = (0, 0, 0, 0), 0
            else:
                assert hw % h == 0
                box, area = mr.interval_box(runs[n, r], n_runs[n, r], h, hw // h)
            out["boxes"][n, r], out["area"][n, r], out["nonempty"][n, r] = box, area, int(area > 0)
    return out


# ---- nms_limits ------------------------------------------------------------------------------------------------------------------------------------
def _dets(scores, classes, R=None):
    """dets f32 [1, R, 6]: NaN but for the score and class columns; rows past the given ones NaN scores of class 1"""
    R = R or len(scores)
    d = np.full((1, R, 6), np.nan, np.float32)
    d[0, :, 5] = 1.0
    d[0, :len(scores), 4], d[0, :len(scores), 5] = scores, classes
    return d


@cached
def nms_limits():
    """-> {name: dict(dets, count, ovr, thresh, mode)}"""
    rs = np.random.RandomState(38)
    R, t = 512, 0.5
    inf = np.inf
    values = [0.1, np.nextafter(t, 0), t, np.nextafter(t, 1), 0.9, np.nan, 0.3, 0.45]
    out = {}
    out["r512_distinct"] = dict(dets=_dets(rs.permutation(R).astype(np.float32) / R, np.ones(R)), count=[R], ovr=np.zeros((1, R, R)), mode="IOU")
    out["r512_equal"] = dict(dets=_dets(np.full(R, 0.25, np.float32), np.ones(R)), count=[R], ovr=np.full((1, R, R), 0.75), mode="IOU")
    seeded = rs.choice(values, (1, R, R), p=[0.55, 0.05, 0.05, 0.05, 0.1, 0.02, 0.1, 0.08])
    sd = _dets((rs.randint(0, 200, R) / np.float32(200)).astype(np.float32), 1 + rs.randint(0, 3, R))
    for mode in ("IOU", "IOMA", "CONTAINMENT"):
        out["r512_seeded_" + mode] = dict(dets=sd, count=[R], ovr=seeded, mode=mode)
    out["r1"] = dict(dets=_dets([0.5], [1]), count=[1], ovr=np.full((1, 1, 1), 0.9), mode="IOU")
    six = _dets([0.3, 0.9, 0.5, 0.1], [1] * 4, R=6)
    out["count_0"] = dict(dets=six, count=[0], ovr=np.zeros((1, 6, 6)), mode="IOU")
    out["count_negative"] = dict(dets=six, count=[-3], ovr=np.zeros((1, 6, 6)), mode="IOU")
    out["count_past_r"] = dict(dets=_dets([0.3, 0.9, 0.5, 0.1, 0.2, 0.4], [1] * 6), count=[1 << 30], ovr=np.zeros((1, 6, 6)), mode="IOU")
    # +inf twice, -inf twice, 0.0 and -0.0 (equal: row order), a NaN: the walk is 1, 4, 2, 5, 0, 6, 3, 7
    sc8 = [-inf, inf, 0.0, np.nan, inf, -0.0, -inf, np.nan]
    zero8 = np.zeros((1, 8, 8))
    out["special_scores"] = dict(dets=_dets(sc8, [1] * 8), count=[8], ovr=zero8, mode="IOU")
    tie = zero8.copy()
    tie[0, 2, 5], tie[0, 1, 4], tie[0, 0, 6] = 0.9, 0.9, 0.9    # the earlier row of each equal pair suppresses the later one
    out["special_scores_suppress"] = dict(dets=_dets(sc8, [1] * 8), count=[8], ovr=tie, mode="IOU")
    # NaN classes on rows 1 and 3 under the count: with every value above thresh only they and the best row survive
    out["nan_class"] = dict(dets=_dets([0.9, 0.8, 0.7, 0.6, 0.5], [1, np.nan, 1, np.nan, 1]), count=[5], ovr=np.full((1, 5, 5), 0.9), mode="IOU")
    # classes 0.0 and -0.0 are one class
    out["zero_classes"] = dict(dets=_dets([0.9, 0.8, 0.7], [0.0, -0.0, 2.0]), count=[3], ovr=np.full((1, 3, 3), 0.9), mode="IOU")
    for c in out.values():
        c["count"], c["thresh"] = np.array(c["count"], np.int32), t
    return out


NMS_HAND = {"r512_equal": [0], "r1": [0], "count_0": [], "count_negative": [], "count_past_r": [1, 2, 5, 0, 4, 3],
            "special_scores": [1, 4, 2, 5, 0, 6, 3, 7], "special_scores_suppress": [1, 2, 0, 3, 7], "nan_class": [0, 1, 3], "zero_classes": [0, 2]}


NB = 65535


@cached
def nms_batch():
    """N = 65535 images of R = 2 rows: image n has the scores (n % 3, 1), the value (n % 5) / 4 both ways round, the classes (1, 1) or,
    where n % 7 == 0, (1, 2); thresh 0.5.  -> (case, keep [N, 2], keep_count [N]) with the expectation as a formula"""
    n = np.arange(NB)
    dets = np.full((NB, 2, 6), np.nan, np.float32)
    dets[:, 0, 4], dets[:, 1, 4], dets[:, 0, 5], dets[:, 1, 5] = n % 3, 1, 1, np.where(n % 7 == 0, 2, 1)
    ovr = np.zeros((NB, 2, 2))
    ovr[:, 0, 1] = ovr[:, 1, 0] = (n % 5) / 4.0
    first = np.where(n % 3 == 0, 1, 0)                          # 0 < 1: row 1 leads; 1 == 1: row order; 2 > 1: row 0
    both = ((n % 5) / 4.0 <= 0.5) | (n % 7 == 0)
    keep = np.stack([first, np.where(both, 1 - first, -1)], axis=1).astype(np.int32)
    case = dict(dets=dets, count=np.full(NB, 2, np.int32), ovr=ovr, thresh=0.5, mode="IOU")
    return case, keep, np.where(both, 2, 1).astype(np.int32)


# ---- batch_limit -----------------------------------------------------------------------------------------------------------------------------------
@cached
def batch_limit():
    """N = 65535 images of h = 3, w = 1 + n % 5 with one list each, strides of 4: a = [s, 2, ..] with s = n % (3 w - 1), b = [t, 2, ..]
    with t = (n // 7) % (3 w - 1); the last word of a row is garbage under a count of 3.  -> dict(a, b, im_size, boxes, area, pairs
    by crowd) with the expectations vectorised"""
    rs = np.random.RandomState(39)
    n = np.arange(NB, dtype=np.int64)
    w = 1 + n % 5
    hw = 3 * w
    s, t = n % (hw - 1), (n // 7) % (hw - 1)

    def lists(start):
        runs = rs.randint(0, 1 << 32, (NB, 1, 4), dtype=np.uint64).astype(np.uint32)
        runs[:, 0, 0], runs[:, 0, 1], runs[:, 0, 2] = start, 2, hw - start - 2
        return runs, np.full((NB, 1), 3, np.int32)
    a, b = lists(s), lists(t)
    last = s + 1                                                # the one-run [s, s + 2) lies inside the image: s <= h w - 2
    wraps = s // 3 != last // 3
    boxes = np.stack([s // 3, np.where(wraps, 0, s % 3), last // 3, np.where(wraps, 2, last % 3)], axis=1).astype(np.int32)[:, None]
    inter = np.maximum(0, np.minimum(s, t) + 2 - np.maximum(s, t))
    pairs = {}
    for crowd in (False, True):
        u = np.full(NB, 2) if crowd else 4 - inter
        pairs[crowd] = np.where(inter == 0, 0.0, inter.astype(np.float64) / u.astype(np.float64)).reshape(NB, 1, 1)
    return dict(a=a, b=b, count=np.ones(NB, np.int32), im_size=np.stack([np.full(NB, 3), w], axis=1).astype(np.float32), boxes=boxes,
                area=np.full((NB, 1), 2, np.int32), pairs=pairs)


# ---- far_offsets: the two images at the far end, built small; the GPU test places them behind 4 GiB of rows it never copies ----------------------
FAR_N, FAR_R = 2049, 512


@cached
def far_boxes():
    """the last two images of the boxes call: 512 lists of up to 10 runs on 20 x 30 and 30 x 20 images (runs_stride 1024, so the rows of
    image 2048 start 4 GiB behind the base).  -> (runs [2,512,1024] with garbage behind the lists, n_runs, im_size)"""
    rs = np.random.RandomState(40)
    images = [[mc._list_of(int(rs.randint(2, 11)), 600, rs) for _ in range(FAR_R)] for _ in range(2)]
    runs, n_runs = mc.pack_lists(images, FAR_R, 1024, 40)
    return runs, n_runs, np.array([(20, 30), (30, 20)], np.float32)


@cached
def far_overlaps():
    """the last image of the overlaps call, 10 x 10: a_i = [i % 50, 1 + i % 7], b_j = [j % 60, 1 + j % 11] (strides of 2: ovr [2049, 512,
    512] float64 is just over 4 GiB).  -> (a_runs [1,512,2], b_runs, expectations by crowd from the intervals)"""
    i, j = np.arange(FAR_R, dtype=np.int64), np.arange(FAR_R, dtype=np.int64)
    a = np.stack([i % 50, 1 + i % 7], axis=1).astype(np.uint32)[None]
    b = np.stack([j % 60, 1 + j % 11], axis=1).astype(np.uint32)[None]
    sa, ea, sb, eb = i % 50, i % 50 + 1 + i % 7, j % 60, j % 60 + 1 + j % 11
    inter = np.maximum(0, np.minimum(ea[:, None], eb[None, :]) - np.maximum(sa[:, None], sb[None, :]))
    aa, ab = (ea - sa)[:, None], (eb - sb)[None, :]
    want = {}
    for crowd in (False, True):
        u = np.broadcast_to(aa, inter.shape) if crowd else aa + ab - inter
        want[crowd] = dict(ovr=np.where(inter == 0, 0.0, inter.astype(np.float64) / u.astype(np.float64))[None],
                           a_area=(ea - sa).astype(np.int32)[None], b_area=(eb - sb).astype(np.int32)[None])
    return a, b, want


# ---- what the GPU test compares with ---------------------------------------------------------------------------------------------------------------
VOTE_LIMIT_CASES = {"many_voters": many_voters, "encoder_edges": encoder_edges, "jumps": jumps, "max_stride": max_stride, "nan_box": nan_box,
                    "im_size_rules": im_size_rules}
WINDOWS = {"jumps": lambda c: JUMP_WINDOWS, "im_size_rules": lambda c: IM_WINDOWS}


@functools.lru_cache(maxsize=None)
def voted(name, method, binarize_thresh=None):
    """the answer of a vote case: vote_sparse on the case's windows (the whole image where it has none), vote itself for a negative
    threshold"""
    case, ovr = (negative_threshold_chunks if name == "negative_threshold_chunks" else VOTE_LIMIT_CASES[name])()
    if binarize_thresh is not None:
        case = dict(case, binarize_thresh=binarize_thresh)
    if method == "AVG" and case["binarize_thresh"] < 0:
        return mr.vote(case, ovr, method)
    return mr.vote_sparse(case, ovr, method, WINDOWS.get(name, full_windows)(case))
