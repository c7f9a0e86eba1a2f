"""Inputs of the NMS / Soft-NMS / segment-sort limit tests (test support, not a test module): shared by tests/test_hip_nms_limits.py
(GPU, against the oracle) and tests/test_oracle_ref.py (CPU, the oracle against the reference's compiled Cython on the same inputs).
numpy only, fixed seeds through synth.rng; every expectation is computed by the oracle at test time.

No builder puts a NaN into the scores of HARD NMS: the oracle's qsort comparator is no total order on NaN."""
import numpy as np

from detectorch_amd import synth

MAX_NMS_ROWS = 16384                             # nms.hip: dtc_nms / dtc_segment_sort_desc accept n <= 16384
MAX_SOFT_ROWS = 6000                             # nms.hip: dtc_soft_nms accepts n <= 6000
NONFINITE = (np.inf, -np.inf, np.nan, 3e38, -3e38, 1e20, 1e19)


def _pack(b, s):
    return np.ascontiguousarray(np.hstack([b, np.asarray(s, np.float32)[:, None]]), np.float32)


# ---- dtc_nms above 8192 rows ---------------------------------------------------------------------------------------------------
BIG_SIZES = (8192, 8193, 12000, 16383, 16384)    # > 8192: 16 keys per thread in the sorts, words 128.. of `removed`, 256 x 16 reduce
TIED_SIZES = (9000, 16384)


def big_dets(n, kind="default"):
    """dets [n, 5]: "default" the boxes and tie-free scores of test_hip_nms._dets(n, n); "sparse" small boxes (sides 4 ... 24: most rows
    survive); "tied" the default set with scores quantised to 1/32; "all_equal" with every score 0.5 (the index half of the sort key
    decides everything)."""
    rs = synth.rng(7, n)
    b = synth.make_rois(rs, n, min_side=4, max_side=24) if kind == "sparse" else synth.make_rois(rs, n)
    s = synth.dedupe_scores(rs.uniform(0.0, 1.0, n).astype(np.float32))
    if kind == "tied":
        s = (np.round(s * 32) / 32).astype(np.float32)
    elif kind == "all_equal":
        s = np.full(n, 0.5, np.float32)
    else:
        assert kind in ("default", "sparse"), kind
    return _pack(b, s)


# ---- non-finite boxes, odd scores -------------------------------------------------------------------------------------------------
def _replace_coords(b, rows, values):
    """one coordinate of each of `rows` replaced: coordinate and value both in turn"""
    for k, r in enumerate(rows):
        b[r, k % 4] = np.float32(values[(k // 4 + k) % len(values)])
    return b


def nonfinite_box_dets():
    """600 make_rois rows with tie-free scores; every tenth row carries one coordinate replaced, in turn, by +inf, -inf, nan, 3e38,
    -3e38, 1e20, 1e19 (differences and areas that overflow, inf - inf, areas whose product is finite but whose sum is not)"""
    rs = synth.rng(71, 0)
    n = 600
    b = _replace_coords(synth.make_rois(rs, n), range(5, n, 10), NONFINITE)
    return _pack(b, synth.dedupe_scores(rs.uniform(0.0, 1.0, n).astype(np.float32)))


def odd_score_dets(tie_free=False):
    """300 rows whose scores include +inf, -inf, -0.0 next to +0.0, negative scores, a denormal (1e-42) and runs of equal values (among
    them two +inf, two -inf and several zeros of either sign); no NaN.  tie_free: the same rows with one of each special value and no
    runs (-0.0 == +0.0 counts as a tie, so only -0.0 stays)."""
    rs = synth.rng(72, 0)
    n = 300
    b = synth.make_rois(rs, n, min_side=40, max_side=300)
    s = synth.dedupe_scores(rs.uniform(0.0, 1.0, n).astype(np.float32))
    s[7] = np.inf; s[150] = -np.inf; s[31] = -0.0; s[90] = -0.25; s[91] = 1e-42; s[200] = -3e38
    if not tie_free:
        s[250] = np.inf; s[2] = -np.inf; s[30] = 0.0; s[32] = 0.0; s[180] = -0.0; s[92] = 1e-42
        s[100:140] = np.float32(0.5); s[210:230:2] = np.float32(0.75); s[260:270] = -0.25
    return _pack(b, s)


# ---- dtc_segment_sort_desc -----------------------------------------------------------------------------------------------------
SORT_CASES = {"long": (16384, [16384, 8193, 1, 0]), "short": (300, [1, 2, 255, 257, 300 + 7])}    # name -> (n_stride, counts)


def sort_scores(S, n_stride, kind):
    """[S, n_stride] float32: "odd" tiles the scores of odd_score_dets() (specials and runs in every segment, shifted per segment),
    "tied" uniform scores quantised to 1/32"""
    rs = synth.rng(73, n_stride)
    if kind == "tied":
        return (np.round(rs.uniform(0.0, 1.0, (S, n_stride)) * 32) / 32).astype(np.float32)
    assert kind == "odd", kind
    base = odd_score_dets()[:, 4]
    out = synth.dedupe_scores(rs.uniform(0.0, 1.0, (S, n_stride)).astype(np.float32))
    for s in range(S):
        idx = (np.arange(base.size) * max(n_stride // base.size, 1) + 3 * s) % n_stride
        out[s, idx] = base
        out[s, :2] = (-0.0, 0.0) if s % 2 else (0.0, -0.0)         # the only row of a 1-row segment, the two of a 2-row one
    return out


def sort_expected(scores_seg, count):
    """order of one segment: score descending, index ascending; -0.0 == +0.0"""
    s = scores_seg[:count]
    return np.lexsort((np.arange(count), -s)).astype(np.int32)


# ---- sorted segments for dtc_nms_sorted ------------------------------------------------------------------------------------------
def spread_boxes(seed, n):
    """n boxes that mostly survive NMS at 0.7 (make_rois, moderate sides)"""
    return synth.make_rois(synth.rng(74, seed), n, min_side=16, max_side=120)


def cluster_boxes(seed, n):
    """n boxes around one place: heavy overlap, a handful of survivors"""
    rs = synth.rng(75, seed)
    base = np.array([300, 200, 520, 380], np.float32)
    return (base + rs.uniform(-14, 14, (n, 4))).astype(np.float32)


def mixed_boxes(seed, n):
    """survivors thin out and come back: alternating runs of cluster and spread rows, run lengths 1 ... 200"""
    rs = synth.rng(76, seed)
    sp, cl = spread_boxes(1000 + seed, n), cluster_boxes(1000 + seed, n)
    out = np.empty((n, 4), np.float32)
    pos, use_cl = 0, False
    while pos < n:
        run = int(rs.randint(1, 201))
        out[pos:pos + run] = (cl if use_cl else sp)[pos:pos + run]
        pos += run
        use_cl = not use_cl
    return out


def as_dets(boxes):
    """sorted boxes [c, 4] -> dets [c, 5] with strictly descending scores, for oracle.nms (kept original index == kept position)"""
    c = boxes.shape[0]
    return _pack(boxes, np.linspace(1.0, 0.0, c, endpoint=False, dtype=np.float64).astype(np.float32)) if c else np.zeros((0, 5), np.float32)


def pack_segments(segs, n_stride, fill=None):
    """list of [c_s, 4] -> (boxes [S, n_stride, 4], counts int32 [S]); rows past a count: `fill` boxes (default: one big box that would
    suppress, and be suppressed by, most rows if it were read)"""
    S = len(segs)
    boxes = np.empty((S, n_stride, 4), np.float32)
    boxes[:] = np.array([0, 0, 1332, 799], np.float32) if fill is None else fill
    counts = np.zeros(S, np.int32)
    for s, b in enumerate(segs):
        assert b.shape[0] <= n_stride
        boxes[s, :b.shape[0]] = b
        counts[s] = b.shape[0]
    return boxes, counts


def n1_of(max_keep):
    """nms.hip, dtc_nms_sorted: rows of the first phase of a keep[:max_keep] call; two phases run when n_stride >= 2 * n1"""
    return max(16, (2 * max_keep + 63) // 64) * 64


def lds_walk(n_seg, n_stride):
    """nms.hip, dtc_nms_sorted: does the LDS walk (nms_reduce_lds_kernel) run, or the one-wave walk"""
    ncb = (n_stride + 63) // 64
    return n_seg <= 160 and 4 <= ncb <= 16 and ncb % 2 == 0 and (ncb * 64 * ncb + ncb * 64) * 8 <= 150 * 1024


KEEP_STRIDE_CASES = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 300), (500, 200)]          # (max_keep, keep_stride)
KEEP_STRIDE_N = (1000, 2500)                                                           # the LDS walk, the one-wave walk

WALK_N_STRIDES = (320, 384, 640, 896, 1024, 1088)                                      # ncb 5, 6, 10, 14, 16, 17


def walk_segments(n_stride):
    """3 ragged segments [n_stride, n_stride - 37, 65]"""
    return [mixed_boxes(n_stride, n_stride), spread_boxes(n_stride + 1, n_stride - 37), mixed_boxes(n_stride + 2, 65)]


def many_long_segments():
    """161 segments of 1024 rows: the first 160 alone take the LDS walk, all 161 the one-wave walk.  Eight distinct box sets, each
    cut to the segment's own count (1024, 1023, ... in steps: counts differ so that a segment read at a neighbour's count shows)."""
    base = [mixed_boxes(50 + k, 1024) if k % 2 else spread_boxes(50 + k, 1024) for k in range(8)]
    return [base[s % 8][:1024 - (s // 8) * 13] for s in range(161)]


GX1_S, GX1_N = 2100, 130                         # n_seg > 2048: the mask grid is (1, 1, n_seg), one workgroup walks all 6 tile groups
GX1_COUNTS = (0, 1, 64, 65, 129, 130)


def gx1_segments():
    rs = synth.rng(77, 0)
    counts = np.array(GX1_COUNTS)[rs.randint(0, len(GX1_COUNTS), GX1_S)]
    counts[:6] = GX1_COUNTS
    pool = [mixed_boxes(80 + k, GX1_N) for k in range(16)]
    return [pool[int(rs.randint(0, 16))][GX1_N - c:] for c in counts]


TWO_PHASE_CASES = [(2047, 100), (2048, 100), (2048, 1), (2048, 64), (2048, 512), (2175, 513), (2176, 513)]   # (n_stride, max_keep)


def two_phase_segments(n_stride, max_keep):
    """4 segments: spread rows (max_keep reached early); n1 tight cluster rows, then a spread tail (max_keep reached past row n1, or
    never); count == n1; count == n1 + 1 (both spread behind a cluster head, so that the last rows matter)."""
    n1 = n1_of(max_keep)
    assert n1 + 1 <= n_stride
    seed = n_stride * 7 + max_keep
    late = np.vstack([cluster_boxes(seed, n1), spread_boxes(seed + 1, n_stride - n1)])
    head = n1 - 40
    at = np.vstack([cluster_boxes(seed + 2, head), spread_boxes(seed + 3, n1 - head)])
    over = np.vstack([cluster_boxes(seed + 4, head), spread_boxes(seed + 5, n1 + 1 - head)])
    return [spread_boxes(seed + 6, n_stride), late, at, over]


# ---- Soft-NMS ---------------------------------------------------------------------------------------------------------------------
SOFT_METHODS = ("hard", "linear", "gaussian")


def soft_cases():
    """name -> (dets [n, 5], dict of sigma / overlap_thresh / score_thresh)"""
    kw = dict(sigma=0.5, overlap_thresh=0.3, score_thresh=0.001)
    out = {}
    rs = synth.rng(78, 0)
    n = 700
    b = synth.make_rois(rs, n, min_side=30, max_side=400)
    s = rs.uniform(0.0, 1.0, n).astype(np.float32)
    out["ties16"] = (_pack(b, (np.round(s * 16) / 16).astype(np.float32)), kw)      # the first maximum of the argmax decides
    out["all_equal"] = (_pack(b, np.full(n, 0.5, np.float32)), kw)
    rs = synth.rng(78, 1)
    n = 300
    b = synth.make_rois(rs, n, min_side=30, max_side=400)
    s = synth.dedupe_scores(rs.uniform(0.0, 1.0, n).astype(np.float32))
    out["inf_boxes"] = (_pack(_replace_coords(b.copy(), range(5, n, 10), [v for v in NONFINITE if v == v]), s), kw)
    sn = s.copy()
    sn[[3, 70, 150, 299]] = np.nan
    out["nan_scores"] = (_pack(b, sn), kw)
    si = s.copy()
    si[11] = np.inf; si[120] = np.inf; si[40] = -np.inf; si[250] = -0.5
    out["inf_scores"] = (_pack(b, si), dict(kw, score_thresh=-1.0))                 # (a negative threshold keeps the -0.5 row in play)
    out["inf_scores_thresh"] = (_pack(b, si), kw)
    rs = synth.rng(78, 2)
    d200 = _pack(synth.make_rois(rs, 200, min_side=30, max_side=400), synth.dedupe_scores(rs.uniform(0.0, 1.0, 200).astype(np.float32)))
    for st in (0.0, 1.0, 2.0):                                                       # nothing discarded ... every decayed row discarded
        out["score_thresh_%g" % st] = (d200, dict(kw, score_thresh=st))
    rs = synth.rng(78, 3)
    n = MAX_SOFT_ROWS
    s = synth.dedupe_scores(rs.uniform(0.0, 1.0, n).astype(np.float32))
    out["n6000"] = (_pack(synth.make_rois(rs, n), s), kw)
    out["n6000_sparse"] = (_pack(synth.make_rois(rs, n, min_side=4, max_side=24), s), kw)
    return out


def same_rows(a, b):
    """bit comparison of float32 arrays with NaN == NaN (any payload) and -0.0 != +0.0"""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    an, bn = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(an, bn) and np.array_equal(a.view(np.uint32)[~an], b.view(np.uint32)[~bn]))
