"""A5 / A6 at the limits of their C ABI: dtc_nms above 8192 rows, dtc_segment_sort_desc on its own, dtc_nms_sorted where keep_stride
caps, on either walk, past 2048 segments, on both sides of the two-phase trigger and on a poisoned workspace; non-finite boxes, odd and
tied scores; Soft-NMS on ties, non-finite values, NaN scores and 6000 rows.  Inputs: tests/nms_limit_cases.py.  Every comparison is an
exact integer or bit comparison against the oracle (pinned to the reference's Cython on the same inputs by tests/test_oracle_ref.py).
-m gpu."""
import numpy as np
import pytest
import torch

import nms_limit_cases as lc
from conftest import BOUNDARY_THRESHOLDS

pytestmark = pytest.mark.gpu

THR = 0.7                                        # of every dtc_nms_sorted test here


@pytest.fixture(scope="module")
def hip():
    from detectorch_amd import hip as h
    h.lib()
    return h


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def gpu_nms(hip, d, thr):
    return hip.nms(cu(d), thr).cpu().numpy()


# ---- a. dtc_nms from 8192 to 16384 rows, non-finite boxes, odd scores ---------------------------------------------------------------
@pytest.mark.parametrize("n", lc.BIG_SIZES)
def test_nms_above_8192_rows(hip, oracle, n):
    """n > 8192: 16 keys per thread in segment_sort_desc_kernel and (with more than 8192 survivors) in nms_finalize_kernel, 128 KB of
    dynamic LDS, words 128 ... 255 of the walk's bit vector, 256 row blocks x 16 column chunks in the reduce"""
    kept = {}
    for kind, thr in (("default", 0.5), ("default", 0.7), ("sparse", 0.5)):
        d = lc.big_dets(n, kind)
        ref = oracle.nms(d, thr)
        kept[kind, thr] = len(ref)
        assert np.array_equal(gpu_nms(hip, d, thr), ref), (kind, thr)
    if n == 16384:                               # the cases are really there: survivors on either side of 8192 and nearly all rows
        assert kept["default", 0.7] > 8192 > kept["default", 0.5] and kept["sparse", 0.5] > 15000


@pytest.mark.parametrize("kind", ["tied", "all_equal"])
@pytest.mark.parametrize("n", lc.TIED_SIZES)
def test_nms_tied_scores_above_8192_rows(hip, oracle, n, kind):
    """the index half of the key decides, through the 16-keys-per-thread network and through the finalize sort"""
    d = lc.big_dets(n, kind)
    assert np.array_equal(gpu_nms(hip, d, 0.5), oracle.nms(d, 0.5))


def test_nms_16385_rows_is_unsupported(hip):
    with pytest.raises(RuntimeError, match="UNSUPPORTED"):
        hip.nms(torch.zeros((lc.MAX_NMS_ROWS + 1, 5), device="cuda"), 0.5)


def test_nms_nonfinite_boxes(hip, oracle):
    """+-inf, nan, +-3e38, 1e20, 1e19 in one coordinate of every tenth row: areas, unions and intersections that are inf or NaN go
    through the 2^-21 band of nms_mask_kernel (its ballot takes the division path whenever `m > 0` is false, NaN included)"""
    d = lc.nonfinite_box_dets()
    for thr in (0.3, 0.5, 0.7) + tuple(t for t in BOUNDARY_THRESHOLDS if t <= 0):
        assert np.array_equal(gpu_nms(hip, d, thr), oracle.nms(d, thr)), thr


def test_nms_odd_scores(hip, oracle):
    """+-inf, -0.0 next to +0.0, negative and denormal scores, runs of equal ones (no NaN)"""
    for d in (lc.odd_score_dets(), lc.odd_score_dets(tie_free=True)):
        for thr in (0.3, 0.5, 0.7):
            assert np.array_equal(gpu_nms(hip, d, thr), oracle.nms(d, thr)), thr


# ---- b. dtc_segment_sort_desc on its own ------------------------------------------------------------------------------------------------
I32_SENTINEL, F32_SENTINEL = -7, np.float32(-12345.0)


@pytest.mark.parametrize("kind", ["odd", "tied"])
@pytest.mark.parametrize("case", sorted(lc.SORT_CASES))
def test_segment_sort_desc(hip, case, kind):
    """several segments in one launch, counts (one above n_stride: clamped) and counts = NULL, score stride 1 and 5, box stride 4 and 5,
    each optional output NULL in turn: order == lexsort(index, -score) per segment, gathered scores and boxes bit-equal (the sign of
    -0.0 kept), a sentinel segment behind every output intact"""
    n_stride, counts = lc.SORT_CASES[case]
    S = len(counts)
    scores = lc.sort_scores(S, n_stride, kind)
    boxes = lc.spread_boxes(n_stride, S * n_stride).reshape(S, n_stride, 4)
    dets = np.concatenate([boxes, scores[:, :, None]], axis=2).astype(np.float32)
    d_scores, d_boxes, d_dets = cu(scores), cu(boxes), cu(dets)
    d_counts = cu(np.array(counts, np.int32))
    score_args = {1: d_scores, 5: d_dets.view(-1)[4:]}
    box_args = {4: d_boxes, 5: d_dets}
    expected = {}
    for use_counts in (True, False):
        cs = [min(c, n_stride) if use_counts else n_stride for c in counts]
        expected[use_counts] = (cs, [lc.sort_expected(scores[s], c) for s, c in enumerate(cs)])
    for use_counts in (True, False):
        cs, orders = expected[use_counts]
        for ss in (1, 5):
            for bs in (4, 5):
                for null in (None, "order", "sorted_boxes", "sorted_scores"):
                    out = dict(order=torch.full((S + 1, n_stride), I32_SENTINEL, dtype=torch.int32, device="cuda"),
                               sorted_boxes=torch.full((S + 1, n_stride, 4), float(F32_SENTINEL), device="cuda"),
                               sorted_scores=torch.full((S + 1, n_stride), float(F32_SENTINEL), device="cuda"))
                    if null:
                        out[null] = None
                    hip.call("dtc_segment_sort_desc", scores=score_args[ss], score_stride_elems=ss,
                             boxes=None if null == "sorted_boxes" and bs == 5 else box_args[bs], box_stride_elems=bs,
                             counts=d_counts if use_counts else None, n_seg=S, n_stride=n_stride, **out)
                    torch.cuda.synchronize()
                    tag = (use_counts, ss, bs, null)
                    got = {k: v.cpu().numpy() for k, v in out.items() if v is not None}
                    for s in range(S):
                        c, o = cs[s], orders[s]
                        if "order" in got:
                            assert np.array_equal(got["order"][s, :c], o), (tag, s)
                        if "sorted_scores" in got:
                            assert np.array_equal(got["sorted_scores"][s, :c].view(np.uint32), scores[s][o].view(np.uint32)), (tag, s)
                        if "sorted_boxes" in got:
                            assert np.array_equal(got["sorted_boxes"][s, :c].view(np.uint32), boxes[s][o].view(np.uint32)), (tag, s)
                    for k, v in got.items():
                        assert (v[S] == (I32_SENTINEL if k == "order" else F32_SENTINEL)).all(), (tag, k)


# ---- dtc_nms_sorted through the C ABI, with sentinels and a chosen workspace fill --------------------------------------------------------
def run_sorted(hip, boxes, counts, max_keep, keep_stride, fill=None):
    """-> (keep [S + 1, keep_stride] with a sentinel row, keep_count [S]); fill: the byte the workspace is filled with before the call"""
    S, N = boxes.shape[0], boxes.shape[1]
    nbytes = hip.call("dtc_nms_sorted_workspace_bytes", n_seg=S, n_stride=N)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device="cuda") if fill is None else \
        torch.full((nbytes,), fill, dtype=torch.uint8, device="cuda")
    keep = torch.full((S + 1, keep_stride), I32_SENTINEL, dtype=torch.int32, device="cuda")
    cnt = torch.full((S,), I32_SENTINEL, dtype=torch.int32, device="cuda")
    hip.call("dtc_nms_sorted", boxes=cu(boxes), counts=None if counts is None else cu(np.asarray(counts, np.int32)), n_seg=S,
             n_stride=N, thresh=THR, max_keep=max_keep, workspace=ws, workspace_bytes=nbytes, keep=keep, keep_stride=keep_stride,
             keep_count=cnt)
    torch.cuda.synchronize()
    return keep.cpu().numpy(), cnt.cpu().numpy()


def sorted_refs(oracle, segs, cap):
    """per segment: the first `cap` (0: all) kept positions of the greedy walk, ascending"""
    return [np.sort(oracle.nms(lc.as_dets(b), THR, max_keep=cap)) if b.shape[0] else np.zeros(0, np.int64) for b in segs]


def check_sorted(keep, cnt, refs, tag=None):
    S = len(refs)
    for s in range(S):
        assert cnt[s] == len(refs[s]), (tag, s, cnt[s], len(refs[s]))
        assert np.array_equal(keep[s, :cnt[s]], refs[s]), (tag, s)
        assert (keep[s, cnt[s]:] == I32_SENTINEL).all(), (tag, s)          # nothing written past the count
    assert (keep[S] == I32_SENTINEL).all(), tag                             # ... nor past the last segment's keep_stride


# ---- c. keep_stride as the cap ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", lc.KEEP_STRIDE_N)
def test_keep_stride_caps_the_kept_positions(hip, oracle, N):
    """cap = max_keep > 0 ? min(max_keep, keep_stride) : keep_stride, on the LDS walk (N = 1000) and the one-wave walk (N = 2500, where
    max_keep = 500 also runs the two phases): segments with more survivors than keep_stride and with fewer"""
    segs = [lc.spread_boxes(N, N), lc.mixed_boxes(N + 1, N - 100), lc.cluster_boxes(N + 2, N // 2)]
    assert lc.lds_walk(len(segs), N) == (N == 1000)
    boxes, counts = lc.pack_segments(segs, N)
    survivors = [len(r) for r in sorted_refs(oracle, segs, 0)]
    assert survivors[0] > 500 and survivors[1] > 300 and survivors[2] < 63
    for max_keep, keep_stride in lc.KEEP_STRIDE_CASES:
        cap = min(max_keep, keep_stride) if max_keep > 0 else keep_stride
        refs = sorted_refs(oracle, segs, cap)
        assert [len(r) for r in refs] == [min(cap, n) for n in survivors]
        keep, cnt = run_sorted(hip, boxes, counts, max_keep, keep_stride)
        check_sorted(keep, cnt, refs, (max_keep, keep_stride))


# ---- d. walk selection ------------------------------------------------------------------------------------------------------------------
def walk_case(n_stride):
    segs = lc.walk_segments(n_stride)
    assert [b.shape[0] for b in segs] == [n_stride, n_stride - 37, 65]
    return segs, lc.pack_segments(segs, n_stride)


@pytest.mark.parametrize("n_stride", lc.WALK_N_STRIDES)
def test_walk_selection_by_column_blocks(hip, oracle, n_stride):
    """ncb = 5, 6, 10, 14, 16, 17: the LDS walk on the even ones up to 16, the one-wave walk on the others; ragged counts, the short
    segment's column blocks past its own count are never written"""
    ncb = (n_stride + 63) // 64
    assert lc.lds_walk(3, n_stride) == (ncb % 2 == 0 and ncb <= 16)
    segs, (boxes, counts) = walk_case(n_stride)
    keep, cnt = run_sorted(hip, boxes, counts, 0, n_stride)
    check_sorted(keep, cnt, sorted_refs(oracle, segs, 0))


def test_walk_selection_by_segment_count(hip, oracle):
    """the same 160 segments of 1024 rows as S = 160 (the LDS walk) and, with one more, as S = 161 (the one-wave walk)"""
    segs = lc.many_long_segments()
    assert len(segs) == 161 and lc.lds_walk(160, 1024) and not lc.lds_walk(161, 1024)
    refs = sorted_refs(oracle, segs, 0)
    boxes, counts = lc.pack_segments(segs, 1024)
    k160, c160 = run_sorted(hip, boxes[:160], counts[:160], 0, 1024)
    k161, c161 = run_sorted(hip, boxes, counts, 0, 1024)
    check_sorted(k160, c160, refs[:160], 160)
    check_sorted(k161, c161, refs, 161)
    assert np.array_equal(k160[:160], k161[:160]) and np.array_equal(c160, c161[:160])


def test_mask_grid_of_one_workgroup_per_segment(hip, oracle):
    """n_seg = 2100 > 2048: the mask grid is (1, 1, n_seg), one workgroup strides over every tile group of its segment; counts from
    {0, 1, 64, 65, 129, 130}, every segment checked"""
    segs = lc.gx1_segments()
    assert len(segs) == lc.GX1_S > 2048 and {b.shape[0] for b in segs} == set(lc.GX1_COUNTS)
    boxes, counts = lc.pack_segments(segs, lc.GX1_N)
    keep, cnt = run_sorted(hip, boxes, counts, 0, lc.GX1_N)
    check_sorted(keep, cnt, sorted_refs(oracle, segs, 0))


# ---- e. the two-phase boundary ----------------------------------------------------------------------------------------------------------
def two_phase_case(oracle, n_stride, max_keep):
    """-> (segments, refs); asserts from the oracle that the cases occur where max_keep allows them"""
    n1 = lc.n1_of(max_keep)
    segs = lc.two_phase_segments(n_stride, max_keep)
    assert [b.shape[0] for b in segs] == [n_stride, n_stride, n1, n1 + 1]
    refs = sorted_refs(oracle, segs, max_keep)
    assert len(refs[0]) == max_keep and refs[0][-1] < n1                    # the cap is reached before row n1
    if max_keep > 1:
        assert len(refs[1]) == max_keep and refs[1][-1] >= n1               # ... after row n1 (a two-phase call redoes the segment)
    if max_keep >= 64:
        assert len(refs[2]) < max_keep and len(refs[3]) < max_keep          # ... never
        assert refs[2][-1] == n1 - 1 and refs[3][-1] == n1                  # the last row of either is kept: it has to be looked at
    return segs, refs


@pytest.mark.parametrize("n_stride,max_keep", lc.TWO_PHASE_CASES)
def test_two_phase_boundary(hip, oracle, n_stride, max_keep):
    """phase one covers n1 = max(16, ceil(2 * max_keep / 64)) * 64 rows, two phases run when n_stride >= 2 * n1: shapes on either side"""
    n1 = lc.n1_of(max_keep)
    assert (n_stride >= 2 * n1) == ((n_stride, max_keep) not in ((2047, 100), (2175, 513)))
    segs, refs = two_phase_case(oracle, n_stride, max_keep)
    boxes, counts = lc.pack_segments(segs, n_stride)
    keep, cnt = run_sorted(hip, boxes, counts, max_keep, max_keep)
    check_sorted(keep, cnt, refs)


# ---- f. poisoned workspace --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", [0xFF, 0x00])
def test_poisoned_workspace(hip, oracle, fill):
    """the workspace needs no initialisation: words left of the diagonal, rows past a count, column blocks past a short segment's own
    ncb and the second phase's counts are never read before they are written.  0xFF: every stale mask word says "suppresses
    everything", a stale count is negative; 0x00: nothing suppresses, a stale count is an empty segment."""
    for n_stride in lc.WALK_N_STRIDES:
        segs, (boxes, counts) = walk_case(n_stride)
        keep, cnt = run_sorted(hip, boxes, counts, 0, n_stride, fill)
        check_sorted(keep, cnt, sorted_refs(oracle, segs, 0), n_stride)
    segs = lc.many_long_segments()
    refs = sorted_refs(oracle, segs, 0)
    boxes, counts = lc.pack_segments(segs, 1024)
    for S in (160, 161):
        keep, cnt = run_sorted(hip, boxes[:S], counts[:S], 0, 1024, fill)
        check_sorted(keep, cnt, refs[:S], S)
    for n_stride, max_keep in lc.TWO_PHASE_CASES:
        if n_stride != 2048:
            continue
        segs, refs = two_phase_case(oracle, n_stride, max_keep)
        boxes, counts = lc.pack_segments(segs, n_stride)
        keep, cnt = run_sorted(hip, boxes, counts, max_keep, max_keep, fill)
        check_sorted(keep, cnt, refs, (n_stride, max_keep))


# ---- g. Soft-NMS ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def soft_inputs():
    return lc.soft_cases()


SOFT_NAMES = ["ties16", "all_equal", "inf_boxes", "nan_scores", "inf_scores", "inf_scores_thresh", "score_thresh_0", "score_thresh_1",
              "score_thresh_2", "n6000", "n6000_sparse"]


@pytest.mark.parametrize("method", lc.SOFT_METHODS)
@pytest.mark.parametrize("name", SOFT_NAMES)
def test_soft_nms_limit_cases(hip, oracle, soft_inputs, name, method):
    """survivors' rows and indices bit-equal to the oracle, NaN compared as NaN.  ties16 / all_equal: the first maximum of the argmax
    decides every pick.  nan_scores: a NaN score is picked only when it sits at the walk's own row i and is otherwise passed over, as
    `maxscore < boxes[pos, 4]` does (cython_nms.pyx:128-132).  n6000: the entry's limit."""
    from detectorch_amd.utils import boxes as box_utils
    assert sorted(soft_inputs) == sorted(SOFT_NAMES)
    dets, kw = soft_inputs[name]
    rd, rk = oracle.soft_nms(dets, kw["sigma"], kw["overlap_thresh"], kw["score_thresh"], method)
    gd, gk = box_utils.soft_nms(dets, kw["sigma"], kw["overlap_thresh"], kw["score_thresh"], method)
    assert np.array_equal(gk, rk)
    assert lc.same_rows(gd, rd)
