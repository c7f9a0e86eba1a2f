"""Pin oracle/oracle.c against the reference's OWN compiled code in oracle/_ref (built by `make -C oracle ref` from
/root/reference; the built .so files travel to the GPU box, the sources do not).  CPU only, bit-exact.

  A1: lib/cppcuda_cffi/src/cpp/roi_align_cpu_loop.cpp (unmodified)   A5/A6: lib/utils_cython/cython_nms.pyx
"""
import os

import numpy as np
import pytest

from detectorch_amd import synth

REF = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "_ref")
pytestmark = pytest.mark.skipif(not os.path.exists(os.path.join(REF, "libref_roialign.so")),
                                reason="oracle/_ref not built (needs /root/reference)")


@pytest.fixture(scope="module")
def ref():
    import ref_harness as rh
    return rh


@pytest.mark.parametrize("ph,pw,sr,scale,C,H,W", [(7, 7, 2, 0.25, 16, 50, 84), (14, 14, 0, 1 / 16., 8, 50, 84),
                                                  (7, 7, 0, 1 / 16., 8, 50, 84), (14, 14, 2, 1 / 32., 16, 25, 42)])
def test_roi_align_vs_reference_cpu_loop(oracle, ref, ph, pw, sr, scale, C, H, W):
    rs = synth.rng(11, ph + sr)
    feat = rs.standard_normal((2, C, H, W)).astype(np.float32)
    rois = synth.make_rois(rs, 64)
    rois5 = np.hstack([rs.randint(0, 2, (64, 1)).astype(np.float32), rois])
    assert np.array_equal(oracle.roi_align_forward(feat, rois5, ph, pw, scale, sr),
                          ref.ref_roi_align(feat, rois5, ph, pw, scale, sr))


@pytest.mark.parametrize("n,thr", [(1, 0.5), (2, 0.5), (1000, 0.7), (3000, 0.7), (1000, 0.3)])
def test_nms_vs_reference_cython(oracle, ref, n, thr):
    cn, _ = ref.load_ref_cython()
    rs = synth.rng(12, n)
    dets = np.hstack([synth.make_rois(rs, n), synth.dedupe_scores(rs.uniform(0, 1, n).astype(np.float32))[:, None]])
    dets = np.ascontiguousarray(dets, np.float32)
    assert np.array_equal(oracle.nms(dets, thr), cn.nms(dets, np.float32(thr)))


def test_nms_threshold_boundary_set_vs_reference_cython(oracle, ref):
    """IoU exactly on / a hair off the threshold, non-positive thresholds, degenerate boxes: oracle == the reference's Cython."""
    from conftest import BOUNDARY_THRESHOLDS, threshold_boundary_dets
    cn, _ = ref.load_ref_cython()
    d = threshold_boundary_dets()
    for thr in BOUNDARY_THRESHOLDS:
        assert np.array_equal(oracle.nms(d, thr), cn.nms(d, np.float32(thr))), thr


@pytest.mark.parametrize("kind", ["default", "sparse"])
@pytest.mark.parametrize("n", [8193, 12000, 16384])
def test_nms_vs_reference_cython_above_8192_rows(oracle, ref, n, kind):
    """the inputs of tests/test_hip_nms_limits.py, part a: oracle == the reference's Cython up to the 16384 rows dtc_nms accepts"""
    import nms_limit_cases as lc
    cn, _ = ref.load_ref_cython()
    d = lc.big_dets(n, kind)
    for thr in (0.5, 0.7):
        assert np.array_equal(oracle.nms(d, thr), cn.nms(d, np.float32(thr))), thr


def test_nms_limit_cases_are_really_there(oracle):
    """more than 8192 survivors (words 128.. of the walk's bit vector hold KEPT rows, the finalize sort takes 16 keys per thread), fewer
    than 8192 (it takes 8), nearly all rows (the reduce ORs rows of every block)"""
    import nms_limit_cases as lc
    d = lc.big_dets(16384, "default")
    assert len(oracle.nms(d, 0.7)) > 8192
    assert len(oracle.nms(d, 0.5)) < 8192
    assert len(oracle.nms(lc.big_dets(16384, "sparse"), 0.5)) > 15000
    for n in lc.TIED_SIZES:
        assert np.unique(lc.big_dets(n, "tied")[:, 4]).size <= 33 and np.unique(lc.big_dets(n, "all_equal")[:, 4]).size == 1


def test_nms_nonfinite_boxes_vs_reference_cython(oracle, ref):
    """+-inf, nan and overflowing coordinates: oracle == the reference's Cython at every threshold the GPU test runs"""
    from conftest import BOUNDARY_THRESHOLDS
    import nms_limit_cases as lc
    cn, _ = ref.load_ref_cython()
    d = lc.nonfinite_box_dets()
    assert np.isnan(d[:, :4]).any() and np.isinf(d[:, :4]).any() and np.unique(d[:, 4]).size == d.shape[0]
    with np.errstate(all="ignore"):
        for thr in (0.3, 0.5, 0.7) + tuple(t for t in BOUNDARY_THRESHOLDS if t <= 0):
            assert np.array_equal(oracle.nms(d, thr), cn.nms(d, np.float32(thr))), thr


def test_nms_odd_scores_vs_reference_cython(oracle, ref):
    """+-inf, -0.0, negative and denormal scores.  Tie-free: oracle == the reference's Cython.  With runs of equal scores (-0.0 == +0.0
    among them) the canonical rule (score descending, index ascending) differs from the reference's on purpose: oracle == a greedy NMS
    in that order, as in test_hip_nms.test_tie_break_orders."""
    import nms_limit_cases as lc
    from test_hip_nms import _greedy_nms
    cn, _ = ref.load_ref_cython()
    d = lc.odd_score_dets(tie_free=True)
    assert np.unique(d[:, 4]).size == d.shape[0] and not np.isnan(d[:, 4]).any()
    for thr in (0.3, 0.5, 0.7):
        assert np.array_equal(oracle.nms(d, thr), cn.nms(d, np.float32(thr))), thr
    d = lc.odd_score_dets()
    s = d[:, 4]
    assert np.isposinf(s).sum() == 2 and np.isneginf(s).sum() == 2 and (s < 0).any() and (s == np.float32(1e-42)).any()
    assert (np.signbit(s) & (s == 0)).any() and (~np.signbit(s) & (s == 0)).any() and not np.isnan(s).any()
    order = np.lexsort((np.arange(d.shape[0]), -s))
    for thr in (0.3, 0.5, 0.7):
        assert np.array_equal(oracle.nms(d, thr), _greedy_nms(d, thr, list(order))), thr


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
def test_soft_nms_limit_cases_vs_reference_cython(oracle, ref, method):
    """the inputs of tests/test_hip_nms_limits.py, part g (tied, non-finite and NaN scores, non-finite boxes, score thresholds):
    oracle == the reference's Cython, NaN compared as NaN.  The 6000-row cases are left out: the Cython needs 13-20 s per method."""
    import nms_limit_cases as lc
    cn, _ = ref.load_ref_cython()
    m = {"hard": 0, "linear": 1, "gaussian": 2}[method]
    ran = 0
    for name, (dets, kw) in lc.soft_cases().items():
        if dets.shape[0] > 1500:
            continue
        with np.errstate(all="ignore"):
            rd, rk = cn.soft_nms(dets.copy(), np.float32(kw["sigma"]), np.float32(kw["overlap_thresh"]), np.float32(kw["score_thresh"]),
                                 np.uint8(m))
        d, k = oracle.soft_nms(dets, kw["sigma"], kw["overlap_thresh"], kw["score_thresh"], method)
        assert np.array_equal(k, np.asarray(rk, np.int64)), name
        assert lc.same_rows(d, rd), name
        ran += 1
    assert ran >= 9


@pytest.mark.parametrize("method", ["hard", "linear", "gaussian"])
def test_soft_nms_vs_reference_cython(oracle, ref, method):
    cn, _ = ref.load_ref_cython()
    rs = synth.rng(13, 0)
    n = 700
    dets = np.hstack([synth.make_rois(rs, n, min_side=30, max_side=400),
                      synth.dedupe_scores(rs.uniform(0, 1, n).astype(np.float32))[:, None]])
    dets = np.ascontiguousarray(dets, np.float32)
    m = {"hard": 0, "linear": 1, "gaussian": 2}[method]
    rd, rk = cn.soft_nms(dets, np.float32(0.5), np.float32(0.3), np.float32(0.001), np.uint8(m))
    d, k = oracle.soft_nms(dets, 0.5, 0.3, 0.001, method)
    assert np.array_equal(k, np.asarray(rk, np.int64))
    assert np.array_equal(d, rd)


def test_bbox_overlaps_and_box_voting_vs_reference(oracle, ref):
    """orc_bbox_overlaps vs the reference's own Cython build; orc_box_voting vs what lib/utils/boxes.py:280 returned on the same
    inputs (tests/golden/box_voting_many_voters.npz, tests/golden/make_golden.py; hundreds of voters per top det: numpy's pairwise
    float32 sum beyond 128 elements is on the path)."""
    from conftest import golden
    _, cb = ref.load_ref_cython()
    g = golden("box_voting_many_voters")
    rs = synth.rng(13, 0)
    for t in range(6):
        b = synth.make_rois(rs, 150 + 37 * t); q = synth.make_rois(rs, 90 + 11 * t)
        assert np.array_equal(oracle.bbox_overlaps(b, q), cb.bbox_overlaps(np.ascontiguousarray(b), np.ascontiguousarray(q)))
    base = np.array([[50, 60, 200, 220], [300, 100, 420, 300], [10, 10, 600, 400]], np.float32)
    for t in range(4):
        n = 400 + 300 * t
        a = base[rs.randint(0, 3, n)] + rs.standard_normal((n, 4)).astype(np.float32) * 3
        all_d = np.ascontiguousarray(np.hstack([a, rs.uniform(0, 1, (n, 1))]), np.float32)
        top = np.ascontiguousarray(all_d[rs.choice(n, 10, replace=False)])
        assert np.array_equal(all_d, g["all_dets%d" % t]) and np.array_equal(top, g["top_dets%d" % t]), t
        assert np.array_equal(oracle.box_voting(top, all_d, 0.5), g["vote%d" % t]), t
