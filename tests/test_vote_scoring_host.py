"""Host side of the bbox-vote scorings (dtc_postprocess_detections_ex2, dtc_box_voting_scored): the exported symbols, their
argument validation and workspace size without a GPU, and the checker the GPU tests compare with (vote_scoring_ref), pinned
against the reference's own outputs (tests/golden/postprocess_vote_scoring.npz, tests/golden/make_vote_scoring_golden.py)."""
import ctypes
import os

import numpy as np
import pytest

from conftest import ROOT, golden
import vote_scoring_ref as vsr

EINVAL = -1


def _opt(hip, method=0, vote=1, vote_thresh=0.8):
    return hip.DetOptions(method, 0.5, 0.0001, vote, vote_thresh)


def test_symbols_declared_exported_and_bound():
    from detectorch_amd import hip
    L = hip.lib()
    hdr = open(os.path.join(ROOT, "include", "detectorch_hip.h")).read()
    for s in ("dtc_postprocess_detections_ex2", "dtc_postprocess_detections_ex2_workspace_bytes", "dtc_box_voting_scored"):
        assert s + "(" in hdr
        assert getattr(L, s).restype is not None
    assert ctypes.sizeof(hip.VoteScoring) == 8
    assert ctypes.sizeof(hip.DetOptions) == 20
    assert hip.vote_scoring('ID') is None
    assert [hip.VOTE_METHODS[m] for m in ('ID',) + vsr.METHODS] == [0, 1, 2, 3, 4, 5]
    with pytest.raises(NotImplementedError):
        hip.vote_scoring('MEDIAN')


def test_ex2_argument_validation_returns_documented_codes():
    from detectorch_amd import hip
    L = hip.lib()
    ws = ctypes.c_void_p(256)

    def call(opt, scoring, fn=L.dtc_postprocess_detections_ex2):
        p = ctypes.c_void_p(256)     # bogus but non-NULL: validation must return before any use
        return fn(p, None, p, 0, p, None, p, p, 2, 1000, 81, 10., 10., 5., 5., .05, .5, 100, opt, scoring, ws, 0, p, p, p, p, 128,
                  None, None)
    S = hip.VoteScoring
    assert call(_opt(hip), S(6, 1.0)) == EINVAL                      # method outside 0..5
    assert call(_opt(hip), S(-1, 1.0)) == EINVAL
    for beta in (0.0, -1.0, float("inf"), float("nan")):
        assert call(_opt(hip), S(2, beta)) == EINVAL                 # beta > 0 and finite
    assert call(_opt(hip, vote=0), S(3, 1.0)) == EINVAL              # a scoring needs bbox_vote == 1
    assert call(None, S(3, 1.0)) == EINVAL
    assert call(_opt(hip, vote=2), None) == EINVAL                   # the options' own checks
    # _ex keeps rejecting bbox_vote = 2
    p = ctypes.c_void_p(256)
    assert L.dtc_postprocess_detections_ex(p, None, p, 0, p, None, p, p, 2, 1000, 81, 10., 10., 5., 5., .05, .5, 100,
                                           _opt(hip, vote=2), ws, 0, p, p, p, p, 128, None, None) == EINVAL
    for sc in (S(7, 1.0), S(1, 0.0), S(4, float("nan"))):
        assert L.dtc_box_voting_scored(p, 4, p, 4, 0.8, sc, p, p, None) == EINVAL


def test_ex2_workspace_bytes():
    from detectorch_amd import hip
    L = hip.lib()
    S = hip.VoteScoring
    for opt in (None, _opt(hip), _opt(hip, method=1), _opt(hip, vote=0)):
        assert L.dtc_postprocess_detections_ex2_workspace_bytes(8, 1000, 81, opt, None) == \
            L.dtc_postprocess_detections_ex_workspace_bytes(8, 1000, 81, opt)
        assert L.dtc_postprocess_detections_ex2_workspace_bytes(8, 1000, 81, opt, S(0, 1.0)) == \
            L.dtc_postprocess_detections_ex_workspace_bytes(8, 1000, 81, opt)
    base = L.dtc_postprocess_detections_ex_workspace_bytes(8, 1000, 81, _opt(hip))
    assert L.dtc_postprocess_detections_ex2_workspace_bytes(8, 1000, 81, _opt(hip), S(3, 1.0)) >= base + 8 * 80 * 1000 * 4
    assert L.dtc_postprocess_detections_ex2_workspace_bytes(8, 1000, 81, _opt(hip, vote=0), S(3, 1.0)) == 0
    assert L.dtc_postprocess_detections_ex2_workspace_bytes(8, 1000, 81, _opt(hip), S(3, -1.0)) == 0


def fixture_case(g, case):
    if case == "pp":
        p = golden("postprocess")
        return p["cls"], p["pred_clipped"]
    return g[case + "_scores"], g[case + "_boxes"]


def check_against_fixture(g, tag, m, dets, exact):
    ref_s, ref_b, ref_c = g[tag + "_%s_scores" % m], g[tag + "_%s_boxes" % m], g[tag + "_%s_cls_id" % m]
    assert len(dets) == len(ref_s), (tag, m, len(dets), len(ref_s))
    assert np.array_equal(dets[:, :4], ref_b), (tag, m)
    assert np.array_equal(dets[:, 5].astype(np.int32), ref_c), (tag, m)
    if exact:
        assert np.array_equal(dets[:, 4], ref_s), (tag, m)
    else:
        np.testing.assert_allclose(dets[:, 4], ref_s, rtol=1e-6, atol=0, err_msg="%s %s" % (tag, m))


@pytest.mark.parametrize("case", vsr.CASES)
def test_checker_reproduces_reference_golden(oracle, case):
    g = golden("postprocess_vote_scoring")
    scores, boxes = fixture_case(g, case)
    for nm in vsr.NMS_METHODS:
        for th in vsr.THRESHOLDS:
            tag = "%s_%s_%d" % (case, nm, round(th * 10))
            for m in vsr.METHODS:
                dets, _ = vsr.compose(oracle, scores, boxes, nm, th, m)
                check_against_fixture(g, tag, m, dets, exact=True)        # the checker is numpy itself: exact everywhere


def test_checker_box_voting_reproduces_reference_golden(oracle):
    g = golden("postprocess_vote_scoring")
    for th in vsr.THRESHOLDS:
        for m in vsr.METHODS:
            for beta in (1.0, 0.5):
                out = vsr.box_voting(oracle, g["bv_top"], g["bv_all"], th, m, beta)
                assert np.array_equal(out, g["bv_%d_%s_%d" % (round(th * 10), m, round(beta * 10))]), (th, m, beta)


def test_fixture_scorings_differ_from_id_where_the_reference_does():
    g = golden("postprocess_vote_scoring")
    assert int(g["crowd_nms_8_ID_n"]) == 104 and len(g["crowd_nms_8_IOU_AVG_scores"]) == 100
    assert int(g["crowd_linear_8_ID_n"]) == 104
    assert all(len(g["crowd_linear_8_%s_scores" % m]) == 103 for m in vsr.METHODS)
