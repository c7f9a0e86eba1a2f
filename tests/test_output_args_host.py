"""The conditions the output-stage argument tests on the GPU rely on (tests/test_hip_mask_output_args.py,
tests/test_hip_det_args.py), pinned on the oracle alone so that none of those tests can pass emptily.  No GPU."""
import numpy as np

import output_args_cases as oc
from conftest import golden
from det_options_ref import compose, decode


def test_tie_case_has_exact_ties_the_oracle_binarises_to_zero(oracle):
    mask, ref_box, val = oc.tie_case()
    box, crop = oracle.mask_resize_binarize(mask, ref_box, 0.5)
    assert list(box) == [98, 98, 157, 157] and crop.shape == (60, 60)
    ties = val == np.float32(0.5)
    assert int(ties.sum()) >= 20
    assert not crop[ties].any()                                              # strict `>`: a tie is background
    assert np.array_equal(crop, (val > np.float32(0.5)).astype(np.uint8))     # the numpy restatement IS the oracle's rule here
    assert (val > np.float32(0.5)).sum() > 500 and (val < np.float32(0.5)).sum() > 500


def test_checkerboard_exceeds_segm_results_first_guess(oracle):
    h, w = oc.CHECKER_FRAME
    _, rect, sub = oc.paste_ref(oracle, oc.checker_mask(), oc.CHECKER_BOX, h, w)
    runs, s = oracle.rle_encode(oc.frame_of(sub, rect, h, w))
    guess_runs, guess_str = oc.segm_first_guess(w)
    assert (len(runs), len(s)) == (16821, 18030)
    assert len(runs) > guess_runs and len(s) > guess_str
    assert len(s) <= 7 * (len(runs) + 8)                                     # the loop's second stride holds the string


def test_overflow_batch_geometry(oracle):
    boxes, cls, masks = oc.overflow_batch()
    exp = oc.paste_expectation(oracle, lambda b, d: masks[b * 16 + d, cls[b][d]], boxes, oc.OVERFLOW_SIZES)
    assert [len(rb) for rb in boxes] == [9, 7, 0]
    e1 = exp[1]
    k, z = oc.OVERFLOW_K, oc.OVERFLOW_Z
    assert e1["area"][k] > 2 * oc.BAND_PIXELS                                # three bands: band 0 + two helper items
    assert 0 < k < len(boxes[1]) - 2 and z == k + 1
    assert e1["area"][z] == 0 and e1["off"][z] == e1["off"][k] + e1["area"][k]
    assert all(e1["area"][d] > 0 for d in range(7) if d != z)
    assert (exp[0]["area"] > oc.BAND_PIXELS).any()                          # image 0 has helper items of its own
    caps = oc.overflow_capacities(exp)
    assert caps[0] == exp[0]["bytes"] > e1["bytes"] > 0 and exp[2]["bytes"] == 0
    assert 0 == caps[5] < caps[3] < caps[2] < caps[4] < caps[1] < caps[0]


def test_noise_frame_runs(oracle):
    runs, s = oracle.rle_encode(oc.noise_frame())
    assert len(runs) > 1000 and len(s) >= len(runs)


def test_mask_geometry_sizes_fixture_equals_oracle(oracle):
    g = golden("mask_geometry_sizes")
    rb = g["ref_boxes"]
    assert np.array_equal(rb, oc.geometry_boxes())
    for M in oc.MASK_SIDES:
        got = np.stack([oracle.expand_box_int(rb[i], M) for i in range(rb.shape[0])])
        assert np.array_equal(got, g["exp_int_M%d" % M]), M
    # the fixture's boxes really differ between mask sides
    assert (g["exp_int_M7"] != g["exp_int_M56"]).any() and (g["exp_int_M1"] != g["exp_int_M2"]).any()


def _keys(dets, roi):
    return set(zip(roi.tolist(), dets[:, 5].astype(int).tolist()))


def test_nms_thresh_expectations_on_the_oracle(oracle):
    rois5, cls, deltas, src, dst = oc.det_batch()
    for b in range(2):
        n = int(oc.DET_N_ROIS[b])
        assert dst[b].max() < n
        run = lambda t: oracle.postprocess_detections(rois5[b, :n, 1:], oc.DET_SF[b], oc.DET_IM[b], cls[b, :n], deltas[b, :n],
                                                      nms_thresh=t, max_det=0)
        cand = cls[b, :n, 1:] > np.float32(0.05)
        nonempty = np.flatnonzero(cand.any(0)) + 1
        for t in (-0.5, 0.0):                                                # IoU >= thresh always holds: one box per class
            d, r = run(t)
            assert np.array_equal(d[:, 5].astype(int), nonempty)
            assert np.array_equal(d[:, 4], cls[b, :n][:, nonempty].max(0))   # ... the class's best
        d15, r15 = run(1.5)                                                  # IoU <= 1 < 1.5: nothing suppressed
        assert d15.shape[0] == int(cand.sum())
        d10, r10 = run(1.0)                                                  # only identical boxes: exactly the copied rows
        want = set((int(r), int(j) + 1) for r in dst[b] for j in np.flatnonzero(cand[r]))
        assert len(want) >= 20 and _keys(d15, r15) - _keys(d10, r10) == want
        counts = [run(t)[0].shape[0] for t in (0.0, 1e-6, 0.3, 0.5, 0.7, 1.0, 1.5)]
        assert counts == sorted(counts) and len(set(counts)) == len(counts)  # every threshold of the sweep decides differently


def test_infinite_union_is_suppressed_at_thresh_zero_on_the_oracle(oracle):
    scores, boxes, huge = oc.overflowing_union_batch()
    for j, r in huge.items():
        b = boxes[0, r, 4 * j:4 * j + 4]
        with np.errstate(over="ignore"):
            assert np.isinf((b[2] - b[0] + np.float32(1)) * (b[3] - b[1] + np.float32(1)))      # float32 area overflows
        assert scores[0, r, j] < scores[0, :, j].max()                                          # not the class's best row
    for t in (0.0, -0.5):
        d, r = compose(oracle, scores[0], boxes[0], "nms", None, nms_thresh=t)
        assert d[:, 5].tolist() == [1.0, 2.0] and np.array_equal(d[:, 4], scores[0, :, 1:].max(0))
    d, r = compose(oracle, scores[0], boxes[0], "nms", None, nms_thresh=1e-6)
    assert all(huge[j] in r[d[:, 5] == j] for j in huge)


def test_max_det_sweep_has_room(oracle):
    rois5, cls, deltas, _, _ = oc.det_batch()
    n = int(oc.DET_N_ROIS[0])
    boxes = decode(oracle, rois5[0, :n, 1:], oc.DET_SF[0], oc.DET_IM[0], deltas[0, :n])
    for method in ("nms", "linear"):
        K = compose(oracle, cls[0, :n], boxes, method, None, max_det=0)[0].shape[0]
        assert K > 1024 + 1                                                  # above det_finalize's fast output path (kFinSurvMax rows), and > 17
    ref, _ = oracle.postprocess_detections(rois5[0, :n, 1:], oc.DET_SF[0], oc.DET_IM[0], cls[0, :n], deltas[0, :n], max_det=0)
    assert np.array_equal(ref, compose(oracle, cls[0, :n], boxes, "nms", None, max_det=0)[0])     # the two checkers agree


def test_signed_scores_cross_the_sign_at_the_limit(oracle):
    scores, boxes, zero_rows = oc.signed_score_batch()
    assert (scores > 0).any() and (scores < 0).any() and (scores[:, zero_rows, 1:] == 0).all()
    for b in range(2):
        d, _ = compose(oracle, scores[b], boxes[b], "nms", None, score_thresh=-1.0, max_det=0)
        pos, zero = int((d[:, 4] > 0).sum()), int((d[:, 4] == 0).sum())
        assert 5 < pos < 50 < pos + zero < 200 < d.shape[0]                  # max_det 5 / 50 / 200: threshold > 0, == 0 (ties), < 0
        d50, _ = compose(oracle, scores[b], boxes[b], "nms", None, score_thresh=-1.0, max_det=50)
        assert d50.shape[0] == pos + zero and d50[:, 4].min() == 0
        d200, _ = compose(oracle, scores[b], boxes[b], "nms", None, score_thresh=-1.0, max_det=200)
        assert d200.shape[0] == 200 and d200[:, 4].min() < 0
