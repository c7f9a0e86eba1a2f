"""Box decoding on saturated and non-finite deltas: oracle/oracle.c against tests/golden/decode_extremes.npz, which the reference's
own GenerateProposals, bbox_transform / clip_tiled_boxes and postprocess_output produced (tests/golden/make_decode_extremes_golden.py).

CPU only.  Counts, scores, class ids: equal.  Boxes: bit-equal except where torch / numpy's float32 exp differs from the correctly
rounded one the oracle uses, and there within 1 ulp (conftest.ulp_close); NaN exactly where the reference has NaN.  The NaN rows of
the RPN cases are the point: the reference's torch.min / torch.max pass a NaN delta through to filter_boxes, which drops the row."""
import numpy as np
import pytest

from conftest import golden, ulp_close
from det_options_ref import compose, decode

RPN_CASES = {"c4": (0, 16), "p3": (0, 16), "p6": (0, 16, 400)}
RPN_RUNS = [(c, t, m) for c, ms in RPN_CASES.items() for t in (0.0, 0.7) for m in ms]
SCALE = 1.6


def close_nan_aware(a, b):
    """same shape, NaN where the other has NaN, infinities equal, finite values within ulp_close"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    fin = np.isfinite(a) & np.isfinite(b)
    if not np.array_equal(a[~fin & ~np.isnan(a)], b[~fin & ~np.isnan(b)]):
        return False
    return ulp_close(a[fin], b[fin])


def rpn_case(g, case):
    cfg = g["rpn_%s_cfg" % case]
    A, H, W, stride, pre, post, im_h, im_w = [float(v) for v in cfg[:8]]
    return int(A), int(H), int(W), stride, int(pre), int(post), im_h, im_w, tuple(cfg[8:])


def min_size_scaled(m):
    """filter_boxes (generate_proposals.py:151-163): min_size *= scale_factor in double, compared with float32 widths"""
    return float(np.float32(m * SCALE))


@pytest.mark.parametrize("case,thr,m", RPN_RUNS)
def test_rpn_extremes_oracle_vs_reference(oracle, case, thr, m):
    g = golden("decode_extremes")
    A, H, W, stride, pre, post, im_h, im_w, sizes = rpn_case(g, case)
    anchors = oracle.generate_anchors(stride, sizes, (0.5, 1, 2))
    props, scores = oracle.generate_proposals(g["rpn_%s_cls" % case][0], g["rpn_%s_bbox" % case][0], anchors, stride, im_h, im_w,
                                              pre, post, thr, min_size_scaled=min_size_scaled(m))
    tag = "rpn_%s_t%02d_m%d" % (case, int(thr * 10), m)
    ref_p, ref_s = g[tag + "_props"], g[tag + "_scores"]
    assert props.shape == ref_p.shape, (props.shape, ref_p.shape)
    assert np.array_equal(scores, ref_s)
    assert np.isfinite(ref_p).all()                          # the reference's filter drops every NaN row
    assert close_nan_aware(props, ref_p)


def test_rpn_extremes_fixture_reaches_the_edges():
    """the fixture holds what it claims: NaN and +-inf deltas among the ranked anchors, rows dropped for NaN alone, boxes collapsed
    onto border lines, a min_size that decides rows and one that filters everything"""
    g = golden("decode_extremes")
    for case in RPN_CASES:
        d = g["rpn_%s_bbox" % case]
        A, H, W, stride, pre, post, im_h, im_w, _ = rpn_case(g, case)
        assert np.isnan(d).sum() >= 4 and np.isposinf(d).any() and np.isneginf(d).any()
        p0 = g["rpn_%s_t00_m0_props" % case]
        assert ((p0[:, 0] == p0[:, 2]) & (p0[:, 0] == im_w - 1)).any() and ((p0[:, 1] == p0[:, 3]) & (p0[:, 1] == 0)).any()
        assert g["rpn_%s_t00_m16_scores" % case].size < g["rpn_%s_t00_m0_scores" % case].size
    assert g["rpn_p6_t00_m0_scores"].size == 140 and g["rpn_p6_t00_m400_scores"].size == 0   # 144 anchors, 4 of them NaN


def test_numpy_decode_extremes_oracle_vs_reference(oracle):
    g = golden("decode_extremes")
    pred = oracle.bbox_transform(g["bt_boxes"], g["bt_deltas"], (10.0, 10.0, 5.0, 5.0))
    assert close_nan_aware(pred, g["bt_pred"])
    assert np.isinf(g["bt_pred"]).any()
    clipped = oracle.clip_tiled_boxes(pred, g["bt_im_shape"][0], g["bt_im_shape"][1])
    assert close_nan_aware(clipped, g["bt_pred_clipped"])
    assert np.isfinite(g["bt_pred_clipped"]).all()


def test_postprocess_extremes_oracle_vs_reference(oracle):
    g = golden("decode_extremes")
    dets, _ = oracle.postprocess_detections(g["pp_rois"], g["pp_sf"][0], g["pp_im_size"], g["pp_cls"], g["pp_deltas"])
    assert dets.shape[0] == g["pp_scores"].shape[0] == 100
    assert np.array_equal(dets[:, 4], g["pp_scores"])
    assert np.array_equal(dets[:, 5].astype(np.int32), g["pp_cls_id"])
    assert ulp_close(dets[:, :4], g["pp_boxes"])


def soft_vote_scores(g):
    """the class scores of the Soft-NMS + vote run: zero-area (roi, class) pairs taken out (make_decode_extremes_golden.py)"""
    cls = g["pp_cls"].copy()
    cls.reshape(-1)[g["pp_soft_vote_drop"]] = 0.0
    return cls


def test_postprocess_soft_vote_extremes_oracle_vs_reference(oracle):
    g = golden("decode_extremes")
    boxes = decode(oracle, g["pp_rois"], g["pp_sf"][0], g["pp_im_size"], g["pp_deltas"])
    dets, _ = compose(oracle, soft_vote_scores(g), boxes, "linear", 0.8)
    assert dets.shape[0] == g["pp_soft_vote_scores"].shape[0]
    assert np.array_equal(dets[:, 4], g["pp_soft_vote_scores"])
    assert np.array_equal(dets[:, 5].astype(np.int32), g["pp_soft_vote_cls_id"])
    assert ulp_close(dets[:, :4], g["pp_soft_vote_boxes"])


def test_postprocess_fixture_collapses_onto_border_lines():
    g = golden("decode_extremes")
    bx, cid = g["pp_boxes"], g["pp_cls_id"]
    im_h, im_w = g["pp_im_size"][:2]
    corner = (bx[:, 0] == im_w - 1) & (bx[:, 2] == im_w - 1) & (bx[:, 1] == im_h - 1) & (bx[:, 3] == im_h - 1)
    assert len(set(cid[corner])) >= 3                # several classes each keep ONE corner point (IoU 1 suppressed the rest)
    for j in set(cid[corner]):
        assert corner[cid == j].sum() == 1
    assert ((bx[:, 0] == 0) & (bx[:, 2] == 0)).any()  # left-border lines
    assert np.isinf(g["pp_deltas"]).any()


# ---- the clamp and the clip themselves ----------------------------------------------------------------------------------------
def test_clip_propagates_nan_and_maps_signed_zero(oracle):
    v = np.array([[np.nan, -0.0, 0.0, -np.inf], [np.inf, 99.0, 99.5, -1e-45], [1e-45, -np.nan, 98.999, 1e30]], np.float32)
    got = oracle.clip_tiled_boxes(v, 80.0, 100.0)                         # x clipped to [0, 99], y to [0, 79]
    want = np.array([[np.nan, 0.0, 0.0, 0.0], [99.0, 79.0, 99.0, 0.0], [1e-45, np.nan, 98.999, 79.0]], np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    assert np.array_equal(got[fin].view(np.uint32), want[fin].view(np.uint32))   # -0 -> +0, bit for bit
    # torch's min / max, the reference's clip, agree on every finite input and on NaN
    import torch
    t = torch.from_numpy(v.copy())
    hi = torch.tensor([99.0, 79.0, 99.0, 79.0])
    ref = torch.max(torch.min(t, hi), torch.zeros(1)).numpy()
    assert np.array_equal(np.isnan(ref), np.isnan(want)) and np.array_equal(ref[fin], want[fin])


def test_clamp_propagates_nan_and_saturates(oracle):
    clip = np.float32(4.135166556742356)
    box = np.array([[10.0, 20.0, 41.0, 51.0]], np.float32)                     # 32 x 32, centre (26, 36)
    dws = np.array([np.nan, np.inf, clip, np.nextafter(clip, np.float32(9)), 30.0, -np.inf, -104.0, -0.0], np.float32)
    d = np.zeros((1, 4 * dws.size), np.float32)
    d[0, 2::4] = dws
    d[0, 3::4] = dws
    out = oracle.bbox_transform(box, d).reshape(-1, 4)
    assert np.isnan(out[0]).tolist() == [True, True, True, True]              # NaN dw/dh: NaN box, not the clamp value
    sat = out[2]
    assert np.array_equal(out[1], sat) and np.array_equal(out[3], sat) and np.array_equal(out[4], sat)
    w = np.float32(np.exp(np.float64(clip))) * np.float32(32)
    assert sat[0] == np.float32(np.float32(26) - np.float32(0.5) * w)
    assert out[5].tolist() == [26.0, 36.0, 25.0, 35.0] and out[6].tolist() == [26.0, 36.0, 25.0, 35.0]  # exp -> 0: width 0
    assert out[7].tolist() == [10.0, 20.0, 41.0, 51.0]                          # exp(-0) = 1
    # the reference's torch.min against the float32 clamp: same values, NaN kept
    import torch
    ref = torch.min(torch.from_numpy(dws), torch.tensor([4.135166556742356])).numpy()
    assert np.isnan(ref[0]) and np.array_equal(ref[1:], np.minimum(dws[1:], clip))
