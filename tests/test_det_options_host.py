"""Host side of the detection post-processing options (dtc_postprocess_detections_ex): the exported symbol, its argument validation
and workspace size without a GPU, and the oracle composition the GPU tests compare with, pinned against the reference's own
box_results_with_nms_and_limit outputs (tests/golden/postprocess_soft_vote.npz, tests/golden/make_det_options_golden.py)."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from det_options_ref import CONFIGS, compose, decode

EINVAL, EUNSUP = -1, -4


def _opt(hip, method=0, sigma=0.5, floor=0.0001, vote=0, vote_thresh=0.8):
    return hip.DetOptions(method, sigma, floor, vote, vote_thresh)


def test_ex_symbol_is_declared_exported_and_bound():
    from detectorch_amd import hip
    L = hip.lib()
    hdr = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "detectorch_hip.h")).read()
    for s in ("dtc_postprocess_detections_ex", "dtc_postprocess_detections_ex_workspace_bytes"):
        assert s + "(" in hdr
        assert getattr(L, s).restype is not None                                   # bound with a prototype in hip.py
    assert L.dtc_postprocess_detections_ex.argtypes[18] is ctypes.POINTER(hip.DetOptions)
    assert ctypes.sizeof(hip.DetOptions) == 20


def test_ex_argument_validation_returns_documented_codes():
    from detectorch_amd import hip
    L = hip.lib()
    ws = ctypes.c_void_p(256)

    def call(opt, R=1000, ncls=81, batch=2):       # every pointer bogus but non-NULL: validation must return before any use
        p = ctypes.c_void_p(256)
        return L.dtc_postprocess_detections_ex(p, None, p, 0, p, None, p, p, batch, R, ncls, 10., 10., 5., 5., .05, .5, 100,
                                               opt, ws, 0, p, p, p, p, 128, None, None)
    assert call(_opt(hip, method=4)) == EINVAL                                         # unknown method
    assert call(_opt(hip, method=-1)) == EINVAL
    assert call(_opt(hip, method=2, sigma=0.0)) == EINVAL                              # gaussian needs sigma > 0
    assert call(_opt(hip, method=2, sigma=-1.0)) == EINVAL
    assert call(_opt(hip, vote=1, vote_thresh=0.0)) == EINVAL                          # vote threshold outside (0, 1]
    assert call(_opt(hip, vote=1, vote_thresh=1.5)) == EINVAL
    assert call(_opt(hip, vote=1, vote_thresh=float("nan"))) == EINVAL
    assert call(_opt(hip, vote=2)) == EINVAL
    assert call(_opt(hip, method=1), ncls=258) == EINVAL                               # n_cls - 1 <= 256
    assert call(_opt(hip, method=1), R=4097) == EUNSUP                                 # R <= 4096
    assert call(_opt(hip, method=1), batch=0) == 0                                     # nothing to do
    assert call(_opt(hip, method=1, sigma=0.0)) == -3                                  # sigma only matters for gaussian: workspace
    p = ctypes.c_void_p(256)                                                           # decoded boxes with det_rois_scaled
    assert L.dtc_postprocess_detections_ex(None, None, p, 0, None, p, None, None, 1, 100, 81, 1., 1., 1., 1., .05, .5, 100,
                                           None, ws, 1 << 40, p, p, p, p, 128, None, None) == EINVAL
    fm = hip.FpnMapOut(256, 256, 256, 256, 256, 256, 0, 0, 2, 5)                       # decoded boxes with the fpn mapping
    assert L.dtc_postprocess_detections_ex(None, None, p, 0, None, p, None, None, 1, 100, 81, 1., 1., 1., 1., .05, .5, 100,
                                           None, ws, 1 << 40, p, p, None, p, 128, fm, None) == EINVAL
    assert L.dtc_postprocess_detections_ex_workspace_bytes(2, 1000, 81, _opt(hip, method=5)) == 0


def test_ex_workspace_bytes():
    from detectorch_amd import hip
    L = hip.lib()
    for B, R, C in ((1, 1, 2), (8, 1000, 81), (4, 4096, 257), (3, 17, 5)):
        base = L.dtc_postprocess_detections_workspace_bytes(B, R, C)
        assert L.dtc_postprocess_detections_ex_workspace_bytes(B, R, C, None) == base
        assert L.dtc_postprocess_detections_ex_workspace_bytes(B, R, C, _opt(hip)) == base     # hard NMS, no vote: the same
        for m, v in ((1, 0), (2, 0), (3, 0), (0, 1), (1, 1)):
            assert L.dtc_postprocess_detections_ex_workspace_bytes(B, R, C, _opt(hip, method=m, vote=v)) >= base + B * (C - 1) * 512
    assert hip.det_options() is None
    o = hip.det_options(do_soft_nms=True, soft_nms_method="gaussian", soft_nms_sigma=0.3, do_bbox_vote=True, bbox_vote_thresh=0.7)
    assert (o.nms_method, o.bbox_vote) == (2, 1)
    assert np.float32(o.soft_sigma) == np.float32(0.3) and np.float32(o.soft_score_thresh) == np.float32(0.0001)
    with pytest.raises(ValueError):
        hip.det_options(do_soft_nms=True, soft_nms_method="cubic")


@pytest.mark.parametrize("case", ["pp", "crowd"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_oracle_composition_reproduces_reference_golden(oracle, case, name):
    g = golden("postprocess_soft_vote")
    if case == "pp":
        p = golden("postprocess")
        scores, boxes = p["cls"], p["pred_clipped"]
    else:
        scores, boxes = g["crowd_scores"], g["crowd_boxes"]
    method, vt = CONFIGS[name]
    dets, roi = compose(oracle, scores, boxes, method, vt)
    key = "%s_%s_" % (case, name)
    assert np.array_equal(dets[:, 4], g[key + "scores"])
    assert np.array_equal(dets[:, :4], g[key + "boxes"])
    assert np.array_equal(dets[:, 5].astype(np.int32), g[key + "cls_id"])
    assert roi.shape[0] == dets.shape[0]
    if case == "crowd":
        assert dets.shape[0] > 100                                       # ties at the limit score: more than max_det rows


def test_oracle_composition_hard_nms_equals_oracle_postprocess(oracle):
    """The composition's hard-NMS form on decoded boxes == oracle.postprocess_detections (what the existing GPU tests pin)."""
    g = golden("postprocess")
    rois = g["rois"]
    boxes = decode(oracle, rois, g["sf"][0], g["im_size"], g["deltas"])
    dets, roi = compose(oracle, g["cls"], boxes)
    ref, ref_roi = oracle.postprocess_detections(rois, g["sf"][0], g["im_size"], g["cls"], g["deltas"])
    assert np.array_equal(dets, ref) and np.array_equal(roi, ref_roi)
