"""Keypoint inference without a GPU (tests/README_keypoints.md):
  * libdetectorch_kps_hip.so exports exactly what include/detectorch_kps_hip.h declares and hip_kps.SIGNATURES binds it; the other
    libraries export no dtc_kps_ name; the constants of header and binding agree; the return codes on bad arguments (validation
    precedes every HIP call, so nothing is launched and the bogus pointers are never used);
  * the numpy restatement (tests/kps_ref.py) against itself: the identity at Wr = Hr = S, a zero map, a tie, a NaN, the explicit-cast
    x / y against the literal numpy expression, prob against the fsum form (the literal float32 form printed beside it);
  * every case (tests/kps_cases.py) holds the condition it was built for;
  * the Python layer on hand-made arrays: keypoint_results, assemble_results(keyps=...), coco_keypoint_results in its three confidence
    modes; CPU tensors are refused."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
import kps_cases as kc
import kps_ref as kr

sys.path.insert(0, GOLDEN)                                    # make_native_host_codes.exports

NAMES = ["dtc_kps_heatmaps_to_keypoints", "dtc_kps_target_arch", "dtc_kps_workspace_bytes"]
OK, EINVAL, EWORKSPACE, EUNSUPPORTED = 0, -1, -3, -4
f32, f64 = np.float32, np.float64


# ---- the library: exports, binding, header, constants ------------------------------------------------------------------------------
def test_header_symbols_are_exported_and_bound():
    import test_binding_signatures_host as tb
    from make_native_host_codes import exports
    from detectorch_amd import hip, hip_kps
    lib = hip_kps.lib()
    protos = tb.prototypes("detectorch_kps_hip.h")
    assert sorted(protos) == NAMES and exports(hip_kps.LIB_PATH) == NAMES and sorted(hip_kps.SIGNATURES) == NAMES
    for entry, (ret, params) in protos.items():
        row = hip_kps.SIGNATURES[entry]
        assert row[0] == ret and [(n, k) for n, k in row[1]] == params, entry
        fn = getattr(lib, entry)
        assert list(fn.argtypes) == [hip._KINDS[k] for _, k in row[1]] and fn.restype == hip._RETURNS[row[0]], entry
    assert lib.dtc_kps_target_arch() == b"gfx950"


def test_the_other_libraries_export_no_kps_name():
    from make_native_host_codes import exports
    from detectorch_amd import (build, hip, hip_aug, hip_eval, hip_flip, hip_grad, hip_loss, hip_mask, hip_mpost, hip_optim, hip_poly,
                                hip_rpn, hip_segm, hip_train)
    build.build()
    sides = (hip_train, hip_loss, hip_grad, hip_optim, hip_rpn, hip_mask, hip_eval, hip_segm, hip_poly, hip_flip, hip_mpost, hip_aug)
    for mod in sides:
        mod.lib()
    for mod in (hip,) + sides:
        assert not [n for n in exports(mod.LIB_PATH) if n.startswith("dtc_kps_")], mod.__name__


def test_constants_are_those_of_the_header():
    from detectorch_amd import hip_kps
    header = open(os.path.join(ROOT, "include", "detectorch_kps_hip.h")).read()
    define = lambda name: eval(re.search(r"#define DTC_KPS_%s (\(?[\d <]+\)?)" % name, header).group(1))
    assert (define("MAX_MAP"), define("MAX_KEYPOINTS"), define("MAX_OUT"), define("MAX_BATCH"), define("MAX_MAPS"), define("MAX_SIDE")) == (
        hip_kps.MAX_MAP, hip_kps.MAX_KEYPOINTS, hip_kps.MAX_OUT, hip_kps.MAX_BATCH, hip_kps.MAX_MAPS, hip_kps.MAX_SIDE) == (
        64, 64, 4096, 65535, 1 << 20, 4096)
    assert kr.MAX_SIDE == hip_kps.MAX_SIDE and (define("BANDS"), define("MIN_BAND")) == (8, 32)
    assert "parity with cv2 and with Detectron\n * themselves is unpinned" in header


# ---- return codes: every refusal comes before the first HIP call, so bogus pointers are never touched -------------------------------
BOGUS = 256                                                    # a bogus, non-NULL, 16-byte aligned device pointer


def _call(**kw):
    from detectorch_amd import hip_kps
    a = dict(heatmaps=BOGUS, dets=BOGUS, det_count=BOGUS, batch=2, max_out=6, K=17, S=56, person_class=-1, min_size=0, workspace=BOGUS,
             workspace_bytes=1 << 40, keyps=BOGUS, kp_status=BOGUS)
    a.update(kw)
    order = [n for n, _ in hip_kps.SIGNATURES["dtc_kps_heatmaps_to_keypoints"][1][:-1]]
    return hip_kps.lib().dtc_kps_heatmaps_to_keypoints(*[a[n] for n in order], None)


EINVAL_ARMS = (dict(batch=0), dict(max_out=0), dict(K=0), dict(S=0), dict(person_class=-2), dict(min_size=-1), dict(heatmaps=None),
               dict(dets=None), dict(det_count=None), dict(workspace=None), dict(keyps=None), dict(kp_status=None), dict(keyps=BOGUS + 4),
               dict(workspace=BOGUS + 8))
EUNSUPPORTED_ARMS = (dict(S=65), dict(K=65), dict(max_out=4097), dict(batch=65536), dict(min_size=4097),
                     dict(batch=65535, max_out=4096, K=1), dict(batch=1024, max_out=1024, K=2))
LAST_INSIDE = (dict(S=64), dict(K=64), dict(max_out=4096), dict(batch=65535, max_out=16, K=1), dict(min_size=4096),
               dict(batch=1024, max_out=1024, K=1))


def test_return_codes():
    from detectorch_amd import hip_kps
    for kw in EINVAL_ARMS:
        assert _call(**kw) == EINVAL, kw
    for kw in EUNSUPPORTED_ARMS:
        assert _call(**kw) == EUNSUPPORTED, kw
    for kw in LAST_INSIDE:                                      # the last value inside each limit (a NULL keeps it from launching)
        assert _call(kp_status=None, **kw) == EINVAL, kw
    assert _call(batch=0, S=65) == EINVAL                       # shapes and parameters in front of limits
    assert _call(S=65, keyps=None) == EUNSUPPORTED              # limits in front of pointers
    assert _call(keyps=None, workspace_bytes=0) == EINVAL       # pointers in front of the workspace
    wb = hip_kps.lib().dtc_kps_workspace_bytes
    need = wb(2, 6, 17)
    assert need == 2 * 6 * 17 * 8 * 16 and _call(workspace_bytes=need - 1) == EWORKSPACE and _call(workspace_bytes=0) == EWORKSPACE
    assert wb(0, 6, 17) == wb(2, 0, 17) == wb(2, 6, 0) == wb(2, 6, 65) == wb(65535, 4096, 1) == 0
    assert wb(1024, 1024, 1) == (1 << 20) * 8 * 16


def test_wrapper_refuses_cpu_tensors_and_bad_shapes():
    import torch
    from detectorch_amd import hip_kps
    heat, dets, cnt = kc.case(1, 4, (0, 5))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hip_kps.heatmaps_to_keypoints(torch.from_numpy(heat), torch.from_numpy(dets), torch.from_numpy(cnt))
    with pytest.raises(ValueError, match="unsupported shape"):
        hip_kps.keypoint_outputs(1, 4097, 17, "cpu")
    with pytest.raises(ValueError, match="unsupported shape"):
        hip_kps.keypoint_outputs(65535, 4096, 1, "cpu")


# ---- the restatement against itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [4, 7, 56, 64])
def test_identity_at_the_maps_own_size(S):
    idx, w = kr.axis_taps(S, S)
    assert np.array_equal(w, np.tile(np.array([0, 1, 0, 0], f32), (S, 1))) and np.array_equal(idx[:, 1], np.arange(S))
    m = (np.random.RandomState(S).randn(S, S) * 3).astype(f32)
    assert kr.resize_cubic(m, S, S).tobytes() == m.tobytes()


@pytest.mark.parametrize("n_dst", [1, 2, 5, 9, 13, 130, 257, 300, 4096])
def test_weights_sum_to_one_and_taps_stay_inside(n_dst):
    for S in (4, 7, 56, 64):
        idx, w = kr.axis_taps(n_dst, S)
        assert idx.min() >= 0 and idx.max() <= S - 1 and np.all(np.diff(idx[:, 1]) >= 0)         # monotonic: a band reads a range of rows
        assert np.abs(w.astype(f64).sum(1) - 1).max() < 1e-6


def test_zero_map_gives_exact_zeros_and_pos_0():
    v = kr.resize_cubic(np.zeros((56, 56), f32), 130, 257)
    assert not v.any()
    (x, y, logit, prob), pos = kr.map_to_keypoint(np.zeros((56, 56), f32), kc.box(3.25, 7.5, 257.0, 130.0))
    assert pos == 0 and logit == 0 and prob == f32(1.0 / (130 * 257))
    assert x == f32(0.5 * 1.0 + 3.25) and y == f32(0.5 * 1.0 + 7.5)


def test_tie_and_nan_at_identity_size_and_nan_in_an_upscale():
    heat, dets, cnt = kc.special_case()
    r = kc.MAX_OUT
    assert kr.row_size(dets[1, 0, :4])[:2] == (7, 7) and kr.row_size(dets[1, 2, :4])[:2] == (7, 7)
    assert kr.map_to_keypoint(heat[r, 0], dets[1, 0, :4])[1] == 2 * 7 + 3                       # the first of two equal maxima
    assert (heat[r, 0] == heat[r, 0].max()).sum() == 2
    (x, y, logit, prob), pos = kr.map_to_keypoint(heat[r, 1], dets[1, 0, :4])
    # 0 * NaN is NaN: the NaN at (3, 2) reaches rows 1 .. 4 and columns 0 .. 3 of the resized map, and (1, 0) is the first of them
    assert pos == 1 * 7 + 0 and np.isnan(logit) and np.isnan(prob) and x == f32(0.5 + 2.5) and y == f32(1.5 - 1.25)
    (x, y, logit, prob), pos = kr.map_to_keypoint(heat[r + 2, 1], dets[1, 2, :4])              # a NaN at (0, 0) picks its own position
    assert pos == 0 and np.isnan(logit) and np.isnan(prob) and (x, y) == (f32(0.5), f32(0.5))
    assert kr.map_to_keypoint(heat[r, 2], dets[1, 0, :4])[1] == 0
    assert kr.map_to_keypoint(heat[r + 2, 0], dets[1, 2, :4])[1] == 0 * 7 + 4                   # the first resized NaN of two source NaNs
    Wr, Hr = kr.row_size(dets[1, 1, :4])[:2]
    assert (Wr, Hr) == (14, 21)
    v = kr.resize_cubic(heat[r + 1, 0], Hr, Wr)
    pos = kr.map_to_keypoint(heat[r + 1, 0], dets[1, 1, :4])[1]
    assert 0 < np.isnan(v).sum() < v.size and pos == np.flatnonzero(np.isnan(v.reshape(-1)))[0]


def test_explicit_cast_xy_is_the_literal_numpy_expression():
    rs = np.random.RandomState(11)
    for _ in range(500):
        x1, y1 = f32(rs.uniform(-50, 1300)), f32(rs.uniform(-50, 800))
        w, h = f32(rs.uniform(0.2, 700)), f32(rs.uniform(0.2, 700))
        Wr, Hr, wc, hc = kr.row_size([x1, y1, x1 + w, y1 + h])
        pos = np.int64(rs.randint(0, Wr * Hr))
        x_int, y_int = pos % Wr, (pos - pos % Wr) // Wr                                          # Detectron's own lines
        lit = np.zeros(2, f32)
        lit[0] = (x_int + 0.5) * wc + x1
        lit[1] = (y_int + 0.5) * hc + y1
        assert ((x_int + 0.5) * wc).dtype == f64
        assert tuple(lit) == kr.keypoint_xy(int(pos), Wr, wc, hc, x1, y1)


def test_prob_is_the_fsum_form_with_the_literal_float32_form_beside_it():
    rs = np.random.RandomState(12)
    worst = 0.0
    for i in range(200):
        Hr, Wr = rs.randint(1, 80), rs.randint(1, 80)
        v = kr.resize_cubic((rs.randn(7, 7) * rs.choice([0.5, 3.0, 30.0])).astype(f32), Hr, Wr)
        m = v.max()
        p, q, lit = kr.prob_of(v, m), kr.prob_fsum(v, m), kr.prob_literal_f32(v, m)
        assert p == q and 0 < p <= 1
        worst = max(worst, abs(float(lit) - float(p)) / float(p))
    print("largest relative distance of numpy's own float32 exp and sum from the restatement's prob on 200 maps: %.3g" % worst)
    assert worst < 1e-5                                         # the literal form is not a reference; it stays in the neighbourhood


def test_row_sizes_and_refusals():
    assert kr.row_size(kc.box(10.0, 20.0, 0.4, 0.7)) == (1, 1, f32(1), f32(1))
    assert kr.row_size(kc.box(10.0, 20.0, 0.4, 0.7), 20) == (20, 20, f32(1) / f32(20), f32(1) / f32(20))
    assert kr.row_size(kc.box(5.0, 6.0, 12.0, 9.0))[:2] == (12, 9) and kr.row_size(kc.box(-7.5, 2.0, 4096.0, 1.0))[:2] == (4096, 1)
    assert kr.row_size(kc.box(0.125, 0.375, 33.7, 64.2))[:2] == (34, 65) and kr.row_size(kc.box(7.0, -3.0, 70.0, 31.01))[:2] == (70, 32)
    heat, dets, cnt, want = kc.refused_case()
    _, status = kr.heatmaps_to_keypoints(heat, dets, cnt)
    assert np.array_equal(status, want)
    for b, d in ((0, 1), (0, 3), (0, 4), (1, 1), (1, 2)):
        assert kr.row_size(dets[b, d, :4]) is None


@pytest.mark.parametrize("counts", kc.COUNTS)
def test_cases_hold_their_conditions(counts):
    for K, S in kc.MAPS:
        heat, dets, cnt = kc.case(K, S, counts)
        assert heat.shape == (12, K, S, S) and dets.shape == (2, 6, 6) and tuple(cnt) == counts
        live = [(b, d) for b in range(2) for d in range(counts[b])]
        assert all(np.isfinite(dets[b, d]).all() and np.isfinite(heat[b * 6 + d]).all() for b, d in live)
        assert all(np.isnan(heat[b * 6 + d]).all() and np.isnan(dets[b, d]).all() for b in range(2) for d in range(counts[b], 6))
        sizes = [kr.row_size(dets[b, d, :4])[:2] for b, d in live]
        assert (S, S) in sizes and (1, 1) in sizes
        assert set(sizes) >= ({(257, 130), (4096, 1), (14, 21)} if counts == (0, 5) else {(12, 9), (5, 9), (2, 300), (300, 2), (34, 65), (1, 40), (70, 32)})
        cls = [int(dets[b, d, 5]) for b, d in live]
        assert 1 in cls and len(set(cls)) > 1                   # mixed classes: person_class = 1 selects some rows and not others
        _, status = kr.heatmaps_to_keypoints(heat[:, :1, :4, :4], dets, cnt, person_class=1)
        assert status.sum() == cls.count(1) and 0 < status.sum() < len(live)


# ---- the Python layer on hand-made arrays ---------------------------------------------------------------------------------------------
def _hand_made():
    """two images of three rows: image 0 = a person, a class-2 box, a person; image 1 = one class-2 box"""
    dets = np.zeros((2, 3, 6), f32)
    dets[0] = [[1, 2, 11, 22, 0.9, 1], [3, 4, 13, 24, 0.8, 2], [5, 6, 15, 26, 0.7, 1]]
    dets[1, 0] = [7, 8, 17, 28, 0.6, 2]
    cnt = np.array([3, 1], np.int32)
    keyps = np.arange(2 * 3 * 4 * 2, dtype=f32).reshape(2, 3, 4, 2)
    status = np.array([[1, 0, 1], [0, 0, 0]], np.int32)
    return dets, cnt, keyps, status


def test_assemble_results_with_keypoints():
    from detectorch_amd.utils import result_utils as ru
    dets, cnt, keyps, status = _hand_made()
    two = ru.assemble_results(dets, cnt, num_classes=3)
    assert len(two) == 2                                        # without the new arguments: as before
    boxes, segms, kps = ru.assemble_results(dets, cnt, num_classes=3, keyps=keyps, kp_status=status)
    assert np.array_equal(boxes[1][0], dets[0, [0, 2], :5]) and len(kps[1][0]) == 2 and kps[1][1] == [] and kps[2] == [[], []]
    assert np.array_equal(kps[1][0][0], keyps[0, 0]) and np.array_equal(kps[1][0][1], keyps[0, 2]) and kps[1][0][0].shape == (4, 2)
    assert all(np.array_equal(a, b) for a, b in zip(two[0][1] + two[0][2], boxes[1] + boxes[2]))
    with pytest.raises(RuntimeError, match="not computed"):     # class 2 was not the kernel's person_class: its rows have status 0
        ru.assemble_results(dets, cnt, num_classes=3, keyps=keyps, kp_status=status, person_class=2)
    # a slice of existing lists
    ab, asg, ak = ru.empty_results(3, 4)
    ru.assemble_results(dets, cnt, num_classes=3, all_boxes=ab, all_segms=asg, first_image=2, keyps=keyps, kp_status=status, all_keyps=ak)
    assert len(ak[1][2]) == 2 and ak[1][0] == [] and np.array_equal(ak[1][2][1], keyps[0, 2])


@pytest.mark.parametrize("confidence", ["logit", "prob", "bbox"])
def test_coco_keypoint_results(confidence):
    from detectorch_amd.utils import result_utils as ru
    dets, cnt, keyps, status = _hand_made()
    boxes, _, kps = ru.assemble_results(dets, cnt, num_classes=3, keyps=keyps, kp_status=status)
    res = ru.coco_keypoint_results(boxes[1], kps[1], [101, 202], 1, confidence)
    assert [r["image_id"] for r in res] == [101, 101] and all(r["category_id"] == 1 for r in res)
    for r, d in zip(res, (0, 2)):
        k = keyps[0, d]
        assert r["keypoints"] == [float(k[0, 0]), float(k[1, 0]), 1, float(k[0, 1]), float(k[1, 1]), 1]
        want = {"logit": (k[2, 0] + k[2, 1]) / 2, "prob": (k[3, 0] + k[3, 1]) / 2, "bbox": np.float64(dets[0, d, 4])}[confidence]
        assert r["score"] == want
    with pytest.raises(ValueError, match="KEYPOINT_CONFIDENCE"):
        ru.coco_keypoint_results(boxes[1], kps[1], [101, 202], 1, "mean")


def test_keypoint_results_wraps_the_person_rows(monkeypatch):
    from detectorch_amd.utils import keypoints as ku
    xy = np.arange(3 * 4 * 2, dtype=f32).reshape(3, 4, 2)
    seen = {}
    monkeypatch.setattr(ku, "heatmaps_to_keypoints", lambda maps, rois, min_size=0: seen.update(maps=maps, rois=rois) or xy)
    cls_boxes = [[], np.zeros((3, 5), f32), np.zeros((2, 5), f32)]
    out = ku.keypoint_results(cls_boxes, "maps", "rois", 3)
    assert seen == dict(maps="maps", rois="rois") and len(out) == 3 and out[0] == [] and out[2] == []
    assert len(out[1]) == 3 and all(np.array_equal(out[1][i], xy[i]) and out[1][i].shape == (4, 2) for i in range(3))
    with pytest.raises(AssertionError):
        ku.keypoint_results(cls_boxes, "maps", "rois", 3, person_class=2)


def test_keypoint_head_shapes_and_state_dict():
    import torch
    from detectorch_amd.model.detector import keypoint_head
    torch.manual_seed(0)
    h = keypoint_head(5)
    assert sorted({k.split(".")[0] for k in h.state_dict()}) == ["conv_fcn%d" % i for i in range(1, 9)] + ["kps_score_lowres"]
    with torch.no_grad():
        y = h(torch.randn(2, 256, 14, 14))
        assert tuple(y.shape) == (2, 5, 56, 56)
        # the fixed bilinear deconvolution reproduces a constant map away from the border
        up = torch.nn.functional.conv_transpose2d(torch.ones(1, 5, 28, 28), h.up_filter, stride=2, padding=1, groups=5)
    assert tuple(up.shape) == (1, 5, 56, 56) and torch.equal(up[:, :, 1:-1, 1:-1], torch.ones(1, 5, 54, 54))
