"""The detection post-processing (detections.hip) away from the reference's default arguments: score_thresh, nms_thresh, the box
weights, max_det, scores of both signs at the limit, and the voting / Soft-NMS parameters -- one argument at a time, the others at
their defaults.  -m gpu.

B = 2, R = 300, n_rois = [300, 173], 81 classes, with twelve roi rows per image repeated under other scores (IoU = 1 pairs:
tests/output_args_cases.py: det_batch).  Hard NMS is compared with oracle.postprocess_detections, the Soft-NMS and voting modes
with det_options_ref.decode + compose; same detections, rois, counts, scores and boxes, bit for bit, as
tests/test_hip_det_options.py::test_mode_matrix_vs_oracle compares.  tests/test_output_args_host.py pins on the oracle alone what makes
these cases non-empty."""
import numpy as np
import pytest
import torch

import output_args_cases as oc
from det_options_ref import compose, decode, kwargs_of
from output_args_cases import check_image

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from detectorch_amd import hip as h
    h.lib()
    return h


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def batch(oracle):
    """the shared inputs, on the host and on the device, and the decoded boxes at the default weights (never modified)"""
    rois5, cls, deltas, src, dst = oc.det_batch()
    logits = oc.as_logits(cls)
    b = dict(rois5=rois5, cls=cls, deltas=deltas, logits=logits, prob_of_logits=oracle.softmax_rows(logits), src=src, dst=dst,
             boxes=[decode(oracle, rois5[i, :n, 1:], oc.DET_SF[i], oc.DET_IM[i], deltas[i, :n]) for i, n in enumerate(oc.DET_N_ROIS)])
    b["dev"] = dict(rois5=cu(rois5), cls=cu(cls), deltas=cu(deltas), logits=cu(logits), n_rois=cu(oc.DET_N_ROIS), sf=cu(oc.DET_SF),
                    im=cu(oc.DET_IM))
    return b


def run_hip(hip, batch, logits=False, **kw):
    d = batch["dev"]
    out = hip.postprocess_detections(d["rois5"], d["n_rois"], d["logits"] if logits else d["cls"], d["deltas"], d["sf"], d["im"],
                                     scores_are_logits=logits, **kw)
    torch.cuda.synchronize()
    return out


def ref_hard(oracle, batch, b, scores=None, **kw):
    n = int(oc.DET_N_ROIS[b])
    sc = batch["cls"] if scores is None else scores
    return oracle.postprocess_detections(batch["rois5"][b, :n, 1:], oc.DET_SF[b], oc.DET_IM[b], sc[b, :n], batch["deltas"][b, :n], **kw)


def ref_compose(oracle, batch, b, method, vote=None, **kw):
    n = int(oc.DET_N_ROIS[b])
    return compose(oracle, batch["cls"][b, :n], batch["boxes"][b], method, vote, **kw)


# ---- score_thresh ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("score_thresh", [0.0, 0.01, 0.3, 0.9, 1.0])
def test_score_thresh(hip, oracle, batch, score_thresh, logits):
    """result_utils.py:127 `scores[:, j] > score_thresh`: 0.0 makes every non-zero score a candidate (300 per class), 1.0 none"""
    out = run_hip(hip, batch, logits, score_thresh=score_thresh)
    scores = batch["prob_of_logits"] if logits else batch["cls"]
    counts = []
    for b in range(2):
        ref, ref_roi = ref_hard(oracle, batch, b, scores, score_thresh=score_thresh)
        check_image(out, b, ref, ref_roi, 128, oc.DET_SF[b])
        counts.append(ref.shape[0])
    if score_thresh == 1.0:
        assert counts == [0, 0]
    elif score_thresh <= 0.3:
        assert min(counts) > 0
    if score_thresh == 0.0:
        n_cand = [int((scores[b, :n, 1:] > 0).sum()) for b, n in enumerate(oc.DET_N_ROIS)]
        assert n_cand == [300 * 80, 173 * 80] and min(counts) >= 100


def test_score_thresh_changes_the_unlimited_result(hip, oracle, batch):
    """the same sweep without the max_det limit, so that the candidate set itself is compared (a threshold folded into a constant
    could hide behind the 100 best rows): det_count differs for every value"""
    seen = []
    for score_thresh in (0.01, 0.05, 0.3):
        out = run_hip(hip, batch, False, score_thresh=score_thresh, max_det=0, max_out=8192)
        for b in range(2):
            ref, ref_roi = ref_hard(oracle, batch, b, score_thresh=score_thresh, max_det=0)
            check_image(out, b, ref, ref_roi, 8192, oc.DET_SF[b])
        seen.append(int(out[3][0]))
    assert seen[0] > seen[1] > seen[2] > 0


# ---- nms_thresh -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_det", [100, 0])
@pytest.mark.parametrize("nms_thresh", [-0.5, 0.0, 1e-6, 0.3, 0.7, 1.0, 1.5])
def test_nms_thresh_hard(hip, oracle, batch, nms_thresh, max_det):
    """cython_nms.pyx:83-84 `ovr >= thresh` inside det_candidates_kernel: thresh <= 0 takes the division for every pair (thr_pos), the
    band test scales with the threshold.  From the oracle alone: thresh <= 0 keeps exactly one box per non-empty class, 1.5
    suppresses nothing, 1.0 drops exactly the copied rows (max_det = 0 shows all of that, max_det = 100 is the default)."""
    max_out = 128 if max_det else 2048
    out = run_hip(hip, batch, nms_thresh=nms_thresh, max_det=max_det, max_out=max_out)
    for b in range(2):
        n = int(oc.DET_N_ROIS[b])
        ref, ref_roi = ref_hard(oracle, batch, b, nms_thresh=nms_thresh, max_det=max_det)
        check_image(out, b, ref, ref_roi, max_out, oc.DET_SF[b])
        if max_det:
            continue
        cand = batch["cls"][b, :n, 1:] > np.float32(0.05)
        if nms_thresh <= 0:
            assert np.array_equal(ref[:, 5].astype(int), np.flatnonzero(cand.any(0)) + 1)
        if nms_thresh == 1.5:
            assert ref.shape[0] == int(cand.sum())
        if nms_thresh == 1.0:
            all_rows, _ = ref_hard(oracle, batch, b, nms_thresh=1.5, max_det=0)
            want = sorted((int(r), int(j) + 1) for r in batch["dst"][b] for j in np.flatnonzero(cand[r]))
            kept = set(zip(ref_roi.tolist(), ref[:, 5].astype(int).tolist()))
            dropped = sorted((int(r), int(j) + 1) for r, j in zip(*np.nonzero(cand)) if (int(r), int(j) + 1) not in kept)
            assert len(want) >= 20 and dropped == want and all_rows.shape[0] - ref.shape[0] == len(want)


@pytest.mark.parametrize("nms_thresh", [0.0, -0.5, 1e-6])
def test_nms_thresh_not_positive_with_infinite_union(hip, oracle, nms_thresh):
    """The one input on which the `thresh <= 0` branch of the fused NMS (thr_pos: always divide) decides differently from the sign
    test of iou_threshold.h: a union that overflows float32.  inter / inf = 0 >= 0 suppresses the pair (cython_nms.pyx:83-84 on
    float32), while inter - 0 * inf is NaN and its sign says nothing.  Finite unions give the same answer either way (thresh * u = 0:
    the sign of inter, and inter = 0 falls into the band and is divided), which is why the ordinary thresh <= 0 cases do not need
    the branch.  Through dtc_box_results_nms_limit, whose boxes are not clipped; one 2e20 x 2e20 box per class."""
    scores, boxes, huge = oc.overflowing_union_batch()
    out = hip.box_results_nms_limit(cu(scores), cu(boxes), nms_thresh=nms_thresh)
    torch.cuda.synchronize()
    ref, ref_roi = compose(oracle, scores[0], boxes[0], "nms", None, nms_thresh=nms_thresh)
    check_image((out[0], out[1], None, out[2]), 0, ref, ref_roi, 128)
    kept_huge = [(int(r), int(c)) for r, c in zip(ref_roi, ref[:, 5]) if huge.get(int(c)) == int(r)]
    if nms_thresh <= 0:
        assert ref.shape[0] == 2 and not kept_huge                           # the class's best box suppresses everything, the huge box too
    else:
        assert len(kept_huge) == 2                                           # IoU 0 < 1e-6: the huge boxes stay


@pytest.mark.parametrize("method", ["linear", "gaussian"])
@pytest.mark.parametrize("nms_thresh", [0.0, 0.3, 0.7])
def test_nms_thresh_soft(hip, oracle, batch, nms_thresh, method):
    out = run_hip(hip, batch, nms_thresh=nms_thresh, **kwargs_of(method, None))
    for b in range(2):
        ref, ref_roi = ref_compose(oracle, batch, b, method, nms_thresh=nms_thresh)
        assert ref.shape[0] > 0
        check_image(out, b, ref, ref_roi, 128, oc.DET_SF[b])


# ---- weights --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weights", [(1, 1, 1, 1), (5, 5, 2.5, 2.5), (10, 5, 3, 7)])
def test_box_weights(hip, oracle, batch, weights):
    """bbox_transform's weights (boxes.py:180-183) through the fused decode of dtc_postprocess_detections and through
    dtc_bbox_transform + dtc_box_results_nms_limit; unequal x / y and w / h weights tell the four apart"""
    out = run_hip(hip, batch, weights=weights)
    for b in range(2):
        n = int(oc.DET_N_ROIS[b])
        ref, ref_roi = ref_hard(oracle, batch, b, weights=tuple(float(w) for w in weights))
        assert ref.shape[0] > 0
        check_image(out, b, ref, ref_roi, 128, oc.DET_SF[b])
        boxes = (batch["rois5"][b, :n, 1:] / np.float32(oc.DET_SF[b])).astype(np.float32)
        dec = hip.bbox_transform(cu(boxes), cu(batch["deltas"][b, :n]), weights, clip_to=(float(oc.DET_IM[b, 0]), float(oc.DET_IM[b, 1])))
        ref_dec = decode(oracle, batch["rois5"][b, :n, 1:], oc.DET_SF[b], oc.DET_IM[b], batch["deltas"][b, :n], weights)
        assert np.array_equal(dec.cpu().numpy(), ref_dec)
        two = hip.box_results_nms_limit(cu(batch["cls"][b:b + 1, :n]), dec[None])
        torch.cuda.synchronize()
        check_image((two[0], two[1], None, two[2]), 0, ref, ref_roi, 128)
    assert not np.array_equal(ref_hard(oracle, batch, 0)[0][:, :4], ref_hard(oracle, batch, 0, weights=tuple(float(w) for w in weights))[0][:, :4])


# ---- max_det --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["nms", "linear"])
def test_max_det_sweep(hip, oracle, batch, method):
    """det_finalize's radix select runs only when total > max_det: K = the unlimited count of image 0, max_det 1, 2, 17, K - 1 (the
    select drops ONE row), K (the boundary: no select), K + 1.  max_out >= K, so nothing is truncated; K is above the 1024 survivors
    the fast output path holds, so K - 1 ... K + 1 also take the general output path."""
    K = ref_compose(oracle, batch, 0, method, max_det=0)[0].shape[0]
    assert K > 1024 + 1                                                      # det_finalize's kFinSurvMax: K - 1 survivors leave the fast path
    max_out = K + 8
    for max_det in (1, 2, 17, K - 1, K, K + 1):
        out = run_hip(hip, batch, max_det=max_det, max_out=max_out, **kwargs_of(method, None))
        for b in range(2):
            ref, ref_roi = ref_compose(oracle, batch, b, method, max_det=max_det)
            check_image(out, b, ref, ref_roi, max_out, oc.DET_SF[b])
            if b == 0:
                assert ref.shape[0] == min(max_det, K), (max_det, ref.shape[0])


# ---- negative and zero scores at the limit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_det", [5, 50, 200])
def test_signed_scores_at_the_limit(hip, oracle, max_det):
    """dtc_box_results_nms_limit with score_thresh = -1: kept scores of both signs and exact zeros reach the limit's radix select, whose
    ordered keys flip at the sign.  max_det 5: the threshold score is positive; 50: it is exactly 0.0 and every kept zero ties with
    it (`>=` keeps them all: det_count > max_det); 200: negative."""
    scores, boxes, _ = oc.signed_score_batch()
    out = hip.box_results_nms_limit(cu(scores), cu(boxes), score_thresh=-1.0, max_det=max_det, max_out=256)
    torch.cuda.synchronize()
    for b in range(2):
        ref, ref_roi = compose(oracle, scores[b], boxes[b], "nms", None, score_thresh=-1.0, max_det=max_det)
        check_image((out[0], out[1], None, out[2]), b, ref, ref_roi, 256)
        lo = ref[:, 4].min()
        assert (lo > 0, lo == 0, lo < 0) == (max_det == 5, max_det == 50, max_det == 200)
        assert (ref.shape[0] > max_det) == (max_det == 50)


# ---- voting and Soft-NMS parameters -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("vote", [0.5, 1.0])
def test_vote_thresh_with_hard_nms_at_03(hip, oracle, batch, vote):
    out = run_hip(hip, batch, nms_thresh=0.3, **kwargs_of("nms", vote))
    moved = 0
    for b in range(2):
        ref, ref_roi = ref_compose(oracle, batch, b, "nms", vote, nms_thresh=0.3)
        check_image(out, b, ref, ref_roi, 128, oc.DET_SF[b])
        moved += int((ref[:, :4] != ref_compose(oracle, batch, b, "nms", None, nms_thresh=0.3)[0][:, :4]).any(1).sum())
    # at 1.0 a row's voters are itself and its copies: the score-weighted mean of equal coordinates, x * s / s, rounds a few dozen
    # of them by one ulp, so the bit-equal comparison above tells the voted rows from the plain NMS rows at 1.0 too
    assert moved >= 20


@pytest.mark.parametrize("sigma", [0.3, 1.0])
def test_gaussian_soft_nms_sigma(hip, oracle, batch, sigma):
    out = run_hip(hip, batch, do_soft_nms=True, soft_nms_method="gaussian", soft_nms_sigma=sigma)
    for b in range(2):
        ref, ref_roi = ref_compose(oracle, batch, b, "gaussian", sigma=sigma)
        check_image(out, b, ref, ref_roi, 128, oc.DET_SF[b])
        assert not np.array_equal(ref[:, 4], ref_compose(oracle, batch, b, "gaussian")[0][:, 4])      # not the default sigma's scores
