"""The evaluation chain on the GPU at the limits of its contracts (tests/eval_limit_cases.py; the "limits" sections of
tests/README_eval.md and tests/README_segm_eval.md): dtc_eval_match, dtc_segm_iou + dtc_segm_match, dtc_eval_accumulate and
dtc_eval_proposal_recall against tests/coco_eval_ref.py, tests/segm_eval_ref.py and the reference's own evaluate_box_proposals
(tests/golden/eval_limits.npz).  No tolerance: every integer output equal, iou, precision, recall, stats and the proposal rounds
BIT-equal; ar within 100 x 2^-53.  Every output is pre-filled with 0xFF, the rows past the counts are poisoned.
tests/test_eval_limits_host.py holds, without a GPU, that every case has the condition it is named for."""
import numpy as np
import pytest
import torch

from conftest import golden
import coco_eval_ref as cr
import eval_limit_cases as lc
import segm_eval_ref as sr
import test_hip_segm as hs

pytestmark = pytest.mark.gpu

_REF = {}
cu, f64, filled, same_bits = hs.cu, hs.f64, hs.filled, hs.same_bits


def thaw(case):
    """the shared case is read-only; torch takes writable arrays"""
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in case.items()}


def reference(name):
    """the case and the box restatement's answer, computed once"""
    if name not in _REF:
        case = thaw(lc.MATCH_CASES[name]())
        _REF[name] = (case, cr.run(case))
    return _REF[name]


def box_match(case, image_base=0, images=slice(None)):
    from detectorch_amd import hip_eval
    cut = lambda k: cu(case[k][images])
    N, max_out = case["dets"][images].shape[:2]
    G, T, A = case["gt_boxes"].shape[1], len(case["iou_thrs"]), len(case["area_rngs"])
    out = filled(hip_eval.match_outputs(N, max_out, G, case["num_classes"], T, A, torch.device("cuda")))
    hip_eval.eval_match(cut("dets"), cut("det_count"), cut("gt_boxes"), cut("gt_classes"), cut("gt_is_crowd"), cut("gt_counts"),
                        cut("gt_area") if "gt_area" in case else None, case["num_classes"], f64(case["iou_thrs"]), f64(case["area_rngs"]),
                        case["max_dets"][-1], image_base=image_base, out=out)
    return out


# ---- dtc_eval_match and dtc_eval_accumulate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.MATCH_CASES))
def test_match_and_accumulate_equal_the_restatement(name):
    case, want = reference(name)
    rec = box_match(case)
    hs.check_records(rec, want)
    hs.check_result(hs.run_accumulate(case, rec), want)


# ---- the same cases through dtc_segm_iou + dtc_segm_match ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(set(lc.MATCH_CASES) - set(lc.BOX_ONLY)))
def test_segm_protocol_equals_the_box_protocol(name):
    """filled integer rectangles through dtc_segm_iou + dtc_segm_match; where the boxes cannot be rectangles, dtc_segm_match on the
    box protocol's own IoU matrix; either way the records and the result are the box protocol's, bit for bit"""
    case, want = reference(name)
    if name in lc.NOT_RECTANGLES:
        iou, det_area, gt_mask_area = lc.crafted_from_boxes(case)
        rec = hs.run_match(case, cu(iou), cu(det_area), cu(gt_mask_area))
        b = case
    else:
        key = ("bridge", name)
        if key not in _REF:
            b, s = lc.bridge(case)
            _REF[key] = (b, s, cr.run(b))
        b, s, want = _REF[key]
        out = hs.run_iou(s)
        rec = hs.run_match(s, out["iou"], out["det_area"], out["gt_mask_area"])
    hs.check_records(rec, want)
    hs.check_result(hs.run_accumulate(b, rec), want)
    box = box_match(b)
    for k in hs.RECORDS + hs.WORDS:
        assert torch.equal(rec[k], box[k]), k


# ---- image_base ----------------------------------------------------------------------------------------------------------------------------
def test_sort_keys_at_the_last_image_base():
    from detectorch_amd import hip_eval
    case, _ = reference("score_bits")
    base = hip_eval.MAX_IMAGES - 4
    want = lc.run_at(case, base)
    rec = box_match(case, image_base=base)
    hs.check_records(rec, want)
    assert int(rec["sort_key"][rec["dt_rank"] >= 0].max()) & (hip_eval.MAX_IMAGES - 1) == hip_eval.MAX_IMAGES - 1
    hs.check_result(hs.run_accumulate(case, rec), want)


@pytest.mark.parametrize("base", [0, (1 << 21) - 4])
def test_two_calls_with_consecutive_image_base_join(base):
    """images 0 .. 1 at image_base and images 2 .. 3 at image_base + 2, concatenated: the stable sort of the joined keys puts equal
    scores of different calls in image order, and the result is the restatement's on the four images"""
    case, _ = reference("score_bits")
    want = lc.run_at(case, base)
    first, second = box_match(case, base, slice(0, 2)), box_match(case, base + 2, slice(2, 4))
    rec = {k: torch.cat([first[k], second[k]]) for k in first}
    hs.check_records(rec, want)
    hs.check_result(hs.run_accumulate(case, rec), want)


# ---- dtc_eval_proposal_recall ----------------------------------------------------------------------------------------------------------------
def proposal_inputs(case):
    roidb, n_gt = case["roidb"], case["n_gt"]
    N, G = len(roidb), max(n_gt)
    boxes, area = np.full((N, G, 4), np.nan, np.float32), np.full((N, G), np.nan, np.float32)
    cls, crowd = np.ones((N, G), np.int32), np.zeros((N, G), np.int32)
    for i, (e, n) in enumerate(zip(roidb, n_gt)):
        boxes[i, :n], area[i, :n], cls[i, :n], crowd[i, :n] = e['boxes'][:n], e['seg_areas'][:n], e['gt_classes'][:n], e['is_crowd'][:n]
    gt = dict(gt_boxes=cu(boxes), gt_classes=cu(cls), gt_is_crowd=cu(crowd), gt_counts=cu(np.asarray(n_gt, np.int32)))
    if not case.get("no_area"):
        gt["gt_area"] = cu(area)
    if "device" in case:
        props, counts = (v.copy() for v in case["device"])
    else:
        rows = [e['boxes'][np.flatnonzero(e['gt_classes'] == 0)] for e in roidb]
        P = max(1, max(len(r) for r in rows))
        props, counts = np.full((N, P, 4), np.nan, np.float32), np.zeros(N, np.int32)
        for i, r in enumerate(rows):
            props[i, :len(r)], counts[i] = r, len(r)
    return cu(props), cu(counts), gt


@pytest.mark.parametrize("name", sorted(lc.proposal_cases()))
def test_proposal_recall_equals_the_reference(name):
    from detectorch_amd import hip_eval
    from detectorch_amd.utils import evaluator as E
    g, case = golden("eval_limits"), lc.proposal_cases()[name]
    rounds, meta, summary, limit = g[name + "_rounds"], g[name + "_meta"], g[name + "_summary"], case["limit"]
    props, counts, gt = proposal_inputs(case)
    at = 0
    for a, area in enumerate(lc.PROPOSAL_AREAS):
        rng = torch.tensor(E.PROPOSAL_AREAS[area], dtype=torch.float64, device="cuda")
        out = hip_eval.proposal_recall(props, counts, gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"],
                                       gt.get("gt_area"), rng, limit=limit or 0)
        ov, n_pos, n_ov = (out[k].cpu().numpy() for k in ("gt_overlaps", "n_pos", "n_overlaps"))
        for i in range(len(case["roidb"])):
            n, want_pos = meta[a, i]
            assert n_pos[i] == want_pos and n_ov[i] == n, (area, i)
            assert same_bits(ov[i, :n], rounds[at:at + n]) and not ov[i, n:].any(), (area, i)
            at += n
        res = E.evaluate_box_proposals_batched(props, counts, gt, area=area, limit=limit)
        assert res['num_pos'] == int(summary[a, 11]) and same_bits(res['recalls'], summary[a, :10])
        # ar is the mean of ten recalls in [0, 1]: nine additions and one division, each within half an ulp of a value <= 10
        if np.isfinite(summary[a, 10]):
            assert abs(res['ar'] - summary[a, 10]) <= 10 * 10 * 2.0 ** -53
        else:
            assert np.isnan(res['ar']) or res['ar'] == summary[a, 10]
    assert at == len(rounds)


# ---- dtc_segm_iou ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(lc.SEGM_CASES))
def test_segm_iou_limits_equal_the_restatement(name):
    make, mode = lc.SEGM_CASES[name]
    key = ("segm", name)
    if key not in _REF:
        case = thaw(make())
        _REF[key] = (case, sr.run(case, counts=sr.interval_counts if mode == "interval" else None))
    case, want = _REF[key]
    out = hs.run_iou(case)
    hs.check_iou(out, want)
    rec = hs.run_match(case, out["iou"], out["det_area"], out["gt_mask_area"])
    hs.check_records(rec, want)
    hs.check_result(hs.run_accumulate(case, rec), want)
