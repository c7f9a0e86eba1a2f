"""The evaluation on the GPU (include/detectorch_eval_hip.h, detectorch_amd/utils/evaluator.py) against its yardsticks:
  * dtc_eval_match and dtc_eval_accumulate against the numpy restatement of COCOeval (tests/coco_eval_ref.py) on the cases of
    tests/eval_cases.py: every integer output equal, precision, recall and stats BIT-equal (both sides do the same correctly rounded
    float64 operations in the same order); outputs pre-filled with 0xFF; the rows past the counts of every case hold NaN;
  * update() in two and three chunks, and captured in a graph and replayed on changed inputs, against one eager call;
  * dtc_eval_proposal_recall against the reference's own evaluate_box_proposals (tests/golden/eval.npz): rounds, n_pos and recalls
    bit for bit, ar within the roundings of a ten-term mean;
  * wrong dtypes and sizes over the limits are refused with the documented errors."""
import warnings

import numpy as np
import pytest
import torch

from conftest import golden
import coco_eval_ref as cr
import eval_cases as ec

pytestmark = pytest.mark.gpu

_REF = {}


def reference(name):
    """the case and the restatement's answer, computed once"""
    if name not in _REF:
        case = ec.MATCH_CASES[name]()
        _REF[name] = (case, cr.run(case))
    return _REF[name]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def on_device(case):
    t = lambda k: torch.from_numpy(case[k]).cuda()
    gt = {k: t(k) for k in ("gt_boxes", "gt_classes", "gt_is_crowd", "gt_counts")}
    if "gt_area" in case:
        gt["gt_area"] = t("gt_area")
    return t("dets"), t("det_count"), gt


def evaluator(case, **kw):
    from detectorch_amd.utils.evaluator import BoxEvaluator
    return BoxEvaluator(num_classes=case["num_classes"], iou_thrs=case["iou_thrs"], rec_thrs=case["rec_thrs"], max_dets=case["max_dets"],
                        area_rngs=case["area_rngs"], **kw)


def check_result(res, want):
    assert np.array_equal(res["counts"], want["counts"])
    for k in ("precision", "recall", "stats"):
        assert res[k].dtype == np.float64 and same_bits(res[k], want[k]), k


@pytest.mark.parametrize("name", sorted(ec.MATCH_CASES))
def test_match_and_accumulate_equal_the_restatement(name):
    from detectorch_amd import hip_eval
    from detectorch_amd.utils.evaluator import summarize_stats
    case, want = reference(name)
    dets, det_count, gt = on_device(case)
    N, max_out = dets.shape[:2]
    G, T, A = gt["gt_boxes"].shape[1], len(case["iou_thrs"]), len(case["area_rngs"])
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()
    out = hip_eval.match_outputs(N, max_out, G, case["num_classes"], T, A, dets.device)
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    hip_eval.eval_match(dets, det_count, gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], gt.get("gt_area"),
                        case["num_classes"], f64(case["iou_thrs"]), f64(case["area_rngs"]), case["max_dets"][-1], out=out)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("dt_rank", "gt_ignore", "gt_match", "npig", "sort_key"):
        assert np.array_equal(got[k], want[k]), k
    for k in ("dt_match", "dt_ignore"):
        assert np.array_equal(got[k].view(np.uint64), want[k]), k
    R, M, K = len(case["rec_thrs"]), len(case["max_dets"]), case["num_classes"] - 1
    acc = hip_eval.accumulate_outputs(T, R, K, A, M, dets.device)
    for v in acc.values():
        v.view(torch.uint8).fill_(0xFF)
    hip_eval.eval_accumulate(out["dt_rank"], out["dt_match"], out["dt_ignore"], out["sort_key"], out["npig"], case["num_classes"], T, A,
                             f64(case["rec_thrs"]), torch.tensor(case["max_dets"], dtype=torch.int32).cuda(), out=acc)
    res = {k: v.cpu().numpy() for k, v in acc.items()}
    res["stats"] = summarize_stats(res["precision"], res["recall"], case["iou_thrs"])
    check_result(res, want)


@pytest.mark.parametrize("chunks", [(6,), (2, 4), (1, 3, 2)])
def test_update_in_chunks(chunks):
    case, want = reference("random")
    dets, det_count, gt = on_device(case)
    ev, at = evaluator(case), 0
    for n in chunks:
        ev.update(dets[at:at + n].contiguous(), det_count[at:at + n].contiguous(), {k: v[at:at + n].contiguous() for k, v in gt.items()})
        at += n
    check_result(ev.accumulate(), want)
    stats, ap = ev.summarize()
    assert same_bits(stats, want["stats"]) and ap["per_class"].shape == (3,)
    p = want["precision"][:, :, :, 0, -1]
    assert ap["mean"] == float(np.mean(p[p > -1]))


def test_overflow_raises_or_truncates():
    case, want = reference("overflow")
    ev = evaluator(case)
    ev.update(*on_device(case))
    with pytest.raises(RuntimeError, match="image 0: 21 detections but only 16 rows"):
        ev.accumulate()
    ev = evaluator(case, on_overflow="truncate")
    ev.update(*on_device(case))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        check_result(ev.accumulate(), want)
    assert any(issubclass(x.category, RuntimeWarning) for x in w)


def test_evaluate_boxes_from_result_lists():
    from detectorch_amd.utils.evaluator import evaluate_boxes
    from detectorch_amd.utils.result_utils import assemble_results
    case, want = reference("random")
    all_boxes, _ = assemble_results(case["dets"], case["det_count"], num_classes=case["num_classes"])
    roidb = []
    for n in range(len(case["dets"])):
        g = int(case["gt_counts"][n])
        roidb.append(dict(boxes=case["gt_boxes"][n, :g], gt_classes=case["gt_classes"][n, :g], is_crowd=case["gt_is_crowd"][n, :g],
                          seg_areas=case["gt_area"][n, :g]))
    ev = evaluate_boxes(all_boxes, roidb, batch=4)
    check_result(ev.accumulate(), want)


def test_update_captured_in_a_graph():
    """update() captured after one eager call and replayed twice on changed inputs equals the eager evaluation of those inputs"""
    cases = [ec.random_case(s) for s in (7, 8, 9)]
    dets, det_count, gt = on_device(cases[0])
    ev = evaluator(cases[0])
    ev.update(dets, det_count, gt)                              # eager: loads the library, warms the allocator
    torch.cuda.synchronize()
    ev.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(dets, det_count, gt)
    for case in cases[1:]:
        d2, c2, g2 = on_device(case)
        dets.copy_(d2), det_count.copy_(c2)
        for k in gt:
            gt[k].copy_(g2[k])
        graph.replay()
        got = ev.accumulate()
        eager = evaluator(case)
        eager.update(d2, c2, g2)
        want = eager.accumulate()
        check_result(got, want)
        check_result(got, cr.run(case))
        assert (got["precision"] > 0).any()


def test_wrong_dtypes_and_sizes_are_refused():
    from detectorch_amd import hip_eval
    from detectorch_amd.utils.evaluator import BoxEvaluator
    case, _ = reference("basic")
    dets, det_count, gt = on_device(case)
    ev = evaluator(case)
    with pytest.raises(TypeError, match="dets"):
        ev.update(dets.double(), det_count, gt)
    with pytest.raises(TypeError, match="det_count"):
        ev.update(dets, det_count.long(), gt)
    with pytest.raises(TypeError, match="gt_classes"):
        ev.update(dets, det_count, dict(gt, gt_classes=gt["gt_classes"].long()))
    with pytest.raises(TypeError, match="gt_boxes"):
        ev.update(dets, det_count, dict(gt, gt_boxes=gt["gt_boxes"][:, :, :3]))
    z = lambda *s, dt=torch.float32: torch.zeros(s, dtype=dt, device="cuda")
    i32 = torch.int32
    with pytest.raises(ValueError, match="at most 512"):
        ev.update(z(4, 513, 6), det_count, gt)
    with pytest.raises(ValueError, match="at most 256 gt"):
        ev.update(dets, det_count, dict(gt_boxes=z(4, 257, 4), gt_classes=z(4, 257, dt=i32), gt_is_crowd=z(4, 257, dt=i32), gt_counts=z(4, dt=i32)))
    with pytest.raises(ValueError, match="unsupported parameters"):
        BoxEvaluator(iou_thrs=np.linspace(0.1, 0.9, 17), area_rngs=np.zeros((4, 2)))
    with pytest.raises(ValueError, match="unsupported parameters"):
        BoxEvaluator(num_classes=1025)
    ev.update(dets, det_count, gt)
    with pytest.raises(ValueError, match="max_out changed"):
        ev.update(z(4, 20, 6), det_count, gt)
    with pytest.raises(TypeError, match="proposals"):
        hip_eval.proposal_recall(z(4, 5, 4).half(), det_count, gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], None,
                                 z(2, dt=torch.float64))
    with pytest.raises(ValueError, match="unsupported shape"):
        hip_eval.proposal_recall(z(4, 65537, 4), det_count, gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], None,
                                 z(2, dt=torch.float64))


# ---- proposal recall -----------------------------------------------------------------------------------------------------------------------
def whole_rows(roidb, nan_pad=True):
    """every row of the roidb entries as gt tensors -- proposals (gt_classes == 0) and crowd rows among them, which the kernel has to
    skip -- or None when an image has more than 256 rows; the rows past the counts hold NaN and a class that would count"""
    G = max(len(e['boxes']) for e in roidb)
    if G > 256:
        return None
    N = len(roidb)
    boxes, area = np.full((N, G, 4), np.nan, np.float32), np.full((N, G), np.nan, np.float32)
    cls, crowd, counts = np.ones((N, G), np.int32), np.zeros((N, G), np.int32), np.zeros(N, np.int32)
    for i, e in enumerate(roidb):
        n = counts[i] = len(e['boxes'])
        boxes[i, :n], area[i, :n], cls[i, :n], crowd[i, :n] = e['boxes'], e['seg_areas'], e['gt_classes'], e['is_crowd']
    t = lambda a: torch.from_numpy(a).cuda()
    return dict(gt_boxes=t(boxes), gt_classes=t(cls), gt_is_crowd=t(crowd), gt_counts=t(counts), gt_area=t(area))


@pytest.mark.parametrize("case", sorted(ec.proposal_cases()))
def test_proposal_recall_equals_the_reference(case):
    from detectorch_amd import hip_eval
    from detectorch_amd.utils import evaluator as E
    g = golden("eval")
    roidb, limit = ec.proposal_cases()[case]
    rounds, meta, summary, whole = g[case + "_rounds"], g[case + "_meta"], g[case + "_summary"], g[case + "_gt_overlaps"]
    props = [e['boxes'][np.flatnonzero(e['gt_classes'] == 0)] for e in roidb]
    N, P = len(roidb), max(1, max(len(p) for p in props))
    boxes, counts = np.full((N, P, 4), np.nan, np.float32), np.zeros(N, np.int32)
    for i, p in enumerate(props):
        boxes[i, :len(p)], counts[i] = p, len(p)
    boxes, counts = torch.from_numpy(boxes).cuda(), torch.from_numpy(counts).cuda()
    gt = whole_rows(roidb) or E.pack_gt(roidb, "cuda")
    at = at_whole = 0
    for a, area in enumerate(ec.AREAS):
        rng = torch.tensor(E.PROPOSAL_AREAS[area], dtype=torch.float64, device="cuda")
        out = hip_eval.proposal_recall(boxes, counts, gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], gt["gt_area"],
                                       rng, limit=limit or 0)
        ov, n_pos, n_ov = (out[k].cpu().numpy() for k in ("gt_overlaps", "n_pos", "n_overlaps"))
        for i in range(N):
            n, want_pos = meta[a, i]
            assert n_pos[i] == want_pos and n_ov[i] == n
            if limit != 0:                           # the library's limit = 0 means none: keeping no proposal is the wrappers' (below)
                assert same_bits(ov[i, :n], rounds[at:at + n]) and not ov[i, n:].any()
            at += n
        # the wrappers: the batched form and the reference's signature
        for res in (E.evaluate_box_proposals_batched(boxes, counts, gt, area=area, limit=limit),
                    E.evaluate_box_proposals(roidb, area=area, limit=limit)):
            n = len(res['gt_overlaps'])
            assert res['num_pos'] == int(summary[a, 11]) and same_bits(res['gt_overlaps'], whole[at_whole:at_whole + n])
            assert same_bits(res['recalls'], summary[a, :10])
            # ar is the mean of ten recalls in [0, 1]: nine additions and one division, each within half an ulp of a value <= 10
            if np.isfinite(summary[a, 10]):
                assert abs(res['ar'] - summary[a, 10]) <= 10 * 10 * 2.0 ** -53
            else:
                assert np.isnan(res['ar']) or res['ar'] == summary[a, 10]
        at_whole += n
    assert at == len(rounds) and at_whole == len(whole)
