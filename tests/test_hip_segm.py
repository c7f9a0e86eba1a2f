"""The mask evaluation on the GPU (include/detectorch_segm_hip.h, detectorch_amd/utils/evaluator.py:MaskEvaluator) against its
yardsticks (tests/README_segm_eval.md).  No tolerance anywhere: every integer output equal, iou, precision, recall and stats BIT-equal
(both sides do the same correctly rounded float64 operations on exact integers).
  * dtc_segm_iou against the numpy restatement on decoded bitmaps (tests/segm_eval_ref.py) on the cases of tests/segm_eval_cases.py;
    outputs and workspace pre-filled with 0xFF; the rows past the counts hold garbage runs and huge or negative run counts;
  * the bridge: on filled integer rectangles, dtc_segm_iou + dtc_segm_match + dtc_eval_accumulate against dtc_eval_match +
    dtc_eval_accumulate on the boxes, and against the box protocol's restatement (tests/coco_eval_ref.py);
  * dtc_segm_match on crafted IoU matrices;
  * MaskEvaluator.update in one and three chunks, and captured in a graph and replayed on rewritten inputs; evaluate_masks from
    result lists with compressed strings; hip.mask_paste -> hip.mask_rle -> MaskEvaluator end to end;
  * masks that did not fit are reported; wrong dtypes and sizes over the limits are refused."""
import warnings

import numpy as np
import pytest
import torch

import coco_eval_ref as cr
import segm_eval_cases as sc
import segm_eval_ref as sr

pytestmark = pytest.mark.gpu

_REF = {}
RECORDS = ("dt_rank", "gt_ignore", "gt_match", "npig", "sort_key")
WORDS = ("dt_match", "dt_ignore")
GT_KEYS = ("gt_runs", "gt_n_runs", "gt_classes", "gt_is_crowd", "gt_counts", "gt_area")


def reference(key, make, **kw):
    """the case and the restatement's answer, computed once"""
    if key not in _REF:
        case = make()
        _REF[key] = (case, sr.run(case, **kw))
    return _REF[key]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def cu(a):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def on_device(case):
    """-> dets, det_count, the dict hip.mask_rle would return, im_size, gt"""
    gt = {k: cu(case[k]) for k in GT_KEYS if k in case}
    return cu(case["dets"]), cu(case["det_count"]), dict(counts=cu(case["det_runs"]), n_runs=cu(case["det_n_runs"])), cu(case["im_size"]), gt


def f64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda()


def filled(out):
    for v in out.values():
        v.view(torch.uint8).fill_(0xFF)
    return out


def run_iou(case):
    from detectorch_amd import hip, hip_segm
    dets, det_count, rle, im_size, gt = on_device(case)
    N, max_out = dets.shape[:2]
    G = gt["gt_classes"].shape[1]
    out = filled(hip_segm.iou_outputs(N, max_out, G, dets.device))
    ws = hip.workspace(hip_segm.iou_workspace_bytes(N, max_out, rle["counts"].shape[2], G, gt["gt_runs"].shape[2]), dets.device).fill_(0xFF)
    hip_segm.segm_iou(dets, det_count, rle["counts"], rle["n_runs"], im_size, gt["gt_runs"], gt["gt_n_runs"], gt["gt_classes"],
                      gt["gt_is_crowd"], gt["gt_counts"], case["num_classes"], out=out, ws=ws)
    return out


def check_iou(out, want):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in ("det_area", "gt_mask_area", "n_bad"):
        assert np.array_equal(got[k], want[k]), k
    assert same_bits(got["iou"], want["iou"])


def run_match(case, iou, det_area, gt_mask_area, gt_area="case"):
    from detectorch_amd import hip_segm
    dets, det_count = cu(case["dets"]), cu(case["det_count"])
    N, max_out = dets.shape[:2]
    G, T, A = case["gt_classes"].shape[1], len(case["iou_thrs"]), len(case["area_rngs"])
    if gt_area == "case":
        gt_area = cu(case["gt_area"]) if "gt_area" in case else None
    out = filled(hip_segm.match_outputs(N, max_out, G, case["num_classes"], T, A, dets.device))
    hip_segm.segm_match(dets, det_count, iou, det_area, cu(case["gt_classes"]), cu(case["gt_is_crowd"]), cu(case["gt_counts"]), gt_area,
                        gt_mask_area, case["num_classes"], f64(case["iou_thrs"]), f64(case["area_rngs"]), case["max_dets"][-1], out=out)
    return out


def check_records(out, want):
    got = {k: v.cpu().numpy() for k, v in out.items()}
    for k in RECORDS:
        assert np.array_equal(got[k], want[k]), k
    for k in WORDS:
        assert np.array_equal(got[k].view(np.uint64), want[k]), k


def run_accumulate(case, rec):
    from detectorch_amd import hip_eval
    from detectorch_amd.utils.evaluator import summarize_stats
    T, A, R, M, K = len(case["iou_thrs"]), len(case["area_rngs"]), len(case["rec_thrs"]), len(case["max_dets"]), case["num_classes"] - 1
    acc = filled(hip_eval.accumulate_outputs(T, R, K, A, M, rec["dt_rank"].device))
    hip_eval.eval_accumulate(rec["dt_rank"], rec["dt_match"], rec["dt_ignore"], rec["sort_key"], rec["npig"], case["num_classes"], T, A,
                             f64(case["rec_thrs"]), torch.tensor(case["max_dets"], dtype=torch.int32).cuda(), out=acc)
    res = {k: v.cpu().numpy() for k, v in acc.items()}
    res["stats"] = summarize_stats(res["precision"], res["recall"], case["iou_thrs"])
    return res


def check_result(res, want):
    assert np.array_equal(res["counts"], want["counts"])
    for k in ("precision", "recall", "stats"):
        assert res[k].dtype == np.float64 and same_bits(res[k], want[k]), k


def evaluator(case, **kw):
    from detectorch_amd.utils.evaluator import MaskEvaluator
    return MaskEvaluator(num_classes=case["num_classes"], iou_thrs=case["iou_thrs"], rec_thrs=case["rec_thrs"], max_dets=case["max_dets"],
                         area_rngs=case["area_rngs"], **kw)


# ---- dtc_segm_iou, then the match and the accumulation on it -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.IOU_CASES))
def test_iou_match_and_accumulate_equal_the_restatement(name):
    case, want = reference(name, sc.IOU_CASES[name])
    out = run_iou(case)
    check_iou(out, want)
    rec = run_match(case, out["iou"], out["det_area"], out["gt_mask_area"])
    check_records(rec, want)
    check_result(run_accumulate(case, rec), want)


def test_huge_image_sums_in_integers():
    """30000 x 30000: an intersection near 9e8; the answer comes from the interval form of the counts, pinned on the host"""
    case, want = reference("huge", sc.huge, counts=sr.interval_counts)
    out = run_iou(case)
    check_iou(out, want)
    assert out["det_area"][0, 0].item() == 900000000 - 1000 and 0.99998 < out["iou"][0, 0, 0].item() < 1.0


def test_second_call_rewrites_every_output():
    """the same buffers and workspace, another case of the same shapes in between: nothing of it is left"""
    from detectorch_amd import hip, hip_segm
    a, b = (reference(("stream", s), lambda s=s: sc.stream_case(s)) for s in (3, 4))
    outs, ws = None, None
    for case, want in (a, b, a):
        dets, det_count, rle, im_size, gt = on_device(case)
        if outs is None:
            outs = hip_segm.iou_outputs(dets.shape[0], dets.shape[1], gt["gt_classes"].shape[1], dets.device)
            ws = hip.workspace(hip_segm.iou_workspace_bytes(dets.shape[0], dets.shape[1], 160, 5, 150), dets.device)
        hip_segm.segm_iou(dets, det_count, rle["counts"], rle["n_runs"], im_size, gt["gt_runs"], gt["gt_n_runs"], gt["gt_classes"],
                          gt["gt_is_crowd"], gt["gt_counts"], case["num_classes"], out=outs, ws=ws)
        check_iou(outs, want)


# ---- the bridge to the box protocol -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gt_area", [True, False])
@pytest.mark.parametrize("name", sorted(sc.BOX_CASES))
def test_filled_rectangles_equal_the_box_protocol(name, with_gt_area):
    from detectorch_amd import hip_eval
    key = ("bridge", name, with_gt_area)
    if key not in _REF:
        b, s = sc.from_boxes(sc.BOX_CASES[name](), with_gt_area=with_gt_area)
        _REF[key] = (b, s, cr.run(b))
    b, s, want = _REF[key]
    out = run_iou(s)
    rec = run_match(s, out["iou"], out["det_area"], out["gt_mask_area"])
    check_records(rec, want)                                    # the box protocol's restatement
    res = run_accumulate(s, rec)
    check_result(res, want)
    N, max_out = b["dets"].shape[:2]
    G, T, A = b["gt_boxes"].shape[1], len(b["iou_thrs"]), len(b["area_rngs"])
    box = filled(hip_eval.match_outputs(N, max_out, G, b["num_classes"], T, A, rec["dt_rank"].device))
    hip_eval.eval_match(cu(b["dets"]), cu(b["det_count"]), cu(b["gt_boxes"]), cu(b["gt_classes"]), cu(b["gt_is_crowd"]), cu(b["gt_counts"]),
                        cu(b["gt_area"]) if "gt_area" in b else None, b["num_classes"], f64(b["iou_thrs"]), f64(b["area_rngs"]),
                        b["max_dets"][-1], out=box)
    for k in RECORDS + WORDS:                                    # dtc_eval_match on the boxes
        assert torch.equal(rec[k], box[k]), k
    box_res = run_accumulate(b, box)
    for k in ("precision", "recall", "stats", "counts"):
        assert same_bits(res[k], box_res[k]), k


# ---- dtc_segm_match on crafted matrices ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_gt_area", [False, True])
@pytest.mark.parametrize("params", ["coco", "nondefault"])
def test_match_on_crafted_matrices(params, with_gt_area):
    case, iou, det_area, gt_mask_area = sc.crafted(None if params == "coco" else sc.NONDEFAULT_PARAMS, with_gt_area)
    want, _ = sr.match_records(case, iou, det_area, gt_mask_area)
    rec = run_match(case, cu(iou), cu(det_area), cu(gt_mask_area))
    check_records(rec, want)
    if with_gt_area:                                            # gt_mask_area may then be NULL: it is not read
        check_records(run_match(case, cu(iou), cu(det_area), None), want)
        bogus = cu(np.full_like(gt_mask_area, 123456))
        check_records(run_match(case, cu(iou), cu(det_area), bogus), want)


# ---- the evaluator ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunks", [(6,), (1, 3, 2)])
def test_update_in_chunks(chunks):
    case, want = reference(("stream", 3), lambda: sc.stream_case(3))
    dets, det_count, rle, im_size, gt = on_device(case)
    ev, at = evaluator(case), 0
    cut = lambda t: t[at:at + n].contiguous()
    for n in chunks:
        rec = ev.update(cut(dets), cut(det_count), {k: cut(v) for k, v in rle.items()}, cut(im_size), {k: cut(v) for k, v in gt.items()})
        assert same_bits(rec["iou"].cpu().numpy(), want["iou"][at:at + n])
        at += n
    check_result(ev.accumulate(), want)
    stats, ap = ev.summarize()
    assert same_bits(stats, want["stats"]) and ap["per_class"].shape == (3,) and (want["precision"] > 0).any()


def test_update_captured_in_a_graph():
    """update() captured after one eager call and replayed twice on rewritten inputs equals the restatement of those inputs"""
    cases = [reference(("stream", s), lambda s=s: sc.stream_case(s)) for s in (3, 4, 5)]
    dets, det_count, rle, im_size, gt = on_device(cases[0][0])
    ev = evaluator(cases[0][0])
    ev.update(dets, det_count, rle, im_size, gt)                # eager: loads the library, warms the allocator
    torch.cuda.synchronize()
    ev.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ev.update(dets, det_count, rle, im_size, gt)
    for case, want in cases[1:]:
        d2, c2, r2, s2, g2 = on_device(case)
        dets.copy_(d2), det_count.copy_(c2), im_size.copy_(s2)
        for k in rle:
            rle[k].copy_(r2[k])
        for k in gt:
            gt[k].copy_(g2[k])
        graph.replay()
        got = ev.accumulate()
        check_result(got, want)
        assert same_bits(ev._records[0]["iou"].cpu().numpy(), want["iou"]) and (got["precision"] > 0).any()


def test_evaluate_masks_from_result_lists():
    """the lists assemble_results leaves (compressed strings), a roidb and the gt masks in every accepted form"""
    from detectorch_amd.utils.evaluator import evaluate_masks
    from detectorch_amd.utils.result_utils import _rle_counts_to_string, assemble_results
    case, want = reference(("stream", 3), lambda: sc.stream_case(3))
    N, max_out = case["dets"].shape[:2]
    strings = [[_rle_counts_to_string(case["det_runs"][n, d, :max(case["det_n_runs"][n, d], 0)].tolist()) if d < case["det_count"][n] else ""
                for d in range(max_out)] for n in range(N)]
    rle_str = np.zeros((N, max_out, max(len(s) for r in strings for s in r)), np.uint8)
    rle_len = np.zeros((N, max_out), np.int32)
    for n in range(N):
        for d, s in enumerate(strings[n]):
            rle_str[n, d, :len(s)], rle_len[n, d] = np.frombuffer(s.encode("ascii"), np.uint8), len(s)
    all_boxes, all_segms = assemble_results(case["dets"], case["det_count"], case["im_size"], rle_str, rle_len, num_classes=case["num_classes"])
    roidb, gt_masks = [], []
    for n in range(N):
        g = int(case["gt_counts"][n])
        roidb.append(dict(boxes=np.zeros((g, 4), np.float32), gt_classes=case["gt_classes"][n, :g], is_crowd=case["gt_is_crowd"][n, :g], seg_areas=case["gt_area"][n, :g],
                          height=24, width=17))
        masks = []
        for j in range(g):
            runs = case["gt_runs"][n, j, :case["gt_n_runs"][n, j]].tolist()
            bitmap = sr.decode(case["gt_runs"][n, j], case["gt_n_runs"][n, j], 24 * 17).reshape(17, 24).T
            masks.append([bitmap, dict(size=[24, 17], counts=runs), dict(size=[24, 17], counts=_rle_counts_to_string(runs))][j % 3])
        gt_masks.append(masks)
    ev = evaluate_masks(all_boxes, all_segms, roidb, gt_masks, batch=4, iou_thrs=case["iou_thrs"], rec_thrs=case["rec_thrs"],
                        max_dets=case["max_dets"], area_rngs=case["area_rngs"])
    check_result(ev.accumulate(), want)


def test_end_to_end_from_the_mask_kernels():
    """hip.mask_paste -> hip.mask_rle on a 2-image synthetic batch, fed into MaskEvaluator as they are; the gt are some of the
    detections' own masks and blobs; checked against the restatement on the runs read back"""
    from detectorch_amd import hip, synth
    from detectorch_amd.utils.evaluator import pack_gt_masks
    rs = synth.rng(11, 2)
    B, D, M, im = 2, 8, 14, [(61, 83), (70, 52)]
    counts = np.array([8, 6], np.int32)
    dets = np.zeros((B, D, 6), np.float32)
    for b, (h, w) in enumerate(im):
        dets[b, :, :4] = synth.make_rois(rs, D, im_h=h, im_w=w, min_side=6, max_side=60)
        dets[b, :, 4], dets[b, :, 5] = rs.rand(D), np.sort(rs.randint(1, 4, D))
    masks = synth.make_masks(rs, B * D, 4, M)
    im_size = cu(np.array(im, np.float32))
    paste = hip.mask_paste(cu(masks), cu(dets), cu(counts), im_size, M, 61 * 83 * D)
    rle = hip.mask_rle(paste, cu(counts), im_size, runs_stride=512, str_stride=1024)
    runs, n_runs = rle["counts"].cpu().numpy().view(np.uint32), rle["n_runs"].cpu().numpy()
    assert (n_runs[0] > 2).all() and (n_runs[1, :6] > 2).all() and (n_runs[1, 6:] == 0).all()
    gt_masks, classes, crowd = [], np.zeros((B, 4), np.int32), np.zeros((B, 4), np.int32)
    for b, (h, w) in enumerate(im):
        ms = []
        for j, d in enumerate((0, 3, 5)):                       # a detection's own mask, a little eroded; then a plain blob
            m = sr.decode(runs[b, d], n_runs[b, d], h * w).reshape(w, h).T & (rs.rand(h, w) < 0.9)
            ms.append(m if j else dict(size=[h, w], counts=sc.runs_of(m)))
            classes[b, j], crowd[b, j] = dets[b, d, 5], int(j == 2)
        yy, xx = np.mgrid[0:h, 0:w]
        ms.append(((yy - h / 2) ** 2 + (xx - w / 2) ** 2) < 200)
        classes[b, 3] = 2
        gt_masks.append(ms)
    gt = dict(gt_classes=cu(classes), gt_is_crowd=cu(crowd), gt_counts=cu(np.array([4, 4], np.int32)), **pack_gt_masks(gt_masks, im, "cuda"))
    case = dict(dets=dets, det_count=counts, det_runs=runs, det_n_runs=n_runs, im_size=np.array(im, np.float32),
                gt_runs=gt["gt_runs"].cpu().numpy().view(np.uint32), gt_n_runs=gt["gt_n_runs"].cpu().numpy(), gt_classes=classes,
                gt_is_crowd=crowd, gt_counts=np.array([4, 4], np.int32), num_classes=4)
    case.update(zip(("iou_thrs", "rec_thrs", "max_dets", "area_rngs"), sc.STREAM_PARAMS))
    want = sr.run(case)
    ev = evaluator(case)
    rec = ev.update(cu(dets), cu(counts), rle, im_size, gt)
    check_iou({k: rec[k] for k in ("iou", "det_area", "gt_mask_area", "n_bad")}, want)
    check_records({k: rec[k] for k in RECORDS + WORDS}, want)
    check_result(ev.accumulate(), want)
    assert (want["iou"] > 0.5).sum() >= 6 and (want["precision"] > 0).any() and want["det_area"][0].min() > 0


def test_masks_that_did_not_fit_are_reported():
    case, want = reference("counts", sc.IOU_CASES["counts"])
    ev = evaluator(case, on_overflow="truncate")
    ev.update(*on_device(case))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        check_result(ev.accumulate(), want)
    assert any("2 masks did not fit" in str(x.message) for x in w) and any("9 detections but only 6 rows" in str(x.message) for x in w)
    keep = np.array([0, 1, 2, 4])                                # without the image whose det_count is above max_out
    sub = {k: (v[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (5,) else v) for k, v in case.items()}
    ev = evaluator(sub)
    ev.update(*on_device(sub))
    with pytest.raises(RuntimeError, match="image 0: 2 masks did not fit"):
        ev.accumulate()
    with pytest.raises(RuntimeError, match="image 0: 2 masks did not fit"):      # no stale result is handed out afterwards
        ev.summarize()


def test_wrong_dtypes_and_sizes_are_refused():
    from detectorch_amd import hip_segm
    case, _ = reference(("stream", 3), lambda: sc.stream_case(3))
    dets, det_count, rle, im_size, gt = on_device(case)
    ev = evaluator(case)
    with pytest.raises(TypeError, match="dets"):
        ev.update(dets.double(), det_count, rle, im_size, gt)
    with pytest.raises(TypeError, match="det_runs"):
        ev.update(dets, det_count, dict(rle, counts=rle["counts"].long()), im_size, gt)
    with pytest.raises(TypeError, match="det_n_runs"):
        ev.update(dets, det_count, dict(rle, n_runs=rle["n_runs"][:, :5]), im_size, gt)
    with pytest.raises(TypeError, match="gt_n_runs"):
        ev.update(dets, det_count, rle, im_size, dict(gt, gt_n_runs=gt["gt_n_runs"].long()))
    with pytest.raises(TypeError, match="im_size"):
        ev.update(dets, det_count, rle, im_size[:, :1], gt)
    z = lambda *s, dt=torch.int32: torch.zeros(s, dtype=dt, device="cuda")
    big = dict(gt_runs=z(6, 257, 4), gt_n_runs=z(6, 257), gt_classes=z(6, 257), gt_is_crowd=z(6, 257), gt_counts=z(6))
    with pytest.raises(ValueError, match="at most 256 gt"):
        ev.update(dets, det_count, rle, im_size, big)
    with pytest.raises(ValueError, match="at most 512"):
        ev.update(z(6, 513, 6, dt=torch.float32), det_count, dict(counts=z(6, 513, 4), n_runs=z(6, 513)), im_size, gt)
    with pytest.raises(TypeError, match="iou"):
        hip_segm.segm_match(dets, det_count, z(6, 10, 5, dt=torch.float32), z(6, 10), gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"],
                            None, z(6, 5), 4, ev._iou_thrs, ev._area_rngs, 100)
    with pytest.raises(TypeError, match="gt_area or gt_mask_area"):
        hip_segm.segm_match(dets, det_count, z(6, 10, 5, dt=torch.float64), z(6, 10), gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"],
                            None, None, 4, ev._iou_thrs, ev._area_rngs, 100)
    ev.update(dets, det_count, rle, im_size, gt)
    with pytest.raises(ValueError, match="max_out changed"):
        ev.update(z(6, 12, 6, dt=torch.float32), det_count, dict(counts=z(6, 12, 160), n_runs=z(6, 12)), im_size, gt)
