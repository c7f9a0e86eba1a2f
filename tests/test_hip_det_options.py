"""The reference's Soft-NMS and bbox-voting options (result_utils.py:96-168, do_soft_nms / do_bbox_vote) on the batched device path
(dtc_postprocess_detections_ex) through every layer: C ABI, hip.py, result_utils, FpnRegionPath / C4RegionPath, forward_batched.
Everything bit-equal, row order included, to the oracle composition of tests/det_options_ref.py (pinned against the reference's own
outputs by tests/test_det_options_host.py) and to the reference goldens.  -m gpu.

Covered: (1) every method with and without voting, probabilities and logits, B = 4 x R = 1000 with short images; (2) the goldens of
tests/golden/postprocess_soft_vote.npz through result_utils; (3) the decoded-boxes entry == the single-segment kernels' per-class loop
== the oracle; (4) a 4096-candidate class, ties past max_det, det_count > max_out, empty / one-candidate segments and an image without
rois, n_cls 2 and 257; (5) FpnRegionPath eager == graph replay, its mask-branch mapping == dtc_fpn_collect_distribute on the voted
boxes, crops and RLE == the oracle's mask chain on them, OverlappedRegionPath and C4RegionPath with options; (6) forward_batched with
the options == box_results_with_nms_and_limit on its own scores and boxes, options in the path cache key; (7) the default options ==
the existing entries bit for bit at the bench's shape (a guard)."""
import numpy as np
import pytest
import torch

from conftest import golden
from det_options_ref import CONFIGS, compose, decode, kwargs_of
from detectorch_amd import synth

pytestmark = pytest.mark.gpu

METHODS = ["nms", "linear", "gaussian", "hard"]


@pytest.fixture(scope="module")
def hip():
    from detectorch_amd import hip as h
    h.lib()
    return h


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def check_image(out, b, ref_dets, ref_roi, max_out, sf=None):
    """image b of (dets, det_roi, det_rois_scaled or None, det_count) == the oracle's rows"""
    dets, det_roi, det_scaled, det_count = out
    D = ref_dets.shape[0]
    assert int(det_count[b]) == D, (b, int(det_count[b]), D)
    n = min(D, max_out)
    got = dets[b, :n].cpu().numpy()
    assert np.array_equal(got, ref_dets[:n]), (b, np.argwhere(got != ref_dets[:n])[:5])
    assert np.array_equal(det_roi[b, :n].cpu().numpy(), ref_roi[:n])
    assert not dets[b, n:].any()                                             # rows past max_out: reported, never written
    if det_scaled is not None:
        assert np.array_equal(det_scaled[b, :n].cpu().numpy(), (ref_dets[:n, :4] * np.float32(sf)).astype(np.float32))


def head_batch(seed, B=4, R=1000, ncls=81):
    rs = synth.rng(31, seed)
    rois = np.stack([np.hstack([np.full((R, 1), b, np.float32), synth.make_rois(rs, R)]) for b in range(B)])
    cls, deltas = zip(*[synth.make_head_outputs(rs, R, n_cls=ncls) for _ in range(B)])
    sf = np.array([1.6, 1.25, 2.0, 1.0][:B], np.float32)
    im = np.array([[500.0, 833.0], [640.0, 480.0], [400.0, 600.0], [800.0, 1200.0]][:B], np.float32)
    n_rois = np.array([R, R - 37, 500, R][:B], np.int32)
    return rois, np.stack(cls), np.stack(deltas), sf, im, n_rois


# ---- 1. mode matrix ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("vote", [None, 0.8])
@pytest.mark.parametrize("method", METHODS)
def test_mode_matrix_vs_oracle(hip, oracle, method, vote, logits):
    B, R = 4, 1000
    rois, cls, deltas, sf, im, n_rois = head_batch(1)
    if logits:
        cls = np.log(np.maximum(cls, 1e-30)).astype(np.float32)
    out = hip.postprocess_detections(cu(rois), cu(n_rois), cu(cls), cu(deltas), cu(sf), cu(im), scores_are_logits=logits,
                                     **kwargs_of(method, vote))
    torch.cuda.synchronize()
    for b in range(B):
        n = int(n_rois[b])
        scores = oracle.softmax_rows(cls[b, :n]) if logits else cls[b, :n]
        boxes = decode(oracle, rois[b, :n, 1:], sf[b], im[b], deltas[b, :n])
        ref, ref_roi = compose(oracle, scores, boxes, method, vote)
        assert ref.shape[0] > 0
        check_image(out, b, ref, ref_roi, 128, sf[b])


# ---- 2. reference goldens ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["pp", "crowd"])
@pytest.mark.parametrize("name", sorted(CONFIGS))
def test_reference_goldens(hip, case, name):
    from detectorch_amd.utils import result_utils
    g = golden("postprocess_soft_vote")
    if case == "pp":
        p = golden("postprocess")
        scores, boxes, ncls = p["cls"], p["pred_clipped"], 81
    else:
        scores, boxes, ncls = g["crowd_scores"], g["crowd_boxes"], 3
    sc, bx, cb = result_utils.box_results_with_nms_and_limit(scores, boxes.copy(), num_classes=ncls, **kwargs_of(*CONFIGS[name]))
    key = "%s_%s_" % (case, name)
    assert np.array_equal(sc, g[key + "scores"]) and np.array_equal(bx, g[key + "boxes"])
    assert np.array_equal(np.concatenate([np.full(len(cb[j]), j, np.int32) for j in range(1, ncls)]), g[key + "cls_id"])


# ---- 3. decoded-boxes entry == the single-segment kernels' per-class loop == the oracle ------------------------------------------
@pytest.mark.parametrize("method", ["linear", "gaussian", "hard"])
def test_decoded_boxes_entry_equals_single_segment_loop(hip, oracle, method):
    from detectorch_amd.utils import boxes as box_utils
    from detectorch_amd.utils import result_utils
    p, g = golden("postprocess"), golden("postprocess_soft_vote")
    for scores, boxes, ncls in ((p["cls"], p["pred_clipped"], 81), (g["crowd_scores"], g["crowd_boxes"], 3)):
        sc, bx, cb = result_utils.box_results_with_nms_and_limit(scores, boxes.copy(), num_classes=ncls, do_soft_nms=True,
                                                                 soft_nms_method=method, do_bbox_vote=True, bbox_vote_thresh=0.8)
        loop, _ = compose(box_utils, scores, boxes, method, 0.8)          # dtc_soft_nms + dtc_box_voting per class
        ref, _ = compose(oracle, scores, boxes, method, 0.8)
        assert np.array_equal(loop, ref)
        assert np.array_equal(sc, ref[:, 4]) and np.array_equal(bx, ref[:, :4])
        assert np.array_equal(np.concatenate([np.full(len(cb[j]), j) for j in range(1, ncls)]), ref[:, 5].astype(np.int64))


# ---- 4. stress ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_crowded_class_r4096(hip, oracle, method):
    """one class, 4096 heavily overlapping candidates: the longest walk the entry allows, many swap-with-last discards"""
    rs = synth.rng(32, 0)
    R = 4096
    c = np.array([400.0, 300.0]) + rs.uniform(-30, 30, (R, 2))
    half = rs.uniform(40, 80, (R, 2))
    b1 = np.clip(np.hstack([c - half, c + half]), 0, 799).astype(np.float32)
    boxes = np.hstack([np.zeros((R, 4), np.float32), b1])
    scores = np.zeros((R, 2), np.float32)
    scores[:, 1] = (rs.permutation(R) / R * 0.9 + 0.06).astype(np.float32)
    out = hip.box_results_nms_limit(cu(scores[None]), cu(boxes[None]), do_soft_nms=True, soft_nms_method=method, do_bbox_vote=True,
                                    bbox_vote_thresh=0.8)
    torch.cuda.synchronize()
    ref, ref_roi = compose(oracle, scores, boxes, method, 0.8)
    check_image((out[0], out[1], None, out[2]), 0, ref, ref_roi, 128)


def test_ties_at_the_limit_and_rows_past_max_out(hip, oracle):
    g = golden("postprocess_soft_vote")
    scores, boxes = g["crowd_scores"], g["crowd_boxes"]
    for method, vote in (("linear", None), ("hard", 0.8), ("nms", 0.6)):
        ref, ref_roi = compose(oracle, scores, boxes, method, vote)
        assert ref.shape[0] > 100                                            # ties: det_count > max_det
        for max_out in (128, 64):
            out = hip.box_results_nms_limit(cu(scores[None]), cu(boxes[None]), max_out=max_out, **kwargs_of(method, vote))
            torch.cuda.synchronize()
            check_image((out[0], out[1], None, out[2]), 0, ref, ref_roi, max_out)


def test_empty_and_single_candidate_segments(hip, oracle):
    """image 0: class 1 without candidates, class 2 with one, classes 3-4 with several; image 1: no score above the threshold;
    image 2: no rois at all"""
    rs = synth.rng(33, 0)
    B, R, ncls = 3, 300, 5
    scores = rs.uniform(0, 0.04, (B, R, ncls)).astype(np.float32)
    scores[0, 17, 2] = 0.5
    scores[0, :, 3:] = rs.uniform(0, 1, (R, 2)) ** 4
    boxes = np.stack([np.hstack([synth.make_rois(rs, R) for _ in range(ncls)]) for _ in range(B)]).astype(np.float32)
    n_rois = np.array([R, R, 0], np.int32)
    for method, vote in (("linear", 0.8), ("gaussian", None), ("nms", 0.8), ("hard", None)):
        out = hip.box_results_nms_limit(cu(scores), cu(boxes), cu(n_rois), **kwargs_of(method, vote))
        torch.cuda.synchronize()
        for b in range(B):
            n = int(n_rois[b])
            ref, ref_roi = compose(oracle, scores[b, :n], boxes[b, :n], method, vote)
            check_image((out[0], out[1], None, out[2]), b, ref, ref_roi, 128)
        assert int(out[2][1]) == 0 and int(out[2][2]) == 0


@pytest.mark.parametrize("method", ["linear", "gaussian", "hard"])
def test_soft_nms_tied_scores_within_a_class(hip, oracle, method):
    """class scores quantised to 1/64 above the score threshold: every class has candidates with exactly equal scores, so the
    first-maximum rule of the shared walk (soft_nms_walk.h, cython_nms.pyx:128-132) decides picks in det_soft_nms_kernel too"""
    rs = synth.rng(35, 0)
    B, R, ncls = 2, 400, 4
    scores = (rs.uniform(0, 1, (B, R, ncls)) ** 3).astype(np.float32)
    scores = np.where(scores > np.float32(0.05), np.ceil(scores * 64) / 64, scores).astype(np.float32)
    boxes = np.stack([np.hstack([synth.make_rois(rs, R, min_side=60, max_side=400) for _ in range(ncls)]) for _ in range(B)])
    boxes = boxes.astype(np.float32)
    for b in range(B):
        for j in range(1, ncls):
            cand = scores[b, :, j][scores[b, :, j] > np.float32(0.05)]
            assert cand.size > 100 and np.unique(cand).size <= 64          # at most 64 distinct values: ties in every class
    out = hip.box_results_nms_limit(cu(scores), cu(boxes), max_det=100, max_out=512, **kwargs_of(method, None))
    torch.cuda.synchronize()
    for b in range(B):
        ref, ref_roi = compose(oracle, scores[b], boxes[b], method, None)
        assert ref.shape[0] >= 100
        check_image((out[0], out[1], None, out[2]), b, ref, ref_roi, 512)


@pytest.mark.parametrize("ncls", [2, 257])
def test_class_count_limits(hip, oracle, ncls):
    rs = synth.rng(34, ncls)
    B, R = 2, 600
    scores = (rs.uniform(0, 1, (B, R, ncls)) ** (8 if ncls == 2 else 30)).astype(np.float32)
    boxes = np.stack([np.hstack([synth.make_rois(rs, R) for _ in range(ncls)]) for _ in range(B)]).astype(np.float32)
    for method, vote in (("linear", 0.8), ("nms", 0.8), ("gaussian", None)):
        out = hip.box_results_nms_limit(cu(scores), cu(boxes), max_det=100, max_out=256, **kwargs_of(method, vote))
        torch.cuda.synchronize()
        for b in range(B):
            ref, ref_roi = compose(oracle, scores[b], boxes[b], method, vote)
            assert ref.shape[0] > 0
            check_image((out[0], out[1], None, out[2]), b, ref, ref_roi, 256)


# ---- 5. region paths ----------------------------------------------------------------------------------------------------------
SOFT_VOTE = dict(do_soft_nms=True, soft_nms_method="linear", do_bbox_vote=True, bbox_vote_thresh=0.8)


def _frame(crop, rect, im_h, im_w):
    x0, y0, x1, y1 = rect
    fr = np.zeros((im_h, im_w), np.uint8)
    fr[y0:y1, x0:x1] = crop
    return fr


def test_fpn_region_path_soft_vote(hip, oracle):
    from detectorch_amd.pipeline import FpnRegionPath, synthetic_batch
    dev = torch.device("cuda", 0)
    B, C = 2, 8
    path = FpnRegionPath(B, dev, channels=C, det_options=SOFT_VOTE, with_rle=True)
    inputs = synthetic_batch(B, dev, seed=3100, channels=C)
    path.bind(*inputs)
    names = ("dets", "det_roi", "det_scaled", "det_count", "m_rois5", "m_levels", "m_n", "m_by_level", "m_level_counts", "m_restore",
             "m_order", "m_desc", "mask_boxes", "mask_rects", "mask_offsets", "mask_bytes", "crops", "rle_str", "rle_str_len")
    path.step(use_graph=False)
    torch.cuda.synchronize()
    eager = {k: getattr(path, k).clone() for k in names}
    path.step(use_graph=True)
    path.step(use_graph=True)
    torch.cuda.synchronize()
    for k in names:
        if k in ("m_by_level",):
            continue
        assert torch.equal(getattr(path, k), eager[k]), k
    D = path.max_out
    # the mask branch's mapping of the VOTED boxes == a separate dtc_fpn_collect_distribute on det_rois_scaled
    sep = hip.fpn_collect_distribute(path.det_scaled.view(B, 1, D, 4), None, path.det_count.view(B, 1), D)
    torch.cuda.synchronize()
    for b in range(B):
        m = min(int(path.det_count[b]), D)
        assert int(path.m_n[b]) == int(sep["n_out"][b]) == m
        for mine, k in (("m_rois5", "rois5"), ("m_levels", "roi_levels"), ("m_restore", "idx_restore"), ("m_order", "roi_order"),
                        ("m_desc", "roi_desc"), ("m_level_counts", "level_counts")):
            assert torch.equal(getattr(path, mine)[b], sep[k][b]), (mine, b)
        assert torch.equal(path.m_by_level[b, :m], sep["rois_by_level"][b, :m])
    # detections == the oracle composition on the path's own inputs; crops / RLE == the oracle's mask chain on the voted boxes
    rois5, n_rois = path.rois5.cpu().numpy(), path.n_rois.cpu().numpy()
    cls, bbox = path.cls_score.cpu().numpy(), path.bbox_pred.cpu().numpy()
    sf, im_size, masks = path.sf.cpu().numpy(), path.im_size.cpu().numpy(), inputs[5].cpu().numpy()
    voted = 0
    for b in range(B):
        n = int(n_rois[b])
        boxes = decode(oracle, rois5[b, :n, 1:], sf[b], im_size[b], bbox[b, :n])
        ref, ref_roi = compose(oracle, cls[b, :n], boxes, "linear", 0.8)
        assert ref.shape[0] > 0
        check_image((path.dets, path.det_roi, path.det_scaled, path.det_count), b, ref, ref_roi, D, sf[b])
        voted += int((ref[:, :4] != compose(oracle, cls[b, :n], boxes, "linear", None)[0][:, :4]).any(1).sum())
        im_h, im_w = int(im_size[b, 0]), int(im_size[b, 1])
        crops = path.crops[b, :int(path.mask_bytes[b])].cpu().numpy()
        rects, offs, mb = path.mask_rects[b].cpu().numpy(), path.mask_offsets[b].cpu().numpy(), path.mask_boxes[b].cpu().numpy()
        for d in range(min(ref.shape[0], D)):
            bx, crop = oracle.mask_resize_binarize(masks[b * D + d, int(ref[d, 5])], ref[d, :4])
            assert np.array_equal(mb[d], bx)
            x0, x1 = max(bx[0], 0), min(bx[2] + 1, im_w)
            y0, y1 = max(bx[1], 0), min(bx[3] + 1, im_h)
            x1, y1 = max(x1, x0), max(y1, y0)
            assert tuple(rects[d]) == (x0, y0, x1, y1)
            exp = crop[y0 - bx[1]:y1 - bx[1], x0 - bx[0]:x1 - bx[0]]
            got = crops[offs[d]:offs[d] + (x1 - x0) * (y1 - y0)].reshape(y1 - y0, x1 - x0)
            assert np.array_equal(got, exp), (b, d)
            _, s = oracle.rle_encode(_frame(exp, (x0, y0, x1, y1), im_h, im_w))
            assert path.rle_str[b, d, :int(path.rle_str_len[b, d])].cpu().numpy().tobytes().decode("ascii") == s, (b, d)
    assert voted > 0                                                         # the vote really moved boxes


def test_overlapped_region_path_forwards_det_options(hip):
    from detectorch_amd.pipeline import FpnRegionPath, OverlappedRegionPath, synthetic_batch
    dev = torch.device("cuda", 0)
    B, C = 2, 8
    ov = OverlappedRegionPath(B, dev, n_split=2, channels=C, det_options=SOFT_VOTE)
    assert all(p.det_opt is not None and p.det_opt.nms_method == 1 and p.det_opt.bbox_vote == 1 for p in ov.sub)
    one = FpnRegionPath(B, dev, channels=C, det_options=SOFT_VOTE)
    inputs = synthetic_batch(B, dev, seed=3200, channels=C)
    one.bind(*inputs)
    one.step(use_graph=False)
    ov.bind(*inputs)
    ov.step(use_graph=True)
    torch.cuda.synchronize()
    for k, p in enumerate(ov.sub):
        n = min(int(one.det_count[k]), one.max_out)
        assert int(p.det_count[0]) == int(one.det_count[k])
        assert torch.equal(p.dets[0, :n], one.dets[k, :n])


def test_c4_region_path_soft_vote(hip, oracle):
    import chain
    from detectorch_amd.pipeline import C4RegionPath, synthetic_c4_batch
    dev = torch.device("cuda", 0)
    B, C = 2, 32
    path = C4RegionPath(B, dev, channels=C, det_options=dict(do_soft_nms=True, soft_nms_method="gaussian", do_bbox_vote=True,
                                                            bbox_vote_thresh=0.7))
    inputs = synthetic_c4_batch(B, dev, seed=2100, channels=C)
    path.bind(*inputs)
    path.step(use_graph=False)
    torch.cuda.synchronize()
    eager = (path.dets.clone(), path.det_roi.clone(), path.det_scaled.clone(), path.det_count.clone())
    path.step(use_graph=True)
    path.step(use_graph=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(eager, (path.dets, path.det_roi, path.det_scaled, path.det_count)))
    rpn_cls, rpn_bbox, feat, cls_score, bbox_pred, sf, im_size = [x.cpu().numpy() for x in inputs]
    for b in range(B):
        ref = chain.c4_hot_path(rpn_cls[b], rpn_bbox[b], feat[b:b + 1], cls_score[b], bbox_pred[b], sf[b], im_size[b],
                                path.im_h, path.im_w, pooled=7)
        n = ref["rois"].shape[0]
        assert np.array_equal(path.rois5[b, :n, 1:].cpu().numpy(), ref["rois"])
        boxes = decode(oracle, ref["rois"], sf[b], im_size[b], bbox_pred[b, :n])
        dets, roi = compose(oracle, cls_score[b, :n], boxes, "gaussian", 0.7)
        check_image((path.dets, path.det_roi, path.det_scaled, path.det_count), b, dets, roi, path.max_out, sf[b])


# ---- 6. forward_batched -------------------------------------------------------------------------------------------------------
def test_forward_batched_soft_nms_and_vote(hip, oracle):
    from test_hip_detector import _boost, _fpn_model
    from detectorch_amd.utils import result_utils
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        model = _boost(_fpn_model())
        rs = synth.rng(35, 0)
        ims = [cu(rs.randint(0, 256, (h, w, 3)).astype(np.uint8)) for h, w in ((200, 280), (180, 300))]
        blob, scales, sizes = hip.prep_images(ims, target_size=320, max_size=448)
        sf = torch.tensor(scales, dtype=torch.float32, device="cuda")
        im_size = torch.tensor([[200.0, 280.0], [180.0, 300.0]], device="cuda")
        blob_hw = [((h + 31) // 32 * 32, (w + 31) // 32 * 32) for h, w in sizes]
        path = model.forward_batched(blob, sf, im_size, blob_hw=blob_hw, do_soft_nms=True, do_bbox_vote=True)
        torch.cuda.synchronize()
        assert path.det_opt is not None and len(model._paths) == 1
        n_rois = path.n_rois.cpu().numpy()
        logits, bbox, rois5 = path.cls_logits_out.cpu().numpy(), path.bbox_pred_out.cpu().numpy(), path.rois5.cpu().numpy()
        total = 0
        for b in range(2):
            n = int(n_rois[b])
            scores = oracle.softmax_rows(logits[b, :n])
            boxes = decode(oracle, rois5[b, :n, 1:], scales[b], im_size[b].cpu().numpy(), bbox[b, :n])
            sc, bx, cb = result_utils.box_results_with_nms_and_limit(scores, boxes, do_soft_nms=True, do_bbox_vote=True)
            D = int(path.det_count[b])
            assert D == len(sc)
            D = min(D, path.max_out)
            dets = path.dets[b, :D].cpu().numpy()
            assert np.array_equal(dets[:, 4], sc[:D]) and np.array_equal(dets[:, :4], bx[:D])
            assert np.array_equal(dets[:, 5].astype(np.int64), np.concatenate([np.full(len(cb[j]), j) for j in range(1, 81)])[:D])
            total += D
        assert total > 0
        plain = model.forward_batched(blob, sf, im_size, blob_hw=blob_hw)            # the options are part of the path cache key
        assert plain is not path and plain.det_opt is None and len(model._paths) == 2
    finally:
        torch.backends.cudnn.deterministic = old


# ---- 7. guard: the default is the existing entries, bit for bit -------------------------------------------------------------------
@pytest.mark.parametrize("logits", [False, True])
def test_default_options_equal_existing_entries(hip, logits):
    from detectorch_amd.pipeline import synthetic_batch
    dev = torch.device("cuda", 0)
    B, D = 8, 128
    _, _, _, cls, bbox, _, sf, im = synthetic_batch(B, dev, seed=3300, channels=8)
    R, ncls = cls.shape[1], cls.shape[2]
    rs = synth.rng(36, 0)
    rois = cu(np.stack([np.hstack([np.full((R, 1), b, np.float32), synth.make_rois(rs, R)]) for b in range(B)]))
    n_rois = torch.tensor([R] * 7 + [R - 100], dtype=torch.int32, device=dev)
    if logits:
        cls = torch.log(cls.clamp_min(1e-30))
    L = hip.lib()
    ws = hip.workspace(L.dtc_postprocess_detections_workspace_bytes(B, R, ncls), dev)
    st = hip.stream_ptr(dev)

    def bufs():
        f32, i32 = torch.float32, torch.int32
        e = lambda *s, dtype=f32: torch.full(s, -3, dtype=dtype, device=dev)
        out = [e(B, D, 6), e(B, D, dtype=i32), e(B, D, 4), e(B, dtype=i32)]
        o = dict(rois5=e(B, D, 5), roi_levels=e(B, D, dtype=i32), n_out=e(B, dtype=i32), rois_by_level=e(B, D, 4),
                 level_counts=e(B, 4, dtype=i32), idx_restore=e(B, D, dtype=i32), roi_order=e(B, D, dtype=i32), roi_desc=e(B, D, 8))
        fm = hip.FpnMapOut(*[o[k].data_ptr() for k in ("rois5", "roi_levels", "n_out", "rois_by_level", "level_counts", "idx_restore",
                                                       "roi_order", "roi_desc")], 2, 5)
        return out, o, fm

    args = lambda out: (ws.data_ptr(), ws.numel(), out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), D)
    head = (rois.data_ptr(), n_rois.data_ptr(), cls.data_ptr())
    rest = (bbox.data_ptr(), sf.data_ptr(), im.data_ptr(), B, R, ncls, 10., 10., 5., 5., .05, .5, 100)
    ref, ref_o, ref_fm = bufs()
    hip.check(L.dtc_postprocess_detections_fpn(*head, 1 if logits else 0, *rest, *args(ref), ref_fm, st), "fpn")
    ref2, _, _ = bufs()
    old = L.dtc_postprocess_detections_logits if logits else L.dtc_postprocess_detections
    hip.check(old(*head, *rest, *args(ref2), st), "plain")
    for opt in (None, hip.DetOptions(0, 0.5, 0.0001, 0, 0.8)):
        for fused in (True, False):
            got, got_o, fm = bufs()
            hip.check(L.dtc_postprocess_detections_ex(*head, 1 if logits else 0, bbox.data_ptr(), None, *rest[1:], opt, *args(got),
                                                      fm if fused else None, st), "ex")
            torch.cuda.synchronize()
            for a, b_ in zip(got, ref if fused else ref2):
                assert torch.equal(a, b_)
            if fused:
                for k in ref_o:
                    assert torch.equal(got_o[k], ref_o[k]), k
