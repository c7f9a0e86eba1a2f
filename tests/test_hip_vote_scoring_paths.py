"""The bbox-vote scorings through every layer above the C ABI (-m gpu): the batched entry with decode from rois + deltas and with
logits, C4RegionPath / OverlappedRegionPath, forward_batched and its path cache, and dtc_postprocess_detections_ex2 with no scoring or
'ID' == dtc_postprocess_detections_ex bit for bit including det_rois_scaled and the fused FPN mask mapping.  Rows, order, boxes and
det_roi exact against the checker (vote_scoring_ref); scores exact or within 1e-6 relative (vote_scoring_ref.exact)."""
import numpy as np
import pytest
import torch

from det_options_ref import decode
from detectorch_amd import synth
from test_hip_det_options import cu, head_batch
import vote_scoring_ref as vsr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from detectorch_amd import hip as h
    h.lib()
    return h


def check_scored(out, b, ref, ref_roi, method, sf=None, max_out=128):
    dets, det_roi, det_scaled, det_count = out
    assert int(det_count[b]) == len(ref), (b, int(det_count[b]), len(ref))
    n = min(len(ref), max_out)
    got = dets[b, :n].cpu().numpy()
    assert np.array_equal(det_roi[b, :n].cpu().numpy(), ref_roi[:n])
    assert np.array_equal(got[:, :4], ref[:n, :4]) and np.array_equal(got[:, 5], ref[:n, 5])
    if vsr.exact(method):
        assert np.array_equal(got[:, 4], ref[:n, 4])
    else:
        np.testing.assert_allclose(got[:, 4], ref[:n, 4], rtol=1e-6, atol=0)
    if det_scaled is not None and sf is not None:
        assert np.array_equal(det_scaled[b, :n].cpu().numpy(), (got[:, :4] * np.float32(sf)).astype(np.float32))


@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("nm", ["nms", "linear", "gaussian", "hard"])
def test_decode_entry_every_scoring_vs_checker(hip, oracle, nm, logits):
    B = 4
    rois, cls, deltas, sf, im, n_rois = head_batch(1)
    if logits:
        cls = np.log(np.maximum(cls, 1e-30)).astype(np.float32)
    for m in vsr.METHODS:
        out = hip.postprocess_detections(cu(rois), cu(n_rois), cu(cls), cu(deltas), cu(sf), cu(im), scores_are_logits=logits,
                                         **vsr.kwargs_of(nm, 0.6, m))
        torch.cuda.synchronize()
        for b in range(B):
            n = int(n_rois[b])
            scores = oracle.softmax_rows(cls[b, :n]) if logits else cls[b, :n]
            boxes = decode(oracle, rois[b, :n, 1:], sf[b], im[b], deltas[b, :n])
            ref, ref_roi = vsr.compose(oracle, scores, boxes, nm, 0.6, m)
            assert len(ref) > 0
            check_scored(out, b, ref, ref_roi, m, sf[b])


def test_ex2_null_and_id_equal_ex_with_fpn_mapping_and_scaled_rois(hip):
    L = hip.lib()
    B, R, ncls, D = 4, 1000, 81, 128
    rois, cls, deltas, sf, im, n_rois = head_batch(2)
    dev = torch.device("cuda")
    t = [cu(x) for x in (rois, n_rois, cls, deltas, sf, im)]
    i32 = torch.int32
    for opt in (None, hip.det_options(do_bbox_vote=True), hip.det_options(do_soft_nms=True, do_bbox_vote=True, bbox_vote_thresh=0.6)):
        outs = []
        for fn, extra in ((L.dtc_postprocess_detections_ex, ()), (L.dtc_postprocess_detections_ex2, (None,)),
                          (L.dtc_postprocess_detections_ex2, (hip.VoteScoring(0, 1.0),))):
            ws = hip.workspace(hip.det_workspace_bytes(B, R, ncls, opt), dev)
            bufs = [torch.full((B, D, 6), 7.0, device=dev), torch.full((B, D), -3, dtype=i32, device=dev),
                    torch.full((B, D, 4), 5.0, device=dev), torch.zeros((B,), dtype=i32, device=dev),
                    torch.zeros((B, D, 5), device=dev), torch.zeros((B, D), dtype=i32, device=dev), torch.zeros((B,), dtype=i32, device=dev),
                    torch.zeros((B, D, 4), device=dev), torch.zeros((B, 4), dtype=i32, device=dev), torch.zeros((B, D), dtype=i32, device=dev),
                    torch.zeros((B, D), dtype=i32, device=dev), torch.zeros((B, D, 8), device=dev)]
            fm = hip.FpnMapOut(*[x.data_ptr() for x in bufs[4:]], 2, 5)
            hip.check(fn(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), 0, t[3].data_ptr(), None, t[4].data_ptr(), t[5].data_ptr(),
                         B, R, ncls, 10., 10., 5., 5., .05, .5, 100, opt, *extra, ws.data_ptr(), ws.numel(), bufs[0].data_ptr(),
                         bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(), D, fm, hip.stream_ptr(dev)), "ex")
            torch.cuda.synchronize()
            outs.append([x.cpu().numpy() for x in bufs])
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def test_c4_and_overlapped_region_paths_with_a_scoring(hip, oracle):
    import chain
    from detectorch_amd.pipeline import C4RegionPath, FpnRegionPath, OverlappedRegionPath, synthetic_batch, synthetic_c4_batch
    dev = torch.device("cuda", 0)
    # C4: eager == graph replay == the checker; a second input set replayed == a fresh path
    B, C = 2, 32
    opts = dict(do_soft_nms=True, soft_nms_method="gaussian", do_bbox_vote=True, bbox_vote_thresh=0.7, bbox_vote_method="AVG")
    path = C4RegionPath(B, dev, channels=C, det_options=opts)
    assert path.det_scoring is not None and path.det_scoring.method == hip.VOTE_METHODS["AVG"]
    in1, in2 = synthetic_c4_batch(B, dev, seed=2100, channels=C), synthetic_c4_batch(B, dev, seed=2177, channels=C)
    names = ("dets", "det_roi", "det_scaled", "det_count")
    path.bind(*in1)
    path.step(use_graph=False)
    torch.cuda.synchronize()
    eager = [getattr(path, k).clone() for k in names]
    path.step(use_graph=True)
    path.step(use_graph=True)
    torch.cuda.synchronize()
    assert all(torch.equal(a, getattr(path, k)) for a, k in zip(eager, names))
    rpn_cls, rpn_bbox, feat, cls_score, bbox_pred, sf, im_size = [x.cpu().numpy() for x in in1]
    for b in range(B):
        ref = chain.c4_hot_path(rpn_cls[b], rpn_bbox[b], feat[b:b + 1], cls_score[b], bbox_pred[b], sf[b], im_size[b],
                                path.im_h, path.im_w, pooled=7)
        n = ref["rois"].shape[0]
        boxes = decode(oracle, ref["rois"], sf[b], im_size[b], bbox_pred[b, :n])
        dets, roi = vsr.compose(oracle, cls_score[b, :n], boxes, "gaussian", 0.7, "AVG")
        check_scored(eager, b, dets, roi, "AVG", sf[b], path.max_out)
    path.bind(*in2)
    path.step(use_graph=True)
    fresh = C4RegionPath(B, dev, channels=C, det_options=opts)
    fresh.bind(*in2)
    fresh.step(use_graph=False)
    torch.cuda.synchronize()
    assert all(torch.equal(getattr(path, k), getattr(fresh, k)) for k in names)
    # OverlappedRegionPath forwards the scoring to its sub-paths: each == the matching image of one FpnRegionPath
    B, C = 2, 8
    fo = dict(do_bbox_vote=True, bbox_vote_thresh=0.6, bbox_vote_method="QUASI_SUM")
    ov = OverlappedRegionPath(B, dev, n_split=2, channels=C, det_options=fo)
    assert all(p.det_scoring is not None and p.det_scoring.method == hip.VOTE_METHODS["QUASI_SUM"] for p in ov.sub)
    one = FpnRegionPath(B, dev, channels=C, det_options=fo)
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


def test_forward_batched_scored_vote_and_path_cache(hip, oracle):
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
        with pytest.raises(NotImplementedError, match="Unknown scoring method"):
            model.forward_batched(blob, sf, im_size, blob_hw=blob_hw, do_bbox_vote=True, bbox_vote_method="MEDIAN")
        path = model.forward_batched(blob, sf, im_size, blob_hw=blob_hw, do_bbox_vote=True, bbox_vote_method="IOU_AVG")
        torch.cuda.synchronize()
        assert path.det_scoring is not None and len(model._paths) == 1
        n_rois = path.n_rois.cpu().numpy()
        logits, bbox, rois5 = path.cls_logits_out.cpu().numpy(), path.bbox_pred_out.cpu().numpy(), path.rois5.cpu().numpy()
        total = 0
        for b in range(2):
            n = int(n_rois[b])
            scores = oracle.softmax_rows(logits[b, :n])
            boxes = decode(oracle, rois5[b, :n, 1:], scales[b], im_size[b].cpu().numpy(), bbox[b, :n])
            sc, bx, cb = result_utils.box_results_with_nms_and_limit(scores, boxes, do_bbox_vote=True, bbox_vote_method="IOU_AVG")
            D = int(path.det_count[b])
            assert D == len(sc)
            D = min(D, path.max_out)
            dets = path.dets[b, :D].cpu().numpy()
            assert np.array_equal(dets[:, 4], sc[:D]) and np.array_equal(dets[:, :4], bx[:D])
            assert np.array_equal(dets[:, 5].astype(np.int64), np.concatenate([np.full(len(cb[j]), j) for j in range(1, 81)])[:D])
            total += D
        assert total > 0
        again = model.forward_batched(blob, sf, im_size, blob_hw=blob_hw, do_bbox_vote=True, bbox_vote_method="IOU_AVG")
        assert again is path and len(model._paths) == 1
        avg = model.forward_batched(blob, sf, im_size, blob_hw=blob_hw, do_bbox_vote=True, bbox_vote_method="AVG")
        idv = model.forward_batched(blob, sf, im_size, blob_hw=blob_hw, do_bbox_vote=True)
        assert len({id(path), id(avg), id(idv)}) == 3 and len(model._paths) == 3       # one cached path per method
        assert idv.det_scoring is None
    finally:
        torch.backends.cudnn.deterministic = old
