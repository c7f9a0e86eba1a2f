"""Every bbox-vote scoring on the device (dtc_box_voting_scored, dtc_postprocess_detections_ex2) against the reference's own outputs
(tests/golden/postprocess_vote_scoring.npz) and the checker (vote_scoring_ref).  Boxes, row sets, row order, det_roi bit-exact;
scores bit-exact for ID / AVG / IOU_AVG / QUASI_SUM / GENERALIZED_AVG at beta 1, within 1e-6 relative otherwise.  -m gpu."""
import numpy as np
import pytest
import torch

from conftest import golden
import vote_scoring_ref as vsr
from test_vote_scoring_host import check_against_fixture, fixture_case

pytestmark = pytest.mark.gpu


def _scores_match(got, ref, exact, msg=""):
    if exact:
        assert np.array_equal(got, ref), msg
    else:
        np.testing.assert_allclose(got, ref, rtol=1e-6, atol=0, err_msg=msg)


@pytest.mark.parametrize("method", vsr.METHODS)
def test_box_voting_scored_golden_and_checker(oracle, method):
    from detectorch_amd.utils import boxes as box_utils
    g = golden("postprocess_vote_scoring")
    for th in vsr.THRESHOLDS:
        for beta in (1.0, 0.5):
            ref = g["bv_%d_%s_%d" % (round(th * 10), method, round(beta * 10))]
            out = box_utils.box_voting(g["bv_top"], g["bv_all"], th, scoring_method=method, beta=beta)
            assert np.array_equal(out[:, :4], ref[:, :4]), (th, beta)
            _scores_match(out[:, 4], ref[:, 4], vsr.exact(method, beta), (th, beta))
    # up to n_all = 8192: a dense cluster voted by thousands
    rs = np.random.RandomState(5)
    c = np.array([300.0, 300.0]) + rs.uniform(-4, 4, (8192, 2))
    alld = np.hstack([c - 60, c + 59, rs.uniform(0.06, 1.0, (8192, 1))]).astype(np.float32)
    top = alld[rs.choice(8192, 40, replace=False)]
    for beta in (1.0, 0.5):
        out = box_utils.box_voting(top, alld, 0.8, scoring_method=method, beta=beta)
        ref = vsr.box_voting(oracle, top, alld, 0.8, method, beta)
        assert np.array_equal(out[:, :4], ref[:, :4])
        _scores_match(out[:, 4], ref[:, 4], vsr.exact(method, beta), beta)
    with pytest.raises(ZeroDivisionError):          # no voter: the reference's np.average raises
        box_utils.box_voting(top[:1], alld[:1] + np.float32([500, 500, 500, 500, 0]), 0.8, scoring_method=method)


@pytest.mark.parametrize("case", vsr.CASES)
def test_result_utils_device_path_matches_fixture_without_host_loop(monkeypatch, case):
    from detectorch_amd.utils import boxes as box_utils
    from detectorch_amd.utils import result_utils

    def boom(*a, **k):
        raise AssertionError("the per-class host loop ran")
    monkeypatch.setattr(box_utils, "nms", boom)
    monkeypatch.setattr(box_utils, "soft_nms", boom)
    g = golden("postprocess_vote_scoring")
    scores, boxes = fixture_case(g, case)
    for nm in vsr.NMS_METHODS:
        for th in vsr.THRESHOLDS:
            tag = "%s_%s_%d" % (case, nm, round(th * 10))
            kw = dict(do_bbox_vote=True, bbox_vote_thresh=th)
            if nm != "nms":
                kw.update(do_soft_nms=True, soft_nms_method=nm)
            for m in vsr.METHODS:
                sc, bx, cb = result_utils.box_results_with_nms_and_limit(scores, boxes, num_classes=scores.shape[1],
                                                                         bbox_vote_method=m, **kw)
                cls = np.concatenate([np.full(len(cb[j]), j, np.float32) for j in range(1, scores.shape[1])])
                dets = np.hstack([bx, sc[:, None], cls[:, None]]).astype(np.float32)
                check_against_fixture(g, tag, m, dets, vsr.exact(m))
            if case == "crowd" and nm == "nms" and th == 0.8:
                assert len(g[tag + "_IOU_AVG_scores"]) == 100 and int(g[tag + "_ID_n"]) == 104


def _batch():
    """B = 3 images of 3 classes with mixed crowding: the crowd case, the dense case, and a sparse slice of the dense one"""
    g = golden("postprocess_vote_scoring")
    ims = [(g["crowd_scores"], g["crowd_boxes"]), (g["dense_scores"], g["dense_boxes"]),
           (g["dense_scores"][::7].copy(), g["dense_boxes"][::7].copy())]
    R = max(s.shape[0] for s, _ in ims)
    sc = np.zeros((3, R, 3), np.float32)
    bx = np.zeros((3, R, 12), np.float32)
    for b, (s, x) in enumerate(ims):
        sc[b, :len(s)], bx[b, :len(s)] = s, x
        sc[b, len(s):] = 0.9                    # rows past the count: never read
    return ims, sc, bx, np.array([len(s) for s, _ in ims], np.int32)


@pytest.mark.parametrize("nm", ["nms", "linear", "gaussian", "hard"])
def test_batched_box_results_nms_limit_per_image_vs_checker(oracle, nm):
    from detectorch_amd import hip
    ims, sc, bx, nr = _batch()
    dev = torch.device("cuda")
    tsc, tbx, tnr = torch.from_numpy(sc).to(dev), torch.from_numpy(bx).to(dev), torch.from_numpy(nr).to(dev)
    for th in (0.8, 0.6):
        for m in vsr.METHODS:
            kw = vsr.kwargs_of(nm, th, m)
            dets, roi, cnt = hip.box_results_nms_limit(tsc, tbx, tnr, 0.05, 0.5, 100, 512, **kw)
            dets, roi, cnt = dets.cpu().numpy(), roi.cpu().numpy(), cnt.cpu().numpy()
            for b, (s, x) in enumerate(ims):
                ref, ref_roi = vsr.compose(oracle, s, x, nm, th, m)
                n = int(cnt[b])
                assert n == len(ref), (nm, th, m, b, n, len(ref))
                assert np.array_equal(roi[b, :n], ref_roi), (nm, th, m, b)
                assert np.array_equal(dets[b, :n, :4], ref[:, :4]), (nm, th, m, b)
                assert np.array_equal(dets[b, :n, 5], ref[:, 5]), (nm, th, m, b)
                _scores_match(dets[b, :n, 4], ref[:, 4], vsr.exact(m), (nm, th, m, b))


def test_ex2_id_and_null_equal_ex_bit_for_bit():
    from detectorch_amd import hip
    L = hip.lib()
    ims, sc, bx, nr = _batch()
    dev = torch.device("cuda")
    tsc, tbx, tnr = torch.from_numpy(sc).to(dev), torch.from_numpy(bx).to(dev), torch.from_numpy(nr).to(dev)
    B, R, C = sc.shape
    for opt in (None, hip.det_options(do_bbox_vote=True), hip.det_options(do_soft_nms=True, do_bbox_vote=True, bbox_vote_thresh=0.6)):
        outs = []
        for fn, extra in ((L.dtc_postprocess_detections_ex, ()), (L.dtc_postprocess_detections_ex2, (None,)),
                          (L.dtc_postprocess_detections_ex2, (hip.VoteScoring(0, 1.0),))):
            ws = hip.workspace(hip.det_workspace_bytes(B, R, C, opt), dev)
            dets = torch.full((B, 256, 6), 7.0, device=dev)
            roi = torch.full((B, 256), -3, dtype=torch.int32, device=dev)
            cnt = torch.zeros((B,), dtype=torch.int32, device=dev)
            hip.check(fn(None, tnr.data_ptr(), tsc.data_ptr(), 0, None, tbx.data_ptr(), None, None, B, R, C, 1., 1., 1., 1., .05, .5,
                         100, opt, *extra, ws.data_ptr(), ws.numel(), dets.data_ptr(), roi.data_ptr(), None, cnt.data_ptr(), 256,
                         None, hip.stream_ptr(dev)), "ex")
            torch.cuda.synchronize()
            outs.append((dets.cpu().numpy(), roi.cpu().numpy(), cnt.cpu().numpy()))
        for o in outs[1:]:
            for a, b in zip(outs[0], o):
                assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("vote_method", ["IOU_AVG", "TEMP_AVG"])
def test_fpn_region_path_scored_vote_eager_graph_and_second_input(oracle, vote_method):
    from det_options_ref import decode
    from detectorch_amd.pipeline import FpnRegionPath, synthetic_batch
    dev = torch.device("cuda", 0)
    B, C = 2, 8
    opts = dict(do_soft_nms=True, soft_nms_method="linear", do_bbox_vote=True, bbox_vote_thresh=0.6, bbox_vote_method=vote_method)
    names = ("dets", "det_roi", "det_scaled", "det_count", "m_n", "m_levels")

    def run(path, inputs, graph):
        path.bind(*inputs)
        path.step(use_graph=graph)
        torch.cuda.synchronize()
        return {k: getattr(path, k).clone() for k in names}

    path = FpnRegionPath(B, dev, channels=C, det_options=opts)
    in1, in2 = synthetic_batch(B, dev, seed=3100, channels=C), synthetic_batch(B, dev, seed=3177, channels=C)
    eager = run(path, in1, False)
    rois5, n_rois = path.rois5.cpu().numpy(), path.n_rois.cpu().numpy()
    cls, bbox = path.cls_score.cpu().numpy(), path.bbox_pred.cpu().numpy()
    sf, im_size = path.sf.cpu().numpy(), path.im_size.cpu().numpy()
    replay = run(path, in1, True)
    for k in names:
        assert torch.equal(replay[k], eager[k]), k
    second = run(path, in2, True)                                 # replay over a second input set
    fresh = run(FpnRegionPath(B, dev, channels=C, det_options=opts), in2, False)
    for k in names:
        assert torch.equal(second[k], fresh[k]), k
    # the eager detections against the checker
    for b in range(B):
        n = int(n_rois[b])
        boxes = decode(oracle, rois5[b, :n, 1:], sf[b], im_size[b], bbox[b, :n])
        ref, ref_roi = vsr.compose(oracle, cls[b, :n], boxes, "linear", 0.6, vote_method)
        cnt = int(eager["det_count"][b])
        assert cnt == len(ref)
        d = eager["dets"][b, :cnt].cpu().numpy()
        assert np.array_equal(eager["det_roi"][b, :cnt].cpu().numpy(), ref_roi)
        assert np.array_equal(d[:, :4], ref[:, :4]) and np.array_equal(d[:, 5], ref[:, 5])
        _scores_match(d[:, 4], ref[:, 4], vsr.exact(vote_method))
