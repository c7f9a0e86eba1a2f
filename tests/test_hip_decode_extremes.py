"""Box decoding on saturated and non-finite deltas on the device: the RPN decode (dtc_rpn_topk_decode[_sized]), the detection
decode (dtc_postprocess_detections_ex) and dtc_bbox_transform against tests/golden/decode_extremes.npz (the reference's own outputs,
tests/golden/make_decode_extremes_golden.py) and bit for bit against the oracle.  -m gpu.

RPN: counts and scores equal to the reference, boxes within 1 ulp (its exp is torch-CPU), bit-equal to the oracle; probabilities and
logits; B = 1, B = 4 (resident decode), B = 8 at pre 8192 (ticket decode) with mixed extents, each image equal to a B = 1 call;
min_size_scaled > 0, with an image whose every row is filtered; the whole chain (FpnRegionPath eager and graph, C4RegionPath) on
extreme RPN deltas.  Detection head: hard NMS (probabilities, logits), linear Soft-NMS + vote 0.8, bbox_transform; NaN head deltas
give finite boxes inside the image (the detection decode keeps fminf / fmaxf on purpose)."""
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, golden, ulp_close
from det_options_ref import compose, decode
from detectorch_amd import synth
from test_decode_extremes_host import RPN_RUNS, close_nan_aware, min_size_scaled, rpn_case, soft_vote_scores

sys.path.insert(0, GOLDEN)
import make_decode_extremes_golden as mk  # noqa: E402  (the fixture's extreme pattern; the reference itself is not imported)

pytestmark = pytest.mark.gpu

FPN_ANCHOR_SIZES = [(32.0 * 2 ** l,) for l in range(5)]


@pytest.fixture(scope="module")
def hip():
    from detectorch_amd import hip as h
    h.lib()
    return h


def cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- RPN against the reference's fixture ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("logits", [False, True])
@pytest.mark.parametrize("case,thr,m", RPN_RUNS)
def test_rpn_extremes_vs_reference_and_oracle(hip, oracle, case, thr, m, logits):
    from detectorch_amd.utils.generate_anchors import generate_anchors
    g = golden("decode_extremes")
    A, H, W, stride, pre, post, im_h, im_w, sizes = rpn_case(g, case)
    cls, d = g["rpn_%s_cls" % case], g["rpn_%s_bbox" % case]
    anchors = generate_anchors(stride=stride, sizes=sizes, aspect_ratios=(0.5, 1, 2))
    out = hip.generate_proposals([cu(g["rpn_%s_lg" % case] if logits else cls)], [cu(d)], [anchors], [stride], im_h, im_w, [pre],
                                 post, thr, min_size_scaled=min_size_scaled(m), scores_are_logits=logits)
    ob, os_, oc = [x.cpu().numpy() for x in out[:3]]
    n = int(oc[0, 0])
    boxes, scores = ob[0, 0, :n], os_[0, 0, :n]
    tag = "rpn_%s_t%02d_m%d" % (case, int(thr * 10), m)
    ref_p, ref_s = g[tag + "_props"], g[tag + "_scores"]
    assert n == ref_s.shape[0], (n, ref_s.shape[0])
    assert np.array_equal(scores, ref_s)
    assert close_nan_aware(boxes, ref_p)
    rb, rs = oracle.generate_proposals(cls[0], d[0], oracle.generate_anchors(stride, sizes, (0.5, 1, 2)), stride, im_h, im_w, pre,
                                       post, thr, min_size_scaled=min_size_scaled(m))
    assert np.array_equal(scores, rs) and np.array_equal(boxes.view(np.uint32), rb.view(np.uint32))


# ---- batched: resident and ticket decode, sized extents, min_size ---------------------------------------------------------------
def _extreme_fpn_batch(seed, B, pre, shapes=None, logits=False):
    """per level [B,3,H,W] scores (probabilities or logits) and [B,12,H,W] deltas; each image gets its own seeded extreme pattern
    on anchors ranked inside its top pre_nms_top_n"""
    shapes = shapes or synth.fpn_level_shapes()
    cls, bbox = [], []
    for l, (H, W) in enumerate(shapes):
        cs, ds = [], []
        for b in range(B):
            rs = synth.rng(19, seed + 10 * l + b)
            lg, p, d = mk.rpn_maps(rs, 3, H, W, pre, copies=1 + b % 3)
            cs.append(lg if logits else p)
            ds.append(d)
        cls.append(np.concatenate(cs))
        bbox.append(np.concatenate(ds))
    return cls, bbox


def _check_batch(hip, oracle, cls, bbox, blob_hw, im_hw, pre, post, thr, min_size=0.0, logits=False):
    """one batched call == a B = 1 call on each image's crop == the oracle on the crop, bit for bit (pre- and post-NMS)"""
    from detectorch_amd.utils.generate_anchors import generate_anchors
    strides = [float(s) for s in synth.FPN_STRIDES][:len(cls)]
    nl, B = len(cls), cls[0].shape[0]
    anchors = [generate_anchors(stride=strides[l], sizes=FPN_ANCHOR_SIZES[l], aspect_ratios=(0.5, 1, 2)) for l in range(nl)]
    oanchors = [oracle.generate_anchors(strides[l], FPN_ANCHOR_SIZES[l], (0.5, 1, 2)) for l in range(nl)]
    got = hip.generate_proposals([cu(c) for c in cls], [cu(d) for d in bbox], anchors, strides, blob_hw[0], blob_hw[1], [pre] * nl,
                                 post, thr, min_size_scaled=min_size, scores_are_logits=logits,
                                 im_hw=None if im_hw is None else torch.tensor(im_hw, dtype=torch.float32))
    ob, os_, oc, pb, ps, pc = [x.cpu().numpy() for x in got]
    pb, ps, pc = pb.reshape(B, nl, -1, 4), ps.reshape(B, nl, -1), pc.reshape(B, nl)
    for b in range(B):
        h, w = im_hw[b] if im_hw is not None else blob_hw
        ch = [int(np.ceil(h / strides[l])) for l in range(nl)]
        cw = [int(np.ceil(w / strides[l])) for l in range(nl)]
        cc = [np.ascontiguousarray(c[b:b + 1, :, :ch[l], :cw[l]]) for l, c in enumerate(cls)]
        cd = [np.ascontiguousarray(d[b:b + 1, :, :ch[l], :cw[l]]) for l, d in enumerate(bbox)]
        one = [x.cpu().numpy() for x in hip.generate_proposals([cu(c) for c in cc], [cu(d) for d in cd], anchors, strides, h, w,
                                                               [pre] * nl, post, thr, min_size_scaled=min_size,
                                                               scores_are_logits=logits)]
        qb, qs, qc, qpb, qps, qpc = one
        for l in range(nl):
            n, m = int(pc[b, l]), int(oc[b, l])
            assert n == int(qpc[l]) and m == int(qc[0, l]), (b, l, n, int(qpc[l]), m, int(qc[0, l]))
            assert np.array_equal(ps[b, l, :n], qps[l, :n]) and np.array_equal(pb[b, l, :n], qpb[l, :n]), (b, l)
            assert np.array_equal(os_[b, l, :m], qs[0, l, :m]) and np.array_equal(ob[b, l, :m], qb[0, l, :m]), (b, l)
            prob = oracle.rpn_sigmoid(cc[l]) if logits else cc[l]
            rb, rsc, rpb, rps = oracle.generate_proposals(prob[0], cd[l][0], oanchors[l], strides[l], h, w, pre, post, thr,
                                                          min_size_scaled=min_size, return_pre_nms=True)
            assert n == rps.shape[0] and np.array_equal(ps[b, l, :n], rps) and np.array_equal(pb[b, l, :n], rpb), (b, l)
            if thr > 0:
                assert m == rsc.shape[0] and np.array_equal(os_[b, l, :m], rsc) and np.array_equal(ob[b, l, :m], rb), (b, l)
            assert np.isfinite(pb[b, l, :n]).all()
    return pc, oc, got


@pytest.mark.parametrize("logits", [False, True])
def test_batch4_resident_decode_extremes(hip, oracle, logits):
    B, pre = 4, 1000
    cls, bbox = _extreme_fpn_batch(100 + logits, B, pre, logits=logits)
    assert ((pre + 255) // 256) * B * 5 <= 1024                                   # resident decode
    pc, _, _ = _check_batch(hip, oracle, cls, bbox, (synth.FPN_PAD_H, synth.FPN_PAD_W), None, pre, 1000, 0.7, logits=logits)
    assert (pc < pre).all() and (pc[:, :4] > pre - 100).all()                   # the NaN rows are filtered out of every segment


def test_batch8_ticket_decode_extremes_sized(hip, oracle):
    B, pre = 8, 8192
    sizes = [(800, 1344), (512, 1000), (300, 200), (96, 160), (416, 640), (800, 32), (32, 1344), (640, 1024)]
    cls, bbox = _extreme_fpn_batch(200, B, pre)
    assert ((pre + 255) // 256) * B * 5 > 1024                                    # ticket decode
    pc, _, _ = _check_batch(hip, oracle, cls, bbox, (synth.FPN_PAD_H, synth.FPN_PAD_W), sizes, pre, 1000, 0.7)
    assert pre - 100 < pc[0, 0] < pre and pc[3, 0] < pre


@pytest.mark.parametrize("thr", [0.0, 0.7])
def test_min_size_with_fully_filtered_image(hip, oracle, thr):
    # min_size 16 at scale 1.6: image 1 is 24 x 24, so every box (clipped to it) is narrower than 25.6 and every segment of the image
    # is empty; image 0 keeps the rows the comparison lets through.  Count 0 then goes through NMS and collect / distribute.
    ms = min_size_scaled(16)
    shapes = synth.fpn_level_shapes()[:3]
    cls, bbox = _extreme_fpn_batch(300, 2, 1000, shapes=shapes)
    pc, oc, got = _check_batch(hip, oracle, cls, bbox, (synth.FPN_PAD_H, synth.FPN_PAD_W), [(800, 1344), (24, 24)], 1000, 1000,
                               thr, min_size=ms)
    assert not pc[1].any() and not oc[1].any()
    assert pc[0].sum() > 0
    if thr > 0:
        out = hip.fpn_collect_distribute(got[0], got[1], got[2], 1000)
        n_out = out["n_out"].cpu().numpy()
        assert n_out[1] == 0 and n_out[0] == min(1000, int(oc[0].sum()))
        assert out["level_counts"].cpu().numpy()[1].sum() == 0


# ---- the whole chain on extreme RPN deltas -------------------------------------------------------------------------------------
def _inject(rpn_cls, rpn_bbox, seed, pre, underflow=True):
    """write the extreme pattern (NaN included) over each image's top-ranked anchors of every level, in place on the device.
    underflow=False leaves out the dw / dh of -20 and below (zero-width proposals): see test_fpn_region_path_extreme_rpn_vs_oracle_chain"""
    for l, (c, d) in enumerate(zip(rpn_cls, rpn_bbox)):
        cn, dn = c.cpu().numpy(), d.cpu().numpy()
        B, A, H, W = cn.shape
        for b in range(B):
            rs = synth.rng(23, seed + 10 * l + b)
            rows = mk.extreme_rows(1 + (b + l) % 2)
            if not underflow:
                rows = [r for r in rows if not any(v is not None and v <= -20 for v in r[2:])]
            K = min(A * H * W, pre)
            ranked = np.argsort(-cn[b].reshape(-1), kind="stable")[:K]
            for flat, row in zip(rs.permutation(ranked)[:min(len(rows), K)], rows):
                a, hw = divmod(int(flat), H * W)
                h, w = divmod(hw, W)
                for k, v in enumerate(row):
                    if v is not None:
                        dn[b, 4 * a + k, h, w] = v
        d.copy_(torch.from_numpy(dn))


@pytest.mark.parametrize("use_graph", [False, True])
def test_fpn_region_path_extreme_rpn_vs_oracle_chain(oracle, use_graph):
    # Without the exp-underflow rows: a zero-width proposal (x2 = x1 - 1, kept at min_size 0) becomes, through the head decode, a
    # detection whose mask-branch box has a negative area; its FPN level is NaN in the reference (multilevel_rois.py:47-52, np.clip
    # passes NaN) and has no defined value anywhere.  C4RegionPath, which has no mask branch, takes the whole pattern.
    import chain
    from detectorch_amd.pipeline import FpnRegionPath, synthetic_batch
    dev = torch.device("cuda", 0)
    B, C = 2, 8
    path = FpnRegionPath(B, dev, channels=C)
    inputs = synthetic_batch(B, dev, seed=3700, channels=C)
    _inject(inputs[0], inputs[1], 400, path.pre, underflow=False)
    path.bind(*inputs)
    path.step(use_graph=use_graph)
    if use_graph:
        path.step(use_graph=True)
    torch.cuda.synchronize()
    rpn_cls, rpn_bbox, feats, cls_score, bbox_pred, masks, sf, im_size = [
        [t.cpu().numpy() for t in x] if isinstance(x, list) else x.cpu().numpy() for x in inputs]
    assert np.isnan(rpn_bbox[0]).any() and np.isinf(rpn_bbox[0]).any()
    for b in range(B):
        ref = chain.fpn_hot_path([c[b] for c in rpn_cls], [d[b] for d in rpn_bbox], [f[b:b + 1] for f in feats],
                                 cls_score[b], bbox_pred[b], masks[b * path.max_out:(b + 1) * path.max_out], sf[b],
                                 im_size[b], path.pad_h, path.pad_w)
        assert chain.compare_with_gpu(path, b, ref, int(im_size[b, 0]), int(im_size[b, 1]))
        # RoIs collapsed onto one-pixel border lines reached collect / distribute (and so RoIAlign)
        rois = path.rois5[b, :int(path.n_rois[b])].cpu().numpy()
        on_x = (rois[:, 1] == rois[:, 3]) & ((rois[:, 1] == 0) | (rois[:, 1] == path.pad_w - 1))
        on_y = (rois[:, 2] == rois[:, 4]) & ((rois[:, 2] == 0) | (rois[:, 2] == path.pad_h - 1))
        assert (on_x | on_y).any()


def test_c4_region_path_extreme_rpn_vs_oracle_chain(oracle):
    import chain
    from detectorch_amd.pipeline import C4RegionPath, synthetic_c4_batch
    dev = torch.device("cuda", 0)
    B, C = 2, 32
    path = C4RegionPath(B, dev, channels=C, pooled=7)
    inputs = synthetic_c4_batch(B, dev, seed=2700, channels=C)
    _inject([inputs[0]], [inputs[1]], 500, 6000)
    path.bind(*inputs)
    path.step(use_graph=True)
    path.step(use_graph=True)
    torch.cuda.synchronize()
    rpn_cls, rpn_bbox, feat, cls_score, bbox_pred, sf, im_size = [x.cpu().numpy() for x in inputs]
    assert np.isnan(rpn_bbox).any()
    for b in range(B):
        ref = chain.c4_hot_path(rpn_cls[b], rpn_bbox[b], feat[b:b + 1], cls_score[b], bbox_pred[b], sf[b], im_size[b],
                                path.im_h, path.im_w, pooled=7)
        assert chain.compare_c4_with_gpu(path, b, ref)


# ---- detection head --------------------------------------------------------------------------------------------------------------
def _pp_inputs(g, logits=False, cls=None):
    R = g["pp_rois"].shape[0]
    rois5 = np.hstack([np.zeros((R, 1), np.float32), g["pp_rois"]])[None]
    sc = g["pp_logits"] if logits else (g["pp_cls"] if cls is None else cls)
    return (cu(rois5), cu(np.array([R], np.int32)), cu(sc[None]), cu(g["pp_deltas"][None]), cu(g["pp_sf"]),
            cu(g["pp_im_size"][None, :2]))


@pytest.mark.parametrize("logits", [False, True])
def test_postprocess_extremes_vs_reference_and_oracle(hip, oracle, logits):
    g = golden("decode_extremes")
    dets, det_roi, _, cnt = hip.postprocess_detections(*_pp_inputs(g, logits), scores_are_logits=logits)
    D = int(cnt[0])
    got = dets[0, :D].cpu().numpy()
    assert D == g["pp_scores"].shape[0] == 100
    assert np.array_equal(got[:, 4], g["pp_scores"]) and np.array_equal(got[:, 5].astype(np.int32), g["pp_cls_id"])
    assert ulp_close(got[:, :4], g["pp_boxes"])
    ref, roi = oracle.postprocess_detections(g["pp_rois"], g["pp_sf"][0], g["pp_im_size"], g["pp_cls"], g["pp_deltas"])
    assert np.array_equal(got, ref) and np.array_equal(det_roi[0, :D].cpu().numpy(), roi)


def test_postprocess_soft_vote_extremes_vs_reference_and_oracle(hip, oracle):
    g = golden("decode_extremes")
    cls = soft_vote_scores(g)
    out = hip.postprocess_detections(*_pp_inputs(g, cls=cls), do_soft_nms=True, soft_nms_method="linear", do_bbox_vote=True,
                                     bbox_vote_thresh=0.8)
    D = int(out[3][0])
    got = out[0][0, :D].cpu().numpy()
    assert D == g["pp_soft_vote_scores"].shape[0]
    assert np.array_equal(got[:, 4], g["pp_soft_vote_scores"])
    assert np.array_equal(got[:, 5].astype(np.int32), g["pp_soft_vote_cls_id"])
    assert ulp_close(got[:, :4], g["pp_soft_vote_boxes"])
    ref, roi = compose(oracle, cls, decode(oracle, g["pp_rois"], g["pp_sf"][0], g["pp_im_size"], g["pp_deltas"]), "linear", 0.8)
    assert np.array_equal(got, ref) and np.array_equal(out[1][0, :D].cpu().numpy(), roi)


@pytest.mark.parametrize("clip", [False, True])
def test_bbox_transform_extremes_vs_reference_and_oracle(hip, oracle, clip):
    g = golden("decode_extremes")
    im = g["bt_im_shape"]
    got = hip.bbox_transform(cu(g["bt_boxes"]), cu(g["bt_deltas"]), (10.0, 10.0, 5.0, 5.0),
                             clip_to=(float(im[0]), float(im[1])) if clip else None).cpu().numpy()
    assert close_nan_aware(got, g["bt_pred_clipped" if clip else "bt_pred"])
    ref = oracle.bbox_transform(g["bt_boxes"], g["bt_deltas"], (10.0, 10.0, 5.0, 5.0))
    if clip:
        ref = oracle.clip_tiled_boxes(ref, im[0], im[1])
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32))


def test_nan_head_deltas_give_finite_boxes_inside_the_image(hip):
    """The detection decode keeps fminf / fmaxf on purpose: a NaN head delta becomes a finite box inside the image, so
    that mask_paste's float -> int conversion never sees a NaN.  Guards against a 'fix' that lets NaN through."""
    g = golden("decode_extremes")
    rs = synth.rng(19, 900)
    R, n_cls = g["pp_rois"].shape[0], 81
    deltas = mk.head_deltas(rs, R, n_cls, (10.0, 10.0, 5.0, 5.0), nan=True)
    assert np.isnan(deltas).any()
    bad = np.isnan(deltas).reshape(R, n_cls, 4).any(2)
    cls = g["pp_cls"].copy()
    cls[:, 1:][bad[:, 1:]] = np.float32(0.9) - np.arange(int(bad[:, 1:].sum()), dtype=np.float32) * np.float32(1e-3)  # they survive
    ins = list(_pp_inputs(g, cls=cls))
    ins[3] = cu(deltas[None])
    dets, det_roi, _, cnt = hip.postprocess_detections(*ins)
    D = int(cnt[0])
    got = dets[0, :D].cpu().numpy()
    im_h, im_w = g["pp_im_size"][:2]
    assert np.isfinite(got).all()
    assert (got[:, :4] >= 0).all() and (got[:, [0, 2]] <= im_w - 1).all() and (got[:, [1, 3]] <= im_h - 1).all()
    roi = det_roi[0, :D].cpu().numpy()
    assert bad[roi, got[:, 5].astype(np.int64)].any()                    # NaN pairs are among the detections
    boxes = hip.bbox_transform(cu(g["pp_rois"] / g["pp_sf"][0]), cu(deltas), (10.0, 10.0, 5.0, 5.0),
                               clip_to=(float(im_h), float(im_w))).cpu().numpy()
    assert np.isfinite(boxes).all() and (boxes >= 0).all()
