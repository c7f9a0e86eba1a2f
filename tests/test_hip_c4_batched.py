"""detector.forward_batched for the C4 models and the precomputed-proposal (Fast R-CNN) flows on the MI355X, with random weights:
e2e Faster / Mask R-CNN R-50-C4 (eval_faster.ipynb, eval_mask.ipynb), Fast R-CNN R-50-C4 / R-50-FPN with proposals= (eval_fast.ipynb,
eval_fast_FPN.ipynb).  Each stage is compared with the oracle on the path's own intermediate tensors, and the whole flow with the
reference-shaped per-image calls within the tolerances of test_hip_detector.py.  -m gpu."""
import numpy as np
import pytest
import torch

import proposal_prep_ref as pr

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, scope="module")
def _deterministic_convs():
    old = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    yield
    torch.backends.cudnn.deterministic = old


def _c4_model(**kw):
    from detectorch_amd.model.detector import detector
    torch.manual_seed(0)
    m = detector(arch='resnet50', **kw).cuda()
    m.classif_head.weight.data *= 60.0          # sharpen the random classifier so that detections exist
    return m


def _images(B, seed, h=256, w=320):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return torch.randn(B, 3, h, w, generator=g, device="cuda")


def _check_stages(oracle, path, b, feat_b, sf, im_size, rpn=None):
    """proposals (rpn: the path's own RPN maps), box RoIAlign and detections of image b against the oracle"""
    n = int(path.n_rois[b])
    rois = path.rois5[b, :n, 1:].cpu().numpy()
    if rpn is not None:
        score, deltas, logits = rpn
        prob = oracle.rpn_sigmoid(score) if logits else score
        want, _ = oracle.generate_proposals(prob, deltas, oracle.generate_anchors(stride=16), 16.0, path.im_h, path.im_w,
                                            path.pre, path.post, path.thresh)
        assert want.shape[0] > 50 and np.array_equal(rois, want)
    T = path.top_n
    rois5 = np.hstack([np.zeros((n, 1), np.float32), rois])
    ref = oracle.roi_align_forward(feat_b, rois5, path.pooled, path.pooled, 0.0625, path.sr)
    assert np.array_equal(path.box_feats[b * T:b * T + n].cpu().numpy(), ref)
    logits = path.cls_logits_out[b, :n].cpu().numpy()
    dets, _ = oracle.postprocess_detections(rois, sf, im_size, oracle.softmax_rows(logits), path.bbox_pred_out[b, :n].cpu().numpy())
    D = int(path.det_count[b])
    assert D == dets.shape[0] and D > 0
    got = path.dets[b, :min(D, path.max_out)].cpu().numpy()
    assert np.array_equal(got[:, 5], dets[:len(got), 5])
    assert np.allclose(got[:, :5], dets[:len(got), :5], rtol=1e-6, atol=1e-5)
    return n, D


def test_faster_rcnn_c4_batched_stages_vs_oracle(oracle):
    """e2e_faster_rcnn_R-50-C4, B = 2: proposals == oracle.generate_proposals on the path's RPN outputs, 14x14 sr 0 box features ==
    oracle.roi_align_forward, detections == the oracle post-processing of the path's head outputs; per_image gives forward()'s tuple"""
    from detectorch_amd.model.detector import detector
    model = _c4_model(use_rpn_head=True)
    images = _images(2, 21)
    sf, im_size = [1.0, 1.25], [[256.0, 320.0], [204.0, 256.0]]
    path = model.forward_batched(images, sf, im_size)
    torch.cuda.synchronize()
    assert path.pre == 6000 and path.post == 1000 and path.thresh == 0.7 and path.pooled == 14 and path.sr == 0
    feats = path.img_features.cpu().numpy()
    assert feats.shape == (2, 1024, 16, 20)
    for b in range(2):
        rpn = (path.rpn_cls[b].cpu().numpy(), path.rpn_bbox[b].cpu().numpy(), model.fuse_rpn_sigmoid)
        _check_stages(oracle, path, b, feats[b:b + 1], sf[b], im_size[b], rpn)
        cls_b, bbox_b, rois_b, f_b = detector.per_image(path, b)
        assert torch.is_tensor(f_b) and tuple(f_b.shape) == (1, 1024, 16, 20) and rois_b.shape[1] == 4
        assert torch.allclose(cls_b.sum(1), torch.ones(cls_b.shape[0], device="cuda"), atol=1e-4)


def test_faster_rcnn_c4_batched_equals_reference_shaped_forward():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.utils import result_utils
    model = _c4_model(use_rpn_head=True)
    image = _images(1, 22)
    sf, im_size = torch.tensor([1.6], device="cuda"), torch.tensor([[160.0, 200.0]], device="cuda")
    path = model.forward_batched(image, sf, im_size)
    torch.cuda.synchronize()
    cls_b, bbox_b, rois_b, _ = detector.per_image(path, 0)
    cls_score, bbox_pred, rois, _ = model(image, scaling_factor=sf)
    assert rois.shape == rois_b.shape and torch.allclose(rois, rois_b, atol=1e-2)
    assert torch.allclose(bbox_pred, bbox_b, rtol=1e-3, atol=1e-3) and torch.allclose(cls_score, cls_b, rtol=1e-2, atol=1e-4)
    scores_final, boxes_final, boxes_per_class = result_utils.postprocess_output(rois, sf, im_size[0], cls_score, bbox_pred)
    D = boxes_final.shape[0]
    assert D > 0 and D == min(int(path.det_count[0]), path.max_out)
    dets = path.dets[0, :D].cpu().numpy()
    assert np.allclose(dets[:, 4], scores_final, rtol=1e-2, atol=1e-4) and np.allclose(dets[:, :4], boxes_final, atol=5e-2)
    all_boxes, _ = result_utils.assemble_results(path.dets, path.det_count)
    assert sum(len(all_boxes[j][0]) for j in range(1, 81)) == D


def test_mask_rcnn_c4_batched_mask_branch(oracle):
    """e2e_mask_rcnn_R-50-C4: the mask branch's 14x14 sr 0 features on res4 == oracle.roi_align_forward of the scaled detections
    (both images of B = 2); B = 1 against forward + postprocess_output + mask_head + segm_results (M = 14); assemble_results"""
    from detectorch_amd.utils import result_utils
    model = _c4_model(use_rpn_head=True, use_mask_head=True)
    images = _images(2, 23)
    sf, im_size = [1.0, 1.0], [[256.0, 320.0], [256.0, 320.0]]
    path = model.forward_batched(images, sf, im_size)
    torch.cuda.synchronize()
    feats = path.img_features.cpu().numpy()
    Dm = path.max_out
    for b in range(2):
        _check_stages(oracle, path, b, feats[b:b + 1], sf[b], im_size[b])
        D = min(int(path.det_count[b]), Dm)
        assert int(path.m_n[b]) == D
        scaled = path.det_scaled[b, :D].cpu().numpy()
        ref = oracle.roi_align_forward(feats[b:b + 1], np.hstack([np.zeros((D, 1), np.float32), scaled]), 14, 14, 0.0625, 0)
        assert np.array_equal(path.mask_feats[b * Dm:b * Dm + D].cpu().numpy(), ref)
    assert tuple(path.masks.shape) == (2 * Dm, 81, 14, 14)
    # reference-shaped flow on image 0 alone
    p1 = model.forward_batched(images[:1], sf[:1], im_size[:1])
    torch.cuda.synchronize()
    sf1 = torch.tensor(sf[:1], device="cuda")
    cls_score, bbox_pred, rois, feat = model(images[:1], scaling_factor=sf1)
    scores_final, boxes_final, boxes_per_class = result_utils.postprocess_output(rois, sf1, torch.tensor(im_size[0]), cls_score, bbox_pred)
    D = boxes_final.shape[0]
    assert D > 0 and D == min(int(p1.det_count[0]), p1.max_out)
    masks = model.mask_head(feat, torch.as_tensor(boxes_final * sf[0], dtype=torch.float32, device="cuda"))
    assert torch.allclose(masks, p1.masks[:D], rtol=1e-2, atol=1e-3)
    segms = result_utils.segm_results(boxes_per_class, masks, boxes_final, 256, 320, M=14)
    _, got = result_utils.assemble_results(p1.dets, p1.det_count, p1.im_size, p1.rle_str, p1.rle_str_len)
    n_same = sum(a == c for j in range(1, 81) for a, c in zip(segms[j], got[j][0]))
    assert sum(len(s) for s in segms) == D and n_same >= int(0.8 * D)


def _proposals(B, n, h, w, seed):
    rs = np.random.RandomState(seed)
    out = []
    for b in range(B):
        k = n - 40 * b
        xy = rs.uniform(0, [w - 30, h - 30], (k // 2, 2))
        wh = rs.uniform(8, [w * 0.9, h * 0.9], (k // 2, 2))
        base = np.hstack([xy, np.minimum(xy + wh, [w - 1, h - 1])])
        rows = base[rs.randint(0, len(base), k)] + rs.uniform(-0.3, 0.3, (k, 4))          # aliases on the 1/16 grid
        out.append(np.clip(rows, 0, [w - 1, h - 1, w - 1, h - 1]).astype(np.float32))
    x = np.zeros((B, n, 4), np.float32)
    for b, r in enumerate(out):
        x[b, :len(r)] = r
        x[b, len(r):] = np.nan                                                              # garbage past the counts
    return out, x, [len(r) for r in out]


@pytest.mark.parametrize("fpn", [False, True])
def test_fast_rcnn_batched_with_precomputed_proposals(oracle, fpn):
    """Fast R-CNN R-50-C4 / R-50-FPN (no RPN head) with proposals=: rois == the restatement of the reference's preprocessing
    (scale, remove_dup_prop, add_multilevel_rois_for_test), pooled features bit-exact against the oracle on each roi's level,
    detections == forward(rois=...) + postprocess_output on those rois within conv tolerance"""
    from detectorch_amd.model.detector import detector
    from detectorch_amd.utils import result_utils
    torch.manual_seed(0)
    if fpn:
        model = detector(arch='resnet50', conv_body_layers=['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'],
                         conv_head_layers='two_layer_mlp', fpn_layers=['layer1', 'layer2', 'layer3', 'layer4'], fpn_extra_lvl=True,
                         roi_height=7, roi_width=7, roi_spatial_scale=[0.25, 0.125, 0.0625, 0.03125], roi_sampling_ratio=2,
                         use_rpn_head=False).cuda()
    else:
        model = detector(arch='resnet50', use_rpn_head=False).cuda()
    model.classif_head.weight.data *= 60.0
    h, w = 256, 320
    sf = [800.0 / 427.0, 1.25]
    im_size = [[h / sf[0], w / sf[0]], [h / sf[1], w / sf[1]]]
    boxes, x, counts = _proposals(2, 300, im_size[0][0], im_size[0][1], 31 + fpn)
    images = _images(2, 24 + fpn, h, w)
    with pytest.raises(ValueError):
        model.forward_batched(images, sf, im_size)
    path = model.forward_batched(images, sf, im_size, proposals=torch.from_numpy(x), proposal_counts=counts)
    torch.cuda.synchronize()
    assert path.top_n == 300
    T = path.top_n
    feats = path.img_features
    for b in range(2):
        k_min, k_max = (2, 5) if fpn else (4, 4)
        want = pr.prepare(boxes[b], sf[b], k_min=k_min, k_max=k_max)
        n = len(want["rois"])
        assert 0 < n < counts[b] and int(path.n_rois[b]) == n
        assert np.array_equal(path.rois5[b, :n, 1:].cpu().numpy().view(np.uint32), want["rois"].view(np.uint32))
        assert np.array_equal(path.prop_src[b, :n].cpu().numpy(), want["src_index"])
        rois5 = np.hstack([np.zeros((n, 1), np.float32), want["rois"]])
        got = path.box_feats[b * T:b * T + n].cpu().numpy()
        if fpn:
            lv = want["levels"]
            assert np.array_equal(path.roi_levels[b, :n].cpu().numpy(), lv) and len(set(lv.tolist())) >= 2
            for l, s in enumerate([0.25, 0.125, 0.0625, 0.03125]):
                sel = lv == l
                if sel.any():
                    ref = oracle.roi_align_forward(feats[l][b:b + 1].cpu().numpy(), rois5[sel], 7, 7, s, 2)
                    assert np.array_equal(got[sel], ref)
        else:
            assert np.array_equal(got, oracle.roi_align_forward(feats[b:b + 1].cpu().numpy(), rois5, 14, 14, 0.0625, 0))
        # the reference-shaped call on the same (deduplicated, level-distributed) rois, image b alone
        sfb = torch.tensor([sf[b]], device="cuda")
        if fpn:
            per, restore, _ = pr.distribute(want["rois"])
            per_level = [torch.from_numpy(np.ascontiguousarray(q)).cuda() for q in per]
            cls_score, bbox_pred, rois, _ = model(images[b:b + 1], rois=per_level, scaling_factor=sfb,
                                                  roi_original_idx=torch.from_numpy(restore).cuda().long())
        else:
            cls_score, bbox_pred, rois, _ = model(images[b:b + 1], rois=torch.from_numpy(want["rois"]).cuda().unsqueeze(0),
                                                  scaling_factor=sfb)
        rois = rois.reshape(-1, rois.shape[-1])[:, -4:]
        cls_b, bbox_b, rois_b, _ = detector.per_image(path, b)
        assert torch.equal(rois_b, rois)
        assert torch.allclose(bbox_pred, bbox_b, rtol=1e-3, atol=1e-3) and torch.allclose(cls_score, cls_b, rtol=1e-2, atol=1e-4)
        scores_final, boxes_final, _ = result_utils.postprocess_output(rois, sfb, torch.tensor(im_size[b]), cls_score, bbox_pred)
        D = boxes_final.shape[0]
        assert D > 0 and D == min(int(path.det_count[b]), path.max_out)
        dets = path.dets[b, :D].cpu().numpy()
        assert np.allclose(dets[:, 4], scores_final, rtol=1e-2, atol=1e-4) and np.allclose(dets[:, :4], boxes_final, atol=5e-2)
    # a model WITH an RPN head rejects precomputed proposals
    with pytest.raises(ValueError):
        _c4_model(use_rpn_head=True).forward_batched(images, sf, im_size, proposals=torch.from_numpy(x))
