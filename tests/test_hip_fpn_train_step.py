"""The training path of the FPN models on the MI355X (-m gpu): roi_levels_batched and collect_sample_distribute on synthetic
proposals, forward_train_boxes against the reference's level-by-level route (detector.py:260-270), fast_rcnn_train_step on the Fast
R-CNN FPN model, and the joint steps faster_rcnn_train_step / mask_rcnn_train_step on FPN models, held to the checks of the C4 steps
(tests/test_hip_rpn_train_step.py, tests/test_hip_mask_train_step.py).  Every equality here is exact.  tests/README_fpn_train.md."""
import numpy as np
import pytest
import torch

from detectorch_amd import synth
from test_hip_rpn_train_step import check_sgd_step, d

pytestmark = pytest.mark.gpu

FPN = dict(conv_body_layers=['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'], conv_head_layers='two_layer_mlp',
           fpn_layers=['layer1', 'layer2', 'layer3', 'layer4'], fpn_extra_lvl=True, roi_height=7, roi_width=7,
           roi_spatial_scale=[0.25, 0.125, 0.0625, 0.03125], roi_sampling_ratio=2)
SIDES = (40.0, 150.0, 300.0, 600.0)           # one per level: sqrt(area) < 112 <= .. < 224 <= .. < 448 <= ..


def fpn_detector(seed, **kw):
    from detectorch_amd.model.detector import detector
    torch.manual_seed(seed)
    return detector(N_classes=5, **dict(FPN, **kw)).cuda()


def np_levels(boxes, k_min=2, k_max=5, margin=0.1):
    """multilevel_rois.py:41-53 with boxes_area's + 1 (boxes.py:77-79), in float64.  No row may come nearer than `margin` to a
    threshold: the kernel's float32 sqrt, division and log2 differ from these by parts in 10^6, so any margin of a few percent makes
    the level independent of the arithmetic."""
    b = np.asarray(boxes, np.float64)
    s = np.sqrt((b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1))
    assert (np.abs(s[:, None] / np.array([112.0, 224.0, 448.0]) - 1) >= margin).all()
    return (np.clip(np.floor(4 + np.log2(s / 224 + 1e-6)), k_min, k_max) - k_min).astype(np.int32)


def square_gt(rs, n_images):
    """Per image four boxes with sides near SIDES (+- 3 %)."""
    gt = np.zeros((n_images, 4, 4), np.float32)
    for b in range(n_images):
        for g, side in enumerate(SIDES):
            x, y = rs.uniform(0, 200, 2)
            w, h = side * rs.uniform(0.97, 1.03, 2)
            gt[b, g] = (x, y, x + w, y + h)
    return gt


def jittered(rs, gt, n):
    """n copies of random rows of gt [4,4], every coordinate moved by at most 4 % of the side: sqrt(area) stays within 8 + 3 % of it."""
    g = rs.randint(0, 4, n)
    return (gt[g] + rs.uniform(-0.04, 0.04, (n, 4)) * np.array(SIDES)[g][:, None]).astype(np.float32)


def test_roi_levels_batched():
    from detectorch_amd.utils.multilevel_rois import roi_levels_batched
    rs = synth.rng(83, 0)
    gt = square_gt(rs, 1)[0]
    N = 2048 + 5
    rows = np.concatenate([rs.randint(0, 2, (N, 1)).astype(np.float32), jittered(rs, gt, N)], 1)
    want = np_levels(rows[:, 1:])
    assert set(want.tolist()) == {0, 1, 2, 3}
    lv = roi_levels_batched(d(rows))
    assert lv.dtype == torch.int32 and tuple(lv.shape) == (N,) and np.array_equal(lv.cpu().numpy(), want)
    # the grouping cannot change a level: the same rows, one [1,R] group per chunk; four columns like five
    chunks = torch.cat([roi_levels_batched(d(rows[None, :2048])).reshape(-1), roi_levels_batched(d(rows[None, 2048:])).reshape(-1)])
    assert torch.equal(lv, chunks) and torch.equal(lv, roi_levels_batched(d(rows[:, 1:])))
    # a row with a non-finite coordinate gets level 0 and shifts nothing
    bad = np.nonzero(want[:20] > 0)[0][:3]
    assert len(bad) == 3
    holes = rows[:20].copy()
    holes[bad[0], 3], holes[bad[1], 4], holes[bad[2], 1] = np.nan, np.inf, -np.inf
    expect = want[:20].copy()
    expect[bad] = 0
    assert np.array_equal(roi_levels_batched(d(holes)).cpu().numpy(), expect)
    # batched with counts: level 0 past them, whatever the rows hold; all-zero rows inside them: level 0
    three = rows[:40].reshape(2, 20, 5).copy()
    three[1, 7:] = np.nan
    three[0, 5] = 0
    expect = want[:40].reshape(2, 20).copy()
    expect[1, 7:] = 0
    expect[0, 5] = 0
    got = roi_levels_batched(d(three), d([20, 7], torch.int32))
    assert tuple(got.shape) == (2, 20) and np.array_equal(got.cpu().numpy(), expect)
    assert tuple(roi_levels_batched(d(np.zeros((0, 5), np.float32))).shape) == (0,)
    with pytest.raises(ValueError):
        roi_levels_batched(d(np.zeros((1, 2049, 4), np.float32)))


def test_collect_sample_distribute():
    from detectorch_amd.model.collect_and_distribute_fpn_rpn_proposals import collect_sample_distribute
    from detectorch_amd.utils.fast_rcnn_sample_rois import sample_rois_batched
    from detectorch_amd.utils.multilevel_rois import roi_levels_batched
    rs = synth.rng(83, 1)
    B, L, P, T, R = 2, 5, 64, 120, 64
    counts = np.array([[40, 0, 64, 17, 5], [64, 33, 1, 0, 20]], np.int32)          # 126 > T and 118 < T rows; one level empty each
    gt_boxes = square_gt(rs, B)
    boxes = np.stack([jittered(rs, gt_boxes[b], L * P).reshape(L, P, 4) for b in range(B)])
    scores = (rs.permutation(B * L * P).reshape(B, L, P).astype(np.float32) + 1) / np.float32(B * L * P)      # distinct
    want = np.zeros((B, T, 4), np.float32)
    for b in range(B):
        cat_b = np.concatenate([boxes[b, l, :counts[b, l]] for l in range(L)])
        cat_s = np.concatenate([scores[b, l, :counts[b, l]] for l in range(L)])
        order = np.argsort(-cat_s, kind='stable')[:T]
        want[b, :len(order)] = cat_b[order]
        for l in range(L):                                                        # rows past the counts hold NaN
            boxes[b, l, counts[b, l]:] = np.nan
            scores[b, l, counts[b, l]:] = np.nan
    # image 1 counts three gt only: the proposals around its fourth box are background
    gt = dict(gt_boxes=d(gt_boxes), gt_classes=d([[1, 2, 3, 4], [4, 3, 2, 1]], torch.int32), gt_is_crowd=d(np.zeros((B, 4)), torch.int32),
              gt_counts=d([4, 3], torch.int32))
    keys = d(rs.randint(0, 2 ** 31 - 1, (B, 4 + T)), torch.int32)
    knobs = dict(rois_per_image=R, fg_fraction=0.5, num_classes=5)
    blobs = collect_sample_distribute(d(boxes), d(scores), d(counts, torch.int32), gt, post_nms_top_n=T, rand_keys=keys, **knobs)
    torch.cuda.synchronize()
    assert blobs["proposal_counts"].cpu().tolist() == [120, 118]
    assert np.array_equal(blobs["proposals"].cpu().numpy(), want)
    again = sample_rois_batched(blobs["proposals"], blobs["proposal_counts"], gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"],
                                gt["gt_counts"], torch.ones(B, device="cuda"), rand_keys=keys, expanded=False, **knobs)
    assert set(again) | {"roi_levels", "proposals", "proposal_counts"} == set(blobs)
    for k, v in again.items():
        assert (blobs[k] is None) if v is None else torch.equal(blobs[k], v), k
    rois, n_rois, lv = blobs["rois"].cpu().numpy(), blobs["n_rois"].cpu().tolist(), blobs["roi_levels"].cpu().numpy()
    assert lv.shape == (B, R) and lv.dtype == np.int32 and all(0 < n <= R for n in n_rois) and min(n_rois) < R
    seen = set()
    for b in range(B):
        n = n_rois[b]
        assert np.array_equal(lv[b, :n], np_levels(rois[b, :n, 1:])) and not lv[b, n:].any() and not rois[b, n:].any()
        seen |= set(lv[b, :n].tolist())
    assert seen == {0, 1, 2, 3}
    assert torch.equal(blobs["roi_levels"], roi_levels_batched(blobs["rois"], blobs["n_rois"]))
    for top_n in (0, 2049):
        with pytest.raises(ValueError):
            collect_sample_distribute(d(boxes), d(scores), d(counts, torch.int32), gt, post_nms_top_n=top_n, rand_keys=keys, **knobs)


# ten rois5 on a 64 x 96 image: levels 0 1 2 3 in mixed order, boxes that reach outside the map (level 3 needs sides of 448 or more),
# fractional coordinates, one all-zero padding row
ROIS10 = np.array([[0, 30.5, 12.25, 70.75, 50.5], [0, -200, -200, 300, 300], [0, -20, -30, 120, 100], [0, 10, 5, 300, 290],
                   [0, 10, 8, 80, 60], [0, 0, 0, 0, 0], [0, 0, 0, 600, 500], [0, -100, -80, 180, 200], [0, 0, 0, 150, 150],
                   [0, 0, 0, 95, 63]], np.float32)
LEVELS10 = [0, 3, 1, 2, 0, 0, 3, 2, 1, 0]


def test_forward_train_boxes_equals_the_level_by_level_route():
    from detectorch_amd.model.roi_align import RoIAlign, roi_align_fpn
    from detectorch_amd.utils.multilevel_rois import roi_levels_batched
    model = fpn_detector(7, use_rpn_head=True)
    rs = synth.rng(83, 2)
    images = torch.from_numpy(rs.standard_normal((1, 3, 64, 96)).astype(np.float32)).cuda()
    with torch.no_grad():
        maps = model.conv_body(images)
    assert [tuple(f.shape[2:]) for f in maps] == [(16, 24), (8, 12), (4, 6), (2, 3)]
    rois = d(ROIS10)
    levels = roi_levels_batched(rois)
    assert levels.cpu().tolist() == LEVELS10 == np_levels(ROIS10[:, 1:]).tolist()
    scales = model.roi_spatial_scale
    # the multi-level route: one launch forward, one call backward
    feats = [f.clone().requires_grad_() for f in maps]
    pooled = roi_align_fpn(feats, scales, rois, levels, 7, 7, 2)
    # the reference's route: the single-level RoIAlign module per level on that level's rows, concatenated and restored
    feats_ref = [f.clone().requires_grad_() for f in maps]
    idx = [torch.nonzero(levels == l)[:, 0] for l in range(4)]
    assert all(len(i) >= 2 for i in idx)
    by_level = torch.cat([RoIAlign(7, 7, scales[l], 2)(feats_ref[l], rois[idx[l]]) for l in range(4)], 0)
    restore = torch.argsort(torch.cat(idx))
    pooled_ref = by_level[restore]
    assert tuple(pooled.shape) == (10, 256, 7, 7) and torch.equal(pooled, pooled_ref)
    assert float(pooled.detach().abs().max()) > 0
    up = torch.from_numpy(rs.standard_normal((10, 256, 7, 7)).astype(np.float32)).cuda()
    grads = torch.autograd.grad(pooled, feats, up)
    grads_ref = torch.autograd.grad(pooled_ref, feats_ref, up)
    for l in range(4):
        assert torch.equal(grads[l], grads_ref[l]) and float(grads[l].abs().max()) > 0, l
    # forward_train_boxes: the heads on those pooled features; the levels it computes itself are the explicit ones
    cls_score, bbox_pred = model.forward_train_boxes(maps, rois, levels)
    x = model._head(pooled_ref.detach())
    assert torch.equal(cls_score, model.classif_head(x)) and torch.equal(bbox_pred, model.bbox_head(x))
    assert tuple(cls_score.shape) == (10, 5) and tuple(bbox_pred.shape) == (10, 20) and cls_score.requires_grad
    cls_none, bbox_none = model.forward_train_boxes(maps, rois)
    assert torch.equal(cls_none, cls_score) and torch.equal(bbox_none, bbox_pred)


def test_fast_rcnn_train_step_on_the_fpn_model():
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import fast_rcnn_train_step, freeze_stem
    from detectorch_amd.utils.fast_rcnn_sample_rois import sample_rois_batched
    from detectorch_amd.utils.multilevel_rois import roi_levels_batched
    model = fpn_detector(12)                                                                   # Fast R-CNN FPN: no RPN head, no mask head
    trainable = freeze_stem(model)
    opt = ClippedSGD(trainable, lr=0.01)
    rs = synth.rng(83, 3)
    B, P = 2, 40
    images = torch.from_numpy(rs.standard_normal((B, 3, 64, 96)).astype(np.float32)).cuda()
    gt_boxes = np.array([[[8, 6, 60, 50], [40, 20, 90, 60]], [[2, 2, 93, 61], [30, 10, 70, 40]]], np.float32)
    # given proposals: around the gt, and of every level's size around the image (RoIAlign reads zeros outside the map)
    props = np.stack([np.concatenate([gt_boxes[b][rs.randint(0, 2, P // 2)] + rs.uniform(-6, 6, (P // 2, 4)),
                                      jittered(rs, square_gt(rs, 1)[0] - 100, P - P // 2)]) for b in range(B)]).astype(np.float32)
    blobs = sample_rois_batched(d(props), d([P, P - 3], torch.int32), d(gt_boxes), d([[1, 3], [2, 4]], torch.int32),
                                d(np.zeros((B, 2)), torch.int32), d([2, 2], torch.int32), torch.ones(B, device="cuda"),
                                rand_keys=d(rs.randint(0, 2 ** 31 - 1, (B, 2 + P)), torch.int32), rois_per_image=16, num_classes=5,
                                expanded=False)
    names = {id(p): n for n, p in model.named_parameters()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss_cls, loss_bbox, acc = fast_rcnn_train_step(model, opt, images, blobs, it=0)
    torch.cuda.synchronize()
    print("loss_cls %r loss_bbox %r accuracy %r" % (float(loss_cls), float(loss_bbox), float(acc)))
    assert np.isfinite(float(loss_cls)) and np.isfinite(float(loss_bbox)) and float(loss_cls) > 0 and 0.0 <= float(acc) <= 1.0
    assert int(blobs["n_fg"].min()) >= 1 and len(set(roi_levels_batched(blobs["rois"], blobs["n_rois"]).reshape(-1).tolist())) > 1
    check_sgd_step(model, opt, trainable, before, names)
    for m in [model.conv_head.fc6, model.conv_head.fc7, model.bbox_head, model.classif_head] + list(model.conv_body.fpn_lateral):
        assert m.weight.grad is not None and bool(torch.isfinite(m.weight.grad).all()) and float(m.weight.grad.abs().max()) > 0
    assert len(model.conv_body.fpn_lateral) == 4


# four gt per image in blob coordinates, one per level, inside each image's own size (480 x 512 and 448 x 512)
GT_BLOB = np.array([[[30, 40, 90, 110], [200, 60, 370, 220], [40, 150, 330, 420], [4, 4, 505, 470]],
                    [[300, 30, 380, 100], [60, 80, 220, 250], [150, 100, 470, 400], [4, 4, 505, 443]]], np.float32)
TOP_N, ROIS_PER_IM = 300, 16


def joint_inputs(seed):
    rs = synth.rng(83, seed)
    images = torch.from_numpy(rs.standard_normal((2, 3, 480, 512)).astype(np.float32)).cuda()
    scale = np.array([1.0, 0.8], np.float32)
    # a box inside a 448 x 512 image cannot be 10 % above 448 (sqrt(449 * 513) = 480): 4 % here
    assert np_levels(GT_BLOB.reshape(-1, 4), margin=0.04).tolist() == [0, 1, 2, 3] * 2
    # the sampling keys: ascending (key, index) order inside the foreground, so with the smallest keys on the gt columns the four gt
    # of an image (IoU 1 with themselves) are sampled whatever the RPN proposes, as long as the foreground quota is at least four
    keys = rs.randint(2 ** 20, 2 ** 31 - 1, (2, 4 + TOP_N))
    keys[:, :4] = rs.randint(0, 2 ** 20, (2, 4))
    gt = dict(gt_boxes=d(GT_BLOB / scale[:, None, None]), gt_classes=d([[1, 3, 2, 4], [4, 1, 3, 2]], torch.int32),
              gt_is_crowd=d(np.zeros((2, 4)), torch.int32), gt_counts=d([4, 4], torch.int32), im_scale=d(scale),
              im_hw=d([[480.0, 512.0], [448.0, 512.0]]), rand_keys=d(keys, torch.int32))
    return rs, images, gt


STEP = dict(rpn_knobs=dict(batch_size_per_im=16), post_nms_top_n=TOP_N, pre_nms_top_n=2000, rois_per_image=ROIS_PER_IM, fg_fraction=0.5)


def check_joint_blobs(model, blobs, gt):
    """What both joint steps promise about the minibatch: the eager recomputation, the levels, the coverage."""
    from detectorch_amd.utils.fast_rcnn_sample_rois import sample_rois_batched
    from detectorch_amd.utils.multilevel_rois import roi_levels_batched
    assert tuple(blobs["proposals"].shape) == (2, TOP_N, 4) and all(0 < n <= TOP_N for n in blobs["proposal_counts"].cpu().tolist())
    gt_blob = gt["gt_boxes"] * gt["im_scale"].reshape(2, 1, 1)
    again = sample_rois_batched(blobs["proposals"], blobs["proposal_counts"].contiguous(), gt_blob, gt["gt_classes"], gt["gt_is_crowd"],
                                gt["gt_counts"], torch.ones_like(gt["im_scale"]), rand_keys=gt["rand_keys"], rois_per_image=ROIS_PER_IM,
                                fg_fraction=0.5, num_classes=5, expanded=False)
    torch.cuda.synchronize()
    assert torch.equal(again["rois"], blobs["rois"]) and torch.equal(again["labels_int32"], blobs["labels_int32"])
    assert tuple(blobs["rois"].shape) == (2, ROIS_PER_IM, 5) and tuple(blobs["roi_levels"].shape) == (2, ROIS_PER_IM)
    assert torch.equal(blobs["roi_levels"], roi_levels_batched(blobs["rois"], blobs["n_rois"]))
    lv, n_rois, keep = blobs["roi_levels"].cpu().numpy(), blobs["n_rois"].cpu().tolist(), blobs["keep_inds"].cpu().numpy()
    for b in range(2):
        assert set(range(4)) <= set(keep[b, :n_rois[b]].tolist())                              # every gt row was sampled
        assert set(lv[b, :n_rois[b]].tolist()) == {0, 1, 2, 3} and int(blobs["n_fg"][b]) >= 4  # so all four levels occur, per image
        rows = [int(np.nonzero(keep[b] == g)[0][0]) for g in range(4)]
        assert np.array_equal(blobs["rois"][b].cpu().numpy()[rows, 1:], gt_blob[b].cpu().numpy()) and lv[b, rows].tolist() == [0, 1, 2, 3]


def check_joint_grads(model):
    mods = [model.rpn.conv_rpn, model.rpn.rpn_cls_prob, model.conv_head.fc6, model.conv_head.fc7, model.bbox_head, model.classif_head,
            model.model.layer2[0].conv1] + list(model.conv_body.fpn_lateral) + list(model.conv_body.fpn_output)
    assert len(model.conv_body.fpn_lateral) == 4
    for m in mods:
        assert m.weight.grad is not None and bool(torch.isfinite(m.weight.grad).all()) and float(m.weight.grad.abs().max()) > 0


def test_faster_rcnn_train_step_on_the_fpn_model():
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import faster_rcnn_train_step, freeze_stem
    from detectorch_amd.utils.solver import get_lr_at_iter
    model = fpn_detector(13, use_rpn_head=True)
    trainable = freeze_stem(model)
    opt = ClippedSGD(trainable, lr=0.01)
    rs, images, gt = joint_inputs(4)
    names = {id(p): n for n, p in model.named_parameters()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    out = faster_rcnn_train_step(model, opt, images, gt, it=0, **STEP)
    torch.cuda.synchronize()
    losses, acc, blobs = [float(v) for v in out[:4]], float(out[4]), out[5]
    print("loss_rpn_cls %r loss_rpn_bbox %r loss_cls %r loss_bbox %r accuracy %r" % (*losses, acc))
    assert len(out) == 6 and all(np.isfinite(v) for v in losses) and losses[0] > 0 and losses[2] > 0 and losses[3] > 0 and 0.0 <= acc <= 1.0
    assert opt.param_groups[0]['lr'] == get_lr_at_iter(0) < 0.01
    lr = check_sgd_step(model, opt, trainable, before, names)
    check_joint_grads(model)
    check_joint_blobs(model, blobs, gt)
    faster_rcnn_train_step(model, opt, images, gt, it=1, **STEP)                               # a second step runs
    torch.cuda.synchronize()
    assert np.isfinite(opt.stats.cpu().numpy()).all() and opt.param_groups[0]['lr'] == get_lr_at_iter(1) > float(lr)
    model_out = model(images[:1])                                                              # forward of the trained model runs
    torch.cuda.synchronize()
    assert model_out[0].shape[1] == 5 and bool(torch.isfinite(model_out[0]).all()) and not model_out[0].requires_grad


def test_mask_rcnn_train_step_on_the_fpn_model():
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import freeze_stem, mask_rcnn_train_step
    from detectorch_amd.utils.mask_rcnn_targets import pack_polygons
    from detectorch_amd.utils.solver import get_lr_at_iter
    model = fpn_detector(14, use_rpn_head=True, use_mask_head=True, mask_head_type='1up4convs')
    trainable = freeze_stem(model)
    opt = ClippedSGD(trainable, lr=0.01)
    rs, images, gt = joint_inputs(5)
    # per gt, in original coordinates like gt_boxes: an octagon inside the box; the last gt of an image a triangle and a rectangle
    polys = []
    for boxes in gt["gt_boxes"].cpu().numpy().tolist():
        per = []
        for g, (x1, y1, x2, y2) in enumerate(boxes):
            cx, cy, qx, qy = (x1 + x2) / 2, (y1 + y2) / 2, (x2 - x1) / 4, (y2 - y1) / 4
            if g < 3:
                per.append([[x1 + qx, y1, x2 - qx, y1, x2, y1 + qy, x2, y2 - qy, x2 - qx, y2, x1 + qx, y2, x1, y2 - qy, x1, y1 + qy]])
            else:
                per.append([[x1, y1, cx, cy, x1, y2], [cx, y1 + qy, x2, y1 + qy, x2, y2 - qy, cx, y2 - qy]])
        polys.append(per)
    gt["poly_xy"], gt["poly_ptr"], gt["gt_poly_ptr"] = pack_polygons(polys, 4, device="cuda")
    names = {id(p): n for n, p in model.named_parameters()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    out = mask_rcnn_train_step(model, opt, images, gt, it=0, **STEP)
    torch.cuda.synchronize()
    losses, acc, blobs = [float(v) for v in out[:5]], float(out[5]), out[6]
    print("loss_rpn_cls %r loss_rpn_bbox %r loss_cls %r loss_bbox %r loss_mask %r accuracy %r" % (*losses, acc))
    assert len(out) == 7 and all(np.isfinite(v) for v in losses) and losses[0] > 0 and losses[2] > 0 and losses[4] > 0 and 0.0 <= acc <= 1.0
    lr = check_sgd_step(model, opt, trainable, before, names)
    check_joint_grads(model)
    mh = model.mask_head
    for m in (mh.conv_head.fcn1, mh.conv_head.fcn2, mh.conv_head.fcn3, mh.conv_head.fcn4, mh.transposed_conv, mh.classif_logits):
        assert m.weight.grad is not None and bool(torch.isfinite(m.weight.grad).all()) and float(m.weight.grad.abs().max()) > 0
    check_joint_blobs(model, blobs, gt)
    # Fm = the foreground quota (half of 16), M = 28; mask_rois: the foreground rows of the minibatch's own rois bit for bit, and
    # their levels
    Fm = ROIS_PER_IM // 2
    assert tuple(blobs["mask_rois"].shape) == (2, Fm, 5) and tuple(blobs["masks_int32"].shape) == (2, Fm, 784)
    assert tuple(blobs["mask_roi_levels"].shape) == (2, Fm)
    for b in range(2):
        n, n_fg = int(blobs["n_mask"][b]), int(blobs["n_fg"][b])
        assert 4 <= n == n_fg <= Fm
        rows = torch.nonzero(blobs["roi_has_mask_int32"][b] == 1)[:, 0]
        assert torch.equal(blobs["mask_rois"][b, :n], blobs["rois"][b][rows]) and bool((blobs["labels_int32"][b][rows] > 0).all())
        assert torch.equal(blobs["mask_roi_levels"][b, :n], blobs["roi_levels"][b][rows])
        assert set(blobs["mask_roi_levels"][b, :n].cpu().tolist()) == {0, 1, 2, 3}
        assert torch.equal(blobs["mask_class_labels"][b, :n], blobs["labels_int32"][b][rows])
        m = blobs["masks_int32"][b]
        assert bool(((m[:n] == 0) | (m[:n] == 1)).all()) and bool((m[n:] == -1).all()) and int((m[:n] == 1).sum()) > 0
    mask_rcnn_train_step(model, opt, images, gt, it=1, **STEP)                                 # a second step runs
    torch.cuda.synchronize()
    assert np.isfinite(opt.stats.cpu().numpy()).all() and opt.param_groups[0]['lr'] == get_lr_at_iter(1) > float(lr)
    model_out = model(images[:1])
    torch.cuda.synchronize()
    assert model_out[0].shape[1] == 5 and bool(torch.isfinite(model_out[0]).all())
