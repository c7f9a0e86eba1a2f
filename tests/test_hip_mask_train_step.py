"""mask_rcnn_train_step on the C4 model and forward_train_mask + mask_rcnn_loss on the FPN model, on the MI355X (-m gpu); the checks
follow test_faster_rcnn_train_step (tests/test_hip_rpn_train_step.py): finite losses, frozen parameters bit-unchanged, every
trainable parameter and momentum buffer BIT-equal to the numpy restatement of the clipped SGD step (tests/optim_ref.py), gradients
where they have to be."""
import numpy as np
import pytest
import torch

from test_hip_rpn_train_step import check_sgd_step, d, inputs

pytestmark = pytest.mark.gpu


def test_mask_rcnn_train_step():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import freeze_stem, mask_rcnn_train_step
    from detectorch_amd.utils.mask_rcnn_targets import pack_polygons
    torch.manual_seed(9)
    model = detector(N_classes=5, use_rpn_head=True, use_mask_head=True).cuda()
    trainable = freeze_stem(model)
    opt = ClippedSGD(trainable, lr=0.01)
    rs, images, gt = inputs(3)
    gt["rand_keys"] = d(rs.randint(0, 2 ** 31 - 1, (1, 2 + 300)), torch.int32)
    # the two gt of inputs(): an octagon inside the first box, a triangle and a rectangle inside the second
    polys = [[[[20, 6, 48, 6, 60, 18, 60, 38, 48, 50, 20, 50, 8, 38, 8, 18]], [[40, 20, 90, 40, 40, 60], [60, 30, 85, 30, 85, 55, 60, 55]]]]
    gt["poly_xy"], gt["poly_ptr"], gt["gt_poly_ptr"] = pack_polygons(polys, 2, device="cuda")
    names = {id(p): n for n, p in model.named_parameters()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    out = mask_rcnn_train_step(model, opt, images, gt, it=0, rpn_knobs=dict(batch_size_per_im=16), post_nms_top_n=300, rois_per_image=16)
    torch.cuda.synchronize()
    losses, acc, blobs = [float(v) for v in out[:5]], float(out[5]), out[6]
    print("loss_rpn_cls %r loss_rpn_bbox %r loss_cls %r loss_bbox %r loss_mask %r accuracy %r" % (*losses, acc))
    assert all(np.isfinite(v) for v in losses) and losses[0] > 0 and losses[2] > 0 and losses[4] > 0 and 0.0 <= acc <= 1.0
    check_sgd_step(model, opt, trainable, before, names)
    mh = model.mask_head
    for p in (mh.transposed_conv.weight, mh.classif_logits.weight, mh.classif_logits.bias, model.rpn.conv_rpn.weight, model.bbox_head.weight,
              model.model.layer2[0].conv1.weight, model.model.layer4[0].conv1.weight):
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
    # mask_rois: the foreground rows of the minibatch's own rois, bit for bit; Fm = the foreground quota; M = 14
    n, n_fg = int(blobs["n_mask"][0]), int(blobs["n_fg"][0])
    assert blobs["mask_rois"].shape == (1, 4, 5) and blobs["masks_int32"].shape == (1, 4, 196) and 1 <= n == n_fg <= 4
    rows = torch.nonzero(blobs["roi_has_mask_int32"][0] == 1)[:, 0]
    assert torch.equal(blobs["mask_rois"][0, :n], blobs["rois"][0][rows]) and bool((blobs["labels_int32"][0][rows] > 0).all())
    assert torch.equal(blobs["mask_class_labels"][0, :n], blobs["labels_int32"][0][rows])
    m = blobs["masks_int32"][0]
    assert bool(((m[:n] == 0) | (m[:n] == 1)).all()) and bool((m[n:] == -1).all()) and int((m[:n] == 1).sum()) > 0
    lr = opt.param_groups[0]['lr']
    mask_rcnn_train_step(model, opt, images, gt, it=1, rpn_knobs=dict(batch_size_per_im=16), post_nms_top_n=300, rois_per_image=16)
    torch.cuda.synchronize()                                                                   # a second step runs
    assert np.isfinite(opt.stats.cpu().numpy()).all() and opt.param_groups[0]['lr'] > float(lr)
    plain = detector(N_classes=5, use_rpn_head=True)
    with pytest.raises(NotImplementedError):
        mask_rcnn_train_step(plain, None, images, gt, it=0)                                    # no mask head: refused before any work
    with pytest.raises(NotImplementedError):
        plain.forward_train_mask(torch.zeros(1, 1024, 4, 6), torch.zeros(1, 5))


def test_fpn_forward_train_mask_and_loss():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.model.loss import mask_rcnn_loss
    torch.manual_seed(11)
    model = detector(N_classes=5, use_rpn_head=True, use_mask_head=True, mask_head_type='1up4convs',
                     conv_body_layers=['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'],
                     conv_head_layers='two_layer_mlp', fpn_layers=['layer1', 'layer2', 'layer3', 'layer4'], fpn_extra_lvl=True,
                     roi_height=7, roi_width=7, roi_spatial_scale=[0.25, 0.125, 0.0625, 0.03125], roi_sampling_ratio=2).cuda()
    rs, images, _ = inputs(5)
    feats = model.conv_body(images)
    mask_rois = d(np.array([[0, 4, 4, 40, 30], [0, 10, 8, 80, 60], [0, 0, 0, 95, 63], [0, 20, 10, 90, 60], [0, 0, 0, 0, 0]], np.float32))
    levels = d([0, 1, 2, 3, 0], torch.int32)
    logits = model.forward_train_mask(feats, mask_rois, levels)
    assert tuple(logits.shape) == (5, 81, 28, 28) and logits.dtype == torch.float32 and logits.requires_grad
    masks = torch.from_numpy(rs.randint(0, 2, (1, 5, 784)).astype(np.int32)).cuda()
    masks[0, 4] = -1                                                                           # a padding row
    blobs = dict(masks_int32=masks, mask_class_labels=d([[1, 4, 2, 3, 0]], torch.int32))
    loss = mask_rcnn_loss(logits, blobs)
    loss.backward()
    torch.cuda.synchronize()
    assert np.isfinite(float(loss)) and float(loss) > 0
    mh = model.mask_head
    for conv in list(model.conv_body.fpn_lateral) + [mh.conv_head.fcn1, mh.conv_head.fcn2, mh.conv_head.fcn3, mh.conv_head.fcn4,
                                                    mh.transposed_conv, mh.classif_logits]:
        gr = conv.weight.grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0
    assert len(model.conv_body.fpn_lateral) == 4 and model.bbox_head.weight.grad is None
    with pytest.raises(ValueError):
        model.forward_train_mask(feats, mask_rois)                                             # FPN needs the levels
