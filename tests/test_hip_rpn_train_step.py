"""rpn_train_step, forward_train_rpn on the FPN model and faster_rcnn_train_step on the MI355X (-m gpu); the checks follow
test_fast_rcnn_train_step (tests/test_hip_optim.py): finite losses, frozen parameters bit-unchanged, every trainable parameter and
momentum buffer BIT-equal to the numpy restatement of the clipped SGD step (tests/optim_ref.py) applied to a saved copy and its
.grad, gradients where they have to be and nowhere else."""
import numpy as np
import pytest
import torch

import optim_ref as orf
from detectorch_amd import synth

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def d(a, t=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a)).to("cuda", t)


def inputs(seed):
    rs = synth.rng(81, seed)
    images = torch.from_numpy(rs.standard_normal((1, 3, 64, 96)).astype(np.float32)).cuda()
    gt = dict(gt_boxes=d(np.array([[[8, 6, 60, 50], [40, 20, 90, 60]]], np.float32)), gt_classes=d([[1, 3]], torch.int32),
              gt_is_crowd=d([[0, 0]], torch.int32), gt_counts=d([2], torch.int32), im_scale=d([1.0]), im_hw=d([[64.0, 96.0]]))
    return rs, images, gt


def check_sgd_step(model, opt, trainable, before, names):
    total, coef = opt.stats.cpu().numpy()[:2]
    assert same(coef, orf.coef32(total, 35.0)) and np.isfinite(total) and total > 0
    frozen = [n for n, p in model.named_parameters() if not p.requires_grad]
    assert frozen and all(torch.equal(before[n], dict(model.named_parameters())[n]) for n in frozen)
    assert all(p.grad is None for n, p in model.named_parameters() if not p.requires_grad)
    stepped = [p for p in trainable if p.grad is not None]
    grads = [p.grad.cpu().numpy().ravel() for p in stepped]
    assert abs(float(total) - orf.norm64(grads)) <= float(np.spacing(np.float32(orf.norm64(grads))))
    want_p = [before[names[id(p)]].cpu().numpy().ravel().copy() for p in stepped]
    want_b = [np.zeros_like(a) for a in want_p]
    lr = np.float32(opt.param_groups[0]['lr'])
    orf.step32(want_p, grads, want_b, coef, [(lr, 1e-4)], [0] * len(stepped), 0.9)
    for p, a, b in zip(stepped, want_p, want_b):
        assert same(p.detach().cpu().numpy().ravel(), a), names[id(p)]
        assert same(opt.state[p]['momentum_buffer'].cpu().numpy().ravel(), b), names[id(p)]
    for p in trainable:                                                                        # no gradient: untouched
        if p.grad is None:
            assert torch.equal(before[names[id(p)]], p.detach()), names[id(p)]
    return lr


def test_rpn_train_step():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import freeze_stem, rpn_train_step
    from detectorch_amd.utils.solver import get_lr_at_iter
    torch.manual_seed(6)
    model = detector(N_classes=5, use_rpn_head=True).cuda()
    trainable = freeze_stem(model)
    opt = ClippedSGD(trainable, lr=0.01)
    _, images, gt = inputs(0)
    names = {id(p): n for n, p in model.named_parameters()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss_cls, loss_bbox = rpn_train_step(model, opt, images, gt, it=0, batch_size_per_im=16)
    torch.cuda.synchronize()
    print("loss_rpn_cls %r loss_rpn_bbox %r stats %r" % (float(loss_cls), float(loss_bbox), opt.stats.cpu().numpy()))
    assert np.isfinite(float(loss_cls)) and np.isfinite(float(loss_bbox)) and float(loss_cls) > 0 and float(loss_bbox) >= 0
    assert opt.param_groups[0]['lr'] == get_lr_at_iter(0) < 0.01                               # the solver's warm-up
    lr = check_sgd_step(model, opt, trainable, before, names)
    assert float(model.rpn.conv_rpn.weight.grad.abs().max()) > 0 and float(model.model.layer2[0].conv1.weight.grad.abs().max()) > 0
    assert float(model.rpn.rpn_bbox_pred.weight.grad.abs().max()) > 0                          # a foreground anchor was sampled
    assert model.bbox_head.weight.grad is None and model.classif_head.weight.grad is None      # the box head takes no part
    rpn_train_step(model, opt, images, gt, it=1, batch_size_per_im=16)                         # a second step runs
    torch.cuda.synchronize()
    assert np.isfinite(opt.stats.cpu().numpy()).all() and opt.param_groups[0]['lr'] > float(lr)
    with pytest.raises(NotImplementedError):
        detector(N_classes=5).forward_train_rpn(images)                                        # no RPN head: refused before any work


def test_fpn_forward_train_rpn_and_losses():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.model.loss import rpn_losses
    from detectorch_amd.utils.rpn_targets import rpn_targets_batched
    torch.manual_seed(7)
    model = detector(N_classes=5, use_rpn_head=True, conv_body_layers=['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'],
                     conv_head_layers='two_layer_mlp', fpn_layers=['layer1', 'layer2', 'layer3', 'layer4'], fpn_extra_lvl=True,
                     roi_height=7, roi_width=7, roi_spatial_scale=[0.25, 0.125, 0.0625, 0.03125], roi_sampling_ratio=2).cuda()
    rs, _, gt = inputs(1)
    images = torch.from_numpy(rs.standard_normal((1, 3, 64, 96)).astype(np.float32)).cuda()
    cls, box, feats = model.forward_train_rpn(images)
    assert len(cls) == len(box) == 5 and len(feats) == 4                                      # the extra pooled level is an RPN level
    assert [tuple(c.shape) for c in cls] == [(1, 3, 16, 24), (1, 3, 8, 12), (1, 3, 4, 6), (1, 3, 2, 3), (1, 3, 1, 2)]
    assert all(c.dtype == torch.float32 and c.requires_grad for c in cls + box)
    blobs = rpn_targets_batched(model.rpn_train_levels(cls), gt["gt_boxes"], gt["gt_is_crowd"], gt["gt_counts"], gt["im_scale"],
                                gt["im_hw"], batch_size_per_im=16, straddle_thresh=-1.0)
    loss_cls, loss_bbox = rpn_losses(cls, box, blobs)
    (loss_cls + loss_bbox).backward()
    torch.cuda.synchronize()
    assert int(blobs["n_fg"][0]) >= 1 and int(blobs["n_fg"][0]) + int(blobs["n_bg"][0]) == 16
    loss_cls, loss_bbox = loss_cls.detach(), loss_bbox.detach()
    assert np.isfinite(float(loss_cls)) and np.isfinite(float(loss_bbox)) and float(loss_cls) > 0
    for conv in model.conv_body.fpn_lateral:
        gr = conv.weight.grad
        assert gr is not None and bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0
    assert model.bbox_head.weight.grad is None


def test_faster_rcnn_train_step():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.optim import ClippedSGD
    from detectorch_amd.train import faster_rcnn_train_step, freeze_stem
    from detectorch_amd.utils.fast_rcnn_sample_rois import sample_rois_batched
    torch.manual_seed(8)
    model = detector(N_classes=5, use_rpn_head=True).cuda()
    trainable = freeze_stem(model)
    opt = ClippedSGD(trainable, lr=0.01)
    rs, images, gt = inputs(2)
    gt["rand_keys"] = d(rs.randint(0, 2 ** 31 - 1, (1, 2 + 300)), torch.int32)
    names = {id(p): n for n, p in model.named_parameters()}
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    out = faster_rcnn_train_step(model, opt, images, gt, it=0, rpn_knobs=dict(batch_size_per_im=16), post_nms_top_n=300,
                                 rois_per_image=16)
    torch.cuda.synchronize()
    losses, acc, blobs = [float(v) for v in out[:4]], float(out[4]), out[5]
    print("loss_rpn_cls %r loss_rpn_bbox %r loss_cls %r loss_bbox %r accuracy %r" % (*losses, acc))
    assert all(np.isfinite(v) for v in losses) and losses[0] > 0 and losses[2] > 0 and 0.0 <= acc <= 1.0
    check_sgd_step(model, opt, trainable, before, names)
    for p in (model.rpn.conv_rpn.weight, model.bbox_head.weight, model.classif_head.weight, model.model.layer2[0].conv1.weight):
        assert p.grad is not None and float(p.grad.abs().max()) > 0
    # blobs['rois'] from an eager recomputation on the proposals of that forward: gt and proposals in blob coordinates, im_scale 1
    assert blobs["proposals"].shape == (1, 300, 4) and 0 < int(blobs["proposal_counts"][0]) <= 300
    again = sample_rois_batched(blobs["proposals"], blobs["proposal_counts"].contiguous(), gt["gt_boxes"] * gt["im_scale"].reshape(1, 1, 1),
                                gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"], torch.ones_like(gt["im_scale"]),
                                rand_keys=gt["rand_keys"], rois_per_image=16, num_classes=5, expanded=False)
    torch.cuda.synchronize()
    assert torch.equal(again["rois"], blobs["rois"]) and torch.equal(again["labels_int32"], blobs["labels_int32"])
    assert blobs["rois"].shape == (1, 16, 5) and int(blobs["n_fg"][0]) >= 1                    # the gt rows are candidates
    # forward of the trained model runs
    model_out = model(images, scaling_factor=torch.tensor([1.0]))
    torch.cuda.synchronize()
    assert model_out[0].shape[1] == 5 and bool(torch.isfinite(model_out[0]).all()) and not model_out[0].requires_grad
