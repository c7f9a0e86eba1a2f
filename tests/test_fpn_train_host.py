"""The training path of the FPN models without a GPU: what forward_train_boxes, the FPN arm of forward_train and the joint steps
refuse, and in which order (a refusal comes before any work: before the optimizer is touched, before a tensor is read).  The models
are built on the CPU; the GPU side is tests/test_hip_fpn_train_step.py."""
import pytest
import torch

FPN = dict(conv_body_layers=['conv1', 'bn1', 'relu', 'maxpool', 'layer1', 'layer2', 'layer3', 'layer4'], conv_head_layers='two_layer_mlp',
           fpn_layers=['layer1', 'layer2', 'layer3', 'layer4'], fpn_extra_lvl=True, roi_height=7, roi_width=7,
           roi_spatial_scale=[0.25, 0.125, 0.0625, 0.03125], roi_sampling_ratio=2)


def fpn_model(**kw):
    from detectorch_amd.model.detector import detector
    return detector(N_classes=5, **dict(FPN, **kw))


@pytest.fixture(scope="module")
def fast_fpn():
    return fpn_model()


@pytest.fixture(scope="module")
def faster_fpn():
    return fpn_model(use_rpn_head=True)


def feats_cpu():
    return [torch.zeros(1, 256, 64 >> k, 96 >> k) for k in range(2, 6)]


def gt_cpu():
    i32 = torch.int32
    return dict(gt_boxes=torch.tensor([[[8., 6., 60., 50.]]]), gt_classes=torch.tensor([[1]], dtype=i32), gt_is_crowd=torch.zeros(1, 1, dtype=i32),
                gt_counts=torch.ones(1, dtype=i32), im_scale=torch.ones(1), im_hw=torch.tensor([[64., 96.]]))


def test_level_range_of_the_fpn_scales(fast_fpn, faster_fpn):
    assert fast_fpn.roi_level_range() == (2, 5) and faster_fpn.roi_level_range() == (2, 5)
    assert fast_fpn.use_fpn_body and fast_fpn.use_two_layer_mlp_head and not fast_fpn.use_rpn_head and not fast_fpn.use_mask_head


def test_cpu_tensors_are_refused(fast_fpn, faster_fpn):
    from detectorch_amd.model.detector import detector
    from detectorch_amd.utils.multilevel_rois import roi_levels_batched
    rois = torch.zeros(4, 5)
    for model in (fast_fpn, faster_fpn):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.forward_train_boxes(feats_cpu(), rois)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            model.forward_train_boxes(feats_cpu(), rois, torch.zeros(4, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fast_fpn.forward_train(torch.zeros(1, 3, 64, 96), rois)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        detector(N_classes=5).forward_train_boxes(torch.zeros(1, 1024, 4, 6), rois)             # the C4 arm
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        roi_levels_batched(rois)


def test_the_refusals_of_forward_train_stay(fast_fpn, faster_fpn):
    from detectorch_amd.model.detector import detector
    images, rois = torch.zeros(1, 3, 64, 96), torch.zeros(4, 5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                  # the two of tests/test_optim_host.py
        detector(N_classes=5).forward_train(images, rois)
    with pytest.raises(NotImplementedError, match="forward_train covers"):
        detector(N_classes=5, use_rpn_head=True).forward_train(images, rois)
    with pytest.raises(NotImplementedError, match="forward_train covers"):                      # FPN with an RPN head: the joint step's model
        faster_fpn.forward_train(images, rois)
    with pytest.raises(NotImplementedError, match="forward_train covers"):                      # FPN body, res5 head
        detector(N_classes=5, conv_body_layers=FPN['conv_body_layers'][:-1], fpn_layers=['layer1', 'layer2', 'layer3'],
                 roi_spatial_scale=[0.25, 0.125, 0.0625]).forward_train(images, rois)
    with pytest.raises(NotImplementedError, match="forward_train covers"):                      # C4 body, MLP head
        detector(N_classes=5, conv_head_layers='two_layer_mlp').forward_train(images, rois)


@pytest.mark.parametrize("kw", [dict(head_dtype=torch.bfloat16), dict(backbone_dtype=torch.float16, head_dtype=torch.float16),
                                dict(channels_last=True)], ids=["head_bf16", "fp16", "channels_last"])
def test_16_bit_and_channels_last_models_are_refused(kw):
    model = fpn_model(**kw)
    with pytest.raises(NotImplementedError, match="forward_train covers"):
        model.forward_train(torch.zeros(1, 3, 64, 96), torch.zeros(4, 5))
    with pytest.raises(NotImplementedError, match="forward_train_boxes covers"):
        model.forward_train_boxes(feats_cpu(), torch.zeros(4, 5), torch.zeros(4, dtype=torch.int32))


def test_optimised_models_are_refused():
    model = fpn_model(use_rpn_head=True).optimize_for_inference()
    with pytest.raises(NotImplementedError, match="forward_train_boxes covers"):
        model.forward_train_boxes(feats_cpu(), torch.zeros(4, 5), torch.zeros(4, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="forward_train covers"):
        model.forward_train(torch.zeros(1, 3, 64, 96), torch.zeros(4, 5))
    low = fpn_model(use_rpn_head=True).optimize_for_inference(torch.bfloat16)
    with pytest.raises(NotImplementedError, match="forward_train_boxes covers"):
        low.forward_train_boxes(feats_cpu(), torch.zeros(4, 5), torch.zeros(4, dtype=torch.int32))


class _Untouched:
    """An optimizer that must not be reached."""

    def __getattr__(self, name):
        raise AssertionError("the optimizer was touched: %s" % name)


@pytest.mark.parametrize("top_n", [0, 2049])
def test_joint_step_on_fpn_checks_the_proposal_rows_first(faster_fpn, top_n):
    from detectorch_amd.model.collect_and_distribute_fpn_rpn_proposals import collect_sample_distribute
    from detectorch_amd.train import faster_rcnn_train_step
    with pytest.raises(ValueError, match="1 .. 2048"):
        faster_rcnn_train_step(faster_fpn, _Untouched(), torch.zeros(1, 3, 64, 96), gt_cpu(), it=0, post_nms_top_n=top_n)
    with pytest.raises(ValueError, match="1 .. 2048"):                                          # before any work: CPU tensors are not reached
        collect_sample_distribute(torch.zeros(1, 5, 8, 4), torch.zeros(1, 5, 8), torch.zeros(1, 5, dtype=torch.int32), gt_cpu(),
                                  post_nms_top_n=top_n)


def test_joint_step_on_fpn_in_range_reaches_the_device_check(faster_fpn):
    """With the range right nothing else refuses an FPN model: the first thing that stops a CPU run is the device check."""
    from detectorch_amd.train import faster_rcnn_train_step
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        faster_rcnn_train_step(faster_fpn, _Untouched(), torch.zeros(1, 3, 64, 96), gt_cpu(), post_nms_top_n=2048)


def test_joint_step_on_fpn_takes_the_mlp_head():
    """What forward_train_boxes would refuse after the RPN forward is refused before any work."""
    from detectorch_amd.model.detector import detector
    from detectorch_amd.train import faster_rcnn_train_step
    res5 = detector(N_classes=5, use_rpn_head=True, conv_body_layers=FPN['conv_body_layers'][:-1], fpn_layers=['layer1', 'layer2', 'layer3'],
                    roi_spatial_scale=[0.25, 0.125, 0.0625])
    with pytest.raises(NotImplementedError, match="two-layer MLP head"):
        faster_rcnn_train_step(res5, _Untouched(), torch.zeros(1, 3, 64, 96), gt_cpu(), it=0)
    with pytest.raises(NotImplementedError, match="forward_train_boxes covers"):
        res5.forward_train_boxes([torch.zeros(1, 256, 16, 24)], torch.zeros(4, 5))


def test_mask_step_on_fpn_takes_the_1up4convs_head():
    from detectorch_amd.model.detector import detector
    from detectorch_amd.train import mask_rcnn_train_step
    # an FPN body with the shared res5 head is the only FPN model the 'upshare' mask head can be built on
    upshare = detector(N_classes=5, use_rpn_head=True, use_mask_head=True, mask_head_type='upshare', conv_body_layers=FPN['conv_body_layers'][:-1],
                       fpn_layers=['layer1', 'layer2', 'layer3'], roi_spatial_scale=[0.25, 0.125, 0.0625])
    with pytest.raises(NotImplementedError, match="1up4convs"):
        mask_rcnn_train_step(upshare, _Untouched(), torch.zeros(1, 3, 64, 96), gt_cpu(), it=0)
    with pytest.raises(NotImplementedError, match="use_mask_head"):
        mask_rcnn_train_step(fpn_model(use_rpn_head=True), _Untouched(), torch.zeros(1, 3, 64, 96), gt_cpu(), it=0)
    ok = fpn_model(use_rpn_head=True, use_mask_head=True, mask_head_type='1up4convs')
    with pytest.raises(ValueError, match="1 .. 2048"):                                          # the head is accepted: the next check speaks
        mask_rcnn_train_step(ok, _Untouched(), torch.zeros(1, 3, 64, 96), gt_cpu(), it=0, post_nms_top_n=0)
