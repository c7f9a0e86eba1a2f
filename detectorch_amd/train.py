"""One training step of Fast R-CNN R-50/101-C4 on given proposals, the loop body of the reference's train_fast.py:125-166 on the
native pieces: the minibatch of sample_rois_batched, detector.forward_train (RoIAlign with its native backward), the fused head
losses (model.loss.fast_rcnn_losses) and ClippedSGD (gradient clipping + momentum SGD in one call); and the two steps that train the
RPN models the project serves: rpn_train_step (RPN only -- stage 1 of alternating training -- C4 and FPN) and faster_rcnn_train_step
(the joint approximate Faster R-CNN step, C4 and FPN), on the anchor minibatch of rpn_targets_batched and the fused RPN losses
(model.loss.rpn_losses); and mask_rcnn_train_step, the joint step of the Mask R-CNN models, C4 and FPN: faster_rcnn_train_step plus
the mask targets of mask_targets_batched (polygons rasterised on the device), detector.forward_train_mask on the shared features and
the fused mask loss (model.loss.mask_rcnn_loss).  On FPN the joint steps take the training branch of collect-and-distribute the
reference left unconverted (model.collect_and_distribute_fpn_rpn_proposals.collect_sample_distribute: collect over the RPN levels,
sample, distribute the SAMPLED rows over the RoIAlign levels) and detector.forward_train_boxes / forward_train_mask with the
multi-level RoIAlign and its one-call backward; fast_rcnn_train_step also takes the Fast R-CNN FPN model (detector.forward_train).
Keypoints and the dataset are not here."""
import torch

from . import hip
from .model import loss as _loss
from .model.collect_and_distribute_fpn_rpn_proposals import collect_sample_distribute
from .utils.fast_rcnn_sample_rois import sample_rois_batched
from .utils.mask_rcnn_targets import mask_targets_batched
from .utils.rpn_targets import rpn_targets_batched
from .utils.solver import adjust_learning_rate, get_lr_at_iter


def freeze_stem(model):
    """train_fast.py:87-90: conv1, bn1 and layer1 of the ResNet body take no gradient.  -> the parameters left trainable, in
    model.parameters() order: what the optimizer gets (train_fast.py:93)."""
    for name in ('conv1', 'bn1', 'layer1'):
        for p in getattr(model.model, name).parameters():
            p.requires_grad = False
    return [p for p in model.parameters() if p.requires_grad]


def fast_rcnn_train_step(model, optimizer, images, blobs, it=None):
    """train_fast.py:125-166 in its order: the learning rate of iteration `it` from the solver (None: the optimizer's own stays),
    forward_train on blobs['rois'], the head losses, zero_grad, backward of loss_cls + loss_bbox, optimizer.step() (ClippedSGD: the
    clipping is part of the step).  images [B,3,H,W]; blobs: the dict of sample_rois_batched (expanded=False is enough).
    -> (loss_cls, loss_bbox, accuracy) as 0-dim device tensors; nothing syncs with the host."""
    if it is not None:
        lr = get_lr_at_iter(it)
        if getattr(optimizer, "capturable", False):
            optimizer.set_lr_(lr)
        else:
            adjust_learning_rate(optimizer, lr)
    rois = blobs['rois']
    cls_score, bbox_pred = model.forward_train(images, rois.reshape(-1, rois.shape[-1]))
    loss_cls, loss_bbox, acc = _loss.fast_rcnn_losses(cls_score, bbox_pred, blobs)
    optimizer.zero_grad()
    (loss_cls + loss_bbox).backward()
    optimizer.step()
    return loss_cls.detach(), loss_bbox.detach(), acc


def _set_lr(optimizer, it):
    if it is not None:
        lr = get_lr_at_iter(it)
        if getattr(optimizer, "capturable", False):
            optimizer.set_lr_(lr)
        else:
            adjust_learning_rate(optimizer, lr)


def _rpn_forward_losses(model, images, gt, rpn_knobs):
    """forward_train_rpn, the anchor minibatch against gt, the two RPN losses.  gt: dict of device tensors -- gt_boxes f32 [B,G,4]
    (original image coordinates), gt_is_crowd i32 [B,G], gt_counts i32 [B], im_scale f32 [B], im_hw f32 [B,2] (the scaled image's own
    size inside the padded blob); optional rpn_rand_keys [B,N]."""
    cls_logits, bbox_pred, feats = model.forward_train_rpn(images)
    levels = model.rpn_train_levels(cls_logits)
    blobs = rpn_targets_batched(levels, gt["gt_boxes"], gt["gt_is_crowd"], gt["gt_counts"], gt["im_scale"], gt["im_hw"],
                                rand_keys=gt.get("rpn_rand_keys"), **rpn_knobs)
    loss_rpn_cls, loss_rpn_bbox = _loss.rpn_losses(cls_logits, bbox_pred, blobs)
    return cls_logits, bbox_pred, feats, blobs, loss_rpn_cls, loss_rpn_bbox


def rpn_train_step(model, optimizer, images, gt, it=None, **rpn_knobs):
    """One RPN-only step (stage 1 of alternating training) of a use_rpn_head=True model, C4 or FPN: the learning rate of iteration
    `it` from the solver, forward_train_rpn, rpn_targets_batched, rpn_losses, zero_grad, backward of loss_rpn_cls + loss_rpn_bbox,
    optimizer.step() (ClippedSGD).  gt: see _rpn_forward_losses; **rpn_knobs: the keywords of rpn_targets_batched
    (batch_size_per_im, ...).  -> (loss_rpn_cls, loss_rpn_bbox) as 0-dim device tensors; nothing syncs with the host."""
    _set_lr(optimizer, it)
    _, _, _, _, loss_rpn_cls, loss_rpn_bbox = _rpn_forward_losses(model, images, gt, rpn_knobs)
    optimizer.zero_grad()
    (loss_rpn_cls + loss_rpn_bbox).backward()
    optimizer.step()
    return loss_rpn_cls.detach(), loss_rpn_bbox.detach()


def _check_joint(model, post_nms_top_n):
    if model.use_fpn_body and not model.use_two_layer_mlp_head:
        raise NotImplementedError("the joint step on an FPN model takes the two-layer MLP head (detector.forward_train_boxes)")
    if post_nms_top_n < 1 or post_nms_top_n > 2048:
        raise ValueError("post_nms_top_n must be in 1 .. 2048 (the proposal rows of sample_rois_batched)")


def _joint_forward_losses(model, images, gt, rpn_knobs, post_nms_top_n, pre_nms_top_n, head_knobs):
    """What the joint steps share, up to the backward: RPN forward and losses; under no_grad, the proposals and the Fast R-CNN
    minibatch (both in blob coordinates) -- C4: the one RPN level's proposals into sample_rois_batched; FPN: the proposals of ALL
    RPN levels into collect_sample_distribute, which also gives the level of every sampled row --; forward_train_boxes on the
    shared features and the two head losses.
    -> (loss_rpn_cls, loss_rpn_bbox, loss_cls, loss_bbox, accuracy, blobs, feats, gt_blob)."""
    cls_logits, bbox_pred, feats, _, loss_rpn_cls, loss_rpn_bbox = _rpn_forward_losses(model, images, gt, rpn_knobs or {})
    B, h, w = images.shape[0], images.shape[2], images.shape[3]
    with torch.no_grad():
        scale = gt["im_scale"].reshape(B, 1, 1)
        gt_blob = (gt["gt_boxes"] * scale).contiguous()                       # one float32 multiply, as the RPN minibatch scales them
        if model.use_fpn_body:
            gens = model.proposal_generator
            boxes, scores, counts, _, _, _ = hip.generate_proposals(
                [c.detach() for c in cls_logits], [b.detach() for b in bbox_pred], [g._anchors for g in gens],
                [1. / s for s in model.rpn_scales], h, w, [pre_nms_top_n] * len(gens), post_nms_top_n, gens[0].rpn_nms_thresh,
                scores_are_logits=True, im_hw=gt["im_hw"])                    # top-n per level; blob coordinates
            k_min, k_max = model.roi_level_range()
            blobs = collect_sample_distribute(boxes, scores, counts, dict(gt, gt_boxes=gt_blob), post_nms_top_n=post_nms_top_n,
                                              k_min=k_min, k_max=k_max, rand_keys=gt.get("rand_keys"), num_classes=model.N_classes,
                                              **head_knobs)
        else:
            gen = model.proposal_generator
            boxes, _, counts, _, _, _ = hip.generate_proposals(
                [cls_logits[0].detach()], [bbox_pred[0].detach()], [gen._anchors], [1. / gen._spatial_scale], h, w, [pre_nms_top_n],
                post_nms_top_n, gen.rpn_nms_thresh, scores_are_logits=True, im_hw=gt["im_hw"])
            proposals = boxes[:, 0].contiguous()                              # [B, P, 4], blob coordinates
            blobs = sample_rois_batched(proposals, counts[:, 0].contiguous(), gt_blob, gt["gt_classes"], gt["gt_is_crowd"],
                                        gt["gt_counts"], torch.ones_like(gt["im_scale"]), rand_keys=gt.get("rand_keys"),
                                        expanded=False, num_classes=model.N_classes, **head_knobs)
            blobs["proposals"], blobs["proposal_counts"] = proposals, counts[:, 0]
    rois = blobs["rois"]
    cls_score, box_deltas = model.forward_train_boxes(feats, rois.reshape(-1, rois.shape[-1]), blobs.get("roi_levels"))
    loss_cls, loss_bbox, acc = _loss.fast_rcnn_losses(cls_score, box_deltas, blobs)
    return loss_rpn_cls, loss_rpn_bbox, loss_cls, loss_bbox, acc, blobs, feats, gt_blob


def faster_rcnn_train_step(model, optimizer, images, gt, it=None, rpn_knobs=None, post_nms_top_n=2000, pre_nms_top_n=12000,
                           **head_knobs):
    """The joint approximate Faster R-CNN step of a use_rpn_head=True model, C4 or FPN: RPN forward and losses; under no_grad,
    the proposals of hip.generate_proposals with the training top-n (post-NMS <= 2048, the minibatch kernel's limit);
    sample_rois_batched on those proposals and the gt, BOTH in blob coordinates with im_scale 1, so that `rois` needs no rescaling;
    forward_train_boxes on the shared features (C4: RoIAlign, the res5 head and the two heads); fast_rcnn_losses; ONE backward of
    the four losses (the proposals carry no gradient: "approximate"), optimizer.step().
    FPN (two-layer MLP head): generate_proposals runs over ALL RPN levels (the extra pooled one included), pre_nms_top_n and
    post_nms_top_n apply PER LEVEL (a level with fewer anchors takes them all; Detectron's FPN recipe passes 2000 for both, the
    default 12000 is the C4 recipe's); collect_sample_distribute keeps the top post_nms_top_n over the levels, samples the minibatch
    and maps every sampled row to its level k_min .. k_max = log2(1 / roi_spatial_scale) (2 .. 5); the box branch is roi_align_fpn
    with those levels (one launch forward, one call backward), fc6 / fc7 and the two heads.
    gt: see _rpn_forward_losses, plus gt_classes i32 [B,G] and optional rand_keys [B,G+P] (FPN: P = post_nms_top_n); **head_knobs:
    the keywords of sample_rois_batched.
    -> (loss_rpn_cls, loss_rpn_bbox, loss_cls, loss_bbox, accuracy, blobs), blobs with proposals, proposal_counts and, on FPN,
    roi_levels [B,R]; nothing syncs with the host."""
    _check_joint(model, post_nms_top_n)
    _set_lr(optimizer, it)
    loss_rpn_cls, loss_rpn_bbox, loss_cls, loss_bbox, acc, blobs, _, _ = _joint_forward_losses(
        model, images, gt, rpn_knobs, post_nms_top_n, pre_nms_top_n, head_knobs)
    optimizer.zero_grad()
    (loss_rpn_cls + loss_rpn_bbox + loss_cls + loss_bbox).backward()
    optimizer.step()
    return loss_rpn_cls.detach(), loss_rpn_bbox.detach(), loss_cls.detach(), loss_bbox.detach(), acc, blobs


def mask_rcnn_train_step(model, optimizer, images, gt, it=None, rpn_knobs=None, post_nms_top_n=2000, pre_nms_top_n=12000,
                         **head_knobs):
    """The joint approximate Mask R-CNN step of a use_rpn_head=True, use_mask_head=True model -- C4 with the 'upshare' head, FPN
    with the '1up4convs' head: everything faster_rcnn_train_step does up to its backward, then, under no_grad, mask_targets_batched
    on the minibatch, at M = 14 on C4 and M = 28 with the levels k_min .. k_max on FPN (the polygons, like the gt boxes, in blob
    coordinates with im_scale 1, so that mask_rois are the foreground rows of `rois` bit for bit and mask_roi_levels their
    roi_levels); detector.forward_train_mask on the shared features; mask_rcnn_loss; ONE backward of the five losses,
    optimizer.step().  gt: as for faster_rcnn_train_step, plus poly_xy f32 [B,PTS,2], poly_ptr i32 [B,NP+1], gt_poly_ptr i32 [B,G+1]
    (utils.mask_rcnn_targets.pack_polygons) in ORIGINAL image coordinates like gt_boxes.
    -> (loss_rpn_cls, loss_rpn_bbox, loss_cls, loss_bbox, loss_mask, accuracy, blobs) with the mask blobs merged into blobs; nothing
    syncs with the host."""
    if not getattr(model, "use_mask_head", False):
        raise NotImplementedError("mask_rcnn_train_step takes a model with use_mask_head=True")
    fpn = model.use_fpn_body
    if fpn and model.mask_head_type != '1up4convs':
        raise NotImplementedError("mask_rcnn_train_step on an FPN model takes the '1up4convs' mask head")
    _check_joint(model, post_nms_top_n)
    _set_lr(optimizer, it)
    loss_rpn_cls, loss_rpn_bbox, loss_cls, loss_bbox, acc, blobs, feats, gt_blob = _joint_forward_losses(
        model, images, gt, rpn_knobs, post_nms_top_n, pre_nms_top_n, head_knobs)
    B = images.shape[0]
    # the mask rows per image: the foreground quota of the minibatch (hip_train.train_params: half to even), so no row is cut
    quota = int(round(head_knobs.get("fg_fraction", 0.25) * head_knobs.get("rois_per_image", 512)))
    # M -- C4: res5 halves, the transposed conv doubles: 14; FPN: the four convs keep 14, the transposed conv doubles: 28
    M = 2 * model.mask_head.roi_height if fpn else model.mask_head.roi_height
    k_min, k_max = model.roi_level_range() if fpn else (0, 0)
    with torch.no_grad():
        poly_blob = (gt["poly_xy"] * gt["im_scale"].reshape(B, 1, 1)).contiguous()   # one float32 multiply, as gt_blob
        mb = mask_targets_batched(blobs, blobs["proposals"], gt_blob, gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"],
                                  torch.ones_like(gt["im_scale"]), (poly_blob, gt["poly_ptr"], gt["gt_poly_ptr"]),
                                  M=M, k_min=k_min, k_max=k_max, mask_rows=min(max(quota, 1), 512))
    mask_rois = mb["mask_rois"]
    mask_logits = model.forward_train_mask(feats, mask_rois.reshape(-1, 5), roi_levels=mb["mask_roi_levels"] if fpn else None)
    loss_mask = _loss.mask_rcnn_loss(mask_logits, mb)
    blobs.update({k: v for k, v in mb.items() if k != "_raw"})
    optimizer.zero_grad()
    (loss_rpn_cls + loss_rpn_bbox + loss_cls + loss_bbox + loss_mask).backward()
    optimizer.step()
    return (loss_rpn_cls.detach(), loss_rpn_bbox.detach(), loss_cls.detach(), loss_bbox.detach(), loss_mask.detach(), acc, blobs)
