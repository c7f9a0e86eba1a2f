"""One training step of Fast R-CNN R-50/101-C4 on given proposals, the loop body of the reference's train_fast.py:125-166 on the
native pieces: the minibatch of sample_rois_batched, detector.forward_train (RoIAlign with its native backward), the fused head
losses (model.loss.fast_rcnn_losses) and ClippedSGD (gradient clipping + momentum SGD in one call).  RPN and mask training and the
dataset are not here."""
from .model import loss as _loss
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
