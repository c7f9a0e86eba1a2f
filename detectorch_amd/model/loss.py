"""The Fast R-CNN head losses -- the call surface of the reference's lib/model/loss.py (smooth_L1 :13, accuracy :22) and of the
cross_entropy it imports (:11), backed by the hand-written gfx950 kernels of detectorch_amd/csrc/loss instead of a chain of
elementwise and reduction kernels; plus the fused forms that read the compact, padded output of sample_rois_batched directly:

    smooth_L1(pred, targets, alpha_in, alpha_out, beta=1.0)     the reference's signature; differentiable in pred
    accuracy(cls_score, cls_labels)                             the reference's signature
    cross_entropy(cls_score, labels)                            mean softmax cross-entropy over the rows with label >= 0
    fast_rcnn_losses(cls_score, bbox_pred, blobs, beta=1.0)     -> (loss_cls, loss_bbox, accuracy), differentiable
    fast_rcnn_losses_fused(cls_score, bbox_pred, blobs, ...)    losses AND both gradients from one call (graph capture)
    rpn_losses(cls_logits_list, bbox_pred_list, blobs, beta=1/9) -> (loss_rpn_cls, loss_rpn_bbox) over the RPN maps, differentiable
    mask_rcnn_loss(mask_logits, blobs)                          -> loss_mask over the blobs of mask_targets_batched, differentiable

Differences a caller can observe (include/detectorch_loss_hip.h has the full contract):
  * GPU only: CPU tensors raise;
  * rows with a negative label (the padding rows of sample_rois_batched) are ignored, and the means divide by the number of the
    others, counted on the device: nothing is compacted and nothing syncs with the host;
  * accuracy takes the argmax over the logits, lowest index among equal ones (the reference: over softmax(logits));
  * no valid row at all gives zeros where the reference would divide by zero;
  * smooth_L1 has no gradient with respect to targets and weights (they are data in the reference's training step).
"""
import torch
from torch.autograd import Function

from .. import hip_loss, hip_mask, hip_rpn
from ..hip import _require_cuda


def _f32(t):
    """contiguous float32 at a 16-byte aligned address (a view at an odd offset is copied)"""
    t = t.detach().to(torch.float32).contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _rows(cls_score, labels):
    """cls_score [..., C] and labels [...] as [N, C] float32 and [N] int32"""
    return _f32(cls_score).reshape(-1, cls_score.shape[-1]), labels.detach().to(torch.int32).reshape(-1).contiguous()


class SmoothL1Function(Function):
    @staticmethod
    def forward(ctx, pred, targets, alpha_in, alpha_out, beta):
        args = tuple(_f32(t) for t in (pred, targets, alpha_in, alpha_out))
        ctx.save_for_backward(*args)
        ctx.beta = float(beta)
        loss, _ = hip_loss.smooth_l1(*args, beta=ctx.beta, loss=True, grad=False)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        upstream = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        _, grad = hip_loss.smooth_l1(*ctx.saved_tensors, beta=ctx.beta, upstream=upstream, loss=False, grad=True)
        return grad, None, None, None, None


def smooth_L1(pred, targets, alpha_in, alpha_out, beta=1.0):
    """lib/model/loss.py:13-20 -> 0-dim device tensor (dtc_smooth_l1); the divisor is pred.size(0)."""
    _require_cuda(pred, targets, alpha_in, alpha_out)
    return SmoothL1Function.apply(pred, targets, alpha_in, alpha_out, beta)


class HeadLossFunction(Function):
    """(loss_cls, loss_bbox, accuracy) of dtc_fast_rcnn_loss over [N, C] / [N, W] rows: forward is one loss-only call, backward one
    gradient-only call that takes the two incoming gradients as its device-side `upstream`."""
    @staticmethod
    def forward(ctx, cls_score, bbox_pred, labels, bbox_targets5, beta):
        ctx.save_for_backward(cls_score, bbox_pred, labels, bbox_targets5)
        ctx.beta = float(beta)
        losses = hip_loss.fast_rcnn_loss(cls_score, labels, bbox_pred, bbox_targets5, beta=ctx.beta, grads=False)["losses"]
        loss_cls, loss_bbox, acc = losses[0], losses[1], losses[2]
        ctx.mark_non_differentiable(acc)
        return loss_cls, loss_bbox, acc

    @staticmethod
    def backward(ctx, grad_cls, grad_bbox, _grad_acc):
        cls_score, bbox_pred, labels, bbox_targets5 = ctx.saved_tensors
        upstream = torch.stack((grad_cls.detach().reshape(()), grad_bbox.detach().reshape(()))).to(torch.float32).contiguous()
        out = hip_loss.fast_rcnn_loss(cls_score, labels, bbox_pred, bbox_targets5, beta=ctx.beta, upstream=upstream, losses=False)
        return out["grad_cls_score"], out["grad_bbox_pred"], None, None, None


def _head_args(cls_score, bbox_pred, blobs):
    """the padded [B, R, ...] tensors viewed as [B * R, ...] rows, never compacted"""
    labels, t5 = blobs["labels_int32"], blobs["bbox_targets5"]
    _require_cuda(cls_score, bbox_pred, labels, t5)
    n = labels.numel()
    labels = labels.reshape(n)
    t5 = t5.reshape(n, 5)
    if labels.dtype != torch.int32 or t5.dtype != torch.float32 or not labels.is_contiguous() or not t5.is_contiguous():
        raise TypeError("blobs must be the dict of sample_rois_batched (labels_int32 int32 [B,R], bbox_targets5 float32 [B,R,5])")
    return cls_score.reshape(n, cls_score.shape[-1]), bbox_pred.reshape(n, bbox_pred.shape[-1]), labels, t5


def _as_input(t):
    """what the kernels read: float32, contiguous, 16-byte aligned; the tensor itself when it already is (autograd then sees
    through the reshape alone)"""
    ok = t.dtype == torch.float32 and t.is_contiguous() and t.data_ptr() % 16 == 0
    return t if ok else t.to(torch.float32).contiguous().clone()


def fast_rcnn_losses(cls_score, bbox_pred, blobs, beta=1.0):
    """train_fast.py:141-154 on the blobs of sample_rois_batched (expanded=False is enough): cls_score [B*R, C] or [B, R, C],
    bbox_pred [B*R, W] or [B, R, W] with W = 4 C (8: class-agnostic) -> (loss_cls, loss_bbox, accuracy), 0-dim device tensors;
    the two losses are differentiable in cls_score and bbox_pred."""
    cls_score, bbox_pred, labels, t5 = _head_args(cls_score, bbox_pred, blobs)
    return HeadLossFunction.apply(_as_input(cls_score), _as_input(bbox_pred), labels, t5, beta)


def fast_rcnn_losses_fused(cls_score, bbox_pred, blobs, out=None, beta=1.0, upstream=None):
    """Losses and both gradients from a SINGLE call of dtc_fast_rcnn_loss, for callers that drive
    torch.autograd.backward(..., grad_tensors=...) themselves and for graph capture.  -> dict(losses f32 [4] = (loss_cls, loss_bbox,
    accuracy, n_valid), grad_cls_score [B*R, C], grad_bbox_pred [B*R, W], workspace); `out`: the dict of an earlier call, written
    in place.  upstream: f32 [2] on the device, the factors on the two gradients (None: 1, 1)."""
    cls_score, bbox_pred, labels, t5 = _head_args(cls_score, bbox_pred, blobs)
    return hip_loss.fast_rcnn_loss(_as_input(cls_score.detach()), labels, _as_input(bbox_pred.detach()), t5, beta=beta,
                                   upstream=upstream, out=out)


class RpnLossFunction(Function):
    """(loss_rpn_cls, loss_rpn_bbox) of dtc_rpn_loss over the per-level maps (n cls_logits maps, then n bbox_pred maps, as
    RoIAlignFPNFunction takes its maps): forward is one loss-only call, backward one call that writes the dense gradient maps with the
    two incoming gradients as its device-side `upstream`."""
    @staticmethod
    def forward(ctx, labels, fg_index, fg_targets, n_fg, n_bg, beta, *maps):
        n = len(maps) // 2
        ctx.save_for_backward(labels, fg_index, fg_targets, n_fg, n_bg, *maps)
        ctx.beta = float(beta)
        levels, _, _ = hip_rpn.map_levels(maps[:n], maps[n:])
        losses = hip_rpn.rpn_loss(levels, labels, fg_index, fg_targets, n_fg, n_bg, beta=ctx.beta)["losses"]
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, grad_cls, grad_bbox):
        labels, fg_index, fg_targets, n_fg, n_bg, *maps = ctx.saved_tensors
        n = len(maps) // 2
        upstream = torch.stack((grad_cls.detach().reshape(()), grad_bbox.detach().reshape(()))).to(torch.float32).contiguous()
        grads = [torch.empty_like(m) for m in maps]
        levels, _, _ = hip_rpn.map_levels(maps[:n], maps[n:], grads[:n], grads[n:])
        hip_rpn.rpn_loss(levels, labels, fg_index, fg_targets, n_fg, n_bg, beta=ctx.beta, upstream=upstream)
        return (None,) * 6 + tuple(grads)


def rpn_losses(cls_logits_list, bbox_pred_list, blobs, beta=1.0 / 9.0):
    """The two RPN losses on the blobs of rpn_targets_batched (expanded=False is enough): cls_logits_list [B,A,H,W] and
    bbox_pred_list [B,4A,H,W] per level, in the level order of the targets -> (loss_rpn_cls, loss_rpn_bbox), 0-dim device tensors,
    differentiable in every map: sigmoid cross-entropy over the sampled anchors / their number, and smooth-L1 (beta 1/9) over the
    sampled foreground anchors / the sample size per image, averaged over the images."""
    maps = [_as_input(t) for t in list(cls_logits_list) + list(bbox_pred_list)]
    return RpnLossFunction.apply(blobs["labels"], blobs["fg_index"], blobs["fg_targets"], blobs["n_fg"], blobs["n_bg"], beta, *maps)


class MaskLossFunction(Function):
    """loss_mask of dtc_mask_loss over mask_logits [Rm,K,M,M]: forward is one loss-only call, backward one call that writes the dense
    gradient with the incoming gradient as its device-side `upstream`."""
    @staticmethod
    def forward(ctx, mask_logits, masks, mask_class):
        ctx.save_for_backward(mask_logits, masks, mask_class)
        return hip_mask.mask_loss(mask_logits, masks, mask_class, grad=False)["loss"].reshape(())

    @staticmethod
    def backward(ctx, grad_loss):
        mask_logits, masks, mask_class = ctx.saved_tensors
        upstream = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        return hip_mask.mask_loss(mask_logits, masks, mask_class, upstream=upstream)["grad_mask_logits"], None, None


def mask_rcnn_loss(mask_logits, blobs):
    """Detectron's loss_mask (class-specific SigmoidCrossEntropyLoss, normalised) on the blobs of mask_targets_batched: mask_logits
    [B*Fm, K, M, M] PRE-sigmoid, one row per row of blobs['masks_int32'] [B,Fm,M*M] (padding rows included: their targets are -1)
    -> a 0-dim device tensor, differentiable in mask_logits: the mean over the elements of channel mask_class_labels[r] whose
    target is 0 or 1; 0 without one."""
    masks, cls = blobs["masks_int32"], blobs["mask_class_labels"]
    _require_cuda(mask_logits, masks, cls)
    return MaskLossFunction.apply(_as_input(mask_logits), masks, cls)


def cross_entropy(cls_score, labels):
    """torch.nn.functional.cross_entropy(cls_score, labels) (lib/model/loss.py:11, train_fast.py:147) as a 0-dim device tensor,
    differentiable in cls_score: dtc_fast_rcnn_loss without the box arguments.  Rows with a negative label are ignored."""
    _require_cuda(cls_score, labels)
    x = cls_score.reshape(-1, cls_score.shape[-1])
    return HeadLossFunction.apply(_as_input(x), None, labels.detach().to(torch.int32).reshape(-1).contiguous(), None, 1.0)[0]


def accuracy(cls_score, cls_labels):
    """lib/model/loss.py:22-26 -> 0-dim device tensor; the argmax is taken over the logits."""
    _require_cuda(cls_score, cls_labels)
    x, labels = _rows(cls_score, cls_labels)
    return hip_loss.fast_rcnn_loss(x, labels, grads=False)["losses"][2]
