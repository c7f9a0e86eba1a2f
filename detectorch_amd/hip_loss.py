"""ctypes binding of libdetectorch_loss_hip.so (C ABI: include/detectorch_loss_hip.h): the Fast R-CNN head losses and their
gradients.

A third library next to libdetectorch_hip.so (hip.py) and libdetectorch_train_hip.so (hip_train.py), built by build.build_loss()
on first use.  PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda

LIB_PATH = os.environ.get("DETECTORCH_LOSS_HIP_LIB") or _build.LOSS_LIB

MAX_CLASSES, MAX_ROWS, MAX_ELEMS = 1024, 65536, 1 << 30

# include/detectorch_loss_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_loss_target_arch()
size dtc_fast_rcnn_loss_workspace_bytes(n:i c:i)
status dtc_fast_rcnn_loss(cls_score labels bbox_pred bbox_targets5 n:i c:i bbox_width:i beta:f upstream workspace workspace_bytes:z
    losses grad_cls_score grad_bbox_pred stream)
size dtc_smooth_l1_workspace_bytes(n:i w:i)
status dtc_smooth_l1(pred targets alpha_in alpha_out n:i w:i beta:f upstream workspace workspace_bytes:z loss grad_pred stream)
""", {})

_lib = None


def lib():
    """Build (when stale or missing) and load the loss library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_LOSS_HIP_LIB" not in os.environ:
        _build.build_loss()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the head losses." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def _dense(name, t, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise TypeError("%s: expected a contiguous %s tensor of shape %s, got %s %s" % (name, dtype, tuple(shape), t.dtype,
                                                                                        tuple(t.shape)))


def loss_outputs(n, c, bbox_width, dev, losses=True, grads=True):
    """The output set and workspace of dtc_fast_rcnn_loss for n rows: losses f32 [4], grad_cls_score [n, c], grad_bbox_pred
    [n, bbox_width] (None for a group that is not wanted, and without box arguments: bbox_width 0), workspace."""
    e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
    need = hip.invoke(lib(), SIGNATURES, "dtc_fast_rcnn_loss_workspace_bytes", dict(n=n, c=c))
    if need == 0:
        raise ValueError("fast_rcnn_loss: unsupported shape: %d rows (1 .. %d) of %d classes (2 .. %d)" % (n, MAX_ROWS, c, MAX_CLASSES))
    return dict(losses=e(4) if losses else None, grad_cls_score=e(n, c) if grads else None,
                grad_bbox_pred=e(n, bbox_width) if grads and bbox_width else None, workspace=hip.workspace(need, dev))


def fast_rcnn_loss(cls_score, labels, bbox_pred=None, bbox_targets5=None, beta=1.0, upstream=None, out=None, losses=True, grads=True):
    """dtc_fast_rcnn_loss on contiguous device tensors: cls_score f32 [N,C], labels i32 [N] (negative: ignored row), bbox_pred f32
    [N,W] (W = 4C, or 8) with bbox_targets5 f32 [N,5], or neither (cross-entropy and accuracy only); upstream f32 [2] or None (1, 1).
    -> the dict of loss_outputs(); `out`: a preallocated one to write into (graph capture).  No host sync."""
    dev = _require_cuda(cls_score, labels, bbox_pred, bbox_targets5, upstream)
    if cls_score.dim() != 2:
        raise TypeError("fast_rcnn_loss: cls_score must be [N, C]")
    n, c = cls_score.shape
    f32 = torch.float32
    _dense("cls_score", cls_score, f32, (n, c))
    _dense("labels", labels, torch.int32, (n,))
    if (bbox_pred is None) != (bbox_targets5 is None):
        raise TypeError("fast_rcnn_loss: bbox_pred and bbox_targets5 go together")
    w = 0
    if bbox_pred is not None:
        w = bbox_pred.shape[-1]
        _dense("bbox_pred", bbox_pred, f32, (n, w))
        _dense("bbox_targets5", bbox_targets5, f32, (n, 5))
    if upstream is not None:
        _dense("upstream", upstream, f32, (2,))
    if out is None:
        out = loss_outputs(n, c, w, dev, losses, grads)
    ws = out["workspace"]
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_fast_rcnn_loss", dict(
            cls_score=cls_score, labels=labels, bbox_pred=bbox_pred, bbox_targets5=bbox_targets5, n=n, c=c, bbox_width=w, beta=beta,
            upstream=upstream, workspace=ws, workspace_bytes=ws.numel(), losses=out["losses"], grad_cls_score=out["grad_cls_score"],
            grad_bbox_pred=out["grad_bbox_pred"]))
    return out


def smooth_l1(pred, targets, alpha_in, alpha_out, beta=1.0, upstream=None, loss=True, grad=True):
    """dtc_smooth_l1 on four contiguous f32 device tensors of one shape [N, ...] (the divisor is N); upstream f32 [1] or None.
    -> (loss f32 [1] or None, grad_pred of pred's shape or None).  No host sync."""
    dev = _require_cuda(pred, targets, alpha_in, alpha_out, upstream)
    f32 = torch.float32
    if pred.dim() < 1 or pred.numel() == 0:
        raise TypeError("smooth_l1: pred must have at least one row")
    n = pred.shape[0]
    w = pred.numel() // n
    for name, t in (("pred", pred), ("targets", targets), ("alpha_in", alpha_in), ("alpha_out", alpha_out)):
        _dense(name, t, f32, pred.shape)
    if upstream is not None:
        _dense("upstream", upstream, f32, (1,))
    out_loss = torch.empty((1,), dtype=f32, device=dev) if loss else None
    out_grad = torch.empty_like(pred) if grad else None
    ws = None
    if loss:
        need = hip.invoke(lib(), SIGNATURES, "dtc_smooth_l1_workspace_bytes", dict(n=n, w=w))
        if need == 0:
            raise ValueError("smooth_l1: unsupported shape: %d x %d elements (at most %d)" % (n, w, MAX_ELEMS))
        ws = hip.workspace(need, dev)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_smooth_l1", dict(
            pred=pred, targets=targets, alpha_in=alpha_in, alpha_out=alpha_out, n=n, w=w, beta=beta, upstream=upstream, workspace=ws,
            workspace_bytes=0 if ws is None else ws.numel(), loss=out_loss, grad_pred=out_grad))
    return out_loss, out_grad
