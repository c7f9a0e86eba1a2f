"""ctypes binding of libdetectorch_rpn_hip.so (C ABI: include/detectorch_rpn_hip.h): RPN training -- the anchor minibatch and the
fused RPN losses with their gradient maps.

A sixth library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_rpn() on first use.
PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda

LIB_PATH = os.environ.get("DETECTORCH_RPN_HIP_LIB") or _build.RPN_LIB

MAX_LEVELS, MAX_ANCHORS_PER_CELL, MAX_GT, MAX_ANCHORS, MAX_BATCH_PER_IM = 8, 16, 256, 1 << 20, 4096
BLOCK, SELECT_BLOCK, LOSS_BLOCK, LOSS_MAX_BLOCKS = 256, 1024, 256, 512      # csrc/rpn_train: kRpnThreads, kRpnSelThreads, ...


class RpnTrainLevel(C.Structure):
    """struct dtc_rpn_train_level (include/detectorch_rpn_hip.h)"""
    _fields_ = [("cls_logits", C.c_void_p), ("bbox_pred", C.c_void_p), ("grad_cls_logits", C.c_void_p), ("grad_bbox_pred", C.c_void_p),
                ("num_anchors", C.c_int32), ("height", C.c_int32), ("width", C.c_int32), ("feat_stride", C.c_float),
                ("anchors", C.c_float * 64)]


class RpnTrainParams(C.Structure):
    """struct dtc_rpn_train_params (include/detectorch_rpn_hip.h)"""
    _fields_ = [("batch_size_per_im", C.c_int32), ("_pad", C.c_int32), ("fg_fraction", C.c_double), ("positive_overlap", C.c_float),
                ("negative_overlap", C.c_float), ("straddle_thresh", C.c_float), ("_pad2", C.c_float)]


def rpn_train_params(batch_size_per_im=256, fg_fraction=0.5, positive_overlap=0.7, negative_overlap=0.3, straddle_thresh=0.0):
    """Detectron's TRAIN.RPN_* knobs as a dtc_rpn_train_params."""
    return RpnTrainParams(int(batch_size_per_im), 0, float(fg_fraction), float(positive_overlap), float(negative_overlap),
                          float(straddle_thresh), 0.0)


def fg_quota(params):
    """F: the rows of fg_index / fg_targets / fg_gt"""
    return int(params.fg_fraction * params.batch_size_per_im)


# include/detectorch_rpn_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_rpn_train_target_arch()
size dtc_rpn_targets_workspace_bytes(levels:RpnTrainLevel n_levels:i batch:i gt_stride:i)
status dtc_rpn_targets(levels:RpnTrainLevel n_levels:i batch:i gt_boxes gt_is_crowd gt_counts gt_stride:i im_scale im_hw rand_keys
    params:RpnTrainParams workspace workspace_bytes:z labels fg_index fg_targets fg_gt n_fg n_bg max_overlaps gt_max bbox_targets
    bbox_inside_weights bbox_outside_weights stream)
size dtc_rpn_loss_workspace_bytes(levels:RpnTrainLevel n_levels:i batch:i)
status dtc_rpn_loss(levels:RpnTrainLevel n_levels:i batch:i labels fg_index fg_targets n_fg n_bg fg_stride:i beta:f upstream workspace
    workspace_bytes:z losses n_valid stream)
""", {"RpnTrainLevel": RpnTrainLevel, "RpnTrainParams": RpnTrainParams})

_lib = None


def lib():
    """Build (when stale or missing) and load the RPN training library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_RPN_HIP_LIB" not in os.environ:
        _build.build_rpn()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for RPN training." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def make_levels(shapes, anchors, feat_strides, cls_logits=None, bbox_pred=None, grad_cls_logits=None, grad_bbox_pred=None):
    """shapes: one (A, H, W) per level; anchors: one [A, 4] array of base anchors per level; the four optional lists hold one
    contiguous float32 device tensor per level ([B,A,H,W] / [B,4A,H,W]).  -> (RpnTrainLevel array, N)."""
    if len(shapes) > MAX_LEVELS:
        raise ValueError("at most %d levels" % MAX_LEVELS)
    arr = (RpnTrainLevel * len(shapes))()
    n = 0
    ptr = lambda lst, l: None if lst is None else lst[l].data_ptr()
    for l, ((a, h, w), base, stride) in enumerate(zip(shapes, anchors, feat_strides)):
        flat = [float(v) for row in base for v in row]
        if len(flat) != 4 * a or a > MAX_ANCHORS_PER_CELL:
            raise ValueError("level %d: %d base anchors of 4 coordinates expected (at most %d)" % (l, a, MAX_ANCHORS_PER_CELL))
        arr[l] = RpnTrainLevel(ptr(cls_logits, l), ptr(bbox_pred, l), ptr(grad_cls_logits, l), ptr(grad_bbox_pred, l), int(a), int(h),
                               int(w), float(stride), (C.c_float * 64)(*flat))
        n += a * h * w
    return arr, n


def map_levels(cls_logits, bbox_pred, grad_cls_logits=None, grad_bbox_pred=None):
    """The level array of dtc_rpn_loss from the maps themselves (the loss reads no anchors): lists of contiguous float32 device
    tensors [B,A,H,W] / [B,4A,H,W] per level, the gradient maps of the same shapes or None.  -> (RpnTrainLevel array, B, N)."""
    _require_cuda(*cls_logits, *bbox_pred, *(grad_cls_logits or ()), *(grad_bbox_pred or ()))
    if len(cls_logits) != len(bbox_pred) or not cls_logits:
        raise TypeError("rpn_loss: one cls_logits and one bbox_pred map per level")
    B = cls_logits[0].shape[0]
    shapes = []
    for l, c in enumerate(cls_logits):
        if c.dim() != 4 or c.shape[0] != B:
            raise TypeError("rpn_loss: cls_logits must be [B,A,H,W]")
        _, a, h, w = c.shape
        for name, lst, ch in (("cls_logits", cls_logits, a), ("bbox_pred", bbox_pred, 4 * a), ("grad_cls_logits", grad_cls_logits, a),
                              ("grad_bbox_pred", grad_bbox_pred, 4 * a)):
            if lst is not None:
                _dense("%s[%d]" % (name, l), lst[l], torch.float32, (B, ch, h, w))
        shapes.append((a, h, w))
    arr, n = make_levels(shapes, [[[0.0] * 4] * a for a, _, _ in shapes], [1.0] * len(shapes), cls_logits, bbox_pred,
                         grad_cls_logits, grad_bbox_pred)
    return arr, B, n


def _dense(name, t, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise TypeError("%s: expected a contiguous %s tensor of shape %s, got %s %s" % (name, dtype, tuple(shape), t.dtype,
                                                                                        tuple(t.shape)))


def targets_outputs(levels, B, N, G, params, dev, expanded=False, assignment=False):
    """The output set and workspace of dtc_rpn_targets for B images of N anchors, in fixed shapes (F = fg_quota(params))."""
    f32, i32 = torch.float32, torch.int32
    F = fg_quota(params)
    e = lambda *shape, dtype=f32: torch.empty(shape, dtype=dtype, device=dev)
    need = hip.invoke(lib(), SIGNATURES, "dtc_rpn_targets_workspace_bytes", dict(levels=levels, n_levels=len(levels), batch=B, gt_stride=G))
    if need == 0:
        raise ValueError("rpn_targets: unsupported shape: %d images x %d anchors (at most %d) against %d gt (at most %d)" %
                         (B, N, MAX_ANCHORS, G, MAX_GT))
    out = dict(labels=e(B, N, dtype=i32), fg_index=e(B, F, dtype=i32), fg_targets=e(B, F, 4), fg_gt=e(B, F, dtype=i32),
               n_fg=e(B, dtype=i32), n_bg=e(B, dtype=i32), workspace=hip.workspace(need, dev))
    out["max_overlaps"] = e(B, N) if assignment else None
    out["gt_max"] = e(B, G) if assignment else None
    for k in ("bbox_targets", "bbox_inside_weights", "bbox_outside_weights"):
        out[k] = e(B, 4 * N) if expanded else None
    return out


def rpn_targets(levels, gt_boxes, gt_is_crowd, gt_counts, im_scale, im_hw, rand_keys, params, out=None, expanded=False,
                assignment=False):
    """dtc_rpn_targets on contiguous device tensors: levels from make_levels; gt_boxes f32 [B,G,4], gt_is_crowd i32 [B,G], gt_counts
    i32 [B], im_scale f32 [B], im_hw f32 [B,2], rand_keys 32-bit integers [B,N] (read as uint32).  -> the dict of targets_outputs();
    `out`: a preallocated one to write into (graph capture).  No host sync."""
    dev = _require_cuda(gt_boxes, gt_is_crowd, gt_counts, im_scale, im_hw, rand_keys)
    B, G = gt_boxes.shape[0], gt_boxes.shape[1]
    N = sum(l.num_anchors * l.height * l.width for l in levels)
    f32, i32 = torch.float32, torch.int32
    for name, t, dt, shape in (("gt_boxes", gt_boxes, f32, (B, G, 4)), ("gt_is_crowd", gt_is_crowd, i32, (B, G)),
                               ("gt_counts", gt_counts, i32, (B,)), ("im_scale", im_scale, f32, (B,)), ("im_hw", im_hw, f32, (B, 2))):
        _dense(name, t, dt, shape)
    if rand_keys.element_size() != 4 or rand_keys.dtype.is_floating_point or tuple(rand_keys.shape) != (B, N) or \
            not rand_keys.is_contiguous():
        raise TypeError("rpn_targets: rand_keys must be contiguous 32-bit integers of shape %s" % ((B, N),))
    if out is None:
        out = targets_outputs(levels, B, N, G, params, dev, expanded, assignment)
    ws = out["workspace"]
    args = {k: v for k, v in out.items() if k != "workspace"}
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_rpn_targets", dict(
            levels=levels, n_levels=len(levels), batch=B, gt_boxes=gt_boxes, gt_is_crowd=gt_is_crowd, gt_counts=gt_counts, gt_stride=G,
            im_scale=im_scale, im_hw=im_hw, rand_keys=rand_keys, params=params, workspace=ws, workspace_bytes=ws.numel(), **args))
    return out


def loss_outputs(levels, B, dev):
    """losses f32 [2], n_valid i32 [1] and the workspace of dtc_rpn_loss"""
    need = hip.invoke(lib(), SIGNATURES, "dtc_rpn_loss_workspace_bytes", dict(levels=levels, n_levels=len(levels), batch=B))
    if need == 0:
        raise ValueError("rpn_loss: unsupported shape")
    return dict(losses=torch.empty(2, dtype=torch.float32, device=dev), n_valid=torch.empty(1, dtype=torch.int32, device=dev),
                workspace=hip.workspace(need, dev))


def rpn_loss(levels, labels, fg_index, fg_targets, n_fg, n_bg, beta=1.0 / 9.0, upstream=None, out=None):
    """dtc_rpn_loss: levels from make_levels with cls_logits and bbox_pred (and the gradient maps, or None for a loss-only call);
    labels i32 [B,N], fg_index i32 [B,F], fg_targets f32 [B,F,4], n_fg / n_bg i32 [B]; upstream f32 [2] or None (1, 1).
    -> the dict of loss_outputs(); the gradient maps are written in place.  No host sync."""
    dev = _require_cuda(labels, fg_index, fg_targets, n_fg, n_bg, upstream)
    B, F = fg_index.shape
    N = sum(l.num_anchors * l.height * l.width for l in levels)
    f32, i32 = torch.float32, torch.int32
    for name, t, dt, shape in (("labels", labels, i32, (B, N)), ("fg_index", fg_index, i32, (B, F)),
                               ("fg_targets", fg_targets, f32, (B, F, 4)), ("n_fg", n_fg, i32, (B,)), ("n_bg", n_bg, i32, (B,))):
        _dense(name, t, dt, shape)
    if upstream is not None:
        _dense("upstream", upstream, f32, (2,))
    if out is None:
        out = loss_outputs(levels, B, dev)
    ws = out["workspace"]
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_rpn_loss", dict(
            levels=levels, n_levels=len(levels), batch=B, labels=labels, fg_index=fg_index, fg_targets=fg_targets, n_fg=n_fg, n_bg=n_bg,
            fg_stride=F, beta=beta, upstream=upstream, workspace=ws, workspace_bytes=ws.numel(), losses=out["losses"],
            n_valid=out["n_valid"]))
    return out
