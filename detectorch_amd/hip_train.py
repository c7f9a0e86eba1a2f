"""ctypes binding of libdetectorch_train_hip.so (C ABI: include/detectorch_train_hip.h): the training-side natives.

A second library next to libdetectorch_hip.so (hip.py), built by build.build_train() on first use.  PyTorch is used for device
memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda

LIB_PATH = os.environ.get("DETECTORCH_TRAIN_HIP_LIB") or _build.TRAIN_LIB

MAX_GT, MAX_PROPOSALS, MAX_ROIS = 256, 2048, 4096


class TrainParams(C.Structure):
    """struct dtc_train_params (include/detectorch_train_hip.h)"""
    _fields_ = [("rois_per_image", C.c_int32), ("num_classes", C.c_int32), ("cls_agnostic_bbox_reg", C.c_int32), ("_pad", C.c_int32),
                ("fg_fraction", C.c_double), ("crowd_thresh", C.c_double), ("fg_thresh", C.c_float), ("bg_thresh_hi", C.c_float),
                ("bg_thresh_lo", C.c_float), ("bbox_thresh", C.c_float), ("reg_weights", C.c_float * 4)]


def train_params(rois_per_image=512, fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0, bbox_thresh=0.5,
                 crowd_thresh=0.7, reg_weights=(10.0, 10.0, 5.0, 5.0), num_classes=81, cls_agnostic_bbox_reg=False):
    """The reference's training knobs (train_fast.py; lib/data/roidb.py:44-55) as a dtc_train_params."""
    return TrainParams(int(rois_per_image), int(num_classes), 1 if cls_agnostic_bbox_reg else 0, 0, float(fg_fraction),
                       float(crowd_thresh), float(fg_thresh), float(bg_thresh_hi), float(bg_thresh_lo), float(bbox_thresh),
                       (C.c_float * 4)(*[float(w) for w in reg_weights]))


# include/detectorch_train_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_train_target_arch()
status dtc_fast_rcnn_targets(gt_boxes gt_classes gt_is_crowd gt_counts proposals proposal_counts im_scale rand_keys batch:i
    gt_stride:i proposal_stride:i params:TrainParams rois5 labels bbox_targets5 bbox_targets bbox_inside_weights
    bbox_outside_weights keep_inds n_fg n_rois max_overlaps max_classes stream)
""", {"TrainParams": TrainParams})

_lib = None


def lib():
    """Build (when stale or missing) and load the training library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_TRAIN_HIP_LIB" not in os.environ:
        _build.build_train()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the training targets." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def targets_outputs(B, n_cand, params, dev, expanded=True, assignment=False):
    """The output set of dtc_fast_rcnn_targets for B images, in fixed shapes (R = params.rois_per_image)."""
    f32, i32 = torch.float32, torch.int32
    R = params.rois_per_image
    W = 4 * (2 if params.cls_agnostic_bbox_reg else params.num_classes)
    e = lambda *shape, dtype=f32: torch.empty(shape, dtype=dtype, device=dev)
    out = dict(rois5=e(B, R, 5), labels=e(B, R, dtype=i32), bbox_targets5=e(B, R, 5), keep_inds=e(B, R, dtype=i32),
               n_fg=e(B, dtype=i32), n_rois=e(B, dtype=i32))
    for k in ("bbox_targets", "bbox_inside_weights", "bbox_outside_weights"):
        out[k] = e(B, R, W) if expanded else None
    out["max_overlaps"] = e(B, n_cand) if assignment else None
    out["max_classes"] = e(B, n_cand, dtype=i32) if assignment else None
    return out


def fast_rcnn_targets(gt_boxes, gt_classes, gt_is_crowd, gt_counts, proposals, proposal_counts, im_scale, rand_keys, params,
                      out=None, expanded=True, assignment=False):
    """dtc_fast_rcnn_targets on contiguous device tensors: gt_boxes f32 [B,G,4], gt_classes / gt_is_crowd i32 [B,G], gt_counts i32
    [B], proposals f32 [B,P,4], proposal_counts i32 [B], im_scale f32 [B], rand_keys 32-bit integers [B,G+P] (read as uint32).
    -> the dict of targets_outputs(); `out`: a preallocated one to write into (graph capture).  No host sync."""
    dev = _require_cuda(gt_boxes, gt_classes, gt_is_crowd, gt_counts, proposals, proposal_counts, im_scale, rand_keys)
    B, G, P = proposals.shape[0], gt_boxes.shape[1], proposals.shape[1]
    f32, i32 = torch.float32, torch.int32
    for t, dt, shape in ((gt_boxes, f32, (B, G, 4)), (gt_classes, i32, (B, G)), (gt_is_crowd, i32, (B, G)), (gt_counts, i32, (B,)),
                         (proposals, f32, (B, P, 4)), (proposal_counts, i32, (B,)), (im_scale, f32, (B,))):
        if t.dtype != dt or tuple(t.shape) != shape or not t.is_contiguous():
            raise TypeError("fast_rcnn_targets: expected a contiguous %s tensor of shape %s, got %s %s" %
                            (dt, shape, t.dtype, tuple(t.shape)))
    if rand_keys.element_size() != 4 or rand_keys.dtype.is_floating_point or tuple(rand_keys.shape) != (B, G + P) or \
            not rand_keys.is_contiguous():
        raise TypeError("fast_rcnn_targets: rand_keys must be contiguous 32-bit integers of shape %s" % ((B, G + P),))
    if out is None:
        out = targets_outputs(B, G + P, params, dev, expanded, assignment)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_fast_rcnn_targets", dict(
            gt_boxes=gt_boxes, gt_classes=gt_classes, gt_is_crowd=gt_is_crowd, gt_counts=gt_counts, proposals=proposals,
            proposal_counts=proposal_counts, im_scale=im_scale, rand_keys=rand_keys, batch=B, gt_stride=G, proposal_stride=P,
            params=params, **out))
    return out
