"""ctypes binding of libdetectorch_grad_hip.so (C ABI: include/detectorch_grad_hip.h): the gradients of the region operators
(RoIAlign backward).

A fourth library next to libdetectorch_hip.so (hip.py), libdetectorch_train_hip.so (hip_train.py) and libdetectorch_loss_hip.so
(hip_loss.py), built by build.build_grad() on first use.  PyTorch is used for device memory and the current HIP stream only; there
is NO CPU fallback: CPU tensors raise.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda

LIB_PATH = os.environ.get("DETECTORCH_GRAD_HIP_LIB") or _build.GRAD_LIB

MAX_POOLED, MAX_SAMPLING, MAX_ROIS, MAX_BATCH, MAX_EXTENT, MAX_GRID = 1024, 1024, 1 << 24, 65536, 1 << 20, 32768


class GradLevel(C.Structure):
    """struct dtc_grad_level (include/detectorch_grad_hip.h)"""
    _fields_ = [("grad", C.c_void_p), ("height", C.c_int32), ("width", C.c_int32), ("spatial_scale", C.c_float), ("_pad", C.c_int32)]


# include/detectorch_grad_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_grad_target_arch()
size dtc_roi_align_backward_workspace_bytes(n_levels:i batch:i n_rois:i)
status dtc_roi_align_backward(levels:GradLevel n_levels:i batch:i channels:i rois roi_cols:i roi_levels n_rois:i pooled_h:i pooled_w:i
    sampling_ratio:i grad_output workspace workspace_bytes:z stream)
""", {"GradLevel": GradLevel})

_lib = None


def lib():
    """Build (when stale or missing) and load the gradient library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_GRAD_HIP_LIB" not in os.environ:
        _build.build_grad()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for RoIAlign backward." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def backward_outputs(feature_shapes, n_rois, dev):
    """The output set of dtc_roi_align_backward: dict(grads = one float32 NCHW tensor per shape of feature_shapes ([B, C, H, W] each,
    equal B and C), workspace).  Nothing is cleared: the call writes every element."""
    if not 1 <= len(feature_shapes) <= hip.DTC_MAX_LEVELS:
        raise ValueError("1 .. %d levels" % hip.DTC_MAX_LEVELS)
    shapes = [tuple(int(v) for v in s) for s in feature_shapes]
    if any(len(s) != 4 or s[:2] != shapes[0][:2] for s in shapes):
        raise ValueError("feature shapes must be [B, C, H, W] with equal B and C")
    need = hip.invoke(lib(), SIGNATURES, "dtc_roi_align_backward_workspace_bytes",
                      dict(n_levels=len(shapes), batch=shapes[0][0], n_rois=n_rois))
    if need == 0:
        raise ValueError("roi_align_backward: unsupported shape: %d levels, batch %d (1 .. %d), %d RoIs (0 .. %d)"
                         % (len(shapes), shapes[0][0], MAX_BATCH, n_rois, MAX_ROIS))
    return dict(grads=[torch.empty(s, dtype=torch.float32, device=dev) for s in shapes], workspace=hip.workspace(need, dev))


def roi_align_backward(grad_output, rois, feature_shapes, spatial_scales, pooled_h, pooled_w, sampling_ratio, roi_levels=None,
                       out=None):
    """dtc_roi_align_backward on contiguous device tensors: grad_output f32 [R, C, pooled_h, pooled_w], rois f32 [R, 4 | 5],
    roi_levels i32 [R] or None (level 0); feature_shapes: the [B, C, H, W] of every level (one shape: a single level), with
    spatial_scales to match.  -> the list of per-level gradients, float32 NCHW, every element written (bit-identical to the
    reference's serial loop).  `out`: a preallocated backward_outputs() to write into (graph capture).  No host sync."""
    if len(feature_shapes) == 4 and not hasattr(feature_shapes[0], "__len__"):
        feature_shapes, spatial_scales = [feature_shapes], [spatial_scales]
    dev = _require_cuda(grad_output, rois, roi_levels)
    f32 = torch.float32
    if rois.dtype != f32 or rois.dim() != 2 or rois.shape[1] not in (4, 5) or not rois.is_contiguous():
        raise TypeError("roi_align_backward: rois must be a contiguous float32 [R, 4 | 5] tensor")
    R, cols = rois.shape
    B, ch = int(feature_shapes[0][0]), int(feature_shapes[0][1])
    if grad_output.dtype != f32 or tuple(grad_output.shape) != (R, ch, pooled_h, pooled_w) or not grad_output.is_contiguous():
        raise TypeError("roi_align_backward: grad_output must be a contiguous float32 tensor of shape %s, got %s %s"
                        % ((R, ch, pooled_h, pooled_w), grad_output.dtype, tuple(grad_output.shape)))
    if roi_levels is not None and (roi_levels.dtype != torch.int32 or tuple(roi_levels.shape) != (R,) or not roi_levels.is_contiguous()):
        raise TypeError("roi_align_backward: roi_levels must be a contiguous int32 [R] tensor")
    if len(spatial_scales) != len(feature_shapes):
        raise ValueError("roi_align_backward: one spatial scale per level")
    if out is None:
        out = backward_outputs(feature_shapes, R, dev)
    grads, ws = out["grads"], out["workspace"]
    lv = (GradLevel * len(grads))()
    for k, (g, shape, s) in enumerate(zip(grads, feature_shapes, spatial_scales)):
        if g.dtype != f32 or tuple(g.shape) != tuple(int(v) for v in shape) or not g.is_contiguous() or g.device != dev:
            raise TypeError("roi_align_backward: out['grads'][%d] must be a contiguous float32 %s tensor on %s" % (k, tuple(shape), dev))
        lv[k] = GradLevel(g.data_ptr(), g.shape[2], g.shape[3], float(s), 0)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_roi_align_backward", dict(
            levels=lv, n_levels=len(grads), batch=B, channels=ch, rois=rois, roi_cols=cols, roi_levels=roi_levels, n_rois=R,
            pooled_h=pooled_h, pooled_w=pooled_w, sampling_ratio=sampling_ratio, grad_output=grad_output, workspace=ws,
            workspace_bytes=ws.numel()))
    return grads
