"""ctypes binding of libdetectorch_mask_hip.so (C ABI: include/detectorch_mask_hip.h): training of the mask branch -- the mask
targets of a minibatch (polygons rasterised into M x M grids) and the class-specific sigmoid cross-entropy fused with its gradient.

A seventh library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_mask() on first use.
PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda

LIB_PATH = os.environ.get("DETECTORCH_MASK_HIP_LIB") or _build.MASK_LIB

MAX_M, MAX_GT, MAX_ROWS, MAX_ROIS, MAX_PROPOSALS, MAX_POLYS, MAX_POINTS = 56, 256, 512, 4096, 65536, 4096, 65536
MAX_LOSS_ROWS, MAX_CLASSES = 1 << 20, 1024
BLOCK, LOSS_BLOCK, LOSS_MAX_BLOCKS = 256, 256, 1024          # csrc/mask_train: kMaskThreads, kLossThreads, kMaskLossMaxBlocks

# include/detectorch_mask_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_mask_train_target_arch()
size dtc_mask_targets_workspace_bytes(batch:i mask_rows:i)
status dtc_mask_targets(labels keep_inds n_rois batch:i rois_per_image:i gt_boxes gt_classes gt_is_crowd gt_counts gt_stride:i proposals
    proposal_stride:i im_scale poly_xy poly_ptr gt_poly_ptr points_stride:i polys_stride:i M:i k_min:i k_max:i mask_rows:i workspace
    workspace_bytes:z mask_rois masks mask_class mask_roi_levels roi_has_mask n_mask mask_gt stream)
size dtc_mask_loss_workspace_bytes(rows:i K:i M:i)
status dtc_mask_loss(mask_logits masks mask_class rows:i K:i M:i upstream workspace workspace_bytes:z loss n_valid grad_mask_logits
    stream)
""", {})

_lib = None


def lib():
    """Build (when stale or missing) and load the mask training library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_MASK_HIP_LIB" not in os.environ:
        _build.build_mask()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for mask training." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def _dense(name, t, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise TypeError("%s: expected a contiguous %s tensor of shape %s, got %s %s" % (name, dtype, tuple(shape), t.dtype,
                                                                                        tuple(t.shape)))


def targets_outputs(B, R, Fm, M, dev, with_gt=True):
    """The output set and workspace of dtc_mask_targets for B images of R minibatch rows, Fm mask rows of M x M each."""
    f32, i32 = torch.float32, torch.int32
    need = hip.invoke(lib(), SIGNATURES, "dtc_mask_targets_workspace_bytes", dict(batch=B, mask_rows=Fm))
    if need == 0 or not 1 <= M <= MAX_M:
        raise ValueError("mask_targets: unsupported shape: %d images x %d mask rows (at most %d) of %d x %d (at most %d)" %
                         (B, Fm, MAX_ROWS, M, M, MAX_M))
    e = lambda *shape, dtype=i32: torch.empty(shape, dtype=dtype, device=dev)
    return dict(mask_rois=e(B, Fm, 5, dtype=f32), masks=e(B, Fm, M * M), mask_class=e(B, Fm), mask_roi_levels=e(B, Fm),
                roi_has_mask=e(B, R), n_mask=e(B), mask_gt=e(B, Fm) if with_gt else None, workspace=hip.workspace(need, dev))


def mask_targets(labels, keep_inds, n_rois, gt_boxes, gt_classes, gt_is_crowd, gt_counts, proposals, im_scale, poly_xy, poly_ptr,
                 gt_poly_ptr, M=28, k_min=2, k_max=5, mask_rows=None, out=None):
    """dtc_mask_targets on contiguous device tensors: labels / keep_inds i32 [B,R] and n_rois i32 [B] (the minibatch of
    dtc_fast_rcnn_targets); gt_boxes f32 [B,G,4], gt_classes / gt_is_crowd i32 [B,G], gt_counts i32 [B], proposals f32 [B,P,4],
    im_scale f32 [B]; poly_xy f32 [B,PTS,2], poly_ptr i32 [B,NP+1], gt_poly_ptr i32 [B,G+1].  mask_rows: Fm (None: min(R, 512)).
    -> the dict of targets_outputs(); `out`: a preallocated one to write into (graph capture).  No host sync."""
    dev = _require_cuda(labels, keep_inds, n_rois, gt_boxes, gt_classes, gt_is_crowd, gt_counts, proposals, im_scale, poly_xy, poly_ptr,
                        gt_poly_ptr)
    B, R = labels.shape
    G, P, PTS, NP = gt_boxes.shape[1], proposals.shape[1], poly_xy.shape[1], poly_ptr.shape[1] - 1
    f32, i32 = torch.float32, torch.int32
    for name, t, dt, shape in (("labels", labels, i32, (B, R)), ("keep_inds", keep_inds, i32, (B, R)), ("n_rois", n_rois, i32, (B,)),
                               ("gt_boxes", gt_boxes, f32, (B, G, 4)), ("gt_classes", gt_classes, i32, (B, G)),
                               ("gt_is_crowd", gt_is_crowd, i32, (B, G)), ("gt_counts", gt_counts, i32, (B,)),
                               ("proposals", proposals, f32, (B, P, 4)), ("im_scale", im_scale, f32, (B,)),
                               ("poly_xy", poly_xy, f32, (B, PTS, 2)), ("poly_ptr", poly_ptr, i32, (B, NP + 1)),
                               ("gt_poly_ptr", gt_poly_ptr, i32, (B, G + 1))):
        _dense(name, t, dt, shape)
    if out is None:
        out = targets_outputs(B, R, min(R, MAX_ROWS) if mask_rows is None else int(mask_rows), M, dev)
    Fm = out["mask_rois"].shape[1]
    ws = out["workspace"]
    args = {k: v for k, v in out.items() if k != "workspace"}
    none_if_empty = lambda t: t if t.numel() else None
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_mask_targets", dict(
            labels=labels, keep_inds=keep_inds, n_rois=n_rois, batch=B, rois_per_image=R, gt_boxes=none_if_empty(gt_boxes),
            gt_classes=none_if_empty(gt_classes), gt_is_crowd=none_if_empty(gt_is_crowd), gt_counts=gt_counts, gt_stride=G,
            proposals=none_if_empty(proposals), proposal_stride=P, im_scale=im_scale, poly_xy=none_if_empty(poly_xy), poly_ptr=poly_ptr,
            gt_poly_ptr=gt_poly_ptr, points_stride=PTS, polys_stride=NP, M=M, k_min=k_min, k_max=k_max, mask_rows=Fm, workspace=ws,
            workspace_bytes=ws.numel(), **args))
    return out


def loss_outputs(Rm, K, M, dev, grad=True):
    """loss f32 [1], n_valid i32 [1], grad_mask_logits f32 [Rm,K,M,M] (None with grad=False) and the workspace of dtc_mask_loss"""
    need = hip.invoke(lib(), SIGNATURES, "dtc_mask_loss_workspace_bytes", dict(rows=Rm, K=K, M=M))
    if need == 0:
        raise ValueError("mask_loss: unsupported shape: %d rows (at most %d) x %d classes (at most %d) of %d x %d (at most %d)" %
                         (Rm, MAX_LOSS_ROWS, K, MAX_CLASSES, M, M, MAX_M))
    return dict(loss=torch.empty(1, dtype=torch.float32, device=dev), n_valid=torch.empty(1, dtype=torch.int32, device=dev),
                grad_mask_logits=torch.empty((Rm, K, M, M), dtype=torch.float32, device=dev) if grad else None,
                workspace=hip.workspace(need, dev))


def mask_loss(mask_logits, masks, mask_class, upstream=None, grad=True, out=None):
    """dtc_mask_loss: mask_logits f32 [Rm,K,M,M], masks i32 [Rm,M*M] (or [B,Fm,M*M] with Rm = B*Fm), mask_class i32 [Rm] (or [B,Fm]);
    upstream f32 [1] on the device or None (1).  -> the dict of loss_outputs(); grad=False: a loss-only call.  No host sync."""
    dev = _require_cuda(mask_logits, masks, mask_class, upstream)
    if mask_logits.dim() != 4 or mask_logits.shape[2] != mask_logits.shape[3]:
        raise TypeError("mask_loss: mask_logits must be [Rm,K,M,M]")
    Rm, K, M, _ = mask_logits.shape
    f32, i32 = torch.float32, torch.int32
    _dense("mask_logits", mask_logits, f32, (Rm, K, M, M))
    if masks.numel() != Rm * M * M or mask_class.numel() != Rm:
        raise TypeError("mask_loss: masks must hold %d x %d and mask_class %d elements" % (Rm, M * M, Rm))
    _dense("masks", masks, i32, masks.shape)
    _dense("mask_class", mask_class, i32, mask_class.shape)
    if upstream is not None:
        _dense("upstream", upstream, f32, (1,))
    if out is None:
        out = loss_outputs(Rm, K, M, dev, grad)
    ws = out["workspace"]
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_mask_loss", dict(
            mask_logits=mask_logits, masks=masks, mask_class=mask_class, rows=Rm, K=K, M=M, upstream=upstream, workspace=ws,
            workspace_bytes=ws.numel(), loss=out["loss"], n_valid=out["n_valid"], grad_mask_logits=out["grad_mask_logits"]))
    return out
