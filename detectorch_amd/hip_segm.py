"""ctypes binding of libdetectorch_segm_hip.so (C ABI: include/detectorch_segm_hip.h): scoring instance masks on the device -- COCO's
rleIou on the run lists dtc_mask_rle leaves there, and COCOeval's evaluateImg on the resulting IoU matrix.  The records have the
layouts of hip_eval.eval_match's and go into hip_eval.eval_accumulate as they are.

A ninth library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_segm() on first use.
PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.  The streaming
evaluator on top of this is detectorch_amd/utils/evaluator.py:MaskEvaluator.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from . import hip_eval
from .hip import _require_cuda
from .hip_eval import MAX_AREAS, MAX_BATCH, MAX_CLASSES, MAX_GT, MAX_IMAGES, MAX_OUT, MAX_PAIRS, _dense

LIB_PATH = os.environ.get("DETECTORCH_SEGM_HIP_LIB") or _build.SEGM_LIB

MAX_RUNS, MAX_PIXELS = 1 << 20, 1 << 30                      # DTC_SEGM_MAX_*
PAIR_WAVES = 4                                               # csrc/segm_eval: kSegmPairWaves

# include/detectorch_segm_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_segm_target_arch()
size dtc_segm_iou_workspace_bytes(batch:i max_out:i det_runs_stride:i gt_stride:i gt_runs_stride:i)
status dtc_segm_iou(dets det_count det_runs det_n_runs im_size gt_runs gt_n_runs gt_classes gt_is_crowd gt_counts batch:i max_out:i
    det_runs_stride:i gt_stride:i gt_runs_stride:i num_classes:i workspace workspace_bytes:z iou det_area gt_mask_area n_bad stream)
status dtc_segm_match(dets det_count iou det_area gt_classes gt_is_crowd gt_counts gt_area gt_mask_area batch:i max_out:i gt_stride:i
    num_classes:i iou_thrs n_thrs:i area_rngs n_areas:i max_det:i image_base:q dt_rank dt_match dt_ignore gt_ignore gt_match npig
    sort_key stream)
""", {})

_lib = None


def lib():
    """Build (when stale or missing) and load the mask-evaluation library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_SEGM_HIP_LIB" not in os.environ:
        _build.build_segm()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the mask evaluation." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def _runs(name, runs, n_runs, N, rows):
    """checks one side's run lists; -> its runs stride"""
    if runs.dim() != 3:
        raise TypeError("%s: expected [N,%d,runs_stride]" % (name, rows))
    stride = runs.shape[2]
    if runs.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)):   # the header's uint32, held as int32 by hip.mask_rle
        raise TypeError("%s: expected an int32 (the uint32 bits) tensor, got %s" % (name, runs.dtype))
    _dense(name, runs, runs.dtype, (N, rows, stride))
    _dense(name.replace("_runs", "_n_runs"), n_runs, torch.int32, (N, rows))
    if not 1 <= stride <= MAX_RUNS:
        raise ValueError("%s: a runs stride of 1 .. %d, got %d" % (name, MAX_RUNS, stride))
    return stride


def iou_workspace_bytes(N, max_out, det_runs_stride, G, gt_runs_stride):
    return lib().dtc_segm_iou_workspace_bytes(N, max_out, det_runs_stride, G, gt_runs_stride)


def iou_outputs(N, max_out, G, dev):
    """The output set of dtc_segm_iou under its parameter names: iou f64 [N,max_out,G]; det_area i32 [N,max_out]; gt_mask_area i32
    [N,G]; n_bad i32 [N]."""
    e = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=dev)
    return dict(iou=e(N, max_out, G, dtype=torch.float64), det_area=e(N, max_out), gt_mask_area=e(N, G), n_bad=e(N))


def segm_iou(dets, det_count, det_runs, det_n_runs, im_size, gt_runs, gt_n_runs, gt_classes, gt_is_crowd, gt_counts, num_classes,
             out=None, ws=None):
    """dtc_segm_iou on contiguous device tensors: dets f32 [N,max_out,6], det_count i32 [N]; det_runs u32 [N,max_out,stride] and
    det_n_runs i32 [N,max_out] (hip.mask_rle's counts / n_runs); im_size f32 [N,2] = (h, w); gt_runs u32 [N,G,stride'], gt_n_runs /
    gt_classes / gt_is_crowd i32 [N,G], gt_counts i32 [N].  -> the dict of iou_outputs(); `out`: a preallocated one to write into;
    `ws`: a uint8 workspace of at least iou_workspace_bytes(...) (allocated when None or too small).  No host sync."""
    dev = _require_cuda(dets, det_count, det_runs, det_n_runs, im_size, gt_runs, gt_n_runs, gt_classes, gt_is_crowd, gt_counts)
    if dets.dim() != 3:
        raise TypeError("dets: expected [N,max_out,6]")
    N, max_out = dets.shape[0], dets.shape[1]
    _dense("dets", dets, torch.float32, (N, max_out, 6))
    _dense("det_count", det_count, torch.int32, (N,))
    _dense("im_size", im_size, torch.float32, (N, 2))
    if gt_classes.dim() != 2:
        raise TypeError("gt_classes: expected [N,G]")
    G = gt_classes.shape[1]
    _dense("gt_classes", gt_classes, torch.int32, (N, G))
    _dense("gt_is_crowd", gt_is_crowd, torch.int32, (N, G))
    _dense("gt_counts", gt_counts, torch.int32, (N,))
    if G > MAX_GT:
        raise ValueError("at most %d gt rows per image, got %d" % (MAX_GT, G))
    det_stride = _runs("det_runs", det_runs, det_n_runs, N, max_out)
    gt_stride = _runs("gt_runs", gt_runs, gt_n_runs, N, G)
    if not (1 <= N <= MAX_BATCH and 1 <= max_out <= MAX_OUT and 2 <= num_classes <= MAX_CLASSES):
        raise ValueError("segm_iou: unsupported shape: %d images (at most %d) x %d rows (at most %d), %d classes (at most %d)" %
                         (N, MAX_BATCH, max_out, MAX_OUT, num_classes, MAX_CLASSES))
    if out is None:
        out = iou_outputs(N, max_out, G, dev)
    need = iou_workspace_bytes(N, max_out, det_stride, G, gt_stride)
    if ws is None or ws.numel() < need:
        ws = hip.workspace(need, dev)
    none_if_empty = lambda t: t if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_segm_iou", dict(
            dets=dets, det_count=det_count, det_runs=det_runs, det_n_runs=det_n_runs, im_size=im_size, gt_runs=none_if_empty(gt_runs),
            gt_n_runs=none_if_empty(gt_n_runs), gt_classes=none_if_empty(gt_classes), gt_is_crowd=none_if_empty(gt_is_crowd),
            gt_counts=gt_counts, batch=N, max_out=max_out, det_runs_stride=det_stride, gt_stride=G, gt_runs_stride=gt_stride,
            num_classes=num_classes, workspace=ws, workspace_bytes=ws.numel(), **{k: none_if_empty(v) for k, v in out.items()}))
    return out


match_outputs = hip_eval.match_outputs                        # dtc_segm_match's output set is dtc_eval_match's


def segm_match(dets, det_count, iou, det_area, gt_classes, gt_is_crowd, gt_counts, gt_area, gt_mask_area, num_classes, iou_thrs,
               area_rngs, max_det, image_base=0, out=None):
    """dtc_segm_match on contiguous device tensors: dets f32 [N,max_out,6], det_count i32 [N]; iou f64 [N,max_out,G] and det_area
    i32 [N,max_out] (segm_iou's, or crafted); gt_classes / gt_is_crowd i32 [N,G], gt_counts i32 [N]; gt_area f32 [N,G] or None: then
    gt_mask_area i32 [N,G] is the area of a gt; iou_thrs f64 [T] and area_rngs f64 [A,2] on the device.  -> the dict of
    match_outputs(), in hip_eval.eval_match's layouts; `out`: a preallocated one to write into (graph capture).  No host sync."""
    dev = _require_cuda(dets, det_count, iou, det_area, gt_classes, gt_is_crowd, gt_counts, gt_area, gt_mask_area, iou_thrs, area_rngs)
    if dets.dim() != 3:
        raise TypeError("dets: expected [N,max_out,6]")
    N, max_out = dets.shape[0], dets.shape[1]
    _dense("dets", dets, torch.float32, (N, max_out, 6))
    _dense("det_count", det_count, torch.int32, (N,))
    if iou.dim() != 3:
        raise TypeError("iou: expected [N,max_out,G]")
    G = iou.shape[2]
    _dense("iou", iou, torch.float64, (N, max_out, G))
    _dense("det_area", det_area, torch.int32, (N, max_out))
    _dense("gt_classes", gt_classes, torch.int32, (N, G))
    _dense("gt_is_crowd", gt_is_crowd, torch.int32, (N, G))
    _dense("gt_counts", gt_counts, torch.int32, (N,))
    if gt_area is not None:
        _dense("gt_area", gt_area, torch.float32, (N, G))
    elif gt_mask_area is None:
        raise TypeError("segm_match: gt_area or gt_mask_area must be given")
    if gt_mask_area is not None:
        _dense("gt_mask_area", gt_mask_area, torch.int32, (N, G))
    if G > MAX_GT:
        raise ValueError("at most %d gt rows per image, got %d" % (MAX_GT, G))
    T, A = iou_thrs.numel(), area_rngs.shape[0]
    _dense("iou_thrs", iou_thrs, torch.float64, (T,))
    _dense("area_rngs", area_rngs, torch.float64, (A, 2))
    if not (1 <= N <= MAX_BATCH and 1 <= max_out <= MAX_OUT and 1 <= T and 1 <= A <= MAX_AREAS and T * A <= MAX_PAIRS and
            2 <= num_classes <= MAX_CLASSES and 0 <= image_base <= MAX_IMAGES - N):
        raise ValueError("segm_match: unsupported shape: %d images (at most %d, %d in a run) x %d rows (at most %d), %d thresholds x %d "
                         "area ranges (at most %d pairs, %d ranges), %d classes (at most %d)" %
                         (N, MAX_BATCH, MAX_IMAGES, max_out, MAX_OUT, T, A, MAX_PAIRS, MAX_AREAS, num_classes, MAX_CLASSES))
    if out is None:
        out = match_outputs(N, max_out, G, num_classes, T, A, dev)
    none_if_empty = lambda t: t if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_segm_match", dict(
            dets=dets, det_count=det_count, iou=none_if_empty(iou), det_area=det_area, gt_classes=none_if_empty(gt_classes),
            gt_is_crowd=none_if_empty(gt_is_crowd), gt_counts=gt_counts, gt_area=none_if_empty(gt_area),
            gt_mask_area=none_if_empty(gt_mask_area), batch=N, max_out=max_out, gt_stride=G, num_classes=num_classes, iou_thrs=iou_thrs,
            n_thrs=T, area_rngs=area_rngs, n_areas=A, max_det=max_det, image_base=image_base,
            **{k: none_if_empty(v) for k, v in out.items()}))
    return out
