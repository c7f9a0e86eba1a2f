"""ctypes binding of libdetectorch_eval_hip.so (C ABI: include/detectorch_eval_hip.h): scoring on the device -- COCO's box-AP protocol
(COCOeval's computeIoU + evaluateImg, then accumulate) and the reference's evaluate_box_proposals.

An eighth library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_eval() on first use.
PyTorch is used for device memory, the one sort of the keys and the current HIP stream only; there is NO CPU fallback: CPU tensors
raise.  The streaming evaluator on top of this is detectorch_amd/utils/evaluator.py.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda

LIB_PATH = os.environ.get("DETECTORCH_EVAL_HIP_LIB") or _build.EVAL_LIB

MAX_GT, MAX_OUT, MAX_PAIRS, MAX_AREAS, MAX_CLASSES, MAX_BATCH = 256, 512, 64, 16, 1024, 65535      # DTC_EVAL_MAX_*
MAX_IMAGES, MAX_ROWS, MAX_REC_THRS, MAX_MAX_DETS, MAX_PROPOSALS = 1 << 21, 1 << 30, 1024, 16, 65536
ACC_TILE, PROP_BLOCK = 256, 256                              # csrc/eval: kAccTile, kPropThreads

# include/detectorch_eval_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_eval_target_arch()
status dtc_eval_match(dets det_count gt_boxes gt_classes gt_is_crowd gt_counts gt_area batch:i max_out:i gt_stride:i num_classes:i
    iou_thrs n_thrs:i area_rngs n_areas:i max_det:i image_base:q dt_rank dt_match dt_ignore gt_ignore gt_match npig sort_key stream)
status dtc_eval_accumulate(dt_rank dt_match dt_ignore sort_key order rows:q npig images:i num_classes:i n_thrs:i n_areas:i rec_thrs
    n_rec:i max_dets n_max_dets:i precision recall counts stream)
status dtc_eval_proposal_recall(proposals prop_counts gt_boxes gt_classes gt_is_crowd gt_counts gt_area batch:i proposal_stride:i
    gt_stride:i area_rng limit:i gt_overlaps n_pos n_overlaps stream)
""", {})

_lib = None


def lib():
    """Build (when stale or missing) and load the evaluation library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_EVAL_HIP_LIB" not in os.environ:
        _build.build_eval()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the evaluation." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def _dense(name, t, dtype, shape):
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise TypeError("%s: expected a contiguous %s tensor of shape %s, got %s %s" % (name, dtype, tuple(shape), t.dtype,
                                                                                        tuple(t.shape)))


def _gt(gt_boxes, gt_classes, gt_is_crowd, gt_counts, gt_area, N):
    """checks the gt tensors of one call; -> G"""
    f32, i32 = torch.float32, torch.int32
    if gt_boxes.dim() != 3:
        raise TypeError("gt_boxes: expected [N,G,4]")
    G = gt_boxes.shape[1]
    _dense("gt_boxes", gt_boxes, f32, (N, G, 4))
    _dense("gt_classes", gt_classes, i32, (N, G))
    _dense("gt_is_crowd", gt_is_crowd, i32, (N, G))
    _dense("gt_counts", gt_counts, i32, (N,))
    if gt_area is not None:
        _dense("gt_area", gt_area, f32, (N, G))
    if G > MAX_GT:
        raise ValueError("at most %d gt rows per image, got %d" % (MAX_GT, G))
    return G


def match_outputs(N, max_out, G, num_classes, T, A, dev):
    """The output set of dtc_eval_match under its parameter names: dt_rank i32 [N,max_out]; dt_match / dt_ignore i64 [N,max_out] (the
    header's uint64 words: bit a * T + t); gt_ignore i32 [N,G]; gt_match i32 [N,G,A,T]; npig i32 [N,K,A]; sort_key i64 [N,max_out]."""
    e = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=dev)
    i64 = torch.int64
    return dict(dt_rank=e(N, max_out), dt_match=e(N, max_out, dtype=i64), dt_ignore=e(N, max_out, dtype=i64), gt_ignore=e(N, G),
                gt_match=e(N, G, A, T), npig=e(N, num_classes - 1, A), sort_key=e(N, max_out, dtype=i64))


def eval_match(dets, det_count, gt_boxes, gt_classes, gt_is_crowd, gt_counts, gt_area, num_classes, iou_thrs, area_rngs, max_det,
               image_base=0, out=None):
    """dtc_eval_match on contiguous device tensors: dets f32 [N,max_out,6], det_count i32 [N]; gt_boxes f32 [N,G,4], gt_classes /
    gt_is_crowd i32 [N,G], gt_counts i32 [N], gt_area f32 [N,G] or None; iou_thrs f64 [T] and area_rngs f64 [A,2] on the device.
    -> the dict of match_outputs(); `out`: a preallocated one to write into (graph capture).  No host sync."""
    dev = _require_cuda(dets, det_count, gt_boxes, gt_classes, gt_is_crowd, gt_counts, gt_area, iou_thrs, area_rngs)
    if dets.dim() != 3:
        raise TypeError("dets: expected [N,max_out,6]")
    N, max_out = dets.shape[0], dets.shape[1]
    _dense("dets", dets, torch.float32, (N, max_out, 6))
    _dense("det_count", det_count, torch.int32, (N,))
    G = _gt(gt_boxes, gt_classes, gt_is_crowd, gt_counts, gt_area, N)
    T, A = iou_thrs.numel(), area_rngs.shape[0]
    _dense("iou_thrs", iou_thrs, torch.float64, (T,))
    _dense("area_rngs", area_rngs, torch.float64, (A, 2))
    if not (1 <= N <= MAX_BATCH and 1 <= max_out <= MAX_OUT and 1 <= T and 1 <= A <= MAX_AREAS and T * A <= MAX_PAIRS and
            2 <= num_classes <= MAX_CLASSES and 0 <= image_base <= MAX_IMAGES - N):
        raise ValueError("eval_match: unsupported shape: %d images (at most %d, %d in a run) x %d rows (at most %d), %d thresholds x %d "
                         "area ranges (at most %d pairs, %d ranges), %d classes (at most %d)" %
                         (N, MAX_BATCH, MAX_IMAGES, max_out, MAX_OUT, T, A, MAX_PAIRS, MAX_AREAS, num_classes, MAX_CLASSES))
    if out is None:
        out = match_outputs(N, max_out, G, num_classes, T, A, dev)
    none_if_empty = lambda t: t if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_eval_match", dict(
            dets=dets, det_count=det_count, gt_boxes=none_if_empty(gt_boxes), gt_classes=none_if_empty(gt_classes),
            gt_is_crowd=none_if_empty(gt_is_crowd), gt_counts=gt_counts, gt_area=none_if_empty(gt_area), batch=N, max_out=max_out,
            gt_stride=G, num_classes=num_classes, iou_thrs=iou_thrs, n_thrs=T, area_rngs=area_rngs, n_areas=A, max_det=max_det,
            image_base=image_base, **{k: none_if_empty(v) for k, v in out.items()}))
    return out


def accumulate_outputs(T, R, K, A, M, dev):
    """The output set of dtc_eval_accumulate under its parameter names: precision f64 [T,R,K,A,M], recall f64 [T,K,A,M], counts i32 [K,A]"""
    e = lambda *shape, dtype=torch.float64: torch.empty(shape, dtype=dtype, device=dev)
    return dict(precision=e(T, R, K, A, M), recall=e(T, K, A, M), counts=e(K, A, dtype=torch.int32))


def eval_accumulate(dt_rank, dt_match, dt_ignore, sort_key, npig, num_classes, T, A, rec_thrs, max_dets, out=None):
    """dtc_eval_accumulate on the concatenated records of a run (flattened to rows = images x max_out); the stable sort of the keys is
    torch's.  rec_thrs f64 [R], max_dets i32 [M] on the device.  -> dict(precision f64 [T,R,K,A,M], recall f64 [T,K,A,M],
    counts i32 [K,A]) on the device; `out`: a preallocated one (accumulate_outputs) to write into.  No host sync."""
    dev = _require_cuda(dt_rank, dt_match, dt_ignore, sort_key, npig, rec_thrs, max_dets)
    rows, K = dt_rank.numel(), num_classes - 1
    for name, t, dt in (("dt_rank", dt_rank, torch.int32), ("dt_match", dt_match, torch.int64), ("dt_ignore", dt_ignore, torch.int64),
                        ("sort_key", sort_key, torch.int64)):
        _dense(name, t, dt, t.shape)
        if t.numel() != rows:
            raise TypeError("%s: expected %d elements" % (name, rows))
    if npig.dim() != 3:
        raise TypeError("npig: expected [images,K,A]")
    images = npig.shape[0]
    _dense("npig", npig, torch.int32, (images, K, A))
    R, M = rec_thrs.numel(), max_dets.numel()
    _dense("rec_thrs", rec_thrs, torch.float64, (R,))
    _dense("max_dets", max_dets, torch.int32, (M,))
    if not (1 <= rows <= MAX_ROWS and 1 <= images <= MAX_IMAGES and T * A <= MAX_PAIRS and A <= MAX_AREAS and 1 <= R <= MAX_REC_THRS and
            1 <= M <= MAX_MAX_DETS and 2 <= num_classes <= MAX_CLASSES):
        raise ValueError("eval_accumulate: unsupported shape: %d rows (at most %d), %d recall thresholds (at most %d), %d max_dets (at "
                         "most %d)" % (rows, MAX_ROWS, R, MAX_REC_THRS, M, MAX_MAX_DETS))
    order = torch.sort(sort_key.reshape(-1), stable=True)[1].to(torch.int32)
    if out is None:
        out = accumulate_outputs(T, R, K, A, M, dev)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_eval_accumulate", dict(
            dt_rank=dt_rank, dt_match=dt_match, dt_ignore=dt_ignore, sort_key=sort_key, order=order, rows=rows, npig=npig, images=images,
            num_classes=num_classes, n_thrs=T, n_areas=A, rec_thrs=rec_thrs, n_rec=R, max_dets=max_dets, n_max_dets=M, **out))
    return out


def proposal_recall(proposals, prop_counts, gt_boxes, gt_classes, gt_is_crowd, gt_counts, gt_area, area_rng, limit=0):
    """dtc_eval_proposal_recall: proposals f32 [N,P,4] in score order, prop_counts i32 [N], the gt tensors of eval_match, area_rng f64
    [2] on the device, limit (0: none).  -> dict(gt_overlaps f64 [N,G], n_pos i32 [N], n_overlaps i32 [N]).  No host sync."""
    dev = _require_cuda(proposals, prop_counts, gt_boxes, gt_classes, gt_is_crowd, gt_counts, gt_area, area_rng)
    if proposals.dim() != 3:
        raise TypeError("proposals: expected [N,P,4]")
    N, P = proposals.shape[0], proposals.shape[1]
    _dense("proposals", proposals, torch.float32, (N, P, 4))
    _dense("prop_counts", prop_counts, torch.int32, (N,))
    G = _gt(gt_boxes, gt_classes, gt_is_crowd, gt_counts, gt_area, N)
    _dense("area_rng", area_rng, torch.float64, (2,))
    if not (1 <= N <= MAX_BATCH and 1 <= P <= MAX_PROPOSALS and limit >= 0):
        raise ValueError("proposal_recall: unsupported shape: %d images (at most %d) x %d proposals (1 .. %d)" % (N, MAX_BATCH, P, MAX_PROPOSALS))
    e = lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=dev)
    out = dict(gt_overlaps=e(N, G, dtype=torch.float64), n_pos=e(N), n_overlaps=e(N))
    none_if_empty = lambda t: t if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_eval_proposal_recall", dict(
            proposals=proposals, prop_counts=prop_counts, gt_boxes=none_if_empty(gt_boxes), gt_classes=none_if_empty(gt_classes),
            gt_is_crowd=none_if_empty(gt_is_crowd), gt_counts=gt_counts, gt_area=none_if_empty(gt_area), batch=N, proposal_stride=P,
            gt_stride=G, area_rng=area_rng, limit=limit, gt_overlaps=none_if_empty(out["gt_overlaps"]), n_pos=out["n_pos"],
            n_overlaps=out["n_overlaps"]))
    return out
