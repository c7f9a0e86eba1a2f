"""ctypes binding of libdetectorch_mpost_hip.so (C ABI: include/detectorch_mpost_hip.h): the mask post-processing block of the
reference's lib/utils/segms.py -- rle_masks_to_boxes, maskUtils.iou on two sets of masks, the greedy walk of rle_mask_nms and
rle_mask_voting -- on the COCO run lists that hip.mask_rle, hip_poly.poly_rle, hip_flip.flip_rle and pack_gt_masks leave on the
device, without a bitmap.

A twelfth library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_mpost() on first use.
PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.  The
reference-shaped functions on top of this are utils/segms.py (rle_mask_nms, rle_mask_voting, rle_masks_to_boxes and their batched
forms).
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda
from .hip_mask import _dense

LIB_PATH = os.environ.get("DETECTORCH_MPOST_HIP_LIB") or _build.MPOST_LIB

MAX_BATCH, MAX_ROWS, MAX_RUNS, MAX_PIXELS = 65535, 512, 1 << 20, 1 << 30      # DTC_MPOST_MAX_*
NMS_MODES = {"IOU": 0, "IOMA": 1, "CONTAINMENT": 2}           # DTC_MPOST_NMS_*
VOTE_METHODS = {"AVG": 0, "UNION": 1}                         # DTC_MPOST_VOTE_*

# include/detectorch_mpost_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_mpost_target_arch()
status dtc_mpost_boxes(runs n_runs counts im_size batch:i rows_stride:i runs_stride:i boxes area nonempty stream)
size dtc_mpost_overlaps_workspace_bytes(batch:i a_rows:i a_runs_stride:i b_rows:i b_runs_stride:i)
status dtc_mpost_overlaps(a_runs a_n_runs a_count b_runs b_n_runs b_count im_size batch:i a_rows:i a_runs_stride:i b_rows:i
    b_runs_stride:i crowd:i workspace workspace_bytes:z ovr a_area b_area stream)
status dtc_mpost_nms(dets count ovr batch:i rows_stride:i thresh:d mode:i keep keep_count stream)
size dtc_mpost_vote_workspace_bytes(batch:i all_rows:i all_runs_stride:i)
status dtc_mpost_vote(top_runs top_n_runs top_count all_runs all_n_runs all_dets all_count ovr im_size batch:i top_rows:i
    top_runs_stride:i all_rows:i all_runs_stride:i dets_stride:i iou_thresh:d binarize_thresh:d method:i workspace workspace_bytes:z
    out_runs out_stride:i out_n_runs need stream)
""", {})

_lib = None


def lib():
    """Build (when stale or missing) and load the mask post-processing library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_MPOST_HIP_LIB" not in os.environ:
        _build.build_mpost()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the mask post-processing." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def _runs(name, runs, n_runs, N=None):
    """checks one side's run lists [N,R,stride] / [N,R]; -> (N, R, stride)"""
    if runs.dim() != 3:
        raise TypeError("%s: expected [N,R,runs_stride]" % name)
    n, R, stride = runs.shape
    if N is not None and n != N:
        raise TypeError("%s: expected %d images, got %d" % (name, N, n))
    _dense(name, runs, torch.int32, (n, R, stride))           # the header's uint32, held as int32 by hip.mask_rle
    _dense(name.replace("runs", "n_runs"), n_runs, torch.int32, (n, R))
    if not (1 <= n <= MAX_BATCH and 1 <= R <= MAX_ROWS and 1 <= stride <= MAX_RUNS):
        raise ValueError("%s: unsupported shape: %d images (1 .. %d) x %d rows (1 .. %d), a runs stride of %d (1 .. %d)" % (
            name, n, MAX_BATCH, R, MAX_ROWS, stride, MAX_RUNS))
    return n, R, stride


def _empty(dev):
    return lambda *shape, dtype=torch.int32: torch.empty(shape, dtype=dtype, device=dev)


def boxes_outputs(N, R, dev):
    """The output set of dtc_mpost_boxes under its parameter names: boxes i32 [N,R,4]; area, nonempty i32 [N,R]"""
    e = _empty(dev)
    return dict(boxes=e(N, R, 4), area=e(N, R), nonempty=e(N, R))


def mask_boxes(runs, n_runs, im_size, counts=None, out=None):
    """dtc_mpost_boxes on contiguous device tensors: runs i32 [N,R,runs_stride] holding uint32 run lengths, n_runs i32 [N,R], im_size
    f32 [N,2] = (h, w), counts i32 [N] or None (all R rows).  -> the dict of boxes_outputs(): the inclusive (x0, y0, x1, y1) of the set
    pixels (an empty mask: zeros), their number, and 1 where there are any.  Rows past counts are not written (allocated here:
    zeros).  No host sync."""
    dev = _require_cuda(runs, n_runs, im_size, counts)
    N, R, S = _runs("runs", runs, n_runs)
    _dense("im_size", im_size, torch.float32, (N, 2))
    if counts is not None:
        _dense("counts", counts, torch.int32, (N,))
    if out is None:
        out = boxes_outputs(N, R, dev)
        if counts is not None:
            out = {k: torch.zeros_like(v) for k, v in out.items()}
    else:
        _dense("boxes", out["boxes"], torch.int32, (N, R, 4))
        _dense("area", out["area"], torch.int32, (N, R))
        _dense("nonempty", out["nonempty"], torch.int32, (N, R))
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_mpost_boxes", dict(
            runs=runs, n_runs=n_runs, counts=counts, im_size=im_size, batch=N, rows_stride=R, runs_stride=S, **out))
    return out


def overlaps_workspace_bytes(N, Ra, a_stride, Rb, b_stride):
    return lib().dtc_mpost_overlaps_workspace_bytes(N, Ra, a_stride, Rb, b_stride)


def overlaps_outputs(N, Ra, Rb, dev):
    """The output set of dtc_mpost_overlaps under its parameter names: ovr f64 [N,Ra,Rb]; a_area i32 [N,Ra]; b_area i32 [N,Rb]"""
    e = _empty(dev)
    return dict(ovr=e(N, Ra, Rb, dtype=torch.float64), a_area=e(N, Ra), b_area=e(N, Rb))


def mask_overlaps(a_runs, a_n_runs, a_count, b_runs, b_n_runs, b_count, im_size, crowd=False, out=None, ws=None):
    """dtc_mpost_overlaps on contiguous device tensors: a_runs i32 [N,Ra,stride] / a_n_runs i32 [N,Ra] / a_count i32 [N], the same for
    b (which may be the same tensors), im_size f32 [N,2].  -> the dict of overlaps_outputs(): maskUtils.iou(a, b, [crowd] * Rb) and
    the areas; with crowd the divisor is the area of a's mask.  `out`: a preallocated dict; `ws`: a uint8 workspace of at least
    overlaps_workspace_bytes(...).  No host sync."""
    dev = _require_cuda(a_runs, a_n_runs, a_count, b_runs, b_n_runs, b_count, im_size)
    N, Ra, Sa = _runs("a_runs", a_runs, a_n_runs)
    _, Rb, Sb = _runs("b_runs", b_runs, b_n_runs, N)
    _dense("a_count", a_count, torch.int32, (N,))
    _dense("b_count", b_count, torch.int32, (N,))
    _dense("im_size", im_size, torch.float32, (N, 2))
    if out is None:
        out = overlaps_outputs(N, Ra, Rb, dev)
    else:
        _dense("ovr", out["ovr"], torch.float64, (N, Ra, Rb))
        _dense("a_area", out["a_area"], torch.int32, (N, Ra))
        _dense("b_area", out["b_area"], torch.int32, (N, Rb))
    nbytes = overlaps_workspace_bytes(N, Ra, Sa, Rb, Sb)
    if ws is None or ws.numel() < nbytes:
        ws = hip.workspace(nbytes, dev)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_mpost_overlaps", dict(
            a_runs=a_runs, a_n_runs=a_n_runs, a_count=a_count, b_runs=b_runs, b_n_runs=b_n_runs, b_count=b_count, im_size=im_size,
            batch=N, a_rows=Ra, a_runs_stride=Sa, b_rows=Rb, b_runs_stride=Sb, crowd=1 if crowd else 0, workspace=ws,
            workspace_bytes=ws.numel(), **out))
    return out


def nms_outputs(N, R, dev):
    """The output set of dtc_mpost_nms under its parameter names: keep i32 [N,R] (kept rows in the order kept, then -1); keep_count
    i32 [N]"""
    e = _empty(dev)
    return dict(keep=e(N, R), keep_count=e(N))


def mask_nms(dets, count, ovr, thresh, mode="IOU", out=None):
    """dtc_mpost_nms on contiguous device tensors: dets f32 [N,R,6] (score in column 4, class in column 5), count i32 [N], ovr f64
    [N,R,R] (mask_overlaps of the masks with themselves -- with crowd for IOMA and CONTAINMENT --, or crafted).  -> the dict of
    nms_outputs().  No host sync."""
    dev = _require_cuda(dets, count, ovr)
    if dets.dim() != 3:
        raise TypeError("dets: expected [N,R,6]")
    N, R = dets.shape[:2]
    _dense("dets", dets, torch.float32, (N, R, 6))
    _dense("count", count, torch.int32, (N,))
    _dense("ovr", ovr, torch.float64, (N, R, R))
    if mode not in NMS_MODES:
        raise NotImplementedError("Mode {} is unknown".format(mode))
    if not (1 <= N <= MAX_BATCH and 1 <= R <= MAX_ROWS):
        raise ValueError("mask_nms: unsupported shape: %d images (1 .. %d) x %d rows (1 .. %d)" % (N, MAX_BATCH, R, MAX_ROWS))
    if out is None:
        out = nms_outputs(N, R, dev)
    else:
        _dense("keep", out["keep"], torch.int32, (N, R))
        _dense("keep_count", out["keep_count"], torch.int32, (N,))
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_mpost_nms", dict(
            dets=dets, count=count, ovr=ovr, batch=N, rows_stride=R, thresh=thresh, mode=NMS_MODES[mode], **out))
    return out


def vote_workspace_bytes(N, A, all_stride):
    return lib().dtc_mpost_vote_workspace_bytes(N, A, all_stride)


def vote_outputs(N, T, out_stride, dev):
    """The output set of dtc_mpost_vote under its parameter names: out_runs i32 [N,T,out_stride] (the uint32 bits); out_n_runs, need
    i32 [N,T]"""
    e = _empty(dev)
    return dict(out_runs=e(N, T, out_stride), out_n_runs=e(N, T), need=e(N, T))


def mask_vote(top_runs, top_n_runs, top_count, all_runs, all_n_runs, all_dets, all_count, ovr, im_size, iou_thresh, binarize_thresh,
              method="AVG", out_stride=None, out=None, ws=None):
    """dtc_mpost_vote on contiguous device tensors: top_runs i32 [N,T,stride] / top_n_runs i32 [N,T] / top_count i32 [N]; all_runs
    i32 [N,A,stride'] / all_n_runs i32 [N,A] / all_dets f32 [N,A,>=5] / all_count i32 [N]; ovr f64 [N,T,A] (mask_overlaps(top, all)
    without crowd); im_size f32 [N,2].  -> the dict of vote_outputs(): the voted run lists, -1 in out_n_runs for a row that did not
    fit out_stride (default: the top stride) or came in with n_runs < 0; `need` says what every row takes.  Rows past top_count are
    not written (allocated here: zeros).  `out`: a preallocated dict (its out_runs fix out_stride, and must not share memory with
    the inputs); `ws`: a uint8 workspace of at least vote_workspace_bytes(...).  No host sync."""
    dev = _require_cuda(top_runs, top_n_runs, top_count, all_runs, all_n_runs, all_dets, all_count, ovr, im_size)
    N, T, St = _runs("top_runs", top_runs, top_n_runs)
    _, A, Sa = _runs("all_runs", all_runs, all_n_runs, N)
    if all_dets.dim() != 3 or all_dets.shape[2] < 5:
        raise TypeError("all_dets: expected [N,A,5 or more]")
    D = all_dets.shape[2]
    _dense("all_dets", all_dets, torch.float32, (N, A, D))
    _dense("top_count", top_count, torch.int32, (N,))
    _dense("all_count", all_count, torch.int32, (N,))
    _dense("ovr", ovr, torch.float64, (N, T, A))
    _dense("im_size", im_size, torch.float32, (N, 2))
    if method not in VOTE_METHODS:
        raise NotImplementedError("Method {} is unknown".format(method))
    if out is not None:
        out_stride = out["out_runs"].shape[2] if out["out_runs"].dim() == 3 else -1
    out_stride = St if out_stride is None else int(out_stride)
    if not 1 <= out_stride <= MAX_RUNS:
        raise ValueError("mask_vote: an out_stride of 1 .. %d, got %d" % (MAX_RUNS, out_stride))
    if out is None:
        out = {k: torch.zeros_like(v) for k, v in vote_outputs(N, T, out_stride, dev).items()}
    else:
        _dense("out_runs", out["out_runs"], torch.int32, (N, T, out_stride))
        _dense("out_n_runs", out["out_n_runs"], torch.int32, (N, T))
        _dense("need", out["need"], torch.int32, (N, T))
    nbytes = vote_workspace_bytes(N, A, Sa)
    if ws is None or ws.numel() < nbytes:
        ws = hip.workspace(nbytes, dev)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_mpost_vote", dict(
            top_runs=top_runs, top_n_runs=top_n_runs, top_count=top_count, all_runs=all_runs, all_n_runs=all_n_runs, all_dets=all_dets,
            all_count=all_count, ovr=ovr, im_size=im_size, batch=N, top_rows=T, top_runs_stride=St, all_rows=A, all_runs_stride=Sa,
            dets_stride=D, iou_thresh=iou_thresh, binarize_thresh=binarize_thresh, method=VOTE_METHODS[method], workspace=ws,
            workspace_bytes=ws.numel(), out_stride=out_stride, **out))
    return out
