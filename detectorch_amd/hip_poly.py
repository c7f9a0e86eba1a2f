"""ctypes binding of libdetectorch_poly_hip.so (C ABI: include/detectorch_poly_hip.h): COCO ground-truth polygons at image size,
straight to run lists on the device -- pycocotools' annToRLE for polygon annotations (rleFrPoly per polygon, merge per instance).
The run lists are hip_segm.segm_iou's gt_runs / gt_n_runs.

A tenth library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_poly() on first use.
PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.  The loader-side
functions on top of this are detectorch_amd/utils/segms.py.
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda
from .hip_mask import _dense

LIB_PATH = os.environ.get("DETECTORCH_POLY_HIP_LIB") or _build.POLY_LIB

MAX_GT, MAX_POLYS, MAX_POINTS, MAX_BATCH, MAX_RUNS, MAX_PIXELS = 256, 4096, 65536, 65535, 1 << 20, 1 << 30      # DTC_POLY_MAX_*
MAX_EVENTS = 8192                                            # DTC_POLY_MAX_EVENTS; csrc/poly_rle: kPolyMaxEvents
SORT_CAPACITIES = (2048, 4096, 8192)                         # csrc/poly_rle: the keys the three workgroup sizes of node 2 sort

# include/detectorch_poly_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_poly_target_arch()
size dtc_poly_rle_workspace_bytes(batch:i gt_stride:i points_stride:i polys_stride:i events_stride:i)
status dtc_poly_rle(poly_xy poly_ptr gt_poly_ptr gt_counts im_size batch:i gt_stride:i points_stride:i polys_stride:i events_stride:i
    workspace workspace_bytes:z runs runs_stride:i n_runs area need stream)
""", {})

_lib = None


def lib():
    """Build (when stale or missing) and load the polygon library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_POLY_HIP_LIB" not in os.environ:
        _build.build_poly()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the polygon conversion." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def rle_workspace_bytes(N, G, PTS, NP, events_stride):
    return lib().dtc_poly_rle_workspace_bytes(N, G, PTS, NP, events_stride)


def rle_outputs(N, G, runs_stride, dev):
    """The output set of dtc_poly_rle under its parameter names: runs i32 [N,G,runs_stride] (the uint32 bits, as hip.mask_rle holds
    them); n_runs, area i32 [N,G]; need i32 [N,G,2]."""
    e = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    return dict(runs=e(N, G, runs_stride), n_runs=e(N, G), area=e(N, G), need=e(N, G, 2))


def poly_rle(poly_xy, poly_ptr, gt_poly_ptr, gt_counts, im_size, runs_stride, events_stride, out=None, ws=None):
    """dtc_poly_rle on contiguous device tensors: poly_xy f64 [N,PTS,2], poly_ptr i32 [N,NP+1], gt_poly_ptr i32 [N,G+1] (the layout of
    utils.segms.pack_polygons64), gt_counts i32 [N], im_size f32 [N,2] = (h, w).  -> the dict of rle_outputs(); `out`: a preallocated
    one to write into (its runs fix runs_stride); `ws`: a uint8 workspace of at least rle_workspace_bytes(...) (allocated when None or
    too small).  No host sync."""
    dev = _require_cuda(poly_xy, poly_ptr, gt_poly_ptr, gt_counts, im_size)
    if poly_xy.dim() != 3 or poly_ptr.dim() != 2 or gt_poly_ptr.dim() != 2:
        raise TypeError("poly_rle: expected poly_xy [N,PTS,2], poly_ptr [N,NP+1], gt_poly_ptr [N,G+1]")
    N, PTS, NP, G = poly_xy.shape[0], poly_xy.shape[1], poly_ptr.shape[1] - 1, gt_poly_ptr.shape[1] - 1
    _dense("poly_xy", poly_xy, torch.float64, (N, PTS, 2))
    _dense("poly_ptr", poly_ptr, torch.int32, (N, NP + 1))
    _dense("gt_poly_ptr", gt_poly_ptr, torch.int32, (N, G + 1))
    _dense("gt_counts", gt_counts, torch.int32, (N,))
    _dense("im_size", im_size, torch.float32, (N, 2))
    if out is not None:
        runs_stride = out["runs"].shape[2] if out["runs"].dim() == 3 else -1
    runs_stride, events_stride = int(runs_stride), int(events_stride)
    if not (1 <= N <= MAX_BATCH and 0 <= G <= MAX_GT and 0 <= NP <= MAX_POLYS and PTS <= MAX_POINTS):
        raise ValueError("poly_rle: unsupported shape: %d images (at most %d) x %d gt rows (at most %d), %d polygons (at most %d), %d "
                         "points (at most %d)" % (N, MAX_BATCH, G, MAX_GT, NP, MAX_POLYS, PTS, MAX_POINTS))
    if not 1 <= runs_stride <= MAX_RUNS:
        raise ValueError("poly_rle: a runs stride of 1 .. %d, got %d" % (MAX_RUNS, runs_stride))
    if not 1 <= events_stride <= MAX_EVENTS:
        raise ValueError("poly_rle: an events stride of 1 .. %d, got %d" % (MAX_EVENTS, events_stride))
    if out is None:
        out = rle_outputs(N, G, runs_stride, dev)
    else:
        _dense("runs", out["runs"], torch.int32, (N, G, runs_stride))
        _dense("n_runs", out["n_runs"], torch.int32, (N, G))
        _dense("area", out["area"], torch.int32, (N, G))
        _dense("need", out["need"], torch.int32, (N, G, 2))
    need = rle_workspace_bytes(N, G, PTS, NP, events_stride)
    if ws is None or ws.numel() < need:
        ws = hip.workspace(need, dev)
    none_if_empty = lambda t: t if t is not None and t.numel() else None
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_poly_rle", dict(
            poly_xy=none_if_empty(poly_xy), poly_ptr=poly_ptr, gt_poly_ptr=gt_poly_ptr, gt_counts=gt_counts, im_size=im_size, batch=N,
            gt_stride=G, points_stride=PTS, polys_stride=NP, events_stride=events_stride, workspace=ws, workspace_bytes=ws.numel(),
            runs_stride=runs_stride, **{k: none_if_empty(out[k]) for k in ("runs", "n_runs", "area", "need")}))
    return out
