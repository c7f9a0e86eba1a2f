"""ctypes binding of libdetectorch_flip_hip.so (C ABI: include/detectorch_flip_hip.h): the horizontal-flip augmentation of the
reference's training data (roidb.py:extend_with_flipped_entries, segms.py:flip_segms, boxes.py:flip_boxes, the image[:, ::-1, :] of
coco_dataset.py:51-53) on the device -- the network input of mirrored images folded into the prep kernel's tap addresses, boxes,
polygons, and COCO run lists mirrored without a bitmap.

An eleventh library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_flip() on first use.
PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.  The loader-side
functions on top of this are utils/blob.py (images_to_blob(flipped=)), utils/boxes.py (flip_boxes), utils/segms.py (flip_segms) and
utils/augment.py (flip_batch, extend_with_flipped_entries).
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda
from .hip_mask import _dense

LIB_PATH = os.environ.get("DETECTORCH_FLIP_HIP_LIB") or _build.FLIP_LIB

MAX_BATCH, MAX_BOX_ROWS, MAX_BOX_COLS, MAX_POINTS, MAX_POLYS = 65535, 1 << 20, 4096, 65536, 4096      # DTC_FLIP_MAX_*
MAX_ROWS, MAX_RUNS, MAX_PIXELS = 65535, 1 << 20, 1 << 30
MAX_PREP_BATCH = 32                                           # csrc/prep_pixel.h: kPrepMaxBatch

# include/detectorch_flip_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_flip_target_arch()
status dtc_flip_prep_images(images:Image batch:i flipped pixel_means im_scales out_hw blob blob_h:i blob_w:i stream)
status dtc_flip_boxes(boxes counts im_width flipped batch:i rows_stride:i cols:i out stream)
status dtc_flip_polygons(poly_xy poly_ptr im_width flipped batch:i points_stride:i polys_stride:i out64 out32 stream)
size dtc_flip_rle_workspace_bytes(batch:i rows_stride:i runs_stride:i)
status dtc_flip_rle(runs n_runs counts im_size flipped batch:i rows_stride:i runs_stride:i workspace workspace_bytes:z out_runs
    out_stride:i out_n_runs need stream)
""", {"Image": hip.Image})

_lib = None


def lib():
    """Build (when stale or missing) and load the flip library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_FLIP_HIP_LIB" not in os.environ:
        _build.build_flip()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the flip augmentation." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def _flags(flipped, B, dev, name="flipped"):
    """per-image flags as an int32 [B] device tensor: a tensor is taken as it is (no sync), a host sequence is uploaded"""
    if torch.is_tensor(flipped):
        _require_cuda(flipped)
        t = flipped if flipped.dtype == torch.int32 else flipped.to(torch.int32)
    else:
        t = torch.tensor([int(v) for v in flipped], dtype=torch.int32, device=dev)
    _dense(name, t, torch.int32, (B,))
    return t


def prep_images(images, flipped, pixel_means=(122.7717, 115.9465, 102.9801), target_size=800, max_size=1333, pad_stride=32):
    """hip.prep_images with image b mirrored left to right where flipped[b] (a HOST sequence of B flags, read at call time):
    dtc_prep_plan + dtc_flip_prep_images.  list of HWC BGR CUDA tensors (uint8 or float32, [h,w,3]) -> (blob float32 [B,3,Hb,Wb] on the
    device, im_scales list of float, resized sizes list of (h, w)).  A mirrored image's plane is bit-equal to hip.prep_images on
    torch.flip(im, [1]); the others to hip.prep_images on the image."""
    dev = _require_cuda(*images)
    B = len(images)
    if torch.is_tensor(flipped):
        raise TypeError("prep_images: flipped is a host sequence (the flags travel as kernel arguments), got a tensor")
    if len(flipped) != B:
        raise ValueError("prep_images: %d flags for %d images" % (len(flipped), B))
    ims = [im if im.stride(2) == 1 and im.stride(1) == 3 else im.contiguous() for im in images]
    hs = (C.c_int32 * B)(*[int(im.shape[0]) for im in ims])
    ws_ = (C.c_int32 * B)(*[int(im.shape[1]) for im in ims])
    scales = (C.c_double * B)()
    out_hw = (C.c_int32 * (2 * B))()
    blob_hw = (C.c_int32 * 2)()
    hip.call("dtc_prep_plan", heights=hs, widths=ws_, batch=B, target_size=target_size, max_size=max_size, pad_stride=pad_stride,
             im_scales=scales, out_hw=out_hw, blob_hw=blob_hw)
    arr = (hip.Image * B)()
    for k, im in enumerate(ims):
        if im.dtype == torch.uint8:
            dt = 2
        elif im.dtype == torch.float32:
            dt = 0
        else:
            raise TypeError("images must be uint8 or float32")
        if im.dim() != 3 or im.shape[2] != 3:
            raise ValueError("images must be [h,w,3] (BGR)")
        arr[k] = hip.Image(im.data_ptr(), int(im.shape[0]), int(im.shape[1]), dt, int(im.stride(0)))
    flags = (C.c_int32 * B)(*[1 if f else 0 for f in flipped])
    means = (C.c_double * 3)(*[float(m) for m in pixel_means])
    blob = torch.empty((B, 3, blob_hw[0], blob_hw[1]), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_flip_prep_images", dict(
            images=arr, batch=B, flipped=flags, pixel_means=means, im_scales=scales, out_hw=out_hw, blob=blob, blob_h=blob_hw[0],
            blob_w=blob_hw[1]))
    del ims
    return blob, [float(s) for s in scales], [(out_hw[2 * k], out_hw[2 * k + 1]) for k in range(B)]


def flip_boxes(boxes, im_width, flipped, counts=None, out=None):
    """dtc_flip_boxes on contiguous device tensors: boxes f32 [B,R,cols] (cols a positive multiple of 4), im_width i32 [B], flipped i32
    [B] (or a host sequence, uploaded), counts i32 [B] or None (all R rows).  -> out f32 [B,R,cols]; `out` may be `boxes` (in place).
    No host sync."""
    dev = _require_cuda(boxes, im_width, counts, out)
    if boxes.dim() != 3:
        raise TypeError("flip_boxes: expected boxes [B,R,cols]")
    B, R, cols = boxes.shape
    _dense("boxes", boxes, torch.float32, (B, R, cols))
    _dense("im_width", im_width, torch.int32, (B,))
    flipped = _flags(flipped, B, dev)
    if counts is not None:
        _dense("counts", counts, torch.int32, (B,))
    if cols < 4 or cols % 4:
        raise ValueError("flip_boxes: cols must be a positive multiple of 4, got %d" % cols)
    if not (1 <= B <= MAX_BATCH and R <= MAX_BOX_ROWS and cols <= MAX_BOX_COLS):
        raise ValueError("flip_boxes: unsupported shape %s: at most %d images x %d rows x %d columns" % (
            tuple(boxes.shape), MAX_BATCH, MAX_BOX_ROWS, MAX_BOX_COLS))
    if out is None:
        out = torch.empty_like(boxes)
    else:
        _dense("out", out, torch.float32, (B, R, cols))
    none_if_empty = lambda t: t if t.numel() else None
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_flip_boxes", dict(
            boxes=none_if_empty(boxes), counts=counts, im_width=im_width, flipped=flipped, batch=B, rows_stride=R, cols=cols,
            out=none_if_empty(out)))
    return out


def flip_polygons(poly_xy, poly_ptr, im_width, flipped, want64=True, want32=True, out64=None, out32=None):
    """dtc_flip_polygons on contiguous device tensors: poly_xy f64 [B,PTS,2], poly_ptr i32 [B,NP+1] (utils.segms.pack_polygons64),
    im_width i32 [B], flipped i32 [B] (or a host sequence).  -> (out64 f64 [B,PTS,2] or None, out32 f32 [B,PTS,2] or None): the x of
    every point below poly_ptr[b][NP] of a flipped image becomes w - x - 1 in double; out32 is the float32 rounding of that double.
    want64 / want32 choose what is allocated when out64 / out32 are not given; out64 may be poly_xy.  No host sync."""
    dev = _require_cuda(poly_xy, poly_ptr, im_width, out64, out32)
    if poly_xy.dim() != 3 or poly_ptr.dim() != 2:
        raise TypeError("flip_polygons: expected poly_xy [B,PTS,2], poly_ptr [B,NP+1]")
    B, PTS, NP = poly_xy.shape[0], poly_xy.shape[1], poly_ptr.shape[1] - 1
    _dense("poly_xy", poly_xy, torch.float64, (B, PTS, 2))
    _dense("poly_ptr", poly_ptr, torch.int32, (B, NP + 1))
    _dense("im_width", im_width, torch.int32, (B,))
    flipped = _flags(flipped, B, dev)
    if not (1 <= B <= MAX_BATCH and PTS <= MAX_POINTS and 0 <= NP <= MAX_POLYS):
        raise ValueError("flip_polygons: unsupported shape: %d images (at most %d), %d points (at most %d), %d polygons (at most %d)" % (
            B, MAX_BATCH, PTS, MAX_POINTS, NP, MAX_POLYS))
    if out64 is None and want64:
        out64 = torch.empty_like(poly_xy)
    if out32 is None and want32:
        out32 = torch.empty((B, PTS, 2), dtype=torch.float32, device=dev)
    if out64 is None and out32 is None:
        raise ValueError("flip_polygons: at least one of out64 / out32")
    if out64 is not None:
        _dense("out64", out64, torch.float64, (B, PTS, 2))
    if out32 is not None:
        _dense("out32", out32, torch.float32, (B, PTS, 2))
    if PTS == 0:                                              # no point: no output element
        return out64, out32
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_flip_polygons", dict(
            poly_xy=poly_xy, poly_ptr=poly_ptr, im_width=im_width, flipped=flipped, batch=B, points_stride=PTS, polys_stride=NP,
            out64=out64, out32=out32))
    return out64, out32


def rle_workspace_bytes(N, R, runs_stride):
    return lib().dtc_flip_rle_workspace_bytes(N, R, runs_stride)


def rle_outputs(N, R, out_stride, dev):
    """The output set of dtc_flip_rle under its parameter names: out_runs i32 [N,R,out_stride] (the uint32 bits); out_n_runs, need
    i32 [N,R]"""
    e = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    return dict(out_runs=e(N, R, out_stride), out_n_runs=e(N, R), need=e(N, R))


def flip_rle(runs, n_runs, im_size, flipped, counts=None, out_stride=None, out=None, ws=None):
    """dtc_flip_rle on contiguous device tensors: runs i32 [N,R,runs_stride] holding uint32 run lengths and n_runs i32 [N,R] (as
    hip.mask_rle, hip_poly.poly_rle and pack_gt_masks leave them), im_size f32 [N,2] = (h, w), flipped i32 [N] (or a host sequence),
    counts i32 [N] or None (all R rows).  -> the dict of rle_outputs(): the run lists of the mirrored masks, -1 in out_n_runs for a
    row that did not fit out_stride (default: runs_stride), came in with n_runs < 0 or does not sum to h w; `need` says what every
    row takes.  Rows past counts are not written (allocated here: zeros).  `out`: a preallocated dict (its out_runs fix out_stride,
    and must not share memory with runs); `ws`: a uint8 workspace of at least rle_workspace_bytes(...).  No host sync."""
    dev = _require_cuda(runs, n_runs, im_size, counts)
    if runs.dim() != 3:
        raise TypeError("flip_rle: expected runs [N,R,runs_stride]")
    N, R, S = runs.shape
    _dense("runs", runs, torch.int32, (N, R, S))
    _dense("n_runs", n_runs, torch.int32, (N, R))
    _dense("im_size", im_size, torch.float32, (N, 2))
    flipped = _flags(flipped, N, dev)
    if counts is not None:
        _dense("counts", counts, torch.int32, (N,))
    if out is not None:
        out_stride = out["out_runs"].shape[2] if out["out_runs"].dim() == 3 else -1
    out_stride = S if out_stride is None else int(out_stride)
    if not (1 <= N <= MAX_BATCH and R <= MAX_ROWS and 1 <= S <= MAX_RUNS and 1 <= out_stride <= MAX_RUNS):
        raise ValueError("flip_rle: unsupported shape: %d images (at most %d) x %d rows (at most %d), strides %d and %d (1 .. %d)" % (
            N, MAX_BATCH, R, MAX_ROWS, S, out_stride, MAX_RUNS))
    if out is None:
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)
        out = dict(out_runs=z(N, R, out_stride), out_n_runs=z(N, R), need=z(N, R)) if counts is not None else rle_outputs(N, R, out_stride, dev)
    else:
        _dense("out_runs", out["out_runs"], torch.int32, (N, R, out_stride))
        _dense("out_n_runs", out["out_n_runs"], torch.int32, (N, R))
        _dense("need", out["need"], torch.int32, (N, R))
    nbytes = rle_workspace_bytes(N, R, S)
    if ws is None or ws.numel() < nbytes:
        ws = hip.workspace(nbytes, dev)
    none_if_empty = lambda t: t if t.numel() else None
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_flip_rle", dict(
            runs=none_if_empty(runs), n_runs=none_if_empty(n_runs), counts=counts, im_size=im_size, flipped=flipped, batch=N,
            rows_stride=R, runs_stride=S, workspace=ws, workspace_bytes=ws.numel(), out_stride=out_stride,
            **{k: none_if_empty(out[k]) for k in ("out_runs", "out_n_runs", "need")}))
    return out
