"""ctypes binding of libdetectorch_aug_hip.so (C ABI: include/detectorch_aug_hip.h): test-time augmentation on the batched path --
the merge of the box-head outputs of several views of a batch into one candidate set per image (im_detect_bbox_aug's rule), which
dtc_postprocess_detections_ex2 takes through decoded_boxes, and the combination of the views' mask probabilities for the final
detections (im_detect_mask_aug's), which dtc_mask_paste takes.

A thirteenth library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_aug() on first use.
PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.  The model-level
entry on top of this is utils/test_aug.py (AugOptions, detect_aug).
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda
from .hip_mask import _dense

LIB_PATH = os.environ.get("DETECTORCH_AUG_HIP_LIB") or _build.AUG_LIB

MAX_VIEWS, MAX_ROIS, MAX_ROWS, MAX_CLASSES, MAX_BATCH = 8, 4096, 32768, 256, 65535      # DTC_AUG_MAX_*
MAX_MASK, MAX_CHANNELS, MAX_MASK_ROWS = 64, 1024, 1 << 20
BOX_HEURS = {"UNION": 0, "AVG": 1, "ID": 2}                   # DTC_AUG_UNION / AVG / ID
MASK_HEURS = {"SOFT_AVG": 0, "SOFT_MAX": 1, "LOGIT_AVG": 2}   # DTC_AUG_SOFT_AVG / SOFT_MAX / LOGIT_AVG


class AugView(C.Structure):
    """struct dtc_aug_view (include/detectorch_aug_hip.h)"""
    _fields_ = [("rois5", C.c_void_p), ("n_rois", C.c_void_p), ("cls_score", C.c_void_p), ("bbox_pred", C.c_void_p),
                ("scale", C.c_void_p), ("flipped", C.c_int32), ("_pad", C.c_int32)]


# include/detectorch_aug_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_aug_target_arch()
status dtc_aug_merge_boxes(views:AugView n_views:i im_size batch:i max_rois:i n_cls:i scores_are_logits:i wx:f wy:f ww:f wh:f
    score_heur:i coord_heur:i out_scores out_boxes out_n out_src stream)
status dtc_aug_combine_masks(masks flipped n_views:i det_count mask_class batch:i max_out:i n_cls:i M:i heur:i out stream)
""", {"AugView": AugView})

_lib = None


def lib():
    """Build (when stale or missing) and load the augmentation library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_AUG_HIP_LIB" not in os.environ:
        _build.build_aug()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the test-time augmentation." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def box_heurs(score_heur, coord_heur):
    """The pair of heuristics as DTC_AUG_* codes.  Detectron's rule (core/test.py:im_detect_bbox_aug): UNION for both or for neither."""
    for h in (score_heur, coord_heur):
        if h not in BOX_HEURS:
            raise NotImplementedError("Heur {} not supported".format(h))
    if (score_heur == "UNION") != (coord_heur == "UNION"):
        raise ValueError("Coord and score heuristics must both be UNION or neither: got score_heur=%s, coord_heur=%s"
                         % (score_heur, coord_heur))
    return BOX_HEURS[score_heur], BOX_HEURS[coord_heur]


def merge_rows(n_views, max_rois, score_heur="UNION"):
    """Output rows per image of merge_boxes: T R under UNION, R otherwise; ValueError past the limits of the header."""
    if not (1 <= n_views <= MAX_VIEWS and 1 <= max_rois <= MAX_ROIS and n_views * max_rois <= MAX_ROWS):
        raise ValueError("merge_boxes: unsupported shape: %d views (1 .. %d) x %d rois (1 .. %d), %d rows in all (.. %d)" % (
            n_views, MAX_VIEWS, max_rois, MAX_ROIS, n_views * max_rois, MAX_ROWS))
    return n_views * max_rois if score_heur == "UNION" else max_rois


def merge_outputs(B, rows, n_cls, dev):
    """The output set of dtc_aug_merge_boxes under its parameter names: out_scores f32 [B,rows,n_cls]; out_boxes f32 [B,rows,4 n_cls];
    out_n i32 [B]; out_src i32 [B,rows]"""
    e = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    return dict(out_scores=e(B, rows, n_cls), out_boxes=e(B, rows, 4 * n_cls), out_n=e(B, dtype=torch.int32),
                out_src=e(B, rows, dtype=torch.int32))


def merge_boxes(views, im_size, score_heur="UNION", coord_heur="UNION", scores_are_logits=False, weights=(10.0, 10.0, 5.0, 5.0),
                out=None):
    """dtc_aug_merge_boxes on contiguous device tensors.  views: a sequence of dicts with rois5 f32 [B,R,5], n_rois i32 [B] or None,
    cls_score f32 [B,R,n_cls], bbox_pred f32 [B,R,4 n_cls], scale f32 [B] and flipped (bool); im_size f32 [B,2] = the original
    (h, w).  -> the dict of merge_outputs(): probabilities and decoded, clipped, un-mirrored boxes in original-image coordinates, the
    rows past out_n zeros (out_src -1).  `out`: a preallocated dict.  No host sync."""
    views = list(views)
    if not views:
        raise ValueError("merge_boxes: at least one view")
    v0 = views[0]
    dev = _require_cuda(im_size, *[t for v in views for t in (v["rois5"], v.get("n_rois"), v["cls_score"], v["bbox_pred"], v["scale"])])
    if v0["cls_score"].dim() != 3:
        raise TypeError("cls_score: expected [B,R,n_cls]")
    B, R, n_cls = v0["cls_score"].shape
    sh, ch = box_heurs(score_heur, coord_heur)
    rows = merge_rows(len(views), R, score_heur)
    if not (2 <= n_cls <= MAX_CLASSES + 1 and 1 <= B <= MAX_BATCH):
        raise ValueError("merge_boxes: unsupported shape: %d classes (2 .. %d), %d images (1 .. %d)" % (n_cls, MAX_CLASSES + 1, B, MAX_BATCH))
    arr = (AugView * len(views))()
    for t, v in enumerate(views):
        _dense("rois5", v["rois5"], torch.float32, (B, R, 5))
        _dense("cls_score", v["cls_score"], torch.float32, (B, R, n_cls))
        _dense("bbox_pred", v["bbox_pred"], torch.float32, (B, R, 4 * n_cls))
        _dense("scale", v["scale"], torch.float32, (B,))
        if v.get("n_rois") is not None:
            _dense("n_rois", v["n_rois"], torch.int32, (B,))
        arr[t] = AugView(v["rois5"].data_ptr(), None if v.get("n_rois") is None else v["n_rois"].data_ptr(), v["cls_score"].data_ptr(),
                         v["bbox_pred"].data_ptr(), v["scale"].data_ptr(), 1 if v.get("flipped") else 0, 0)
    _dense("im_size", im_size, torch.float32, (B, 2))
    if out is None:
        out = merge_outputs(B, rows, n_cls, dev)
    else:
        _dense("out_scores", out["out_scores"], torch.float32, (B, rows, n_cls))
        _dense("out_boxes", out["out_boxes"], torch.float32, (B, rows, 4 * n_cls))
        _dense("out_n", out["out_n"], torch.int32, (B,))
        _dense("out_src", out["out_src"], torch.int32, (B, rows))
    wx, wy, ww, wh = (float(w) for w in weights)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_aug_merge_boxes", dict(
            views=arr, n_views=len(views), im_size=im_size, batch=B, max_rois=R, n_cls=n_cls, scores_are_logits=bool(scores_are_logits),
            wx=wx, wy=wy, ww=ww, wh=wh, score_heur=sh, coord_heur=ch, **out))
    return out


def combine_masks(masks, flipped, det_count, mask_class=None, heur="SOFT_AVG", out=None):
    """dtc_aug_combine_masks on contiguous device tensors.  masks: a sequence of T tensors f32 [B*max_out,K,M,M] (the mask-head
    probabilities of the same detections in each view); flipped: T bools (read mirrored along the last axis); det_count i32 [B];
    mask_class i32 [B*max_out] or None (every channel).  -> out f32 [B*max_out,K,M,M]: every element written; rows past det_count and,
    with mask_class, the channels that are not the row's class are +0.0.  No host sync."""
    masks, flipped = list(masks), list(flipped)
    if not masks or len(masks) != len(flipped):
        raise ValueError("combine_masks: as many flip flags as views, and at least one view")
    if heur not in MASK_HEURS:
        raise NotImplementedError("Heuristic {} not supported".format(heur))
    dev = _require_cuda(det_count, mask_class, out, *masks)
    if masks[0].dim() != 4 or masks[0].shape[2] != masks[0].shape[3]:
        raise TypeError("masks: expected [B*max_out,K,M,M]")
    N, K, M, _ = masks[0].shape
    T, B = len(masks), int(det_count.shape[0]) if det_count.dim() == 1 else 0
    if B < 1 or N % B or N < 1:
        raise TypeError("det_count: expected [B] with B dividing the %d mask rows" % N)
    if not (T <= MAX_VIEWS and M <= MAX_MASK and K <= MAX_CHANNELS and B <= MAX_BATCH and N <= MAX_MASK_ROWS):
        raise ValueError("combine_masks: unsupported shape: %d views (.. %d), M = %d (.. %d), %d channels (.. %d), %d images (.. %d), "
                         "%d rows (.. %d)" % (T, MAX_VIEWS, M, MAX_MASK, K, MAX_CHANNELS, B, MAX_BATCH, N, MAX_MASK_ROWS))
    for m in masks:
        _dense("masks", m, torch.float32, (N, K, M, M))
    _dense("det_count", det_count, torch.int32, (B,))
    if mask_class is not None:
        _dense("mask_class", mask_class, torch.int32, (N,))
    if out is None:
        out = torch.empty((N, K, M, M), dtype=torch.float32, device=dev)
    else:
        _dense("out", out, torch.float32, (N, K, M, M))
    ptrs = (C.c_void_p * T)(*[m.data_ptr() for m in masks])
    flags = (C.c_int32 * T)(*[1 if f else 0 for f in flipped])
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_aug_combine_masks", dict(
            masks=ptrs, flipped=flags, n_views=T, det_count=det_count, mask_class=mask_class, batch=B, max_out=N // B, n_cls=K, M=M,
            heur=MASK_HEURS[heur], out=out))
    return out
