"""ctypes binding of libdetectorch_kps_hip.so (C ABI: include/detectorch_kps_hip.h): keypoint inference on the batched path -- the
keypoint head's K heatmaps per detection to K keypoints (x, y, logit, prob) in image coordinates, Detectron's
utils/keypoints.py:heatmaps_to_keypoints with cv2.resize(INTER_CUBIC), without the resized maps ever existing in memory.

A fourteenth library next to libdetectorch_hip.so (hip.py) and the other side libraries, built by build.build_kps() on first use.
PyTorch is used for device memory and the current HIP stream only; there is NO CPU fallback: CPU tensors raise.  The entries with
Detectron's shapes on top of this are in utils/keypoints.py; the model-level one is detector(use_keypoint_head=True).
"""
import ctypes as C
import os

import torch

from . import build as _build
from . import hip
from .hip import _require_cuda
from .hip_mask import _dense

LIB_PATH = os.environ.get("DETECTORCH_KPS_HIP_LIB") or _build.KPS_LIB

MAX_MAP, MAX_KEYPOINTS, MAX_OUT, MAX_BATCH, MAX_MAPS, MAX_SIDE = 64, 64, 4096, 65535, 1 << 20, 4096      # DTC_KPS_MAX_*

# include/detectorch_kps_hip.h, one row per exported function (the format of hip._SIGNATURES)
SIGNATURES = hip.signatures("""
str dtc_kps_target_arch()
size dtc_kps_workspace_bytes(batch:i max_out:i K:i)
status dtc_kps_heatmaps_to_keypoints(heatmaps dets det_count batch:i max_out:i K:i S:i person_class:i min_size:i workspace
    workspace_bytes:z keyps kp_status stream)
""", {})

_lib = None


def lib():
    """Build (when stale or missing) and load the keypoint library, or fail loudly."""
    global _lib
    if _lib is not None:
        return _lib
    if "DETECTORCH_KPS_HIP_LIB" not in os.environ:
        _build.build_kps()
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("detectorch_amd: %s is missing. Build it with `python -m detectorch_amd.build` (hipcc, gfx950). "
                           "There is no CPU/PyTorch fallback for the keypoint inference." % LIB_PATH)
    _lib = hip.typed(C.CDLL(LIB_PATH), SIGNATURES)
    return _lib


def _check_shape(B, max_out, K):
    if not (1 <= B <= MAX_BATCH and 1 <= max_out <= MAX_OUT and 1 <= K <= MAX_KEYPOINTS and B * max_out * K <= MAX_MAPS):
        raise ValueError("heatmaps_to_keypoints: unsupported shape: %d images (1 .. %d) x %d rows (1 .. %d) x %d keypoints (1 .. %d), "
                         "%d maps in all (.. %d)" % (B, MAX_BATCH, max_out, MAX_OUT, K, MAX_KEYPOINTS, B * max_out * K, MAX_MAPS))


def keypoint_outputs(B, max_out, K, dev):
    """The output set of dtc_kps_heatmaps_to_keypoints under its parameter names: keyps f32 [B,max_out,4,K]; kp_status i32
    [B,max_out]"""
    _check_shape(B, max_out, K)
    return dict(keyps=torch.empty((B, max_out, 4, K), dtype=torch.float32, device=dev),
                kp_status=torch.empty((B, max_out), dtype=torch.int32, device=dev))


def workspace(B, max_out, K, dev):
    """The workspace of one (B, max_out, K): a uint8 tensor of dtc_kps_workspace_bytes."""
    _check_shape(B, max_out, K)
    return torch.empty((max(int(hip.invoke(lib(), SIGNATURES, "dtc_kps_workspace_bytes", dict(batch=B, max_out=max_out, K=K))), 16),),
                       dtype=torch.uint8, device=dev)


def heatmaps_to_keypoints(heatmaps, dets, det_count, person_class=-1, min_size=0, out=None, ws=None):
    """dtc_kps_heatmaps_to_keypoints on contiguous device tensors.  heatmaps f32 [B*max_out,K,S,S] (row b*max_out+d belongs to
    detection (b,d)); dets f32 [B,max_out,6]; det_count i32 [B]; person_class >= 0: only the rows of that class, -1: every row below
    the count; min_size: KRCNN.INFERENCE_MIN_SIZE (0: off).  -> the dict of keypoint_outputs(): keyps [B,max_out,4,K] = x, y, logit,
    prob and kp_status [B,max_out] = 1 computed, 0 not a live row, -1 refused (a non-finite box or a resized side above 4096), the
    rows that are not computed zeros.  `out`: a preallocated dict; `ws`: a preallocated workspace().  No host sync."""
    dev = _require_cuda(heatmaps, dets, det_count, ws, *(out or {}).values())
    if dets.dim() != 3 or dets.shape[2] != 6:
        raise TypeError("dets: expected [B,max_out,6]")
    B, max_out = int(dets.shape[0]), int(dets.shape[1])
    if heatmaps.dim() != 4 or heatmaps.shape[0] != B * max_out or heatmaps.shape[2] != heatmaps.shape[3]:
        raise TypeError("heatmaps: expected [B*max_out,K,S,S] with B*max_out = %d" % (B * max_out))
    K, S = int(heatmaps.shape[1]), int(heatmaps.shape[2])
    _check_shape(B, max_out, K)
    if not (1 <= S <= MAX_MAP and 0 <= int(min_size) <= MAX_SIDE and int(person_class) >= -1):
        raise ValueError("heatmaps_to_keypoints: S = %d (1 .. %d), min_size = %d (0 .. %d), person_class = %d (>= -1)"
                         % (S, MAX_MAP, min_size, MAX_SIDE, person_class))
    _dense("heatmaps", heatmaps, torch.float32, (B * max_out, K, S, S))
    _dense("dets", dets, torch.float32, (B, max_out, 6))
    _dense("det_count", det_count, torch.int32, (B,))
    if out is None:
        out = keypoint_outputs(B, max_out, K, dev)
    else:
        _dense("keyps", out["keyps"], torch.float32, (B, max_out, 4, K))
        _dense("kp_status", out["kp_status"], torch.int32, (B, max_out))
    if ws is None:
        ws = workspace(B, max_out, K, dev)
    with torch.cuda.device(dev):
        hip.invoke(lib(), SIGNATURES, "dtc_kps_heatmaps_to_keypoints", dict(
            heatmaps=heatmaps, dets=dets, det_count=det_count, batch=B, max_out=max_out, K=K, S=S, person_class=person_class,
            min_size=min_size, workspace=ws, workspace_bytes=ws.numel(), **out))
    return out
