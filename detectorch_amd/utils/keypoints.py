"""Keypoint post-processing with Detectron's names and shapes (utils/keypoints.py:heatmaps_to_keypoints, core/test.py:
keypoint_results), the arithmetic done by the HIP kernels of detectorch_amd/csrc/kps (include/detectorch_kps_hip.h).  The
reference has no keypoint code; the rule is restated in tests/kps_ref.py and parity with Detectron and cv2 themselves is unpinned
(tests/README_keypoints.md).

    heatmaps_to_keypoints   utils/keypoints.py:heatmaps_to_keypoints
    keypoint_results        core/test.py:keypoint_results

The batched path does the same without leaving the device: detector(use_keypoint_head=True).forward_batched leaves path.keyps and
path.kp_status, which result_utils.assemble_results(keyps=..., kp_status=...) turns into all_keyps.
"""
import numpy as np
import torch

from .. import hip_kps
from .result_utils import _dev


def heatmaps_to_keypoints(maps, rois, min_size=0):
    """maps [N, K, S, S] keypoint logits (ndarray or device tensor), rois [N, 4] (x1, y1, x2, y2) -> ndarray float32 [N, 4, K] of
    (x, y, logit, prob): the N rows as the detections of one image.  A refused row (a non-finite box, a resized side above 4096)
    raises ValueError."""
    dev = _dev(maps, rois)
    maps_t = maps if torch.is_tensor(maps) else torch.from_numpy(np.ascontiguousarray(maps, np.float32))
    maps_t = maps_t.to(device=dev, dtype=torch.float32).contiguous()
    rois = np.ascontiguousarray(rois.detach().cpu().numpy() if torch.is_tensor(rois) else rois, np.float32).reshape(-1, 4)
    N = rois.shape[0]
    if maps_t.dim() != 4 or maps_t.shape[0] != N:
        raise ValueError("maps [N,K,S,S] and rois [N,4] must have as many rows")
    if N == 0:
        return np.zeros((0, 4, maps_t.shape[1]), np.float32)
    dets = np.zeros((1, N, 6), np.float32)
    dets[0, :, :4] = rois
    out = hip_kps.heatmaps_to_keypoints(maps_t, torch.from_numpy(dets).to(dev), torch.tensor([N], dtype=torch.int32, device=dev),
                                        person_class=-1, min_size=min_size)
    status = out["kp_status"][0].cpu().numpy()
    if (status != 1).any():
        raise ValueError("heatmaps_to_keypoints: rows %s have a non-finite box or a resized side above %d"
                         % (np.flatnonzero(status != 1).tolist(), hip_kps.MAX_SIDE))
    return out["keyps"][0].cpu().numpy()


def keypoint_results(cls_boxes, pred_heatmaps, ref_boxes, num_classes=81, person_class=1, min_size=0):
    """core/test.py:keypoint_results: cls_boxes as box_results_with_nms_and_limit returns them, pred_heatmaps [N, K, S, S] and ref_boxes
    [N, 4] for the N boxes of the person class -> cls_keyps, a list of num_classes lists of which cls_keyps[person_class] holds one
    [4, K] array per person box."""
    xy_preds = heatmaps_to_keypoints(pred_heatmaps, ref_boxes, min_size)
    num_persons = xy_preds.shape[0]
    assert len(cls_boxes[person_class]) == num_persons
    cls_keyps = [[] for _ in range(num_classes)]
    cls_keyps[person_class] = [xy_preds[i] for i in range(num_persons)]
    return cls_keyps
