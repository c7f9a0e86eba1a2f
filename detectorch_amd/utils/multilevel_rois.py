"""FPN RoI -> level distribution -- same functions as the reference's lib/utils/multilevel_rois.py, computed on the GPU
(detectorch_amd/csrc/fpn.hip).  numpy in / numpy out like the reference (this is the mask-branch helper the notebooks
call between postprocess_output and model.mask_head, eval_mask_FPN.ipynb:249)."""
import numpy as np
import torch

from .. import hip


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("detectorch_amd needs the MI355X HIP path (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def _run(rois, k_min, k_max):
    rois = np.ascontiguousarray(rois, dtype=np.float32)
    n = rois.shape[0]
    box = torch.from_numpy(rois[:, -4:].copy()).to(_dev()).reshape(1, 1, max(n, 0), 4)
    if n == 0:
        return np.zeros(0, np.float32), [rois[:0] for _ in range(k_min, k_max + 1)], np.zeros(0, np.int32)
    counts = torch.tensor([[n]], dtype=torch.int32, device=box.device)
    res = hip.fpn_collect_distribute(box, None, counts, n, k_min, k_max)
    lv = res["roi_levels"][0].cpu().numpy()
    restore = res["idx_restore"][0].cpu().numpy().astype(np.int32)
    order = np.empty(n, np.int64)
    order[restore] = np.arange(n)
    cnt = res["level_counts"][0].cpu().numpy()
    per, p = [], 0
    for c in cnt:
        per.append(rois[order[p:p + int(c)], :])
        p += int(c)
    return (lv + k_min).astype(np.float32), per, restore


MAX_ROWS = 2048          # rows per image of dtc_prepare_proposals


def roi_levels_batched(rois, counts=None, k_min=2, k_max=5):
    """The FPN level (index into k_min .. k_max) of arbitrary device rows, for training: map_rois_to_fpn_levels (:41-53) without the
    numpy round trip and without a host sync.  rois float32 [B,R,4|5] or flat [N,4|5] on the GPU (the last four columns are the
    box); counts int32 [B] or None (every row; flat input takes none).  -> int32 [B,R] / [N].
    Decided by hip.prepare_proposals(im_scale = 1, dedup_scale = 0): every row kept in input order, the level from the one text of
    the formula (csrc/fpn_map.h).  That entry takes at most 2048 rows per image: flat input is cut into groups of at most 2048 rows
    (the mapping is per row, the grouping cannot change a level) and a batched R > 2048 is refused.  Level 0 goes to the rows past
    counts[b], to all-zero rows (the padding of a minibatch: area 1) and to rows with a non-finite coordinate -- the entry DROPS
    those, which would shift the rows behind them, so they go down as zeros."""
    dev = hip._require_cuda(rois, counts)
    if rois.dtype != torch.float32 or rois.dim() not in (2, 3) or rois.shape[-1] not in (4, 5):
        raise TypeError("rois must be float32 [B,R,4|5] or [N,4|5]")
    box = rois.detach()[..., -4:]
    box = torch.where(torch.isfinite(box).all(-1, keepdim=True), box, torch.zeros((), dtype=box.dtype, device=dev))
    if rois.dim() == 2:
        if counts is not None:
            raise ValueError("counts go with [B,R,4|5] rois")
        N = box.shape[0]
        if N == 0:
            return torch.zeros((0,), dtype=torch.int32, device=dev)
        R = min(N, MAX_ROWS)
        G = (N + R - 1) // R
        if G * R != N:                                          # the last group is filled with zero rows
            box = torch.cat((box, torch.zeros((G * R - N, 4), dtype=box.dtype, device=dev)), 0)
        box = box.reshape(G, R, 4)
    else:
        N = None
        G, R = box.shape[0], box.shape[1]
        if R > MAX_ROWS:
            raise ValueError("at most %d rows per image (flat [N,4|5] input has no limit)" % MAX_ROWS)
        if G == 0 or R == 0:
            return torch.zeros((G, R), dtype=torch.int32, device=dev)
    if counts is None:
        counts = torch.full((G,), R, dtype=torch.int32, device=dev)
    elif tuple(counts.shape) != (G,):
        raise ValueError("counts must be int32 [B]")
    lv = hip.prepare_proposals(box.contiguous(), counts, torch.ones((G,), dtype=torch.float32, device=dev), dedup_scale=0.0,
                               k_min=k_min, k_max=k_max)["roi_levels"].clamp_(min=0)          # -1: a row past counts[b]
    return lv if N is None else lv.reshape(-1)[:N]


def map_rois_to_fpn_levels(rois, k_min, k_max, roi_canonical_scale=224, roi_canonical_level=4):
    """multilevel_rois.py:41-53 (canonical scale/level are the Detectron constants 224 / 4, fixed in the kernel)."""
    assert roi_canonical_scale == 224 and roi_canonical_level == 4
    return _run(rois, k_min, k_max)[0]


def add_multilevel_rois_for_test(blobs, name, roi_min_level=2, roi_max_level=5):
    """multilevel_rois.py:19-39 + add_multilevel_roi_blobs :56-82."""
    rois = blobs[name]
    _, per, restore = _run(rois, roi_min_level, roi_max_level)
    for i, lvl in enumerate(range(roi_min_level, roi_max_level + 1)):
        blobs[name + '_fpn' + str(lvl)] = per[i]
    blobs[name + '_idx_restore_int32'] = restore
    stacked = np.vstack(per) if len(per) else rois
    assert (stacked[restore] == np.asarray(rois, np.float32)).all()      # the reference's sanity check, :82
    return blobs
