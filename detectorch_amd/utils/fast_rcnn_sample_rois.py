"""Fast R-CNN training minibatches -- the reference's lib/utils/fast_rcnn_sample_rois.py together with the roidb preparation it
relies on (lib/data/json_dataset.py:333-435, lib/data/roidb.py:176-206), computed on the GPU in one launch for a batch of images
(detectorch_amd/csrc/train/fast_rcnn_targets.hip).

    sample_rois_batched(...)      device tensors in, fixed-shape device tensors out, no host sync
    compact(blobs)                the valid rows concatenated like train_fast.py's list_to_tensor (one host sync)
    fast_rcnn_sample_rois(...)    the reference's signature for one roidb entry, numpy in / numpy out

The sampling order is a tensor of 32-bit keys (ascending (key, index) order inside fg and inside bg) instead of numpy's global
generator: the result is one of the samples npr.choice(..., replace=False) may draw, and the same on every run for the same keys.
"""
import numpy as np
import torch

from .. import hip_train


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("detectorch_amd needs the MI355X HIP path (no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device())


def sample_rois_batched(proposals, proposal_counts, gt_boxes, gt_classes, gt_is_crowd, gt_counts, im_scale, *, rand_keys=None,
                        generator=None, rois_per_image=512, fg_fraction=0.25, fg_thresh=0.5, bg_thresh_hi=0.5, bg_thresh_lo=0,
                        bbox_thresh=0.5, crowd_thresh=0.7, reg_weights=(10.0, 10.0, 5.0, 5.0), num_classes=81,
                        cls_agnostic_bbox_reg=False, expanded=True, out=None):
    """proposals f32 [B,P,4] and gt_boxes f32 [B,G,4] in ORIGINAL image coordinates, gt_classes / gt_is_crowd int32 [B,G], the
    counts int32 [B] (rows past them are ignored), im_scale f32 [B]; all on the GPU.  rand_keys: 32-bit integers [B,G+P] indexed by
    candidate (the image's gt rows, then its proposals); None draws them on the device from `generator`.
    -> dict of device tensors with R = rois_per_image rows per image:
         rois [B,R,5], labels_int32 [B,R], bbox_targets / bbox_inside_weights / bbox_outside_weights [B,R,4*num_classes]
         (None with expanded=False), bbox_targets5 [B,R,5], keep_inds [B,R], n_fg [B], n_rois [B]
       rows past n_rois[b]: label -1, keep_inds -1, zeros.  `out`: the dict of an earlier call, written in place (graph capture)."""
    B, P, G = proposals.shape[0], proposals.shape[1], gt_boxes.shape[1]
    params = hip_train.train_params(rois_per_image, fg_fraction, fg_thresh, bg_thresh_hi, bg_thresh_lo, bbox_thresh, crowd_thresh,
                                    reg_weights, num_classes, cls_agnostic_bbox_reg)
    if rand_keys is None:
        rand_keys = torch.randint(-2 ** 31, 2 ** 31, (B, G + P), dtype=torch.int32, device=proposals.device, generator=generator)
    raw = None
    if out is not None:
        raw = {k: out[k] for k in ("bbox_targets5", "bbox_targets", "bbox_inside_weights", "bbox_outside_weights", "keep_inds", "n_fg",
                                   "n_rois")}                         # the entry's own names only: invoke refuses unknown ones
        raw.update(rois5=out["rois"], labels=out["labels_int32"], max_overlaps=None, max_classes=None)
    raw = hip_train.fast_rcnn_targets(gt_boxes, gt_classes, gt_is_crowd, gt_counts, proposals, proposal_counts, im_scale, rand_keys,
                                      params, out=raw, expanded=expanded)
    return dict(rois=raw["rois5"], labels_int32=raw["labels"], bbox_targets=raw["bbox_targets"],
                bbox_inside_weights=raw["bbox_inside_weights"], bbox_outside_weights=raw["bbox_outside_weights"],
                bbox_targets5=raw["bbox_targets5"], keep_inds=raw["keep_inds"], n_fg=raw["n_fg"], n_rois=raw["n_rois"])


BLOB_NAMES = ("rois", "labels_int32", "bbox_targets", "bbox_inside_weights", "bbox_outside_weights")


def compact(blobs):
    """The valid rows of every image, concatenated in image order -- what train_fast.py:139-144 builds with list_to_tensor from the
    per-image blobs.  One host sync (n_rois)."""
    n = blobs["n_rois"].cpu().tolist()
    R = blobs["rois"].shape[1]
    idx = torch.tensor([b * R + r for b in range(len(n)) for r in range(n[b])], dtype=torch.int64, device=blobs["rois"].device)
    return {k: blobs[k].reshape((-1,) + tuple(blobs[k].shape[2:])).index_select(0, idx) for k in BLOB_NAMES if blobs[k] is not None}


def fast_rcnn_sample_rois(roidb, im_scale, batch_idx, train_batch_size_per_image=512, train_fg_roi_fraction=0.25,
                          train_fg_thresh=0.5, train_bg_thresh_hi=0.5, train_bg_thresh_lo=0, mask_on=False, keypoints_on=False,
                          rand_keys=None, generator=None, **knobs):
    """fast_rcnn_sample_rois.py:41-137 for ONE roidb entry whose proposals were merged in (json_dataset.py:333): reads 'boxes',
    'gt_classes' and 'is_crowd' (the gt rows -- gt_classes > 0 -- first, as the reference appends the proposals behind them), runs
    the device path and returns the reference's blob dict as numpy arrays.  **knobs: bbox_thresh, crowd_thresh, reg_weights,
    num_classes, cls_agnostic_bbox_reg (the roidb-preparation arguments of lib/data/roidb.py:44-55)."""
    dev = _dev()
    boxes = np.ascontiguousarray(roidb['boxes'], dtype=np.float32)
    cls = np.asarray(roidb['gt_classes']).astype(np.int32)
    n_gt = int(np.sum(cls > 0))
    assert np.all(cls[:n_gt] > 0), "the gt rows must come first"
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev).unsqueeze(0).contiguous()
    i32 = torch.int32
    cnt = lambda v: torch.tensor([v], dtype=i32, device=dev)
    if rand_keys is not None:
        rand_keys = t(np.asarray(rand_keys).astype(np.uint32).view(np.int32), i32)
    blobs = sample_rois_batched(t(boxes[n_gt:], torch.float32), cnt(len(boxes) - n_gt), t(boxes[:n_gt], torch.float32),
                                t(cls[:n_gt], i32), t(np.asarray(roidb['is_crowd'])[:n_gt].astype(np.int32), i32), cnt(n_gt),
                                torch.tensor([float(im_scale)], dtype=torch.float32, device=dev), rand_keys=rand_keys,
                                generator=generator, rois_per_image=train_batch_size_per_image, fg_fraction=train_fg_roi_fraction,
                                fg_thresh=train_fg_thresh, bg_thresh_hi=train_bg_thresh_hi, bg_thresh_lo=train_bg_thresh_lo, **knobs)
    n = int(blobs["n_rois"][0])
    res = {k: blobs[k][0, :n].cpu().numpy() for k in BLOB_NAMES}
    res["rois"][:, 0] = batch_idx                                           # :113
    return res
