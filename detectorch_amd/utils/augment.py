"""Horizontal-flip augmentation of the training data, the reference's use_flipped=True (lib/data/roidb.py:67-69, 103-135), on the
device (hip_flip.py, include/detectorch_flip_hip.h).

    blob, scales = images_to_blob(images, ..., flipped=f)        # utils/blob.py: the mirror folded into the prep kernel
    gt_f = flip_batch(gt, f, widths)                             # boxes, proposals, polygons, run lists of the images with f[b]
    mask_rcnn_train_step(model, opt, blob, gt_f, ...)            # the train steps do not change

    roidb.extend(extend_with_flipped_entries(roidb))             # the reference's roidb with its mirror image appended

Out of scope, as in the rest of the loader side: scale jitter, keypoint flipping (commented out in the reference), flip test-time
augmentation, and the json side of the roidb (annotation files, proposal files, filter_for_training).  There is no CPU fallback.
"""
import numpy as np
import torch

from .. import hip_flip
from . import segms as segm_utils


def _i32(v, B, dev):
    if torch.is_tensor(v):
        return v if v.dtype == torch.int32 else v.to(torch.int32)
    return torch.tensor([int(x) for x in v], dtype=torch.int32, device=dev).reshape(B)


def flip_batch(gt, flipped, im_width, im_height=None, rle_out_stride=None):
    """gt: the dict the train steps take (device tensors); flipped, im_width: one flag and the ORIGINAL width per image (the
    coordinates of gt_boxes), int32 [B] device tensors or host sequences (uploaded).  -> a new dict in which, for the images with
    flipped[b] != 0, these are mirrored left to right, and everything else is shared with gt:
      gt_boxes      f32 [B,G,4], the rows below gt_counts (roidb.py:112-117)
      proposals     f32 [B,P,4], when present: the rows below proposal_counts (all rows when that key is absent)
      poly_xy       f32 [B,PTS,2], when present, with poly_ptr: the float32 rounding of the flip in double (segms.py:37-40).  The
                    doubles are taken from gt["poly_xy64"] (utils.segms.pack_polygons64) when present -- then the result is bit-equal
                    to pack_polygons of the host-flipped lists, and poly_xy64 is mirrored too --, else from poly_xy itself
      gt_runs, gt_n_runs   when present (the run lists of pack_gt_masks / pack_gt_segms): mirrored by dtc_flip_rle; needs im_height
    Sync-free, with one exception: gt_runs without rle_out_stride sizes the new lists from what the rows need -- one sync, and a
    second call when a mirrored list is longer than gt_runs' stride (a flip can lengthen a list).  With rle_out_stride the call is
    sync-free and a row that does not fit gets gt_n_runs = -1."""
    boxes = gt["gt_boxes"]
    dev, B = boxes.device, boxes.shape[0]
    flipped, im_width = _i32(flipped, B, dev), _i32(im_width, B, dev)
    out = dict(gt)
    out["gt_boxes"] = hip_flip.flip_boxes(boxes, im_width, flipped, counts=gt.get("gt_counts"))
    if gt.get("proposals") is not None:
        out["proposals"] = hip_flip.flip_boxes(gt["proposals"], im_width, flipped, counts=gt.get("proposal_counts"))
    if gt.get("poly_xy") is not None:
        src = gt.get("poly_xy64")
        xy64, xy32 = hip_flip.flip_polygons(gt["poly_xy"].to(torch.float64) if src is None else src, gt["poly_ptr"], im_width, flipped,
                                            want64=src is not None)
        out["poly_xy"] = xy32
        if src is not None:
            out["poly_xy64"] = xy64
    if gt.get("gt_runs") is not None:
        if im_height is None:
            raise ValueError("flip_batch: gt_runs needs im_height (the run lists are column-major)")
        im_size = torch.stack([_i32(im_height, B, dev), im_width], 1).to(torch.float32).contiguous()
        res = hip_flip.flip_rle(gt["gt_runs"], gt["gt_n_runs"], im_size, flipped, out_stride=rle_out_stride)
        if rle_out_stride is None:
            want = int(res["need"].max()) if res["need"].numel() else 0        # the one sync
            if want > res["out_runs"].shape[2]:
                res = hip_flip.flip_rle(gt["gt_runs"], gt["gt_n_runs"], im_size, flipped, out_stride=want)
        out["gt_runs"], out["gt_n_runs"] = res["out_runs"], res["out_n_runs"]
    return out


def extend_with_flipped_entries(roidb, device="cuda"):
    """roidb.py:103-135 on roidb dicts with 'boxes' [n,4], 'segms', 'width', 'height': -> the list of the flipped copies -- 'boxes'
    and 'segms' mirrored (all boxes in one dtc_flip_boxes call; utils.segms.flip_segms), 'flipped': True, every other key shared
    (gt_keypoints left out, as the reference's dont_copy does) -- for the caller to append: roidb.extend(...).  Every original entry
    gets 'flipped': False when it has no such key.  Asserts x2' >= x1', as the reference does."""
    for entry in roidb:
        entry.setdefault('flipped', False)
    if not roidb:
        return []
    dev = torch.device(device)
    N, R = len(roidb), max([1] + [len(e['boxes']) for e in roidb])
    packed = np.zeros((N, R, 4), np.float32)
    for i, e in enumerate(roidb):
        packed[i, :len(e['boxes'])] = np.asarray(e['boxes'], np.float32).reshape(-1, 4)
    counts = torch.tensor([len(e['boxes']) for e in roidb], dtype=torch.int32, device=dev)
    widths = torch.tensor([int(e['width']) for e in roidb], dtype=torch.int32, device=dev)
    mirrored = hip_flip.flip_boxes(torch.from_numpy(packed).to(dev), widths, [1] * N, counts=counts).cpu().numpy()
    flipped_roidb = []
    for i, entry in enumerate(roidb):
        boxes = mirrored[i, :len(entry['boxes'])].astype(np.asarray(entry['boxes']).dtype, copy=True)
        assert (boxes[:, 2] >= boxes[:, 0]).all()
        flipped_entry = {k: v for k, v in entry.items() if k not in ('boxes', 'segms', 'gt_keypoints', 'flipped')}
        flipped_entry['boxes'] = boxes
        flipped_entry['segms'] = segm_utils.flip_segms(entry['segms'], entry['height'], entry['width'], device=dev)
        flipped_entry['flipped'] = True
        flipped_roidb.append(flipped_entry)
    return flipped_roidb
