"""Mask R-CNN training targets -- Detectron's add_mask_rcnn_blobs (the reference keeps only the commented-out call,
lib/utils/fast_rcnn_sample_rois.py:125-127) on the compact minibatch of sample_rois_batched, computed on the GPU for a batch of
images at once (detectorch_amd/csrc/mask_train/mask_targets.hip; include/detectorch_mask_hip.h has the contract): every foreground
RoI gets the polygons of the ground truth it overlaps most, rasterised into an M x M grid relative to the RoI.

    pack_polygons(polys_per_image, G)      lists of COCO polygon lists -> the three fixed-shape polygon tensors
    mask_targets_batched(blobs, ...)       device tensors in, fixed-shape device tensors out, no host sync
    add_mask_rcnn_blobs(blobs, ...)        Detectron's signature for one roidb entry, numpy in / numpy out

RLE-format (crowd) segmentations are not rasterised: crowd ground truth takes no part in the mask targets, as in Detectron.
"""
import numpy as np
import torch

from .. import hip_mask


def pack_polygons(polys_per_image, G, device=None, points=None, polys=None):
    """polys_per_image: per image, per gt row (at most G), a list of COCO polygons [x0, y0, x1, y1, ...] (a gt without polygons, such
    as a crowd row with an RLE dict: an empty list or None).  -> (poly_xy f32 [B,PTS,2], poly_ptr i32 [B,NP+1], gt_poly_ptr i32
    [B,G+1]); `points` / `polys` fix PTS / NP (default: the largest image's, at least 1).  Rows past an image's own counts repeat the
    last offset (empty ranges)."""
    B = len(polys_per_image)
    per = []
    for im in polys_per_image:
        if len(im) > G:
            raise ValueError("an image has %d gt rows, more than G = %d" % (len(im), G))
        xy, ptr, gptr = [], [0], [0]
        for gt in im:
            for poly in (gt if isinstance(gt, (list, tuple)) else []):
                p = np.asarray(poly, np.float32).reshape(-1, 2)
                xy.append(p)
                ptr.append(ptr[-1] + len(p))
            gptr.append(len(ptr) - 1)
        per.append((np.concatenate(xy, 0) if xy else np.zeros((0, 2), np.float32), ptr, gptr))
    PTS = max([1] + [len(x) for x, _, _ in per]) if points is None else int(points)
    NP = max([1] + [len(p) - 1 for _, p, _ in per]) if polys is None else int(polys)
    poly_xy = np.zeros((B, PTS, 2), np.float32)
    poly_ptr = np.zeros((B, NP + 1), np.int32)
    gt_poly_ptr = np.zeros((B, G + 1), np.int32)
    for b, (xy, ptr, gptr) in enumerate(per):
        if len(xy) > PTS or len(ptr) - 1 > NP:
            raise ValueError("image %d has %d points in %d polygons: more than PTS = %d / NP = %d" % (b, len(xy), len(ptr) - 1, PTS, NP))
        poly_xy[b, :len(xy)] = xy
        poly_ptr[b, :len(ptr)] = ptr
        poly_ptr[b, len(ptr):] = ptr[-1]
        gt_poly_ptr[b, :len(gptr)] = gptr
        gt_poly_ptr[b, len(gptr):] = gptr[-1]
    out = tuple(torch.from_numpy(a) for a in (poly_xy, poly_ptr, gt_poly_ptr))
    return out if device is None else tuple(t.to(device) for t in out)


def mask_targets_batched(blobs, proposals, gt_boxes, gt_classes, gt_is_crowd, gt_counts, im_scale, polys, *, M=28, k_min=2, k_max=5,
                         mask_rows=None, out=None):
    """blobs: the dict of sample_rois_batched (labels_int32, keep_inds, n_rois are read); proposals f32 [B,P,4] and gt_boxes f32
    [B,G,4]: the candidates that call sampled from, in ORIGINAL image coordinates; gt_classes / gt_is_crowd i32 [B,G], gt_counts i32
    [B], im_scale f32 [B]; polys = (poly_xy, poly_ptr, gt_poly_ptr) of pack_polygons, in the coordinates of gt_boxes.  All on the GPU.
    mask_rows: Fm, the mask rows per image (None: min(R, 512); the foreground quota of the minibatch is enough).
    -> dict of device tensors named after Detectron's blobs, Fm rows per image:
         mask_rois [B,Fm,5], masks_int32 [B,Fm,M*M] in {0, 1, -1}, mask_class_labels [B,Fm], roi_has_mask_int32 [B,R],
         mask_roi_levels [B,Fm] (index into the FPN levels k_min .. k_max; 0 when k_min == k_max), n_mask [B]; plus mask_gt [B,Fm]
       rows past n_mask[b]: masks -1, class 0.  `out`: the dict of an earlier call, written in place (graph capture)."""
    poly_xy, poly_ptr, gt_poly_ptr = polys
    raw = None if out is None else out["_raw"]
    raw = hip_mask.mask_targets(blobs["labels_int32"], blobs["keep_inds"], blobs["n_rois"], gt_boxes, gt_classes, gt_is_crowd, gt_counts,
                                proposals, im_scale, poly_xy, poly_ptr, gt_poly_ptr, M=M, k_min=k_min, k_max=k_max, mask_rows=mask_rows,
                                out=raw)
    return dict(mask_rois=raw["mask_rois"], masks_int32=raw["masks"], mask_class_labels=raw["mask_class"],
                roi_has_mask_int32=raw["roi_has_mask"], mask_roi_levels=raw["mask_roi_levels"], n_mask=raw["n_mask"],
                mask_gt=raw["mask_gt"], _raw=raw)


def add_mask_rcnn_blobs(blobs, sampled_boxes, roidb, im_scale, batch_idx, M=28):
    """Detectron's add_mask_rcnn_blobs for ONE roidb entry, numpy in / numpy out: blobs['labels_int32'] [n] are the labels of the
    sampled rows, sampled_boxes f32 [n,4] their boxes (original coordinates); roidb has 'boxes', 'gt_classes', 'is_crowd' and
    'segms' (per row a list of polygons; anything else, such as an RLE dict, counts as no polygon).  Adds 'mask_rois' [m,5],
    'roi_has_mask_int32' [n] and 'masks_int32' [m, M*M] (the compact class-specific form, with 'mask_class_labels' [m] beside it)
    to blobs, m = n_mask."""
    if not torch.cuda.is_available():
        raise RuntimeError("detectorch_amd needs the MI355X HIP path (no CPU fallback)")
    dev = torch.device("cuda", torch.cuda.current_device())
    labels = np.asarray(blobs['labels_int32']).astype(np.int32)
    n = len(labels)
    cls = np.asarray(roidb['gt_classes']).astype(np.int32)
    gt = np.where(cls > 0)[0]
    G = max(len(gt), 1)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(dev).unsqueeze(0).contiguous()
    i32, f32 = torch.int32, torch.float32
    gt_boxes = np.zeros((G, 4), np.float32)
    gt_boxes[:len(gt)] = np.asarray(roidb['boxes'], np.float32)[gt]
    pad = lambda a: np.concatenate([np.asarray(a)[gt].astype(np.int32), np.zeros(G - len(gt), np.int32)])
    polys = pack_polygons([[roidb['segms'][i] for i in gt]], G, device=dev)
    mini = dict(labels_int32=t(labels, i32), keep_inds=t(len(gt) + np.arange(n), i32), n_rois=torch.tensor([n], dtype=i32, device=dev))
    out = mask_targets_batched(mini, t(np.asarray(sampled_boxes, np.float32).reshape(n, 4), f32), t(gt_boxes, f32), t(pad(cls), i32),
                               t(pad(roidb['is_crowd']), i32), torch.tensor([len(gt)], dtype=i32, device=dev),
                               torch.tensor([float(im_scale)], dtype=f32, device=dev), polys, M=M, k_min=0, k_max=0)
    m = int(out["n_mask"][0])
    rois = out["mask_rois"][0, :m].cpu().numpy()
    rois[:, 0] = batch_idx
    blobs['mask_rois'] = rois
    blobs['roi_has_mask_int32'] = out["roi_has_mask_int32"][0].cpu().numpy()
    blobs['masks_int32'] = out["masks_int32"][0, :m].cpu().numpy()
    blobs['mask_class_labels'] = out["mask_class_labels"][0, :m].cpu().numpy()
    return blobs
