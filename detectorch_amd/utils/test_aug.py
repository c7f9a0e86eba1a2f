"""Test-time augmentation on the batched path: several VIEWS of every image -- mirrored and / or rescaled network inputs -- run through
the model up to the box-head outputs, their candidates merged on the device (hip_aug.merge_boxes -> dtc_postprocess_detections_ex2
through decoded_boxes), and the mask-head probabilities every view gives for the final detections combined (hip_aug.combine_masks
-> paste -> RLE).  No host round trip between the stages.

The reference has no test-time augmentation; the rule is Detectron's core/test.py (im_detect_bbox_aug, im_detect_mask_aug and their
flipped and scaled forms) as restated in tests/tta_ref.py -- parity with Detectron itself is unpinned (tests/README_tta.md).

    AugOptions     TEST.BBOX_AUG / TEST.MASK_AUG: h_flip, scales, max_size, scale_h_flip, the heuristics, the base scale
    detect_aug     the entry (also detector.forward_batched_aug)

At this level the box heuristic is UNION (AVG and ID need the views' rows aligned, which holds only when proposal deduplication
agrees across scales: hip_aug.merge_boxes has them, this entry raises NotImplementedError); aspect-ratio views, SCALE_SIZE_DEP and
RPN-only mode are out of scope.
"""
import math

import torch

from .. import hip, hip_aug, hip_flip
from .blob import images_to_blob

MAX_ROWS = 4096        # candidate rows per image dtc_postprocess_detections_ex2 takes


class AugOptions(object):
    """Detectron's TEST.BBOX_AUG.* / TEST.MASK_AUG.* in one place (the two share their views here).
      h_flip         the mirrored view of the base scale                          H_FLIP
      scales         extra target sizes (the shorter side), each one view        SCALES
      max_size       cap on the longer side of the extra scales                  MAX_SIZE
      scale_h_flip   every extra scale also mirrored                             SCALE_H_FLIP
      score_heur / coord_heur   'UNION' | 'AVG' | 'ID' for the boxes             SCORE_HEUR / COORD_HEUR
      mask_heur      'SOFT_AVG' | 'SOFT_MAX' | 'LOGIT_AVG'                        MASK_AUG.HEUR
      test_scale / test_max_size   the base scale of the identity view           TEST.SCALE / TEST.MAX_SIZE"""

    def __init__(self, h_flip=False, scales=(), max_size=4000, scale_h_flip=False, score_heur='UNION', coord_heur='UNION',
                 mask_heur='SOFT_AVG', test_scale=800, test_max_size=1333):
        self.h_flip, self.scales, self.max_size, self.scale_h_flip = bool(h_flip), tuple(int(s) for s in scales), int(max_size), bool(scale_h_flip)
        self.score_heur, self.coord_heur, self.mask_heur = score_heur, coord_heur, mask_heur
        self.test_scale, self.test_max_size = int(test_scale), int(test_max_size)
        self.validate()

    def validate(self):
        hip_aug.box_heurs(self.score_heur, self.coord_heur)         # unknown: NotImplementedError; a mixed UNION pair: ValueError
        if self.mask_heur not in hip_aug.MASK_HEURS:
            raise NotImplementedError('Heuristic {} not supported'.format(self.mask_heur))
        if any(s < 1 for s in self.scales + (self.test_scale, self.max_size, self.test_max_size)):
            raise ValueError("AugOptions: scales and sizes must be positive")
        if len(self.views()) > hip_aug.MAX_VIEWS:
            raise ValueError("AugOptions: %d views, at most %d" % (len(self.views()), hip_aug.MAX_VIEWS))
        return self

    def views(self):
        """[(target_size, max_size, flipped)] in Detectron's order (im_detect_bbox_aug): the flip of the base scale, every extra
        scale followed by its flip with scale_h_flip, and the identity view last."""
        v = []
        if self.h_flip:
            v.append((self.test_scale, self.test_max_size, True))
        for s in self.scales:
            v.append((s, self.max_size, False))
            if self.scale_h_flip:
                v.append((s, self.max_size, True))
        v.append((self.test_scale, self.test_max_size, False))
        return v

    def check_rows(self, top_n):
        """T views of top_n candidate rows each must fit the detection entry"""
        T = len(self.views())
        if T * top_n > MAX_ROWS:
            raise ValueError("test-time augmentation: %d views x %d rois = %d candidate rows per image, the detection entry takes %d"
                             % (T, top_n, T * top_n, MAX_ROWS))
        return T


def _blob_hw(images, target_size, max_size, stride):
    """each image's own blob size inside the padded one (dtc_prep_plan's resized size, rounded up to the stride), or None when
    every image has the same shape"""
    import ctypes as C
    if len({tuple(im.shape[:2]) for im in images}) == 1:
        return None
    B = len(images)
    hs, ws = (C.c_int32 * B)(*[int(im.shape[0]) for im in images]), (C.c_int32 * B)(*[int(im.shape[1]) for im in images])
    scales, out_hw, blob_hw = (C.c_double * B)(), (C.c_int32 * (2 * B))(), (C.c_int32 * 2)()
    hip.call("dtc_prep_plan", heights=hs, widths=ws, batch=B, target_size=target_size, max_size=max_size, pad_stride=stride,
             im_scales=scales, out_hw=out_hw, blob_hw=blob_hw)
    return [(stride * math.ceil(out_hw[2 * b] / stride), stride * math.ceil(out_hw[2 * b + 1] / stride)) for b in range(B)]


@torch.no_grad()
def detect_aug(model, raw_images, aug=None, proposals=None, proposal_counts=None, **det_kw):
    """Mask / Faster R-CNN on a batch with test-time augmentation.
      model        a detector forward_batched serves (RPN or precomputed-proposal FPN models, the C4 ones)
      raw_images   list of B HWC BGR images (CUDA tensors or numpy arrays, uint8 / float32), as images_to_blob takes them
      aug          AugOptions (None: the defaults -- the identity view alone, which gives forward_batched's bits)
      proposals / proposal_counts, do_soft_nms ... bbox_vote_method: as forward_batched takes them (proposals in original-image
      coordinates; a mirrored view gets them mirrored)
    Every view gets its own blob (images_to_blob, the mirror folded into the prep kernel) and its own region path, and runs up to the
    box-head outputs; dtc_aug_merge_boxes stacks the views' decoded, un-mirrored candidates; the detection stage (Soft-NMS, vote and
    its scoring as in forward_batched) runs once on them.  With a mask head the final boxes go back to every view -- mirrored where
    the view is, times the view's scale -- for the level mapping, the 14 x 14 RoIAlign on that view's maps and the mask head;
    dtc_aug_combine_masks merges the probabilities of the detections' classes, paste and RLE stay as they are.
    Returns the region path of the identity view, holding the fixed-shape results forward_batched leaves (dets, det_count, det_roi,
    crops, rle_str ...: assemble_results and the evaluators take it), plus
      det_src int32 [B,max_out]   view * top_n + row of each detection's candidate (-1 past det_count)
      aug_views                   the views' region paths, in view order (their feature maps and head outputs)
      aug_merged                  hip_aug.merge_boxes' outputs; aug_mask_probs: the views' mask probabilities
    det_roi indexes the merged rows.  The returned path is a cached object, as forward_batched's is."""
    aug = aug or AugOptions()
    aug.validate()
    if aug.score_heur != 'UNION':
        raise NotImplementedError("detect_aug merges boxes by UNION; AVG and ID need aligned rows across views (hip_aug.merge_boxes "
                                  "has them)")
    views = aug.views()
    fpn = model.use_fpn_body
    B = len(raw_images)
    dev = torch.device("cuda", torch.cuda.current_device())
    if proposals is not None:
        proposals, proposal_counts = model._proposal_inputs(proposals, proposal_counts, B, dev)
        top_n = int(proposals.shape[1])
    else:
        g = getattr(model, "proposal_generator", None)
        top_n = 1000 if fpn or g is None else int(g.rpn_post_nms_top_n)
    T = aug.check_rows(top_n)
    sz = torch.tensor([[float(im.shape[0]), float(im.shape[1])] for im in raw_images], dtype=torch.float32, device=dev)
    width = sz[:, 1].to(torch.int32).contiguous()
    ones = [1] * B
    paths = []
    for t, (target, max_size, flipped) in enumerate(views):
        blob, scales = images_to_blob(raw_images, target_size=target, max_size=max_size, fpn_on=fpn, flipped=[flipped] * B)
        props = proposals
        if proposals is not None and flipped:                    # im_detect_bbox_hflip: box_proposals_hf = flip_boxes(box_proposals, w)
            props = hip_flip.flip_boxes(proposals, width, ones, counts=proposal_counts, out=proposals.clone())
        paths.append(model.forward_batched(blob, scales, sz, blob_hw=_blob_hw(raw_images, target, max_size, 32 if fpn else 1),
                                           proposals=props, proposal_counts=proposal_counts, view=t, **det_kw))
    path = paths[-1]                                             # the identity view: its buffers take the merged results
    with torch.cuda.device(dev):
        merged = hip_aug.merge_boxes([dict(rois5=p.rois5, n_rois=p.n_rois, cls_score=p.cls_logits_out, bbox_pred=p.bbox_pred_out, scale=p.sf,
                                           flipped=v[2]) for p, v in zip(paths, views)], sz, aug.score_heur, aug.coord_heur,
                                      scores_are_logits=True)
        rows = T * top_n
        need = hip.det_workspace_bytes(B, rows, path.n_cls, path.det_opt, scoring=path.det_scoring)
        if getattr(path, "aug_det_ws", None) is None or path.aug_det_ws.numel() < need:
            path.aug_det_ws = hip.workspace(need, dev)
        hip.call("dtc_postprocess_detections_ex2", "postprocess_detections_ex2(aug)", rois5=None, n_rois=merged["out_n"],
                 cls_score=merged["out_scores"], scores_are_logits=False, bbox_pred=None, decoded_boxes=merged["out_boxes"],
                 scaling_factor=None, im_size=None, batch=B, max_rois=rows, n_cls=path.n_cls, wx=10.0, wy=10.0, ww=5.0, wh=5.0,
                 score_thresh=0.05, nms_thresh=0.5, max_det=path.max_det, opt=path.det_opt, scoring=path.det_scoring,
                 workspace=path.aug_det_ws, workspace_bytes=path.aug_det_ws.numel(), max_out=path.max_out, fpn=None, dets=path.dets,
                 det_roi=path.det_roi, det_rois_scaled=None, det_count=path.det_count)
        live = torch.arange(path.max_out, device=dev)[None, :] < path.det_count[:, None]
        src = torch.gather(merged["out_src"], 1, path.det_roi.clamp(0, rows - 1).long())
        path.det_src = torch.where(live, src, torch.full_like(src, -1))
        path.aug_views, path.aug_merged, path.aug_mask_probs = paths, merged, None
        if not model.use_mask_head:
            return path
        boxes = path.dets[:, :, :4].contiguous()
        probs = []
        for p, (_, _, flipped) in zip(paths, views):
            b = hip_flip.flip_boxes(boxes, width, ones, counts=path.det_count, out=boxes.clone()) if flipped else boxes
            p.det_scaled.copy_(b * p.sf[:, None, None])          # the view's coordinates: (mirrored,) times the view's scale
            if p is not path:
                p.det_count.copy_(path.det_count)
            st = hip.stream_ptr(dev)
            p._map_mask_levels(st)
            p._roi_align_mask(st)
            probs.append(model._mask_probs(p.mask_feats))
        mask_class = path.dets[:, :, 5].to(torch.int32).reshape(-1).contiguous()
        combined = hip_aug.combine_masks(probs, [v[2] for v in views], path.det_count, mask_class, aug.mask_heur)
        path.aug_mask_probs = probs
        path.bind_masks(combined)
        path.launch_masks()
    return path
