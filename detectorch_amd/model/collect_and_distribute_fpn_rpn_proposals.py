"""CollectAndDistributeFpnRpnProposals -- same call surface as the reference's
lib/model/collect_and_distribute_fpn_rpn_proposals.py:35-81, computed by one HIP workgroup per image
(detectorch_amd/csrc/fpn.hip) instead of torch.sort + D2H + numpy.

forward(roi_list, roi_score_list) -> (list of per-level roi tensors [R_l,4] for levels k_min..k_max, idx_restore ndarray)
exactly like :81/:128 (idx_restore is a numpy array used to index torch tensors, lib/model/detector.py:269-270).
"""
from math import log2

import numpy as np
import torch

from .. import hip
from ..utils.fast_rcnn_sample_rois import sample_rois_batched
from ..utils.multilevel_rois import roi_levels_batched


class CollectAndDistributeFpnRpnProposals(torch.nn.Module):
    def __init__(self, spatial_scales, train=False):
        super(CollectAndDistributeFpnRpnProposals, self).__init__()
        self._train = train
        self.rpn_levels = [int(log2(1 / s)) for s in spatial_scales]      # :39
        self.rpn_min_level = self.rpn_levels[0]
        self.rpn_max_level = self.rpn_levels[-1]

    def forward(self, roi_list, roi_score_list):
        post_nms_topN = 2000 if self._train else 1000                    # :86
        res = collect_and_distribute(roi_list, roi_score_list, post_nms_topN, self.rpn_min_level, self.rpn_max_level)
        n = int(res["n_out"][0].item())
        counts = res["level_counts"][0].cpu().numpy()
        by_level = res["rois_by_level"][0]
        distr, p = [], 0
        for c in counts:
            distr.append(by_level[p:p + int(c), :])
            p += int(c)
        return distr, res["idx_restore"][0, :n].cpu().numpy().astype(np.int64)


def collect_sample_distribute(boxes, scores, counts, gt, *, post_nms_top_n=2000, k_min=2, k_max=5, rand_keys=None, **head_knobs):
    """The training branch the reference left as Detectron's comment (:54-80, "TRAINING CODE BELOW NOT CONVERTED TO PYTORCH"), for a
    batch and without a host sync: collect the top post_nms_top_n proposals by score over the RPN levels, add the gt boxes as
    candidates and sample the minibatch with its labels and box targets (add_fast_rcnn_blobs), then distribute the SAMPLED rows over
    the levels k_min .. k_max.
      boxes f32 [B,L,P,4], scores f32 [B,L,P], counts i32 [B,L]: the per-level proposals of hip.generate_proposals (rows past the
      counts are ignored); gt: dict of gt_boxes f32 [B,G,4], gt_classes / gt_is_crowd i32 [B,G], gt_counts i32 [B].  Everything is in
      blob coordinates (im_scale 1), so that `rois` needs no rescaling.  rand_keys [B,G+post_nms_top_n] and **head_knobs: the keywords
      of sample_rois_batched.
    Each stage is an existing entry: hip.fpn_collect_distribute (only its rois5[..., 1:] and n_out are used: the levels of the
    collected rows are not the levels of the sampled ones), sample_rois_batched(expanded=False), roi_levels_batched.
    -> the dict of sample_rois_batched plus roi_levels i32 [B,R] (0 on padding rows), proposals f32 [B,T,4] (zeros past
    proposal_counts) and proposal_counts i32 [B], T = post_nms_top_n."""
    T = int(post_nms_top_n)
    if T < 1 or T > 2048:
        raise ValueError("post_nms_top_n must be in 1 .. 2048 (the proposal rows of sample_rois_batched)")
    res = hip.fpn_collect_distribute(boxes, scores, counts, T, k_min, k_max)
    proposals = res["rois5"][..., 1:].contiguous()
    blobs = sample_rois_batched(proposals, res["n_out"], gt["gt_boxes"], gt["gt_classes"], gt["gt_is_crowd"], gt["gt_counts"],
                                torch.ones((proposals.shape[0],), dtype=torch.float32, device=proposals.device), rand_keys=rand_keys,
                                expanded=False, **head_knobs)
    blobs["roi_levels"] = roi_levels_batched(blobs["rois"], blobs["n_rois"], k_min, k_max)
    blobs["proposals"], blobs["proposal_counts"] = proposals, res["n_out"]
    return blobs


def collect_and_distribute(roi_list, roi_score_list, post_nms_topN, lvl_min, lvl_max):
    """Single image: pack the per-level lists into the batched layout of dtc_fpn_collect_distribute."""
    L = len(roi_list)
    dev = roi_list[0].device
    P = max(1, max(int(r.shape[0]) for r in roi_list))
    boxes = torch.zeros((1, L, P, 4), dtype=torch.float32, device=dev)
    scores = torch.zeros((1, L, P), dtype=torch.float32, device=dev)
    counts = torch.tensor([[int(r.shape[0]) for r in roi_list]], dtype=torch.int32, device=dev)
    for l in range(L):
        n = int(roi_list[l].shape[0])
        if n:
            boxes[0, l, :n] = roi_list[l].reshape(n, -1)[:, -4:]
            scores[0, l, :n] = roi_score_list[l].reshape(-1)
    return hip.fpn_collect_distribute(boxes, scores, counts, post_nms_topN, lvl_min, lvl_max)
