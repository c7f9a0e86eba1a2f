"""Device-resident region-proposal hot path for a BATCH of images (Mask R-CNN FPN flavour, BASELINE cfg3/cfg4).

This is the MI355X-first composition of the kernels behind the reference-shaped modules: everything the reference does
between the RPN-head outputs and the box/mask-head GEMMs, and after them, for B images at once, with zero host round
trips and (optionally) replayed from one hipGraph:

    RPN outputs (5 levels) --[rpn_topk_decode, nms_sorted, gather]--> per-level proposals      generate_proposals.py:31-122
      --[fpn_collect_distribute]--> rois5 [B,1000,5] + level ids                               collect_and_distribute...py:84-128
      --[roi_align 7x7, all levels, one launch]--> box-head features [B*1000,256,7,7]          detector.py:263-270
      (box head fc6/fc7/cls/bbox: hipBLASLt GEMMs, not part of the hot path -- supplied by the caller / synthetic)
      --[postprocess_detections]--> dets [B,128,6]                                             result_utils.py:76-168
      --[fpn_collect_distribute (no sort)]--> mask-branch level ids                            multilevel_rois.py:19-39
      --[roi_align 14x14]--> mask-head features [B*128,256,14,14]                              detector.py:99-106
      (mask head convs: MIOpen, not part of the hot path -- supplied by the caller / synthetic)
      --[mask_paste]--> binarised crops                                                        result_utils.py:170-214
"""
import numpy as np
import torch

from . import hip, synth
from .utils.generate_anchors import generate_anchors


def _device_hw(im_hw, B, dev):
    """Per-image (h, w) sizes -> an owned float32 [B,2] device tensor (None stays None: the dtc_rpn_topk_decode_sized NULL path)."""
    if im_hw is None:
        return None
    return torch.as_tensor(im_hw, dtype=torch.float32).to(dev).reshape(B, 2).clone().contiguous()


def _device_input(t, dtype, shape, dev):
    """A bound input: the caller's tensor itself when it already is a contiguous device tensor of that type (new values copied into
    it apply at the next step / replay), otherwise an owned copy."""
    t = torch.as_tensor(t)
    if t.device == torch.device(dev) and t.dtype == dtype and t.is_contiguous() and tuple(t.shape) == tuple(shape):
        return t
    return t.to(device=dev, dtype=dtype).reshape(shape).contiguous().clone()


class _GraphStep:
    """step(): one pass of self._launch() on the current stream of self.dev, captured once into a hipGraph and replayed.  A rebind
    sets self.graph = None, which drops the capture."""

    def step(self, use_graph=True):
        """One pass over the bound batch on the current stream.  With use_graph the launch sequence is captured once into
        a hipGraph (after an eager warm-up call) and replayed: the path is ~17 short launches, i.e. launch-bound."""
        with torch.cuda.device(self.dev):
            if not use_graph:
                self._launch()
                return
            if self.graph is None:
                self._launch()                       # eager warm-up (sets function attributes, primes allocations)
                torch.cuda.synchronize(self.dev)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch()
                self.graph = g
            self.graph.replay()


class RegionPath(_GraphStep):
    """What FpnRegionPath and C4RegionPath share: the buffers (allocated once; the step itself never allocates), the bind_*
    bookkeeping (pointers are baked into the launch descriptors and the graph, so every rebind drops the graph and new data is COPIED
    into the bound tensors between steps), one method per launch, the three stages and the captured step.  A flavour is its
    constructor signature plus the facts passed to this constructor:
      strides / anchors   one entry per RPN level (segments = batch * levels)
      roi_scales          one entry per feature level RoIAlign reads; levels k_min .. k_min + len(roi_scales) - 1
      kmax                row stride of the pre-NMS arrays
      ra_workspace        RoIAlign through dtc_roi_align_forward_packed_ws (single-level, map-stationary kernel) with a workspace
      with_masks          the mask branch (its buffers exist only then)
    and, set after it, fused_gather (collect reads proposals[keep] in place: dtc_fpn_collect_distribute_kept) and fused_mask_map (the
    mask branch's level mapping comes out of the detection launch); both are read at launch time."""

    def __init__(self, batch, device, *, channels, n_cls, pre, post, top_n, rpn_thresh, box_p, mask_p, sr, max_det, max_out, mask_res,
                 pad_h, pad_w, feat_dtype, det_options, cls_logits, with_masks, with_rle, crop_capacity, rle_runs_stride,
                 rle_str_stride, strides, anchors, roi_scales, k_min, kmax, ra_workspace):
        self.B, self.dev, self.C, self.n_cls = batch, device, channels, n_cls
        self.det_opt, self.det_scoring = hip.det_options_scoring(det_options)
        self.cls_logits = cls_logits       # the bound cls_score is the classifier's raw output; softmax folded into the kernel
        self.with_masks, self.with_rle = with_masks, with_rle
        self.rle_runs_stride, self.rle_str_stride, self.crop_capacity = int(rle_runs_stride), int(rle_str_stride), crop_capacity
        self.pre, self.post, self.top_n, self.rpn_thresh = pre, post, top_n, rpn_thresh
        self.box_p, self.mask_p, self.sr, self.M = box_p, mask_p, sr, mask_res
        self.max_det, self.max_out = max_det, max_out
        self.pad_h, self.pad_w = pad_h, pad_w                     # the blob size the RPN decode clips to (without per-image sizes)
        self.strides, self.anchors, self.roi_scales = strides, anchors, roi_scales
        self.k_min, self.k_max, self.kmax = k_min, k_min + len(roi_scales) - 1, kmax
        self.feat_dtype = feat_dtype
        self.graph = self.prop_in = self.masks = None
        self.fused_gather = False
        self.fused_mask_map = with_masks and max_out <= 512
        self._alloc(ra_workspace)

    def _alloc(self, ra_workspace):
        B, dev, f32, i32 = self.B, self.dev, torch.float32, torch.int32
        e = lambda *shape, dtype=f32: torch.empty(shape, dtype=dtype, device=dev)
        zeros = lambda *shape, dtype=f32: torch.zeros(shape, dtype=dtype, device=dev)
        S, T, D, nl = B * len(self.strides), self.top_n, self.max_out, len(self.roi_scales)
        self.pre_boxes, self.pre_scores, self.pre_counts = e(S, self.kmax, 4), e(S, self.kmax), e(S, dtype=i32)
        self.P = min(self.post, self.kmax)
        self.keep, self.keep_cnt = e(S, self.P, dtype=i32), e(S, dtype=i32)
        # per-level proposals after NMS (generate_proposals.py:119-120), written by the gather launch
        self._prop_boxes, self._prop_scores = zeros(S, self.P, 4), zeros(S, self.P)
        self.nms_ws = hip.workspace(hip.call("dtc_nms_sorted_workspace_bytes", n_seg=S, n_stride=self.kmax), dev)
        # (each output set is kept twice: as the dict a by-name call takes, and under the attribute names its readers use)
        self._roi_out = hip.collect_outputs(B, T, nl, dev)
        (self.rois5, self.roi_scores, self.roi_levels, self.n_rois, self.rois_by_level, self.level_counts, self.idx_restore,
         self.roi_order, self.roi_desc) = self._roi_out.values()
        self.box_feats = e(B * T, self.C, self.box_p, self.box_p, dtype=self.feat_dtype)
        # (RoIAlign workspace: the per-RoI records the map-stationary kernel's preparation pass writes, csrc/roi_align_map.hip)
        ra_ws = lambda rows: hip.workspace(hip.call("dtc_roi_align_workspace_bytes", n_rois=rows), dev) if ra_workspace else None
        self.ra_ws = ra_ws(B * T)
        self._det_out = hip.det_outputs(B, D, dev)
        self.dets, self.det_roi, self.det_scaled, self.det_count = self._det_out.values()
        self.det_ws = hip.workspace(hip.det_workspace_bytes(B, T, self.n_cls, self.det_opt, scoring=self.det_scoring), dev)
        if not self.with_masks:
            return
        # the mask branch's rois / level ids / visiting order: out of the detection launch itself (dtc_fpn_map_out, <= 512 rows), or
        # of a separate mapping launch
        self._mask_roi_out = hip.collect_outputs(B, D, nl, dev, scores=False)
        (self.m_rois5, _, self.m_levels, self.m_n, self.m_by_level, self.m_level_counts, self.m_restore, self.m_order,
         self.m_desc) = self._mask_roi_out.values()
        self.m_map = hip.FpnMapOut(k_min=self.k_min, k_max=self.k_max,
                                   **{k: t.data_ptr() for k, t in self._mask_roi_out.items() if t is not None})
        self.mask_feats = e(B * D, self.C, self.mask_p, self.mask_p, dtype=self.feat_dtype)
        self.m_ra_ws = ra_ws(B * D)
        self._paste_out = hip.paste_outputs(B, D, self.crop_capacity, dev)
        self.crops, self.mask_boxes, self.mask_rects, self.mask_offsets, self.mask_bytes = self._paste_out.values()
        if self.with_rle:    # COCO RLE of every pasted mask, on the device (dtc_mask_rle): ~100 bytes per mask leave the GPU
            self._rle_out = hip.rle_outputs(B, D, self.rle_runs_stride, self.rle_str_stride, dev, zero_str=True)
            self.rle_counts, self.rle_n_runs, self.rle_str, self.rle_str_len = self._rle_out.values()

    # ---- binding.  The three stages can be bound / launched one by one by a model that runs its head GEMMs / convs in between
    # (detector.forward_batched):  launch_proposals -> box head -> launch_detections -> mask head -> launch_masks ------------------
    def _bind_rpn(self, rpn_cls, rpn_bbox, feats, scores_are_logits, im_hw):
        """rpn_cls / rpn_bbox / feats: one tensor per level.  im_hw [B,2]: each image's own blob size (h_b, w_b) inside the padded
        batch (dtc_rpn_topk_decode_sized); its proposals are those of a batch-1 run on that blob.  Kept in the device tensor
        self.rpn_im_hw, which every launch (and a captured graph) reads: sizes written into it in place apply to the next step.
        None: every image is (pad_h, pad_w)."""
        self.rpn_cls, self.rpn_bbox = rpn_cls, rpn_bbox
        self.prop_in = None
        self.rpn_im_hw = _device_hw(im_hw, self.B, self.dev)
        n = len(self.strides)
        self.rpn_lv, self._alive = hip.make_rpn_levels(rpn_cls, rpn_bbox, self.anchors, self.strides, [self.pre] * n,
                                                       scores_are_logits=scores_are_logits)
        need = hip.call("dtc_rpn_topk_decode_workspace_bytes", levels=self.rpn_lv, n_levels=n, batch=self.B, k_stride=self.kmax)
        if getattr(self, "rpn_ws", None) is None or self.rpn_ws.numel() < need:
            self.rpn_ws = hip.workspace(need, self.dev)
        self._bind_feats(feats)

    def _bind_feats(self, feats):
        self.feats = feats
        self.feat_lv, _, _ = hip.make_levels(feats, self.roi_scales)
        self.feat_code, self.out_code = hip._dtype_code(feats[0].dtype), hip._dtype_code(self.feat_dtype)
        self.graph = None

    def _bind_proposals(self, boxes, counts, im_scale, feats, dedup_scale):
        """Precomputed proposals instead of the RPN (the Fast R-CNN flows).  boxes float32 [B,N,4] (original-image coordinates,
        N <= top_n and <= 2048), counts int32 [B] (rows past them are ignored), im_scale float32 [B] (the blob scale of each image).
        Kept as self.prop_in / prop_in_counts / prop_im_scale, which every launch (and a captured graph) reads; self.prop_src [B,T] =
        the input row of each roi (np.unique's index).  launch_proposals then runs dtc_prepare_proposals -- scale, remove_dup_prop,
        add_multilevel_rois_for_test -- instead of the RPN, NMS and collect launches."""
        dev, B = self.dev, self.B
        boxes = torch.as_tensor(boxes)
        if boxes.dim() != 3 or boxes.shape[0] != B or boxes.shape[2] != 4:
            raise ValueError("proposals must be [B, N, 4]")
        N = int(boxes.shape[1])
        if N < 1 or N > self.top_n or N > 2048:
            raise ValueError("proposals per image: 1 <= N <= min(%d, 2048) (the path's roi rows), got %d" % (self.top_n, N))
        self._bind_feats(feats)
        self.prop_in = _device_input(boxes, torch.float32, (B, N, 4), dev)
        self.prop_in_counts = _device_input(counts, torch.int32, (B,), dev)
        self.prop_im_scale = _device_input(im_scale, torch.float32, (B,), dev)
        self.prop_dedup = float(dedup_scale)
        self.prop_src = torch.zeros((B, self.top_n), dtype=torch.int32, device=dev)
        self._prep_out = dict(self._roi_out, src_index=self.prop_src)             # dtc_prepare_proposals writes no roi_scores
        del self._prep_out["roi_scores"]
        self.prep_ws = hip.workspace(hip.call("dtc_prepare_proposals_workspace_bytes", batch=B, max_out=self.top_n), dev)

    def bind_heads(self, cls_score, bbox_pred, scaling_factor, im_size):
        self.cls_score, self.bbox_pred = cls_score, bbox_pred
        self.sf, self.im_size = scaling_factor, im_size
        self.graph = None

    def bind_masks(self, masks):
        """mask-head output [B*max_out, n_cls, M, M] (probabilities)"""
        self.masks = masks
        self.graph = None

    # ---- one method per launch (st: the HIP stream handle) -----------------------------------------------------------------
    def _rpn_topk_decode(self, st):
        hip.call("dtc_rpn_topk_decode_sized", "rpn_topk_decode", levels=self.rpn_lv, n_levels=len(self.strides), batch=self.B,
                 im_h=self.pad_h, im_w=self.pad_w, im_hw=self.rpn_im_hw, min_size_scaled=0.0, workspace=self.rpn_ws,
                 workspace_bytes=self.rpn_ws.numel(), out_boxes=self.pre_boxes, out_scores=self.pre_scores, out_counts=self.pre_counts,
                 k_stride=self.kmax, stream=st)

    def _nms_sorted(self, st):
        hip.call("dtc_nms_sorted", "nms_sorted", boxes=self.pre_boxes, counts=self.pre_counts, n_seg=self.B * len(self.strides),
                 n_stride=self.kmax, thresh=self.rpn_thresh, max_keep=self.P, workspace=self.nms_ws, workspace_bytes=self.nms_ws.numel(),
                 keep=self.keep, keep_stride=self.P, keep_count=self.keep_cnt, stream=st)

    def _gather_kept(self, st=None):
        hip.call("dtc_gather_kept", "gather_kept", sorted_boxes=self.pre_boxes, sorted_scores=self.pre_scores,
                 n_seg=self.B * len(self.strides), k_stride=self.kmax, keep=self.keep, keep_count=self.keep_cnt, keep_stride=self.P,
                 out_boxes=self._prop_boxes, out_scores=self._prop_scores, stream=st or hip.stream_ptr(self.dev))

    def _collect_kept(self, st):
        hip.call("dtc_fpn_collect_distribute_kept", "fpn_collect_kept", sorted_boxes=self.pre_boxes, sorted_scores=self.pre_scores,
                 k_stride=self.kmax, keep=self.keep, keep_count=self.keep_cnt, keep_stride=self.P, batch=self.B,
                 n_in_levels=len(self.strides), post_nms_top_n=self.top_n, k_min=self.k_min, k_max=self.k_max, stream=st,
                 **self._roi_out)

    def _collect_distribute(self, what, st, outputs, **lists):
        hip.call("dtc_fpn_collect_distribute", what, batch=self.B, k_min=self.k_min, k_max=self.k_max, stream=st, **lists, **outputs)

    def _collect(self, st):
        """the gathered per-level lists (one per image and level, already in score order) -> rois5 (b, box), level ids, the RoIAlign
        visiting order; k_min == k_max -> level 0"""
        self._collect_distribute("fpn_collect", st, self._roi_out, in_boxes=self._prop_boxes, in_scores=self._prop_scores,
                                 in_counts=self.keep_cnt, n_in_levels=len(self.strides), in_stride=self.P, post_nms_top_n=self.top_n,
                                 inputs_sorted=1)

    def _prepare_proposals(self, st):
        hip.call("dtc_prepare_proposals", "prepare_proposals", boxes=self.prop_in, counts=self.prop_in_counts,
                 im_scale=self.prop_im_scale, batch=self.B, in_stride=self.prop_in.shape[1], dedup_scale=self.prop_dedup,
                 k_min=self.k_min, k_max=self.k_max, max_out=self.top_n, workspace=self.prep_ws, workspace_bytes=self.prep_ws.numel(),
                 stream=st, **self._prep_out)

    def _roi_align_box(self, st=None):
        hip.roi_align_packed(self.feat_lv, self.C, self.feats[0].dtype, self.roi_desc, self.B * self.top_n, self.box_p, self.box_p,
                             self.sr, self.box_feats, self.ra_ws, st, "roi_align(box)")

    def _roi_align_mask(self, st=None):
        hip.roi_align_packed(self.feat_lv, self.C, self.feats[0].dtype, self.m_desc, self.B * self.max_out, self.mask_p, self.mask_p,
                             self.sr, self.mask_feats, self.m_ra_ws, st, "roi_align(mask)")

    def _postprocess_detections(self, st):
        # one entry for both forms (dtc_postprocess_detections_ex2): with the fused mask-branch mapping (fpn != NULL), or without
        hip.call("dtc_postprocess_detections_ex2", "postprocess_detections_ex2", rois5=self.rois5, n_rois=self.n_rois,
                 cls_score=self.cls_score, scores_are_logits=bool(self.cls_logits), bbox_pred=self.bbox_pred, decoded_boxes=None,
                 scaling_factor=self.sf, im_size=self.im_size, batch=self.B, max_rois=self.top_n, n_cls=self.n_cls, wx=10.0, wy=10.0,
                 ww=5.0, wh=5.0, score_thresh=0.05, nms_thresh=0.5, max_det=self.max_det, opt=self.det_opt, scoring=self.det_scoring,
                 workspace=self.det_ws, workspace_bytes=self.det_ws.numel(), max_out=self.max_out,
                 fpn=self.m_map if self.fused_mask_map else None, stream=st, **self._det_out)

    def _map_mask_levels(self, st):
        """mask branch: level ids of the (scaled) detection boxes, multilevel_rois.py:19-39, as a launch of its own"""
        self._collect_distribute("fpn_map_levels", st, self._mask_roi_out, in_boxes=self.det_scaled, in_scores=None,
                                 in_counts=self.det_count, n_in_levels=1, in_stride=self.max_out, post_nms_top_n=self.max_out,
                                 inputs_sorted=0)

    def _mask_paste(self, st):
        hip.call("dtc_mask_paste", "mask_paste", masks=self.masks, mask_index=None, n_cls=self.n_cls, M=self.M, dets=self.dets,
                 det_count=self.det_count, im_size=self.im_size, batch=self.B, max_out=self.max_out, thresh_binarize=0.5,
                 cls_specific_mask=1, per_image_capacity=self.crop_capacity, stream=st, **self._paste_out)

    def _mask_rle(self, st):
        hip.call("dtc_mask_rle", "mask_rle", crops=self.crops, per_image_capacity=self.crop_capacity, mask_rects=self.mask_rects,
                 mask_offsets=self.mask_offsets, det_count=self.det_count, im_size=self.im_size, batch=self.B, max_out=self.max_out,
                 runs_stride=self.rle_runs_stride, str_stride=self.rle_str_stride, stream=st, **self._rle_out)

    # ---- one pass of the hot path over the bound batch: three stages.  A stage called with a stream handle launches on it;
    # without, on the device's current stream ------------------------------------------------------------------------------------
    def launch_proposals(self, st=None):
        """RPN outputs (or bound precomputed proposals) -> rois5 / level ids / visiting order -> box-head features
        (self.box_feats [B*T, C, box_p, box_p])."""
        st = st or hip.stream_ptr(self.dev)
        if self.prop_in is not None:
            self._prepare_proposals(st)
        else:
            self._rpn_topk_decode(st)
            self._nms_sorted(st)
            if self.fused_gather:
                self._collect_kept(st)
            else:
                self._gather_kept(st)
                self._collect(st)
        self._roi_align_box(st)

    def launch_detections(self, st=None):
        """cls_score (probabilities, or logits with cls_logits=True) + bbox_pred -> dets (-> with the mask branch: the level mapping of
        the scaled detection boxes, fused into the detection launch or separate, and the mask-head features)."""
        st = st or hip.stream_ptr(self.dev)
        self._postprocess_detections(st)
        if not self.with_masks:
            return
        if not self.fused_mask_map:
            self._map_mask_levels(st)
        self._roi_align_mask(st)

    def launch_masks(self, st=None):
        """mask-head outputs [B*D, n_cls, M, M] -> binarised crops (+ COCO RLE strings on the device with with_rle=True)."""
        st = st or hip.stream_ptr(self.dev)
        self._mask_paste(st)
        if self.with_rle:
            self._mask_rle(st)

    def _launch(self):
        st = hip.stream_ptr(self.dev)
        self.launch_proposals(st)
        self.launch_detections(st)
        if self.with_masks and self.masks is not None:       # (a path whose mask-head outputs are not bound yet stops at the features)
            self.launch_masks(st)

    # ---- algorithmic (compulsory) bytes, SURVEY.md section 8(d) ------------------------------------------------------
    def box_roialign_bytes(self):
        fb = sum(f.numel() * f.element_size() for f in self.feats)
        return fb + self.B * self.top_n * 5 * 4 + self.box_feats.numel() * self.box_feats.element_size()

    def results(self, on_overflow="raise"):
        """Host copy of the detections of the last step: list of dict(boxes, scores, classes) per image.

        The reference keeps every detection that ties at the image threshold (result_utils.py:159-163); the fixed-shape rows hold
        max_out of them.  More ties than rows must not disappear silently: on_overflow="raise" (default: an evaluation run must stop),
        or "truncate" for a serving loop that must not abort on a rare tie -- the first max_out rows (class-major order) are returned,
        a warning is issued and the image's dict carries truncated=True and n_detections = the true count."""
        if on_overflow not in ("raise", "truncate"):
            raise ValueError("on_overflow must be 'raise' or 'truncate'")
        cnt = self.det_count.cpu().numpy()
        dets = self.dets.cpu().numpy()
        out = []
        for b in range(self.B):
            n, over = int(cnt[b]), int(cnt[b]) > self.max_out
            if over:
                msg = ("image %d has %d detections (ties at the image threshold) but max_out = %d rows: raise max_out"
                       % (b, n, self.max_out))
                if on_overflow == "raise":
                    raise RuntimeError(msg)
                import warnings
                warnings.warn(msg + " -- truncated", RuntimeWarning)
                n = self.max_out
            d = dict(boxes=dets[b, :n, :4].copy(), scores=dets[b, :n, 4].copy(), classes=dets[b, :n, 5].astype(np.int32))
            if over:
                d["truncated"], d["n_detections"] = True, int(cnt[b])
            out.append(d)
        return out


class FpnRegionPath(RegionPath):
    """The FPN flavour (module docstring): 5 RPN levels, RoIAlign over 4 feature levels (k_min 2 .. k_max 5), always with the mask
    branch."""

    def __init__(self, batch, device, channels=256, n_cls=81, pre_nms_top_n=1000, post_nms_top_n=1000,
                 collect_top_n=1000, rpn_nms_thresh=0.7, max_det=100, max_out=128, mask_res=28,
                 box_pooled=7, mask_pooled=14, sampling_ratio=2, pad_h=synth.FPN_PAD_H, pad_w=synth.FPN_PAD_W,
                 feat_dtype=torch.float32, crop_capacity=8 << 20, cls_logits=False, with_rle=False,
                 rle_runs_stride=4096, rle_str_stride=8192, det_options=None):
        """det_options: dict of the reference's test-time options of box_results_with_nms_and_limit (do_soft_nms, soft_nms_sigma,
        soft_nms_method, do_bbox_vote, bbox_vote_thresh, bbox_vote_method; hip.det_options_scoring), baked into the detection
        launch; None: hard NMS."""
        strides = [float(s) for s in synth.FPN_STRIDES]
        anchors = [generate_anchors(stride=strides[l], sizes=(32.0 * 2 ** l,), aspect_ratios=(0.5, 1, 2))
                   for l in range(5)]                                   # detector.py:203-205
        super().__init__(batch, device, channels=channels, n_cls=n_cls, pre=pre_nms_top_n, post=post_nms_top_n, top_n=collect_top_n,
                         rpn_thresh=rpn_nms_thresh, box_p=box_pooled, mask_p=mask_pooled, sr=sampling_ratio, max_det=max_det,
                         max_out=max_out, mask_res=mask_res, pad_h=pad_h, pad_w=pad_w, feat_dtype=feat_dtype, det_options=det_options,
                         cls_logits=cls_logits, with_masks=True, with_rle=with_rle, crop_capacity=crop_capacity,
                         rle_runs_stride=rle_runs_stride, rle_str_stride=rle_str_stride, strides=strides, anchors=anchors,
                         roi_scales=list(synth.FPN_ROI_SCALES), k_min=2, kmax=pre_nms_top_n, ra_workspace=False)
        # collect reads proposals[keep] in place (dtc_fpn_collect_distribute_kept) where its merge kernel holds the shape; otherwise
        # the gather launch + the plain entry point
        self.fused_gather = self.top_n <= 2048 and self.P <= 1024 and 5 * self.P <= 8192
        self.det_count_c = torch.empty((batch, 1), dtype=torch.int32, device=device)

    def bind(self, rpn_cls, rpn_bbox, feats, cls_score, bbox_pred, masks, scaling_factor, im_size):
        """Attach the (device) inputs of one batch."""
        self.bind_rpn(rpn_cls, rpn_bbox, feats)
        self.bind_heads(cls_score, bbox_pred, scaling_factor, im_size)
        self.bind_masks(masks)

    def bind_rpn(self, rpn_cls, rpn_bbox, feats, scores_are_logits=False, im_hw=None):
        """RPN outputs and feature maps, one tensor per level (RegionPath._bind_rpn)."""
        self._bind_rpn(rpn_cls, rpn_bbox, feats, scores_are_logits, im_hw)

    def bind_proposals(self, boxes, counts, im_scale, feats, dedup_scale=0.0625):
        """Precomputed proposals instead of the RPN: boxes [B,N,4] in original-image coordinates, counts [B], im_scale [B]
        (RegionPath._bind_proposals)."""
        self._bind_proposals(boxes, counts, im_scale, feats, dedup_scale)

    # The fused step does not materialise the per-level proposals (collect reads proposals[keep] in place); readers -- the parity
    # checks -- get them from the gather kernel on demand.
    @property
    def prop_boxes(self):
        if self.fused_gather:
            with torch.cuda.device(self.dev):
                self._gather_kept()
        return self._prop_boxes

    @property
    def prop_scores(self):
        if self.fused_gather:
            with torch.cuda.device(self.dev):
                self._gather_kept()
        return self._prop_scores


class C4RegionPath(RegionPath):
    """The region-proposal hot path of the C4 flavour (BASELINE configs[1]: Faster R-CNN R-50-C4, "1000 RPN proposals,
    RoIAlign 7x7 + NMS only") for a batch of images, device-resident, one hipGraph:

        RPN outputs [B,15,50,84] / [B,60,50,84] --[rpn_topk_decode 63 000 -> 6000, nms_sorted 0.7 -> 1000, gather]-->  generate_proposals.py:31-122
          --[collect (1 level: rois5 + visiting order)]--> rois5 [B,1000,5]
          --[roi_align on res4 [B,1024,50,84], adaptive sampling (sampling_ratio 0)]--> [B*1000,1024,P,P]               detector.py:240-248
          (res5 head + cls/bbox: convs / GEMMs, not part of the hot path -- synthetic outputs)
          --[postprocess_detections]--> dets [B,128,6]                                                                  result_utils.py:76-168
        with_masks (Mask R-CNN C4, eval_mask.ipynb): the detection launch also maps the scaled detection boxes to one level
          --[roi_align 14x14 on res4, sampling_ratio 0]--> mask-head features [B*128,1024,14,14]                         detector.py:99-112
          (shared res5 + deconv + classifier: the caller)  --[mask_paste (M = mask_res), mask_rle]--> crops / COCO RLE  result_utils.py:170-220
        bind_proposals (Fast R-CNN C4, eval_fast.ipynb): precomputed proposals --[prepare_proposals]--> rois5 replaces the RPN stages.
    One RPN level (stride 16, 15 anchors), one feature level (k_min == k_max == 4), RoIAlign through the map-stationary kernel's
    workspace form; the per-level proposals are plain buffers (prop_boxes / prop_scores) the step fills.
    """

    def __init__(self, batch, device, channels=1024, n_cls=81, pre_nms_top_n=6000, post_nms_top_n=1000, rpn_nms_thresh=0.7,
                 pooled=7, sampling_ratio=0, max_det=100, max_out=128, im_h=synth.IM_H, im_w=synth.IM_W,
                 feat_dtype=torch.float32, det_options=None, cls_logits=False, with_masks=False, mask_res=14, with_rle=False,
                 crop_capacity=8 << 20, rle_runs_stride=4096, rle_str_stride=8192):
        """det_options: as FpnRegionPath's (the reference's Soft-NMS / bbox-vote options; None: hard NMS).  cls_logits: the bound
        cls_score is the classifier's raw output (softmax folded into the detection kernel).  with_masks: the mask branch (14x14
        RoIAlign of the detections on res4, paste with M = mask_res, COCO RLE on the device with with_rle)."""
        if with_masks and max_out > 512:
            raise ValueError("with_masks needs max_out <= 512 (the detection launch's fused level mapping)")
        H, W = synth.c4_shape(im_h, im_w)
        super().__init__(batch, device, channels=channels, n_cls=n_cls, pre=pre_nms_top_n, post=post_nms_top_n, top_n=post_nms_top_n,
                         rpn_thresh=rpn_nms_thresh, box_p=pooled, mask_p=14, sr=sampling_ratio, max_det=max_det, max_out=max_out,
                         mask_res=mask_res, pad_h=im_h, pad_w=im_w, feat_dtype=feat_dtype, det_options=det_options,
                         cls_logits=cls_logits, with_masks=with_masks, with_rle=with_rle, crop_capacity=crop_capacity,
                         rle_runs_stride=rle_runs_stride, rle_str_stride=rle_str_stride, strides=[16.0],
                         anchors=[generate_anchors(stride=16.0)],                    # 15 anchors, detector.py:197-199
                         roi_scales=[1.0 / 16.0], k_min=4, kmax=min(pre_nms_top_n, 15 * H * W), ra_workspace=True)
        # the names this flavour's callers read
        self.im_h, self.im_w, self.pooled, self.thresh = im_h, im_w, pooled, rpn_nms_thresh
        self.prop_boxes, self.prop_scores = self._prop_boxes, self._prop_scores

    def bind(self, rpn_cls, rpn_bbox, feat, cls_score, bbox_pred, scaling_factor, im_size, im_hw=None):
        """im_hw [B,2]: each image's own size inside the padded batch, kept in self.rpn_im_hw (RegionPath._bind_rpn)."""
        self.bind_rpn_outputs(rpn_cls, rpn_bbox, feat, im_hw=im_hw)
        self.bind_heads(cls_score, bbox_pred, scaling_factor, im_size)

    # (not named bind_rpn: callers tell the two paths apart by FpnRegionPath's multi-level bind_rpn)
    def bind_rpn_outputs(self, rpn_cls, rpn_bbox, feat, scores_are_logits=False, im_hw=None):
        """The counterpart of FpnRegionPath.bind_rpn: RPN outputs [B,15,H,W] / [B,60,H,W] (scores_are_logits: pre-sigmoid) and res4
        [B,C,H,W]."""
        self._bind_rpn([rpn_cls], [rpn_bbox], [feat], scores_are_logits, im_hw)
        self.rpn_cls, self.rpn_bbox = rpn_cls, rpn_bbox                      # the single tensors, as bound

    def _bind_feats(self, feats):
        super()._bind_feats(feats)
        self.feat = feats[0]

    def bind_proposals(self, boxes, counts, im_scale, feat, dedup_scale=0.0625):
        """Precomputed proposals instead of the RPN (eval_fast.ipynb): as FpnRegionPath.bind_proposals, one level (res4)."""
        self._bind_proposals(boxes, counts, im_scale, [feat], dedup_scale)


def synthetic_c4_batch(batch, device, seed, channels=1024, n_cls=81, top_n=1000, feat_dtype=torch.float32):
    """SURVEY.md section 8(d) cfg2 inputs on the device: argument tuple of C4RegionPath.bind()."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    H, W = synth.c4_shape()
    rn = lambda *s: torch.randn(s, generator=g, device=device)
    rpn_cls = torch.sigmoid(rn(batch, 15, H, W) * 2.0 - 2.0)
    rpn_bbox = rn(batch, 60, H, W) * 0.2
    feat = torch.relu(rn(batch, channels, H, W)).to(feat_dtype)
    cls_score = torch.softmax(rn(batch, top_n, n_cls) * 2.0, dim=2).contiguous()
    bbox_pred = (rn(batch, top_n, 4 * n_cls) * 0.1).contiguous()
    sf = torch.full((batch,), 1.6, device=device)
    im_size = torch.tensor([[500.0, 833.0]] * batch, device=device)
    return rpn_cls, rpn_bbox, feat, cls_score, bbox_pred, sf, im_size


class OverlappedRegionPath(_GraphStep):
    """The same hot path with the batch split into `n_split` sub-batches that run on separate HIP streams inside ONE
    hipGraph (fork/join).  The path alternates chip-filling RoIAlign launches with short latency-bound kernels (radix
    select, NMS reduce, collect, detection finalize) that occupy a handful of CUs; with two sub-batches in flight the
    small kernels of one overlap the RoIAlign of the other instead of serialising behind it."""

    def __init__(self, batch, device, n_split=2, **kw):
        assert batch % n_split == 0
        self.B, self.dev, self.n = batch, device, n_split
        self.sub = [FpnRegionPath(batch // n_split, device, **kw) for _ in range(n_split)]
        self.streams = [torch.cuda.Stream(device=device) for _ in range(n_split)]
        self.graph = None
        p0 = self.sub[0]
        self.max_out, self.top_n, self.pad_h, self.pad_w = p0.max_out, p0.top_n, p0.pad_h, p0.pad_w
        self.box_p, self.mask_p, self.C, self.feat_dtype = p0.box_p, p0.mask_p, p0.C, p0.feat_dtype

    def bind(self, rpn_cls, rpn_bbox, feats, cls_score, bbox_pred, masks, scaling_factor, im_size):
        k = self.B // self.n
        for i, p in enumerate(self.sub):
            sl = slice(i * k, (i + 1) * k)
            p.bind([t[sl] for t in rpn_cls], [t[sl] for t in rpn_bbox], [t[sl] for t in feats], cls_score[sl], bbox_pred[sl],
                   masks[i * k * p.max_out:(i + 1) * k * p.max_out], scaling_factor[sl], im_size[sl])
        self.graph = None

    def _launch(self):
        cur = torch.cuda.current_stream(self.dev)
        for st, p in zip(self.streams, self.sub):
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                p._launch()
        for st in self.streams:
            cur.wait_stream(st)

    @property
    def dets(self):
        return torch.cat([p.dets for p in self.sub], 0)

    @property
    def box_feats(self):
        return torch.cat([p.box_feats for p in self.sub], 0)

    @property
    def det_count(self):
        return torch.cat([p.det_count for p in self.sub], 0)

    def _roi_align_box(self):
        for p in self.sub:
            p._roi_align_box()

    def box_roialign_bytes(self):
        return sum(p.box_roialign_bytes() for p in self.sub)

    def results(self):
        out = []
        for p in self.sub:
            out += p.results()
        return out


class StepPipeline:
    """Consecutive steps in flight.  A step alternates two chip-filling RoIAlign launches (65 % of its time) with a dozen
    latency-bound kernels that occupy a handful of CUs (radix select, NMS reduce, collect, detection finalize, paste); the
    steps of a serving loop are independent batches, so step k+1 is issued on another HIP stream while step k is still
    running and the small kernels of one fill the gaps of the other (one MI355X, batch 8: 0.78 -> 0.60 ms per step).
    `paths` are bound region paths (FpnRegionPath / C4RegionPath), at least `n_inflight` of them: a path owns its workspaces
    and results, so a path is only ever replayed on ITS stream and steps on the same path serialise.  Sub-batches of one
    step on two streams (OverlappedRegionPath) do not give this: they run in phase, RoIAlign against RoIAlign."""

    def __init__(self, paths, device, n_inflight=2):
        assert len(paths) >= n_inflight >= 1
        self.paths, self.dev, self.n = list(paths), device, n_inflight
        self.streams = [torch.cuda.Stream(device=device) for _ in range(n_inflight)] if n_inflight > 1 else [None]
        self.count = 0

    def step(self, use_graph=True):
        """Issue the next step; returns (path, stream) so that the caller can enqueue work behind it on the same stream."""
        i = self.count
        self.count += 1
        p = self.paths[i % len(self.paths)]
        st = self.streams[(i % len(self.paths)) % self.n]        # path j always runs on stream j % n
        if st is None:
            p.step(use_graph=use_graph)
        else:
            # whatever the caller enqueued on ITS stream before this call (binding inputs at first, refilling the bound input
            # tensors between steps later) is ordered before the step; the converse -- do not overwrite the inputs of a step
            # that is still running -- is the caller's: enqueue the refill on the returned stream, or synchronize() first
            st.wait_stream(torch.cuda.current_stream(self.dev))
            with torch.cuda.stream(st):
                p.step(use_graph=use_graph)
        return p, st

    def synchronize(self):
        for st in self.streams:
            if st is not None:
                st.synchronize()


def synthetic_batch(batch, device, seed, channels=256, n_cls=81, top_n=1000, max_out=128, mask_res=28,
                    feat_dtype=torch.float32, channels_last=False):
    """COCO-shaped synthetic inputs of SURVEY.md section 8(d), generated on the device (random-init: there are no
    Detectron weights / COCO images offline).  Returns the argument tuple of FpnRegionPath.bind()."""
    g = torch.Generator(device=device)
    g.manual_seed(int(seed))
    shapes = synth.fpn_level_shapes()
    rn = lambda *s: torch.randn(s, generator=g, device=device)
    rpn_cls = [torch.sigmoid(rn(batch, 3, h, w) * 2.0 - 2.0) for (h, w) in shapes]
    rpn_bbox = [rn(batch, 12, h, w) * 0.2 for (h, w) in shapes]
    feats = [torch.relu(rn(batch, channels, h, w)).to(feat_dtype) for (h, w) in shapes[:4]]
    if channels_last:
        feats = [f.contiguous(memory_format=torch.channels_last) for f in feats]
    cls_score = torch.softmax(rn(batch, top_n, n_cls) * 2.0, dim=2).contiguous()
    bbox_pred = (rn(batch, top_n, 4 * n_cls) * 0.1).contiguous()
    masks = torch.sigmoid(rn(batch * max_out, n_cls, mask_res, mask_res) * 1.5)
    sf = torch.full((batch,), 1.6, device=device)
    im_size = torch.tensor([[500.0, 833.0]] * batch, device=device)
    return rpn_cls, rpn_bbox, feats, cls_score, bbox_pred, masks, sf, im_size
