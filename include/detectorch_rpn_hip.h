/*
 * detectorch_rpn_hip.h -- C ABI of libdetectorch_rpn_hip.so: RPN training for the MI355X (gfx950 / CDNA4): the anchor minibatch
 * (labels, sampling, box targets) and the two RPN losses fused with their dense gradient maps.  A sixth shared library next to
 * libdetectorch_hip.so (include/detectorch_hip.h) and the four other side libraries, whose export lists are pinned and do not grow;
 * the conventions are the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers, workspace; a call that returns an error has enqueued nothing and written nothing.
 * The reference (detectorch) has no text for the anchor assignment -- its train_fast.py stops at Fast R-CNN -- so the contract below
 * IS the specification.  Its building blocks are the reference's own and are pinned to it: cython_bbox.bbox_overlaps,
 * bbox_transform_inv (lib/utils/boxes.py:211-242), generate_anchors, the anchor enumeration of lib/model/generate_proposals.py:124-149
 * and smooth_L1 (lib/model/loss.py:13-20).
 */
#ifndef DETECTORCH_RPN_HIP_H_
#define DETECTORCH_RPN_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the RPN training library ("gfx950"). */
const char* dtc_rpn_train_target_arch(void);

#define DTC_RPN_TRAIN_MAX_LEVELS 8
#define DTC_RPN_TRAIN_MAX_ANCHORS_PER_CELL 16
#define DTC_RPN_TRAIN_MAX_GT 256
#define DTC_RPN_TRAIN_MAX_ANCHORS (1 << 20) /* N: anchors per image, all levels */
#define DTC_RPN_TRAIN_MAX_BATCH_PER_IM 4096

/* One RPN output map (one FPN level, or the single C4 map) for a whole batch, modelled on dtc_rpn_level.  anchors: the A base
 * anchors, row-major [A, 4], as DATA (generate_anchors(stride = feat_stride, ...) in the models; tests pass hand-made ones).
 * The four pointers are read by dtc_rpn_loss only (dtc_rpn_targets ignores them): cls_logits float32 [B, A, H, W] (pre-sigmoid),
 * bbox_pred float32 [B, 4A, H, W], and the gradient maps of the same shapes.
 * ANCHOR NUMBERING.  Anchor (l, a, h, w) has the box anchors_l[a] + (w * stride, h * stride, w * stride, h * stride), each sum one
 * float32 addition of a float32 product (generate_proposals.py:130-148).  Its image-wide index is
 *     i = off_l + (a * H_l + h) * W_l + w,     off_l = sum over the levels before l of A * H * W,     N = off_{n_levels}
 * -- the conv output's own layout: labels[b, off_l : off_l + A H W] viewed as [A, H, W] lines up element for element with cls_logits
 * of level l.  labels, rand_keys, fg_index and max_overlaps are indexed by i. */
typedef struct dtc_rpn_train_level {
  const float* cls_logits;
  const float* bbox_pred;
  float* grad_cls_logits;
  float* grad_bbox_pred;
  int32_t num_anchors, height, width;
  float feat_stride;
  float anchors[DTC_RPN_TRAIN_MAX_ANCHORS_PER_CELL * 4];
} dtc_rpn_train_level;

/* The knobs of the RPN minibatch (defaults in brackets: Detectron's TRAIN.RPN_*). */
typedef struct dtc_rpn_train_params {
  int32_t batch_size_per_im; /* [256]  1 .. 4096 */
  int32_t _pad;
  double fg_fraction;        /* [0.5]  in [0, 1]; the quota F = (int)(fg_fraction * batch_size_per_im), truncated */
  float positive_overlap;    /* [0.7] */
  float negative_overlap;    /* [0.3]  <= positive_overlap */
  float straddle_thresh;     /* [0]    negative: every anchor of the padded maps is kept */
  float _pad2;
} dtc_rpn_train_params;

/* The RPN minibatch of B images at once: a label for every anchor, the sample of batch_size_per_im of them, box targets of the
 * sampled foreground.
 * Inputs (rows past a count may hold any bits, NaN included, and are never read):
 *   gt_boxes float32 [B, G, 4] in ORIGINAL image coordinates, gt_is_crowd int32 [B, G], gt_counts int32 [B] (clamped to [0, G] on
 *   the device; with G = 0 the three may be NULL); im_scale float32 [B]: every gt coordinate is multiplied by it once, in float32
 *   (as rois5 of dtc_fast_rcnn_targets is); im_hw float32 [B, 2]: the scaled image's own (h, w) before padding, read at run time;
 *   rand_keys uint32 [B, N]: the sampling order, supplied by the caller.
 *   n_levels <= 8, A <= 16, G <= 256, N <= 2^20, batch_size_per_im <= 4096: DTC_EUNSUPPORTED beyond.  gt_boxes 16-byte aligned.
 * Per image:
 *   1 inside    x1 >= -st && y1 >= -st && x2 < w_b + st && y2 < h_b + st  (st = straddle_thresh; st < 0: every anchor).  An anchor
 *               that is not inside gets label -1 and takes part in nothing below.
 *   2 overlaps  IoU of every inside anchor against every NON-crowd gt row (crowd rows take no part), each through the pinned element
 *               of cython_bbox.bbox_overlaps (boxes = anchors, query = scaled gt).  max_i: the maximum over gt, 0 without one; arg_i:
 *               the first gt index on ties; gtmax_g: the maximum over the inside anchors.
 *   3 groups    disjoint, FOREGROUND WINS: fg if max_i >= positive_overlap, or if ov(i, g) == gtmax_g and gtmax_g > 0 for some g
 *               (EVERY anchor that ties a gt's best overlap, even when that overlap is below negative_overlap); otherwise bg if
 *               max_i < negative_overlap; otherwise ignored.  A gt whose best overlap is 0 marks nothing.
 *               The last rule and "fg wins" are DELIBERATE departures from Detectron's _get_rpn_blobs, which lets an untouched gt
 *               (gtmax 0) turn every zero-overlap anchor positive, and lets the sampled background overwrite low-quality positives.
 *   4 sampling  as dtc_fast_rcnn_targets: the first min(|fg|, F) foreground anchors in ascending (rand_key, i) order, then the first
 *               min(|bg|, batch_size_per_im - fg_taken) background anchors the same way -- one of the draws npr.choice / npr.randint
 *               may make, the same on every run.  Anchors not taken get label -1.
 *   5 targets   of the taken fg: bbox_transform_inv(anchor, scaled gt[arg_i], weights (1, 1, 1, 1)) in the operation order and with
 *               the dw / dh rule of detectorch_train_hip.h: the logarithm of the float32 ratio is evaluated in double, rounded once.
 * Outputs, every element written on every call (no memset needed; a replay over stale buffers is clean):
 *   labels int32 [B, N] in {1, 0, -1}; fg_index int32 [B, F] in sampling order; fg_targets float32 [B, F, 4]; fg_gt int32 [B, F]: the
 *   matched row among the image's gt rows; n_fg, n_bg int32 [B]; rows >= n_fg[b]: index -1, gt -1, zero targets.  (F = 0: the
 *   three fg arrays are not touched and may be NULL.)
 *   Nullable: max_overlaps float32 [B, N] (0 where not inside); gt_max float32 [B, G] (0 for crowd rows and rows past the count).
 *   Nullable, all three or none: bbox_targets, bbox_inside_weights, bbox_outside_weights float32 [B, 4N], per level laid out as
 *   [4A, H, W] with channel 4a + k (bbox_pred's layout): the targets and inside weight 1 on taken fg anchors, outside weight
 *   1 / (n_fg + n_bg) (one float32 division) on every anchor with label >= 0, zero everywhere else.
 * Eight kernel nodes on the stream; no workgroup waits for another and every loop is bounded by an argument.  The per-gt maximum is
 * an integer maximum on the bits of non-negative floats, the sample a radix select on (rand_key, i) whose integer counters do not
 * depend on arrival order: the same bits on every run.  Capturable in a hipGraph; a replay picks up inputs rewritten in place.
 * The workspace (dtc_rpn_targets_workspace_bytes, 0 for an unsupported shape; 16-byte aligned; needs no initialisation) must be
 * EXCLUSIVE to one in-flight call, like dtc_rpn_topk_decode's. */
size_t dtc_rpn_targets_workspace_bytes(const dtc_rpn_train_level* levels, int n_levels, int batch, int gt_stride);
int dtc_rpn_targets(const dtc_rpn_train_level* levels, int n_levels, int batch, const float* gt_boxes, const int32_t* gt_is_crowd,
                    const int32_t* gt_counts, int gt_stride, const float* im_scale, const float* im_hw, const uint32_t* rand_keys,
                    const dtc_rpn_train_params* params, void* workspace, size_t workspace_bytes, int32_t* labels, int32_t* fg_index,
                    float* fg_targets, int32_t* fg_gt, int32_t* n_fg, int32_t* n_bg, float* max_overlaps, float* gt_max,
                    float* bbox_targets, float* bbox_inside_weights, float* bbox_outside_weights, dtc_stream_t stream);

/* The two RPN losses with their gradients, read from the outputs of dtc_rpn_targets.  labels int32 [B, N]; fg_index int32
 * [B, fg_stride], fg_targets float32 [B, fg_stride, 4]; n_fg, n_bg int32 [B] (n_fg is clamped to [0, fg_stride], negative counts read
 * as 0); beta > 0 (1/9 for the RPN); upstream: NULL or a DEVICE float32 [2] that scales the two GRADIENTS only (as in
 * detectorch_loss_hip.h).  With n_valid = sum_b (n_fg_b + n_bg_b), read on the device:
 *   loss_cls  = sum over the elements with label 0 or 1 of  max(x, 0) - x y + log1p(exp(-|x|))  / max(n_valid, 1); any other label
 *               value is ignored (its logit is not even read);
 *   loss_bbox = (1 / B) sum_b 1 / max(n_fg_b + n_bg_b, 1) sum_{j < n_fg_b} sum_k smoothL1_beta(pred[b, 4a + k, h, w] - fg_targets[b, j, k])
 *               -- the reference's smooth_L1 on the expanded blobs of dtc_rpn_targets; a row whose fg_index is outside [0, N) is
 *               skipped and never becomes an address.
 * Every term is evaluated in double from the float32 inputs (the way the loss library evaluates its terms) and the sums go through
 * per-workgroup partial results added in a fixed order: no float atomics, two calls give the same bits.
 * Outputs: losses float32 [2] = (loss_cls, loss_bbox); n_valid int32 [1]; per level
 *   grad_cls_logits = upstream[0] * (sigmoid(x) - y) / max(n_valid, 1) on the elements with label 0 or 1, +0.0 elsewhere;
 *   grad_bbox_pred  = upstream[1] * d loss_bbox / d pred on the four channels of the rows counted above, +0.0 elsewhere
 *                     (fg_index rows of one image are distinct, as dtc_rpn_targets writes them);
 * every element of both gradient maps is written.  Either gradient group may be NULL (in every level, or in none) for a loss-only
 * call: the loss bits equal the fused call's.  batch >= 1, fg_stride <= 4096.  Three kernel nodes; capturable.  Workspace as above. */
size_t dtc_rpn_loss_workspace_bytes(const dtc_rpn_train_level* levels, int n_levels, int batch);
int dtc_rpn_loss(const dtc_rpn_train_level* levels, int n_levels, int batch, const int32_t* labels, const int32_t* fg_index,
                 const float* fg_targets, const int32_t* n_fg, const int32_t* n_bg, int fg_stride, float beta, const float* upstream,
                 void* workspace, size_t workspace_bytes, float* losses, int32_t* n_valid, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_RPN_HIP_H_ */
