/*
 * detectorch_train_hip.h -- C ABI of libdetectorch_train_hip.so: the training-side natives of detectorch for the MI355X
 * (gfx950 / CDNA4).  A second shared library next to libdetectorch_hip.so (include/detectorch_hip.h), whose export list is
 * pinned and does not grow; the conventions are the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf).
 * Each entry cites the reference code it replaces (paths relative to the detectorch tree).
 */
#ifndef DETECTORCH_TRAIN_HIP_H_
#define DETECTORCH_TRAIN_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the training library ("gfx950"). */
const char* dtc_train_target_arch(void);

/* The knobs of the Fast R-CNN minibatch (train_fast.py's arguments; defaults in brackets).  The thresholds that the reference
 * compares with float32 overlaps are float32 here (numpy compares a float32 array with a Python float in float32); the two that it
 * uses in double arithmetic are doubles. */
typedef struct dtc_train_params {
  int32_t rois_per_image;         /* R: train_batch_size_per_image [512] */
  int32_t num_classes;            /* [81], background included */
  int32_t cls_agnostic_bbox_reg;  /* [0] */
  int32_t _pad;
  double fg_fraction;             /* [0.25]  quota = int(np.round(fg_fraction * R)), half to even */
  double crowd_thresh;            /* [0.7]   <= 0 disables the crowd filter (json_dataset.py:328) */
  float fg_thresh;                /* [0.5] */
  float bg_thresh_hi;             /* [0.5] */
  float bg_thresh_lo;             /* [0] */
  float bbox_thresh;              /* [0.5] */
  float reg_weights[4];           /* [10, 10, 5, 5] */
} dtc_train_params;

#define DTC_TRAIN_MAX_GT 256
#define DTC_TRAIN_MAX_PROPOSALS 2048
#define DTC_TRAIN_MAX_ROIS 4096

/* Fast R-CNN training minibatches for a batch of images, in ONE launch (one workgroup per image): which proposals are foreground
 * and background, their labels, box-regression targets and loss weights.  The device form of the reference's host chain
 *   lib/data/json_dataset.py:333-394  _merge_proposal_boxes_into_roidb      lib/data/json_dataset.py:397-414  _filter_crowd_proposals
 *   lib/data/json_dataset.py:417-435  _add_class_assignments                lib/data/roidb.py:176-206         _compute_targets
 *   lib/utils/fast_rcnn_sample_rois.py:41-137  fast_rcnn_sample_rois        lib/utils/fast_rcnn_sample_rois.py:139-163  _expand_bbox_targets
 * Inputs (all coordinates are ORIGINAL image coordinates, as in the roidb; rows past a count may hold any bits and are never read):
 *   gt_boxes float32 [B, G, 4], gt_classes int32 [B, G] (> 0, < num_classes), gt_is_crowd int32 [B, G], gt_counts int32 [B];
 *   proposals float32 [B, P, 4], proposal_counts int32 [B]; im_scale float32 [B] (the Python-float scale rounded to float32);
 *   rand_keys uint32 [B, G + P]: the sampling order, supplied by the caller.
 *   G <= 256, P <= 2048, R <= 4096 (DTC_EUNSUPPORTED beyond); G or P may be 0 (the pointers of an empty input may be NULL), G + P >= 1;
 *   gt_boxes and proposals 16-byte aligned.  Inputs must be FINITE boxes with x2 >= x1, y2 >= y1: this is not checked.
 *   A count outside [0, stride] is CLAMPED on the device (a negative one reads as 0, one above the stride as the stride): no row
 *   past the stride is read, and the result is that of the call with the clamped counts.  With a stride of 0 the counts pointer
 *   of that input is not read either.
 * The CANDIDATES of image b are its gt rows (all gt_counts[b] of them, crowd included) followed by its proposal_counts[b] proposals:
 * candidate index c < n_cand = gt_counts[b] + proposal_counts[b]; rand_keys[b, c], keep_inds, max_overlaps and max_classes are
 * indexed by c.
 * Semantics (the reference's, bit for bit except dw / dh, see below):
 *   assignment   a non-crowd gt row: overlap 1, its class; a crowd gt row: overlap -1, class 0; a proposal: IoU (cython bbox_overlaps)
 *                against ALL gt, first index on ties; max > 0: (max, that gt's class), else (0, 0)                 json_dataset.py:350-367
 *   crowd filter a proposal becomes (-1, 0) when max over the crowd gt of intersection / proposal area > crowd_thresh  :408-413
 *                computed as pycocotools' bbIou does for iscrowd: in double, on (x, y, w, h) with w = x2 - x1 + 1 formed in float32
 *                (boxes.py:121).  pycocotools is not available where this library is tested: the formula is written from its
 *                published C (common/maskApi.c, bbIou) and is pinned only against a restatement of that text -- parity unpinned.
 *   targets      all zero when the image has no non-crowd gt; else every candidate with overlap >= bbox_thresh gets class =
 *                max_classes (1 when class-agnostic) and the deltas of bbox_transform_inv (boxes.py:211-242, float32, the reference's
 *                operation order) to its IoU-argmax among the NON-crowd gt, first index on ties                       roidb.py:182-205
 *   sampling     fg: overlap >= fg_thresh; bg: bg_thresh_lo <= overlap < bg_thresh_hi; the fg quota, or fewer, in ascending
 *                (rand_key, index) order, then bg up to R - fg_taken the same way; output rows: fg first, then bg, each in that order
 *                -- one of the samples npr.choice(..., replace=False) may draw, the same on every run   fast_rcnn_sample_rois.py:57-88
 *                bg_thresh_hi <= fg_thresh is required (DTC_EINVAL): a candidate is in one group at the most.
 *   labels       max_classes[keep], the bg part 0                                                                          :90-91
 *   expansion    keyed by the TARGET class (> 0), not the label: 4 targets and inside weights 1 at [4 cls, 4 cls + 4), outside
 *                weights = inside > 0; width 4 * num_classes, or 8 when class-agnostic                                 :139-163, :107
 *   dw, dh       w * log(ratio): the logarithm of the float32 ratio is evaluated in double and rounded to float32 (the reference's
 *                np.log is another float32 implementation, a few ulp apart), then one float32 multiply.
 * Outputs, R = rois_per_image, written on EVERY row on every call (no memset needed, a replay over stale buffers is clean):
 *   rois5 float32 [B, R, 5] = (b, box * im_scale), one float32 multiply per coordinate; labels int32 [B, R];
 *   bbox_targets5 float32 [B, R, 5] = (class, dx, dy, dw, dh); keep_inds int32 [B, R]; n_fg, n_rois int32 [B];
 *   bbox_targets, bbox_inside_weights, bbox_outside_weights float32 [B, R, W] (16-byte aligned; all three or none: NULL skips them);
 *   max_overlaps float32, max_classes int32 [B, G + P] (nullable, both or none; entries past n_cand: 0).
 *   Rows >= n_rois[b]: label -1, keep_inds -1, zero targets and weights, rois5 = (b, 0, 0, 0, 0).
 * No workspace, no atomics, one kernel node: capturable in a hipGraph, and a replay picks up inputs rewritten in place. */
int dtc_fast_rcnn_targets(const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_is_crowd, const int32_t* gt_counts,
                          const float* proposals, const int32_t* proposal_counts, const float* im_scale, const uint32_t* rand_keys,
                          int batch, int gt_stride, int proposal_stride, const dtc_train_params* params, float* rois5,
                          int32_t* labels, float* bbox_targets5, float* bbox_targets, float* bbox_inside_weights,
                          float* bbox_outside_weights, int32_t* keep_inds, int32_t* n_fg, int32_t* n_rois, float* max_overlaps,
                          int32_t* max_classes, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_TRAIN_HIP_H_ */
