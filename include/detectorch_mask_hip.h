/*
 * detectorch_mask_hip.h -- C ABI of libdetectorch_mask_hip.so: training of the mask branch of Mask R-CNN for the MI355X (gfx950 /
 * CDNA4): the mask targets of a minibatch (Detectron's add_mask_rcnn_blobs: polygons rasterised into M x M grids) and the
 * class-specific sigmoid cross-entropy fused with its dense gradient.  A seventh shared library next to libdetectorch_hip.so
 * (include/detectorch_hip.h) and the five other side libraries, whose export lists are pinned and do not grow; the conventions are
 * the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers, workspace; a call that returns an error has enqueued nothing and written nothing.
 * The reference (detectorch) has add_mask_rcnn_blobs only as a commented-out call (lib/utils/fast_rcnn_sample_rois.py:125-127); the
 * pieces it rests on are the reference's own: segms.polys_to_boxes (lib/utils/segms.py:120-131), the normalisation of
 * segms.polys_to_mask_wrt_box (:99-110) and cython_bbox.bbox_overlaps.  The rasterisation itself is pycocotools' (frPyObjects and
 * decode), which is not available where this library is tested: it is written from the published algorithm (common/maskApi.c,
 * rleFrPoly and rleDecode), the RASTERISATION RULE below is the specification, and its parity with pycocotools is unpinned.
 */
#ifndef DETECTORCH_MASK_HIP_H_
#define DETECTORCH_MASK_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the mask training library ("gfx950"). */
const char* dtc_mask_train_target_arch(void);

#define DTC_MASK_MAX_M 56             /* mask resolution M: 1 .. 56 */
#define DTC_MASK_MAX_GT 256           /* G: gt rows per image */
#define DTC_MASK_MAX_ROWS 512         /* Fm: mask rows per image */
#define DTC_MASK_MAX_ROIS 4096        /* R: minibatch rows per image */
#define DTC_MASK_MAX_PROPOSALS 65536  /* P: proposal rows per image */
#define DTC_MASK_MAX_POLYS 4096       /* NP: polygons per image */
#define DTC_MASK_MAX_POINTS 65536     /* PTS: polygon points per image */
#define DTC_MASK_MAX_LOSS_ROWS (1 << 20) /* Rm of dtc_mask_loss */
#define DTC_MASK_MAX_CLASSES 1024     /* K of dtc_mask_loss */

/* The mask targets of B images at once, on the compact minibatch that dtc_fast_rcnn_targets wrote (detectorch_train_hip.h).
 * Inputs (rows past a count may hold any bits, NaN included):
 *   labels int32 [B, R], keep_inds int32 [B, R], n_rois int32 [B]: the minibatch outputs; n_rois is clamped to [0, R];
 *   gt_boxes float32 [B, G, 4] and proposals float32 [B, P, 4] in ORIGINAL image coordinates: the candidates keep_inds indexes, the
 *   image's gt rows (gt_counts[b] of them, clamped to [0, G]) followed by its proposals; gt_classes, gt_is_crowd int32 [B, G];
 *   im_scale float32 [B];
 *   the polygons of image b as three fixed-shape tensors: poly_xy float32 [B, PTS, 2], the image's points (x, y) concatenated;
 *   poly_ptr int32 [B, NP + 1], polygon q owns the points poly_ptr[q] .. poly_ptr[q + 1] - 1; gt_poly_ptr int32 [B, G + 1], gt g owns
 *   the polygons gt_poly_ptr[g] .. gt_poly_ptr[g + 1] - 1;
 *   M in 1 .. 56; k_min <= k_max, both in 0 .. 15; mask_rows = Fm in 1 .. 512.
 *   G <= 256, R in 1 .. 4096, P <= 65536, NP <= 4096, PTS <= 65536: DTC_EUNSUPPORTED beyond.  G, P, NP and PTS may be 0 (G + P >= 1);
 *   with G = 0 the gt pointers and gt_poly_ptr, with P = 0 proposals, with G, NP or PTS = 0 poly_xy and poly_ptr may be NULL.
 *   gt_boxes and proposals 16-byte aligned.
 * Per image:
 *   mask rows    the minibatch rows r < n_rois with labels > 0, in row order, the first Fm of them: roi_has_mask is 1 on those rows
 *                and 0 on every other row r < R; mask_class = the label; box = candidates[keep_inds] (original coordinates);
 *                mask_rois = (b, box * im_scale[b]), one float32 multiply per coordinate: bit-equal to the minibatch's own rois5 row;
 *                mask_roi_levels = fpn_level(scaled box, k_min, k_max) - k_min (csrc/fpn_map.h: multilevel_rois.py:41-53), 0 when
 *                k_min == k_max.
 *   no fg row    row 0 is the first minibatch row with label 0, with masks all -1 and class 0; n_mask = 1 and roi_has_mask = 1 on
 *                that row (Detectron's fallback, so that the mask head never sees an empty batch); no such row either: n_mask = 0.
 *   valid        a polygon q is VALID when 0 <= poly_ptr[q], poly_ptr[q] + 3 <= poly_ptr[q + 1] <= PTS and all its points are finite;
 *                any other polygon (Detectron's loader drops those of fewer than 3 points) takes part in nothing.
 *   eligible gt  g < gt_counts with gt_classes > 0, gt_is_crowd == 0, 0 <= gt_poly_ptr[g] <= gt_poly_ptr[g + 1] <= NP and at least one
 *                valid polygon.  Its poly-box is the tight (min x, min y, max x, max y) over the points of its valid polygons
 *                (segms.polys_to_boxes).
 *   matching     each mask row goes to the eligible gt with the largest bbox_overlaps(boxes = box, query = poly-box) (the pinned
 *                element of cython_bbox.bbox_overlaps, the `+ 1` form); the first maximum on ties (np.argmax).  Without an eligible
 *                gt, with keep_inds outside the candidates or with a non-finite box the row is KEPT and matches nothing: masks all
 *                -1 (a row whose keep_inds is out of range has a zero box as well).  keep_inds is never used as an address unchecked.
 *   raster       for the matched gt, every valid polygon is normalised as polys_to_mask_wrt_box does, in float32 with one rounding per
 *                operation: w = max(x2 - x1, 1), px = ((px - x1) * M) / w, h and py likewise; a polygon with a normalised coordinate
 *                that is not finite or of magnitude >= 2^26 contributes nothing; the values are widened to double and rasterised by the
 *                rule below on an M x M grid; the mask is the OR over the gt's polygons (0 when none contributes).
 * RASTERISATION RULE (h = w = M; trunc is C's (int): toward zero):
 *   vertices   X = trunc(5 x + 0.5), Y = trunc(5 y + 0.5); the polygon is closed back to its first vertex.
 *   edges      each edge is traced on its own from (xs, ys) to (xe, ye), dx = |xe - xs|, dy = |ye - ys|, the ends swapped so that the
 *              major coordinate increases.  dx >= dy and dx > 0: the trace points are u = xs + t, v = trunc(ys + s t + 0.5) with
 *              s = (ye - ys) / dx in double, t = 0 .. dx.  dx < dy: v = ys + t, u = trunc(xs + s t + 0.5) with s = (xe - xs) / dy,
 *              t = 0 .. dy.  dx = dy = 0: nothing.
 *   events     every pair of consecutive trace points whose u differ is a candidate with us = min(u), vs = min(v); it is an event only
 *              if us = 5 i + 2 for a pixel column 0 <= i <= w - 1 (the crossing of the column's centre line); its row is
 *              j = ceil(clamp((vs + 0.5) / 5 - 0.5, 0, h)); it toggles the column-major position i h + j (j = h: the start of the next
 *              column; position h w is past the end and dropped).
 *   result     pixel (row y, column x) is on iff the number of events at positions <= x h + y is odd.
 * Outputs, every element written on every call (no memset needed; a replay over stale buffers is clean):
 *   mask_rois float32 [B, Fm, 5]; masks int32 [B, Fm, M * M] in {0, 1, -1}, row-major [y][x]; mask_class int32 [B, Fm];
 *   mask_roi_levels int32 [B, Fm]; n_mask int32 [B]; nullable: roi_has_mask int32 [B, R], mask_gt int32 [B, Fm]: the matched gt row,
 *   -1 where the row matches nothing.  Rows >= n_mask[b]: masks -1, class 0, mask_gt -1, zeros elsewhere.
 * Two kernel nodes (one workgroup per image: rows, poly-boxes, matching; one workgroup per mask row: rasterisation); integer LDS
 * atomics only: the same bits on every run.  Capturable in a hipGraph; a replay picks up inputs rewritten in place.  The workspace
 * (dtc_mask_targets_workspace_bytes, 0 for an unsupported shape; 16-byte aligned; needs no initialisation) must be exclusive to one
 * in-flight call. */
size_t dtc_mask_targets_workspace_bytes(int batch, int mask_rows);
int dtc_mask_targets(const int32_t* labels, const int32_t* keep_inds, const int32_t* n_rois, int batch, int rois_per_image,
                     const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_is_crowd, const int32_t* gt_counts,
                     int gt_stride, const float* proposals, int proposal_stride, const float* im_scale, const float* poly_xy,
                     const int32_t* poly_ptr, const int32_t* gt_poly_ptr, int points_stride, int polys_stride, int M, int k_min,
                     int k_max, int mask_rows, void* workspace, size_t workspace_bytes, float* mask_rois, int32_t* masks,
                     int32_t* mask_class, int32_t* mask_roi_levels, int32_t* roi_has_mask, int32_t* n_mask, int32_t* mask_gt,
                     dtc_stream_t stream);

/* Detectron's class-specific SigmoidCrossEntropyLoss (normalised, weight 1) on the compact targets, fused with its gradient.
 *   mask_logits float32 [Rm, K, M, M] (pre-sigmoid); masks int32 [Rm, M * M]; mask_class int32 [Rm]; upstream: NULL or a DEVICE
 *   float32 scalar that scales the GRADIENT only.  Rm = rows in 1 .. 2^20, K in 1 .. 1024, M in 1 .. 56.
 * An element (r, e) is VALID when 0 <= mask_class[r] < K and masks[r, e] is 0 or 1 (any other target -- 2, negative values, INT_MIN --
 * is ignored and its logit not read).  n_valid, counted on the device, is their number.
 *   loss   = sum over the valid elements of  max(x, 0) - x t + log1p(exp(-|x|)),  x = mask_logits[r, mask_class[r], e], t = masks[r, e],
 *            divided by n_valid; 0 when n_valid = 0.
 *   grad   = upstream * (sigmoid(x) - t) / n_valid on the valid elements of channel mask_class[r], +0.0 on every other element of
 *            [Rm, K, M, M]: every element is written exactly once, with 16-byte stores wherever the address allows.
 * Every term is evaluated in double from the float32 inputs and rounded once; the sums go through per-workgroup partial results in a
 * launch shape that depends on Rm alone, added in a fixed order: no float atomics, two calls give the same bits, and a loss-only call
 * (grad_mask_logits NULL) gives the fused call's bits.  Outputs: loss float32 [1], n_valid int32 [1], grad_mask_logits (nullable).
 * Three kernel nodes; capturable.  Workspace as above (dtc_mask_loss_workspace_bytes, monotone, 0 for a rejected shape). */
size_t dtc_mask_loss_workspace_bytes(int rows, int K, int M);
int dtc_mask_loss(const float* mask_logits, const int32_t* masks, const int32_t* mask_class, int rows, int K, int M,
                  const float* upstream, void* workspace, size_t workspace_bytes, float* loss, int32_t* n_valid,
                  float* grad_mask_logits, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_MASK_HIP_H_ */
