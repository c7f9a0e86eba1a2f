/*
 * detectorch_eval_hip.h -- C ABI of libdetectorch_eval_hip.so: scoring detections and proposals on the MI355X (gfx950 / CDNA4): the
 * COCO box-AP protocol (pycocotools' COCOeval for iouType 'bbox': computeIoU + evaluateImg, then accumulate) and the reference's
 * evaluate_box_proposals (lib/utils/json_dataset_evaluator.py:238-319), on the fixed-shape tensors the rest of the project produces.
 * An eighth shared library next to libdetectorch_hip.so (include/detectorch_hip.h) and the six other side libraries, whose export
 * lists are pinned and do not grow; the conventions are the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers; a call that returns DTC_EINVAL or DTC_EUNSUPPORTED has enqueued nothing and written
 *     nothing; DTC_ELAUNCH is the runtime refusing a launch, which in the two-node dtc_eval_accumulate can follow an enqueued
 *     first node,
 *   - every entry can be captured in a hipGraph after one eager call; a replay picks up inputs rewritten in place,
 *   - every output element is rewritten on every call (no memset needed); rows past a count may hold any bits, NaN included, and
 *     never reach an output.
 * pycocotools is not available where this library is tested: the protocol is written from the published algorithm
 * (pycocotools/cocoeval.py, common/maskApi.c:bbIou), the text below is the specification, tests/coco_eval_ref.py restates it in numpy,
 * and parity with pycocotools itself is unpinned.  Out of scope: segm and keypoint evaluation, json files and category ids,
 * non-finite scores, reducing records across ranks (gather the detections first).
 * No float atomics anywhere: the same bits on every run.
 */
#ifndef DETECTORCH_EVAL_HIP_H_
#define DETECTORCH_EVAL_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the evaluation library ("gfx950"). */
const char* dtc_eval_target_arch(void);

#define DTC_EVAL_MAX_GT 256            /* G: gt rows per image */
#define DTC_EVAL_MAX_OUT 512           /* max_out: detection rows per image */
#define DTC_EVAL_MAX_PAIRS 64          /* T * A: (threshold, area range) pairs, one lane each */
#define DTC_EVAL_MAX_AREAS 16          /* A */
#define DTC_EVAL_MAX_CLASSES 1024      /* num_classes, background included */
#define DTC_EVAL_MAX_BATCH 65535       /* N of one dtc_eval_match / dtc_eval_proposal_recall call */
#define DTC_EVAL_MAX_IMAGES (1 << 21)  /* image_base + N: images of a whole run (21 bits of sort_key) */
#define DTC_EVAL_MAX_ROWS (1 << 30)    /* rows = images x max_out of dtc_eval_accumulate */
#define DTC_EVAL_MAX_REC_THRS 1024     /* R */
#define DTC_EVAL_MAX_MAX_DETS 16       /* M */
#define DTC_EVAL_MAX_PROPOSALS 65536   /* P: proposal rows per image */

/* COCOeval's computeIoU + evaluateImg for boxes, N images at once.
 * Inputs:
 *   dets float32 [N, max_out, 6] = (x1, y1, x2, y2, score, class) and det_count int32 [N] (dtc_postprocess_detections*): the rows
 *   d < min(max(det_count, 0), max_out) take part; a row whose class is not in 1 .. num_classes - 1 takes part in nothing;
 *   gt_boxes float32 [N, G, 4] xyxy in original image coordinates, 16-byte aligned (DTC_EINVAL otherwise: rows are read as one
 *   16-byte load), gt_classes / gt_is_crowd int32 [N, G], gt_counts int32 [N]
 *   (clamped to [0, G]); gt_area float32 [N, G] or NULL (the area is then the box area below); iou_thrs float64 [T] and area_rngs
 *   float64 [A, 2] = (lo, hi) on the DEVICE, used as given (np.linspace(.5, .95, 10) is the host's, never re-derived here);
 *   max_det = COCO's maxDets[-1]; image_base: the index of image 0 of this call in the whole run (a captured call replays with the
 *   image_base it was captured with).
 *   G <= 256 (0 allowed: the gt pointers may then be NULL), 1 <= max_out <= 512, T * A <= 64, A <= 16, 2 <= num_classes <= 1024,
 *   N <= 65535, 0 <= image_base, image_base + N <= 2^21: DTC_EUNSUPPORTED beyond.  max_det >= 1.
 * Semantics, everything in float64 from the float32 inputs, one rounding per operation, in this order (no contraction):
 *   box      x = x1, y = y1, w = x2 - x1 + 1, h = y2 - y1 + 1 (the reference's xyxy_to_xywh), detections and gt alike; area w * h.
 *   IoU      iw = min(dx + dw, gx + gw) - max(dx, gx), ih likewise; iw <= 0 or ih <= 0: 0; i = iw * ih;
 *            u = crowd ? da : da + ga - i (da, ga: the BOX areas); i / u.
 *   per image and class k in 1 .. num_classes - 1: its detections in score-descending order, ties by row order (a stable sort), the
 *   first max_det of them; a detection's place in that order is its RANK.  Its gt rows g < gt_counts with gt_classes == k;
 *   gtIg[a][g] = crowd || area < lo_a || area > hi_a (area: gt_area, or the box area); the gt are visited "not ignored first",
 *   stable.  For every threshold t, area range a and detection d in rank order: best = min(t, 1 - 1e-10), m = none; walk the gt:
 *   skip one already matched at (t, a) unless it is crowd; stop when m is a not-ignored gt and this one is ignored; IoU < best:
 *   next; else best = IoU, m = g (an equal IoU moves the match to the later gt).  A match marks the detection matched, copies
 *   gtIg[a][m] into its ignore bit and marks the gt matched.  An unmatched detection whose own area is < lo_a or > hi_a is ignored.
 * Outputs (BIT(a, t) = a * T + t):
 *   dt_rank   int32 [N, max_out]: the rank, or -1 (a row past the count, of no class, or cut by max_det);
 *   dt_match, dt_ignore  uint64 [N, max_out]: bit BIT(a, t) set iff matched / ignored at (a, t); 0 where dt_rank is -1;
 *   gt_ignore int32 [N, G]: bit a = gtIg[a][g]; 0 on a row past the count or of no class;
 *   gt_match  int32 [N, G, A, T]: the detection ROW matched at (a, t), or -1 (for tests; a crowd gt keeps the last one);
 *   npig      int32 [N, num_classes - 1, A]: the gt of class k + 1 with gtIg[a] == 0;
 *   sort_key  int64 [N, max_out]: class << 53 | (score key) << 21 | (image_base + n), where the score key is the float32 score
 *             mapped to an unsigned integer that DEcreases with the score (-0 counts as +0); INT64_MAX where dt_rank is -1.  A STABLE
 *             ascending sort of the keys of a whole run, rows concatenated image by image, orders them by class ascending, score
 *             descending, image ascending and rank ascending (equal scores of one image and class are ranked by row).
 * One kernel node: one wave per (image, class), one lane per (a, t); the IoU is recomputed in float64, the matched-gt bitmask of
 * every lane lives in LDS. */
int dtc_eval_match(const float* dets, const int32_t* det_count, const float* gt_boxes, const int32_t* gt_classes,
                   const int32_t* gt_is_crowd, const int32_t* gt_counts, const float* gt_area, int batch, int max_out, int gt_stride,
                   int num_classes, const double* iou_thrs, int n_thrs, const double* area_rngs, int n_areas, int max_det,
                   long long image_base, int32_t* dt_rank, uint64_t* dt_match, uint64_t* dt_ignore, int32_t* gt_ignore,
                   int32_t* gt_match, int32_t* npig, long long* sort_key, dtc_stream_t stream);

/* COCOeval's accumulate over the match records of a whole run.
 * Inputs: dt_rank int32 [rows], dt_match / dt_ignore uint64 [rows], sort_key int64 [rows]: the outputs of dtc_eval_match
 *   concatenated image by image (rows = images x max_out); order int32 [rows]: the permutation that sorts sort_key, ascending and
 *   STABLE (the caller's sort; this library has none); npig int32 [images, num_classes - 1, A]; rec_thrs float64 [R] on the device,
 *   NON-DECREASING; max_dets int32 [M] on the device.
 *   1 <= rows <= 2^30, 1 <= images, T * A <= 64, A <= 16, R <= 1024, M <= 16, num_classes <= 1024: DTC_EUNSUPPORTED beyond.
 * Semantics per class k, area range a, max_dets[m] and threshold t (K = num_classes - 1):
 *   counts[k, a] = the sum of npig over the images; 0: every output of that (k, a) is -1.  A row with dt_rank -1 (its key is
 *   INT64_MAX) belongs to no class, whatever num_classes is.  The detections of k in sorted order with
 *   rank < max_dets[m] take part; tp / fp are the running counts, as float64, of matched & !ignored and !matched & !ignored;
 *   rc = tp / counts, pr = tp / ((fp + tp) + 2^-52) (np.spacing(1)); recall[t, k, a, m] = the last rc, 0 without detections; pr is
 *   made non-increasing from the right (a reverse running maximum); precision[t, r, k, a, m] = pr at the first index with
 *   rc >= rec_thrs[r] (np.searchsorted, side 'left'), 0 past the end.
 * Outputs: precision float64 [T, R, K, A, M], recall float64 [T, K, A, M], counts int32 [K, A].  COCO's summarize (the twelve stats)
 * is NOT computed here: it is numpy's mean over the entries > -1 of slices of these two arrays, taken on the host
 * (detectorch_amd.utils.evaluator.summarize_stats) so that its summation order is numpy's own.
 * Two kernel nodes (counts; then one wave per (class, m), one lane per (a, t): the class's segment of the sorted rows is staged
 * through LDS tile by tile, once forward for the totals and once backward for the running maximum -- any segment length). */
int dtc_eval_accumulate(const int32_t* dt_rank, const uint64_t* dt_match, const uint64_t* dt_ignore, const long long* sort_key,
                        const int32_t* order, long long rows, const int32_t* npig, int images, int num_classes, int n_thrs,
                        int n_areas, const double* rec_thrs, int n_rec, const int32_t* max_dets, int n_max_dets, double* precision,
                        double* recall, int32_t* counts, dtc_stream_t stream);

/* The reference's evaluate_box_proposals (lib/utils/json_dataset_evaluator.py:238-319) for N images at once.
 * Inputs: proposals float32 [N, P, 4] (16-byte aligned) and prop_counts int32 [N] (clamped to [0, P]), already in score order; the
 *   gt tensors of dtc_eval_match (gt_boxes 16-byte aligned), gt_area (the roidb's seg_areas) or NULL (the float64 box area
 *   (x2 - x1 + 1) * (y2 - y1 + 1)); area_rng float64 [2] = (lo, hi) on the device; limit: 0 = none, else P' = min(count, limit).
 *   1 <= P <= 65536, G <= 256 (0: gt pointers may be NULL), N <= 65535: DTC_EUNSUPPORTED beyond.
 * Semantics: the gt taking part are those with gt_is_crowd == 0, gt_classes > 0 and lo <= area <= hi, G' of them, numbered in row
 *   order.  Overlaps are cython_bbox.bbox_overlaps(proposals, gt) in the reference's own float32 arithmetic (iou_bbox of
 *   csrc/box_vote.h).  min(P', G') rounds: each takes the largest remaining overlap, ties to the smallest gt index and then the
 *   smallest proposal index (what the two argmax calls amount to), records it as round j's value and retires that proposal and gt.
 * Outputs: gt_overlaps float64 [N, G]: the value of round j at [n, j], 0 on every other element; n_pos int32 [N] = G';
 *   n_overlaps int32 [N]: the entries the reference appends for the image: G' when P' > 0, else 0 (its `continue`).
 * One kernel node, one workgroup per image; each gt caches its best remaining proposal, refreshed only when that one is retired. */
int dtc_eval_proposal_recall(const float* proposals, const int32_t* prop_counts, const float* gt_boxes, const int32_t* gt_classes,
                             const int32_t* gt_is_crowd, const int32_t* gt_counts, const float* gt_area, int batch,
                             int proposal_stride, int gt_stride, const double* area_rng, int limit, double* gt_overlaps,
                             int32_t* n_pos, int32_t* n_overlaps, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_EVAL_HIP_H_ */
