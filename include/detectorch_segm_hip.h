/*
 * detectorch_segm_hip.h -- C ABI of libdetectorch_segm_hip.so: scoring instance masks on the MI355X (gfx950 / CDNA4): the two things in
 * which COCOeval's iouType 'segm' differs from 'bbox' -- the IoU is common/maskApi.c:rleIou on run-length-encoded masks, and a
 * detection's area is its mask's pixel count (loadRes: ann['area'] = maskUtils.area(segm)) -- on the run lists dtc_mask_rle
 * (include/detectorch_hip.h) leaves on the device.  Everything after the match records is the box protocol's: the records of
 * dtc_segm_match have the layouts of dtc_eval_match's and go into dtc_eval_accumulate (include/detectorch_eval_hip.h) as they are.
 * A ninth shared library next to libdetectorch_hip.so and the seven other side libraries, whose export lists are pinned and do not
 * grow; the conventions are the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers; a call that returns DTC_EINVAL or DTC_EUNSUPPORTED has enqueued nothing and written
 *     nothing; DTC_ELAUNCH is the runtime refusing a launch, which in the two-node dtc_segm_iou can follow an enqueued first node,
 *   - every entry can be captured in a hipGraph after one eager call; a replay picks up inputs rewritten in place,
 *   - every output element is rewritten on every call (no memset needed); rows past a count may hold any bits -- garbage runs, huge or
 *     negative run counts, NaN -- and never reach an output; no run count or run value is used as an address.
 * pycocotools is not available where this library is tested: the protocol is written from the published algorithm
 * (pycocotools/cocoeval.py, common/maskApi.c:rleIou / rleArea), the text below is the specification, tests/segm_eval_ref.py restates
 * it on decoded numpy bitmaps, and parity with pycocotools itself is unpinned.  Out of scope: polygon -> RLE at image size (the
 * loader's), compressed RLE strings on the device (the host unpacks the gt's once), keypoint evaluation (OKS: a further IoU entry
 * in front of dtc_segm_match), json files and category ids.
 * Integer sums and one float64 division per pair; no float atomics anywhere: the same bits on every run.
 */
#ifndef DETECTORCH_SEGM_HIP_H_
#define DETECTORCH_SEGM_HIP_H_

#include "detectorch_eval_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the mask-evaluation library ("gfx950"). */
const char* dtc_segm_target_arch(void);

#define DTC_SEGM_MAX_RUNS (1 << 20)    /* det_runs_stride, gt_runs_stride: runs of one mask (a binary search of depth 20) */
#define DTC_SEGM_MAX_PIXELS (1 << 30)  /* h * w of an image: pixel counts and positions are 32-bit integers */

/* maskApi.c:rleIou (and rleArea) for N images at once: every detection mask against every gt mask of its class.
 * Inputs:
 *   dets float32 [N, max_out, 6] and det_count int32 [N] (dtc_postprocess_detections*): only the class column (5) is read; the rows
 *   d < min(max(det_count, 0), max_out) whose class is in 1 .. num_classes - 1 take part;
 *   det_runs uint32 [N, max_out, det_runs_stride] and det_n_runs int32 [N, max_out]: dtc_mask_rle's rle_counts / rle_n_runs as they
 *   are; im_size float32 [N, 2] = (h, w), truncated to integers as in dtc_mask_rle;
 *   gt_runs uint32 [N, G, gt_runs_stride], gt_n_runs int32 [N, G], gt_classes / gt_is_crowd int32 [N, G], gt_counts int32 [N]
 *   (clamped to [0, G]): the rows g < gt_counts whose class is in 1 .. num_classes - 1 take part.
 *   1 <= det_runs_stride, gt_runs_stride <= 2^20, G <= 256 (0 allowed: the gt pointers may then be NULL), 1 <= max_out <= 512,
 *   2 <= num_classes <= 1024, N <= 65535: DTC_EUNSUPPORTED beyond.  h * w <= 2^30 is the caller's to keep: im_size lives on the
 *   device, so the entry cannot refuse it; an image whose h or w is below 1 (NaN included) has 0 pixels, and a product above 2^30
 *   is clipped to 2^30 (a wrong answer for that image, never a wrong address).
 * A run list is COCO's uncompressed RLE: column-major (pixel (x, y) at position x * h + y), the runs alternate zeros and ones and
 *   start with zeros; a zero-length run is allowed anywhere, the first included.  The run ends are the prefix sums of the runs, taken
 *   in 64 bits and clipped to h * w; pixels past the last run are 0.  n_runs is clamped to the stride; n_runs <= 0 is an EMPTY
 *   mask (dtc_mask_rle's "did not fit" markers, a gt without a segmentation).
 * Semantics for a pair (d, g) of rows that take part and have the same class: i = the pixels set in both masks, da / ga = the pixels
 *   set in each (integers); u = gt_is_crowd ? da : da + ga - i; iou = (i == 0) ? 0 : (double)i / (double)u -- one correctly rounded
 *   division, which is what rleIou amounts to, its "i == 0 -> u = 1" included.  Every other element of iou is 0.
 * Outputs:
 *   iou float64 [N, max_out, G]; det_area int32 [N, max_out] and gt_mask_area int32 [N, G]: the pixel counts, 0 on rows that take
 *   part in nothing; n_bad int32 [N]: the rows d < min(max(det_count, 0), max_out) with det_n_runs < 0 (a mask that did not fit: it
 *   is scored as empty, the caller decides what that is worth).
 * Two kernel nodes.  The first, one wave per run list, turns it into clipped run ends -- for a gt paired with the ones accumulated
 *   up to each end -- in the workspace, and writes the areas.  The second runs one wave per same-class pair: the lanes stride over the
 *   detection's one-runs [s, e) and add ones_g(e) - ones_g(s), each found by a binary search in the gt's run ends; the 32-bit partial
 *   sums are reduced across the wave and lane 0 divides.  No bitmap is decoded.
 * The workspace (dtc_segm_iou_workspace_bytes, 0 for an unsupported shape; 16-byte aligned; needs no initialisation) must be
 * exclusive to one in-flight call. */
size_t dtc_segm_iou_workspace_bytes(int batch, int max_out, int det_runs_stride, int gt_stride, int gt_runs_stride);
int dtc_segm_iou(const float* dets, const int32_t* det_count, const uint32_t* det_runs, const int32_t* det_n_runs,
                 const float* im_size, const uint32_t* gt_runs, const int32_t* gt_n_runs, const int32_t* gt_classes,
                 const int32_t* gt_is_crowd, const int32_t* gt_counts, int batch, int max_out, int det_runs_stride, int gt_stride,
                 int gt_runs_stride, int num_classes, void* workspace, size_t workspace_bytes, double* iou, int32_t* det_area,
                 int32_t* gt_mask_area, int32_t* n_bad, dtc_stream_t stream);

/* COCOeval's evaluateImg on a GIVEN IoU matrix, N images at once: dtc_eval_match (include/detectorch_eval_hip.h) with two
 * differences -- the IoU of (d, g) is read from iou instead of being computed from boxes, and a detection's own area is
 * (double)det_area.  Kept apart from dtc_segm_iou so that the walk can be tested on crafted matrices and a further IoU (OKS) needs
 * no second copy of it.
 * Inputs:
 *   dets float32 [N, max_out, 6] and det_count int32 [N]: the score (4) and class (5) columns are read; the rows
 *   d < min(max(det_count, 0), max_out) take part; a row whose class is not in 1 .. num_classes - 1 takes part in nothing;
 *   iou float64 [N, max_out, G], used as given where d and g take part and have the same class, never read elsewhere;
 *   det_area int32 [N, max_out]; gt_classes / gt_is_crowd int32 [N, G], gt_counts int32 [N] (clamped to [0, G]);
 *   gt_area float32 [N, G] or NULL: the area of a gt; NULL: (double)gt_mask_area int32 [N, G], which may be NULL when gt_area is not;
 *   iou_thrs float64 [T] and area_rngs float64 [A, 2] = (lo, hi) on the DEVICE, used as given; max_det = COCO's maxDets[-1];
 *   image_base: the index of image 0 of this call in the whole run (a captured call replays with the image_base it was captured with).
 *   G <= 256 (0 allowed: iou and the gt pointers may then be NULL), 1 <= max_out <= 512, T * A <= 64, A <= 16,
 *   2 <= num_classes <= 1024, N <= 65535, 0 <= image_base, image_base + N <= 2^21: DTC_EUNSUPPORTED beyond.  max_det >= 1.
 * Semantics:
 *   per image and class k in 1 .. num_classes - 1: its detections in score-descending order, ties by row order (a stable sort), the
 *   first max_det of them; a detection's place in that order is its RANK.  Its gt rows g < gt_counts with gt_classes == k;
 *   gtIg[a][g] = crowd || area < lo_a || area > hi_a; the gt are visited "not ignored first", stable.  For every threshold t, area
 *   range a and detection d in rank order: best = min(t, 1 - 1e-10), m = none; walk the gt: skip one already matched at (t, a)
 *   unless it is crowd; stop when m is a not-ignored gt and this one is ignored; IoU < best: next; else best = IoU, m = g (an equal
 *   IoU moves the match to the later gt).  A match marks the detection matched, copies gtIg[a][m] into its ignore bit and marks the
 *   gt matched.  An unmatched detection whose own area is < lo_a or > hi_a is ignored.
 * Outputs, exactly dtc_eval_match's (BIT(a, t) = a * T + t):
 *   dt_rank   int32 [N, max_out]: the rank, or -1 (a row past the count, of no class, or cut by max_det);
 *   dt_match, dt_ignore  uint64 [N, max_out]: bit BIT(a, t) set iff matched / ignored at (a, t); 0 where dt_rank is -1;
 *   gt_ignore int32 [N, G]: bit a = gtIg[a][g]; 0 on a row past the count or of no class;
 *   gt_match  int32 [N, G, A, T]: the detection ROW matched at (a, t), or -1 (for tests; a crowd gt keeps the last one);
 *   npig      int32 [N, num_classes - 1, A]: the gt of class k + 1 with gtIg[a] == 0;
 *   sort_key  int64 [N, max_out]: class << 53 | (score key) << 21 | (image_base + n), INT64_MAX where dt_rank is -1, as there.
 * One kernel node: one wave per (image, class), one lane per (a, t); a detection's row of the IoU matrix is staged in LDS, the
 * matched-gt bitmask of every lane lives in LDS. */
int dtc_segm_match(const float* dets, const int32_t* det_count, const double* iou, const int32_t* det_area,
                   const int32_t* gt_classes, const int32_t* gt_is_crowd, const int32_t* gt_counts, const float* gt_area,
                   const int32_t* gt_mask_area, int batch, int max_out, int gt_stride, int num_classes, const double* iou_thrs,
                   int n_thrs, const double* area_rngs, int n_areas, int max_det, long long image_base, int32_t* dt_rank,
                   uint64_t* dt_match, uint64_t* dt_ignore, int32_t* gt_ignore, int32_t* gt_match, int32_t* npig, long long* sort_key,
                   dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_SEGM_HIP_H_ */
