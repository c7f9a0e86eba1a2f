/*
 * detectorch_mpost_hip.h -- C ABI of libdetectorch_mpost_hip.so: the mask post-processing block of the reference's
 * lib/utils/segms.py -- rle_masks_to_boxes, the mask_util.iou(a, b, iscrowd) under rle_mask_nms and rle_mask_voting, the greedy
 * walk of rle_mask_nms and rle_mask_voting itself -- on the MI355X (gfx950 / CDNA4), on COCO run lists that already sit on the
 * device, without a bitmap.
 * A twelfth shared library next to libdetectorch_hip.so and the ten other side libraries, whose export lists are pinned and do not
 * grow; no other library exports a name that starts with dtc_mpost_.  The conventions are those of detectorch_segm_hip.h:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers, workspace; a call that returns DTC_EINVAL, DTC_EUNSUPPORTED or DTC_EWORKSPACE has
 *     enqueued nothing and written nothing; DTC_ELAUNCH is the runtime refusing a launch,
 *   - every entry can be captured in a hipGraph after one eager call; a replay picks up inputs rewritten in place (thresholds, modes
 *     and methods are baked into the captured kernel arguments),
 *   - every output element of a row that takes part is rewritten on every call; rows past a count may hold any bits and never reach
 *     an output,
 *   - no run value, run count, box coordinate or row count is used as an address: counts are clamped to their strides, positions to
 *     h w,
 *   - no float atomics; float64 sums are taken in a stated order: the same bits on every run.
 *
 * A RUN LIST follows detectorch_segm_hip.h word for word: column-major (position x h + y), zeros first, zero-length runs allowed
 * anywhere; run ends are 64-bit prefix sums clipped to h w (what lies past the last run is zeros); n_runs is clamped to the runs
 * stride; n_runs <= 0 is an empty mask.  im_size float32 [N, 2] = (h, w), each side truncated to an integer (below 1, NaN: 0; above
 * 2^30: 2^30), h w clipped to 2^30.
 * Limits: 1 <= N <= 65535; 1 <= rows per image and side (R, Ra, Rb, T, A) <= 512; 1 <= runs strides, out_stride <= 2^20:
 * DTC_EUNSUPPORTED beyond, DTC_EINVAL below.
 */
#ifndef DETECTORCH_MPOST_HIP_H_
#define DETECTORCH_MPOST_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0. Build identification of the mask post-processing library ("gfx950"). */
const char* dtc_mpost_target_arch(void);

#define DTC_MPOST_MAX_BATCH 65535       /* N */
#define DTC_MPOST_MAX_ROWS 512          /* masks per image and side */
#define DTC_MPOST_MAX_RUNS (1 << 20)    /* runs strides and out_stride: DTC_SEGM_MAX_RUNS */
#define DTC_MPOST_MAX_PIXELS (1 << 30)  /* h * w of an image: DTC_SEGM_MAX_PIXELS */

#define DTC_MPOST_NMS_IOU 0             /* mode of dtc_mpost_nms */
#define DTC_MPOST_NMS_IOMA 1
#define DTC_MPOST_NMS_CONTAINMENT 2
#define DTC_MPOST_VOTE_AVG 0            /* method of dtc_mpost_vote */
#define DTC_MPOST_VOTE_UNION 1

/* 1. rle_masks_to_boxes.  runs uint32 [N, R, runs_stride], n_runs int32 [N, R]; counts int32 [N] or NULL (all R rows; clamped to
 * [0, R]); im_size.  Outputs, for the rows below counts[n] (the others are not written): boxes int32 [N, R, 4] = (x0, y0, x1, y1),
 * the INCLUSIVE pixel bounds of the ones -- an empty mask gives 0, 0, 0, 0, as the reference's np.zeros leaves it --; area int32
 * [N, R], the ones; nonempty int32 [N, R], 1 where area > 0: the reference's `keep`.
 * No bitmap: x0 and x1 are the first and the last one-pixel position divided by h; a one-run [s, e) that crosses a column boundary
 * (s / h != (e - 1) / h) contributes the rows 0 and h - 1, any other s % h and (e - 1) % h.  One wave per list, integer
 * reductions. */
int dtc_mpost_boxes(const uint32_t* runs, const int32_t* n_runs, const int32_t* counts, const float* im_size, int batch,
                    int rows_stride, int runs_stride, int32_t* boxes, int32_t* area, int32_t* nonempty, dtc_stream_t stream);

/* 2. maskUtils.iou(a, b, iscrowd) for two sets of masks of the same images, iscrowd the same for every mask of the call.
 * a_runs uint32 [N, Ra, a_runs_stride], a_n_runs int32 [N, Ra], a_count int32 [N]; b_* likewise with Rb; im_size; crowd: 0 or not.
 * Outputs: ovr float64 [N, Ra, Rb]; a_area int32 [N, Ra]; b_area int32 [N, Rb].
 * With i = |a & b|, aa = |a|, ab = |b| as integers:  u = crowd ? aa : aa + ab - i;  ovr = i == 0 ? 0 : (double)i / (double)u, one
 * correctly rounded division.  With crowd the divisor is the area of the FIRST argument's mask: that is what maskApi.c:rleIou does
 * (dtc_segm_iou states the same).  The comments in the reference's rle_mask_nms say "/ area(m2)"; they are wrong about their own
 * call: ious[m1, m2] = |m1 & m2| / area(m1).
 * No class filtering: every row below a_count[n] pairs with every row below b_count[n].  Everything else -- ovr where either row is
 * past its count, the areas of rows past the counts -- is 0.  a and b may be the same lists.
 * Two kernel nodes: one wave per list leaves clipped run ends (a) and (run end, ones up to it) pairs (b) in the workspace; then one
 * wave per pair walks a's one-runs and takes ones_b(e) - ones_b(s) by binary search.
 * The workspace (dtc_mpost_overlaps_workspace_bytes, 0 for an unsupported shape; 16-byte aligned; needs no initialisation) must be
 * exclusive to one in-flight call. */
size_t dtc_mpost_overlaps_workspace_bytes(int batch, int a_rows, int a_runs_stride, int b_rows, int b_runs_stride);
int dtc_mpost_overlaps(const uint32_t* a_runs, const int32_t* a_n_runs, const int32_t* a_count, const uint32_t* b_runs,
                       const int32_t* b_n_runs, const int32_t* b_count, const float* im_size, int batch, int a_rows, int a_runs_stride,
                       int b_rows, int b_runs_stride, int crowd, void* workspace, size_t workspace_bytes, double* ovr, int32_t* a_area,
                       int32_t* b_area, dtc_stream_t stream);

/* 3. The greedy walk of rle_mask_nms on a GIVEN matrix (kept apart from entry 2 as dtc_segm_match is from dtc_segm_iou: threshold
 * edges need crafted matrices).  dets float32 [N, R, 6] (score in column 4, class in column 5; the boxes are not read); count int32
 * [N] (clamped to [0, R]); ovr float64 [N, R, R]; thresh; mode.
 * Outputs: keep int32 [N, R]: the kept row indices in the order kept, then -1; keep_count int32 [N].
 * The rows below count[n] are walked by descending score; equal scores go by row order, NaN scores come last in row order.  (The
 * reference's np.argsort(-scores) is an unstable sort and leaves ties unspecified: this is the one deliberate choice.)  The first
 * row alive is kept and suppresses every later row j alive OF THE SAME CLASS (the float32 class columns compare equal; a NaN class
 * equals nothing) unless  value(i, j) <= thresh  in float64 -- a NaN value suppresses, as np.where(ovr <= thresh) drops it --:
 *   DTC_MPOST_NMS_IOU          value = ovr[i, j]
 *   DTC_MPOST_NMS_IOMA         value = max(ovr[i, j], ovr[j, i]) on a matrix made with crowd (np.maximum: NaN if either is)
 *   DTC_MPOST_NMS_CONTAINMENT  value = ovr[i, j] on a matrix made with crowd
 * The walk covers all classes together, so keep is in global score order; with one class it is the reference's.  Any other mode:
 * DTC_EINVAL.  One workgroup per image. */
int dtc_mpost_nms(const float* dets, const int32_t* count, const double* ovr, int batch, int rows_stride, double thresh, int mode,
                  int32_t* keep, int32_t* keep_count, dtc_stream_t stream);

/* 4. rle_mask_voting.  top_runs uint32 [N, T, top_runs_stride], top_n_runs int32 [N, T], top_count int32 [N]; all_runs uint32
 * [N, A, all_runs_stride], all_n_runs int32 [N, A], all_dets float32 [N, A, dets_stride] (dets_stride >= 5: box in columns 0..3,
 * score in column 4), all_count int32 [N]; ovr float64 [N, T, A]: entry 2 on (top, all) without crowd, or crafted; im_size;
 * iou_thresh, binarize_thresh; method.
 * Outputs, under dtc_flip_rle's contract: out_runs uint32 [N, T, out_stride], which must not overlap top_runs or all_runs
 * (DTC_EINVAL); out_n_runs int32 [N, T]; need int32 [N, T], the runs the row takes, written whatever the capacity; out_n_runs = need
 * when need <= out_stride, else -1.  Nothing is written past a row's out_stride; rows past top_count[n] are not written.
 *
 * The support box of voter k:  b = all_dets[k, 0:4] truncated TOWARD ZERO to int32 (astype(np.int32); NaN: 0; a magnitude above 2^30
 * is the caller's to avoid: it saturates and never reaches an address);  x_0 = max(b0, 0), x_1 = min(b2 + 1, w), y_0 = max(b1, 0),
 * y_1 = min(b3 + 1, h), used as the NUMPY SLICE [y_0:y_1, x_0:x_1]: a negative end counts from the far edge (x_1 < 0 becomes
 * max(w + x_1, 0)), an empty slice is no support.  On an 8-wide image the x-range 2 .. -5 gives x_1 = -4 -> 4: columns 2 and 3.
 * The weight of voter k at pixel p:  w_k(p) = np.maximum(inside the support ? (double)score_k : 0.0, 1e-5)  (NaN stays NaN).
 *
 * A row t below top_count[n]:
 *   top_n_runs < 0 or > top_runs_stride (a mask that did not fit upstream), or h w > 2^30 before clipping (the caller's to keep,
 *   as in dtc_flip_rle): out_n_runs = -1, need = 0;
 *   the top mask has area 0: the row is copied as it is (need = n_runs, out_n_runs = n_runs when it fits, else -1);
 *   voters = { k < all_count[n] : ovr[t, k] >= iou_thresh } in index order (NaN is no voter); fewer than two: copied as it is (the
 *   reference returns its input when it "only matches itself" and raises on none);
 *   DTC_MPOST_VOTE_AVG: per pixel  num = sum_k w_k(p) m_k(p),  den = sum_k w_k(p),  both float64, added SEQUENTIALLY IN VOTER INDEX
 *   ORDER from 0.0, m_k(p) = 1.0 or 0.0; the pixel is on iff  num / den > binarize_thresh  (one correctly rounded division): bit for
 *   bit np.average(masks, axis=0, weights=ws) > binarize_thresh;
 *   DTC_MPOST_VOTE_UNION: the pixel is on iff some voter has it;
 *   the output is the canonical COCO list of the voted bitmap, as rleEncode gives it: the runs alternate and start with zeros, only
 *   the first may have length 0, they sum to h w; nothing on: [h w].
 * Any other method: DTC_EINVAL.
 * Two kernel nodes: one wave per voter list leaves its clipped run ends and the span of its ones in the workspace; then one
 * workgroup per (image, top) lists the voters and walks the pixels in chunks of one per thread -- for binarize_thresh >= 0 (and
 * UNION) only those between the first and the last one of any voter, where alone a pixel can be on --, each thread looking its pixel
 * up in every voter's run ends; a pixel that differs from the one before starts a run (a scan carried across the chunks numbers
 * them), and the differences of the starts are the runs.  A chunk in which no voter has a pixel costs one lookup per voter, and
 * stretches of them are jumped over.  No h x w frame exists anywhere.
 * The workspace (dtc_mpost_vote_workspace_bytes, 0 for an unsupported shape; 16-byte aligned; needs no initialisation) holds 4 bytes
 * per voter run and must be exclusive to one in-flight call. */
size_t dtc_mpost_vote_workspace_bytes(int batch, int all_rows, int all_runs_stride);
int dtc_mpost_vote(const uint32_t* top_runs, const int32_t* top_n_runs, const int32_t* top_count, const uint32_t* all_runs,
                   const int32_t* all_n_runs, const float* all_dets, const int32_t* all_count, const double* ovr, const float* im_size,
                   int batch, int top_rows, int top_runs_stride, int all_rows, int all_runs_stride, int dets_stride, double iou_thresh,
                   double binarize_thresh, int method, void* workspace, size_t workspace_bytes, uint32_t* out_runs, int out_stride,
                   int32_t* out_n_runs, int32_t* need, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_MPOST_HIP_H_ */
