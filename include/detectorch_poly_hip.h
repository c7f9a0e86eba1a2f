/*
 * detectorch_poly_hip.h -- C ABI of libdetectorch_poly_hip.so: COCO ground-truth polygons at IMAGE size, straight to run lists, on the
 * MI355X (gfx950 / CDNA4): pycocotools' annToRLE for a polygon annotation (common/maskApi.c:rleFrPoly per polygon, then rleMerge of
 * the polygons of one instance), with no bitmap in between.  The run lists are the gt_runs / gt_n_runs of dtc_segm_iou
 * (include/detectorch_segm_hip.h), so MaskEvaluator can be fed from an annotation file.
 * A tenth shared library next to libdetectorch_hip.so and the eight other side libraries, whose export lists are pinned and do not
 * grow; the conventions are the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers, workspace; a call that returns DTC_EINVAL, DTC_EUNSUPPORTED or DTC_EWORKSPACE has
 *     enqueued nothing and written nothing; DTC_ELAUNCH is the runtime refusing a launch, which can follow an enqueued first node,
 *   - the entry can be captured in a hipGraph after one eager call; a replay picks up inputs rewritten in place,
 *   - every output element is rewritten on every call (no memset needed), `runs` past a row's n_runs excepted: those are
 *     unspecified; rows past a count may hold any bits; no input value is used as an address unchecked.
 * pycocotools is not available where this library is tested: the conversion is written from the published algorithm
 * (common/maskApi.c: rleFrPoly, rleMerge), the RASTERISATION RULE below -- the one of include/detectorch_mask_hip.h, restated here
 * for a height h and a width w of their own -- is the specification, tests/poly_rle_ref.py restates it in numpy, and parity with
 * pycocotools itself is unpinned.
 * Integer arithmetic after the trace; integer atomics only and a sort in between: the same bits on every run.
 */
#ifndef DETECTORCH_POLY_HIP_H_
#define DETECTORCH_POLY_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the polygon library ("gfx950"). */
const char* dtc_poly_target_arch(void);

#define DTC_POLY_MAX_GT 256          /* G: gt rows per image */
#define DTC_POLY_MAX_POLYS 4096      /* NP: polygons per image */
#define DTC_POLY_MAX_POINTS 65536    /* PTS: polygon points per image */
#define DTC_POLY_MAX_BATCH 65535     /* N */
#define DTC_POLY_MAX_RUNS (1 << 20)  /* runs_stride: DTC_SEGM_MAX_RUNS */
#define DTC_POLY_MAX_PIXELS (1 << 30) /* h * w of an image: DTC_SEGM_MAX_PIXELS */
/* events_stride at the most.  The events of one gt row are sorted by one workgroup in LDS, by an LSD radix sort that ping-pongs
 * between two buffers of 64-bit keys: 2 * 8 * 8192 = 128 KiB, plus 17 KiB of digit counters, of the 160 KiB of a gfx950 CU; twice
 * as many do not fit.  A convex object as wide as a 1333-pixel image has about 2700 events. */
#define DTC_POLY_MAX_EVENTS 8192

/* annToRLE of polygon annotations for N images at once: one run list per gt row.
 * Inputs:
 *   the polygons of image n as three fixed-shape tensors, the layout of dtc_mask_targets (detectorch_mask_hip.h) with the points in
 *   FLOAT64 -- COCO's coordinates are JSON doubles and rleFrPoly rounds 5 x + 0.5 in double; a coordinate such as 100.1 lands on
 *   another integer after a round trip through float32 --: poly_xy float64 [N, PTS, 2], the image's points (x, y) concatenated;
 *   poly_ptr int32 [N, NP + 1], polygon q owns the points poly_ptr[q] .. poly_ptr[q + 1] - 1; gt_poly_ptr int32 [N, G + 1], gt g owns
 *   the polygons gt_poly_ptr[g] .. gt_poly_ptr[g + 1] - 1; gt_counts int32 [N], clamped to [0, G];
 *   im_size float32 [N, 2] = (h, w), truncated to integers as in dtc_mask_rle and dtc_segm_iou; an image whose h or w is below 1
 *   (NaN included) has 0 pixels.  h * w <= 2^30 is the caller's to keep: im_size lives on the device, so the entry cannot refuse
 *   it; each side and the product are clipped to 2^30 (a wrong answer for that image, never a wrong address).
 *   1 <= N <= 65535, G <= 256, NP <= 4096, PTS <= 65536, 1 <= runs_stride <= 2^20, 1 <= events_stride <= DTC_POLY_MAX_EVENTS:
 *   DTC_EUNSUPPORTED beyond.  G, NP and PTS may be 0; with G = 0 gt_poly_ptr, gt_counts and every output, with G, NP or PTS = 0
 *   poly_xy and poly_ptr may be NULL.  poly_xy 8-byte aligned.
 * valid       a polygon q is VALID when 0 <= poly_ptr[q], poly_ptr[q] + 3 <= poly_ptr[q + 1] <= PTS and all its points are finite;
 *             any other polygon takes part in nothing.  A valid polygon with a coordinate of magnitude >= 2^26 contributes no
 *             pixel (5 x + 0.5 stays far inside an int for every other one).
 * RASTERISATION RULE of one polygon in an image of height h and width w (trunc is C's (int): toward zero):
 *   vertices   X = trunc(5 x + 0.5), Y = trunc(5 y + 0.5) in double; the polygon is closed back to its first vertex.
 *   edges      each edge is traced on its own from (xs, ys) to (xe, ye), dx = |xe - xs|, dy = |ye - ys|, the ends swapped so that the
 *              major coordinate increases.  dx >= dy and dx > 0: the trace points are u = xs + t, v = trunc(ys + s t + 0.5) with
 *              s = (ye - ys) / dx in double, t = 0 .. dx.  dx < dy: v = ys + t, u = trunc(xs + s t + 0.5) with s = (xe - xs) / dy,
 *              t = 0 .. dy.  dx = dy = 0: nothing.
 *   events     every pair of consecutive trace points whose u differ is a candidate with us = min(u), vs = min(v); it is an event only
 *              if us = 5 i + 2 for a pixel column 0 <= i <= w - 1 (the crossing of the column's centre line); its row is
 *              j = ceil(clamp((vs + 0.5) / 5 - 0.5, 0, h)); its column-major position is i h + j (j = h: the start of the next
 *              column; position h w is past the end and dropped).
 *   result     a pixel at column-major position p (row p mod h, column p / h) is on in that polygon iff the number of the
 *              polygon's events at positions <= p is odd.
 * one gt row  g < gt_counts with 0 <= gt_poly_ptr[g] <= gt_poly_ptr[g + 1] <= NP: its mask is the OR over its valid polygons (annToRLE's
 *             merge of the per-polygon RLEs: a polygon nested in another does not cut a hole; a polygon entered twice counts once).
 * run list    the canonical COCO uncompressed RLE of that bitmap: column-major, the runs alternate zeros and ones and start with
 *             zeros, only the first run may have length 0, the runs sum to exactly h w; an all-zero mask of an image with pixels is
 *             the single run [h w].  It is what dtc_mask_rle produces and what dtc_segm_iou takes as gt_runs.
 * Outputs:
 *   runs uint32 [N, G, runs_stride]; n_runs int32 [N, G]; area int32 [N, G], the pixel count (COCO's "area" is often absent from a
 *   converted dataset); need int32 [N, G, 2] = (the events the row produced, the runs the row needs), written whatever the
 *   capacities; the second is -1 when the events did not fit, the run count being unknown then.
 *   A row g >= gt_counts, a row with a malformed polygon range or without a valid polygon, and every row of an image of 0 pixels:
 *   n_runs = 0, area = 0, need = (0, 0) -- the "no segmentation" of pack_gt_masks, an empty mask to dtc_segm_iou.
 *   A row whose events exceed events_stride or whose runs exceed runs_stride: n_runs = -1, area = 0, no valid data in runs.
 *   Nothing is written past a row's runs_stride; runs past a row's n_runs are unspecified.
 * Two kernel nodes, one workgroup per (image, gt row) each.  The first traces the edges -- one edge per thread, and one edge per
 * wavefront with its lanes over the pixel columns where an edge spans many; the closed form per column when dx >= dy, a bisection
 * on the monotone trace per column when dx < dy, so no loop is as long as a coordinate -- and leaves the events of the row, keyed
 * (polygon, position), in the workspace.  The second sorts them in LDS, tags each event by the parity of its rank within its
 * polygon as the start or the end of a span (equal positions cancel by themselves), sorts again by position, scans the coverage
 * count, keeps the positions where the coverage passes between 0 and at least 1 once all events of the position are applied, and
 * writes their differences.  The order in which the first node leaves the events depends on timing; the sorted order does not.
 * The time of a row grows with the pixel columns its edges cross inside the image, whatever the capacities (`need` counts them all).
 * The workspace (dtc_poly_rle_workspace_bytes, 0 for an unsupported shape; 16-byte aligned; needs no initialisation) must be
 * exclusive to one in-flight call. */
size_t dtc_poly_rle_workspace_bytes(int batch, int gt_stride, int points_stride, int polys_stride, int events_stride);
int dtc_poly_rle(const double* poly_xy, const int32_t* poly_ptr, const int32_t* gt_poly_ptr, const int32_t* gt_counts,
                 const float* im_size, int batch, int gt_stride, int points_stride, int polys_stride, int events_stride,
                 void* workspace, size_t workspace_bytes, uint32_t* runs, int runs_stride, int32_t* n_runs,
                 int32_t* area, int32_t* need, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_POLY_HIP_H_ */
