/*
 * detectorch_flip_hip.h -- C ABI of libdetectorch_flip_hip.so: the horizontal-flip augmentation of the reference's training data
 * (lib/data/roidb.py:extend_with_flipped_entries, lib/utils/segms.py:flip_segms, lib/utils/boxes.py:flip_boxes and the
 * image[:, ::-1, :] of lib/data/coco_dataset.py:51-53) on the MI355X (gfx950 / CDNA4): the network input of a mirrored image, its
 * boxes, its polygons and its COCO run lists, each mirrored where a per-image flag says so.
 * An eleventh shared library next to libdetectorch_hip.so and the nine other side libraries, whose export lists are pinned and do
 * not grow; the conventions are the same:
 *   - DEVICE pointers, caller-owned (dtc_flip_prep_images' descriptor arrays are HOST arrays read at call time, as dtc_prep_images');
 *     nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers, workspace; a call that returns DTC_EINVAL, DTC_EUNSUPPORTED or DTC_EWORKSPACE has
 *     enqueued nothing and written nothing; DTC_ELAUNCH is the runtime refusing a launch,
 *   - every entry can be captured in a hipGraph after one eager call; a replay picks up inputs rewritten in place (the flags and
 *     widths of entries 2-4 are device data; dtc_flip_prep_images' flags are baked into the captured kernel arguments),
 *   - no input value is used as an address unchecked.
 * Exact arithmetic only (two float32 subtractions, two float64 subtractions and a cast, integers): the same bits on every run.
 * Out of scope: scale jitter, keypoint flipping (commented out in the reference).  (Flip test-time augmentation is
 * detectorch_aug_hip.h's.)
 */
#ifndef DETECTORCH_FLIP_HIP_H_
#define DETECTORCH_FLIP_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the flip library ("gfx950"). */
const char* dtc_flip_target_arch(void);

#define DTC_FLIP_MAX_BATCH 65535       /* B / N of entries 2-4 (dtc_flip_prep_images: 32 images, as dtc_prep_images) */
#define DTC_FLIP_MAX_BOX_ROWS (1 << 20) /* R of dtc_flip_boxes */
#define DTC_FLIP_MAX_BOX_COLS 4096     /* cols of dtc_flip_boxes */
#define DTC_FLIP_MAX_POINTS 65536      /* PTS: DTC_POLY_MAX_POINTS */
#define DTC_FLIP_MAX_POLYS 4096        /* NP: DTC_POLY_MAX_POLYS */
#define DTC_FLIP_MAX_ROWS 65535        /* R of dtc_flip_rle: masks per image */
#define DTC_FLIP_MAX_RUNS (1 << 20)    /* runs_stride and out_stride: DTC_SEGM_MAX_RUNS */
#define DTC_FLIP_MAX_PIXELS (1 << 30)  /* h * w of an image: DTC_SEGM_MAX_PIXELS */

/* 1. The network input of a batch in which image b is mirrored left to right where flipped[b] != 0: dtc_prep_images (detectorch_hip.h)
 * with one more argument.  images, pixel_means, im_scales, out_hw and flipped are HOST arrays read at call time ([batch], [3],
 * [batch], [batch, 2], [batch]); the flag travels in the kernel-argument descriptor with the rest of the image.  dtc_prep_plan is
 * used as it is: scales and sizes do not depend on the flip.  For a mirrored image the result is BIT-EQUAL to dtc_prep_images on
 * image[:, ::-1, :]: the taps and weights of destination column x are those of the mirrored image, read from the source columns
 * w - 1 - sx and w - 1 - sx1 -- mirrored about the image's own width, not the blob's: the zero padding stays on the right.  An
 * image with flipped[b] == 0 gets dtc_prep_images' bits.  Arguments, checks and codes are dtc_prep_images'; flipped NULL: DTC_EINVAL. */
int dtc_flip_prep_images(const dtc_image* images, int batch, const int32_t* flipped, const double* pixel_means,
                         const double* im_scales, const int32_t* out_hw, float* blob, int blob_h, int blob_w, dtc_stream_t stream);

/* 2. Boxes (ground truth, given proposals): boxes float32 [B, R, cols], cols a positive multiple of 4 (the reference's flip_boxes
 * handles [:, 0::4] and [:, 2::4]); counts int32 [B] or NULL (all R rows; a count is clamped to [0, R]); im_width int32 [B];
 * flipped int32 [B]; out float32 [B, R, cols], which may BE boxes (in place); any other overlap of the two: DTC_EINVAL.
 * Where flipped[b] != 0, for a row below counts[b] and every group of four columns, in float32 and in this order (roidb.py:114-117;
 * numpy keeps float32 against the Python-int width):  x1' = (float)w - x2 - 1.f,  x2' = (float)w - x1 - 1.f.  Everything else --
 * y1, y2, rows past the count, images that are not flipped -- is copied bit for bit.
 * 1 <= B <= 65535, 0 <= R <= 2^20, 4 <= cols <= 4096: DTC_EUNSUPPORTED beyond; cols % 4 != 0: DTC_EINVAL.  R = 0: nothing to do. */
int dtc_flip_boxes(const float* boxes, const int32_t* counts, const int32_t* im_width, const int32_t* flipped, int batch,
                   int rows_stride, int cols, float* out, dtc_stream_t stream);

/* 3. Polygons, in the layout of dtc_poly_rle (detectorch_poly_hip.h) and dtc_mask_targets: poly_xy FLOAT64 [B, PTS, 2], poly_ptr int32
 * [B, NP + 1]; im_width, flipped int32 [B].  Outputs out64 float64 [B, PTS, 2] and / or out32 float32 [B, PTS, 2]; either may be NULL,
 * both NULL: DTC_EINVAL.  out64 may BE poly_xy; any other overlap: DTC_EINVAL.
 * Where flipped[b] != 0, the x of every point below poly_ptr[b][NP] (clamped to [0, PTS]) becomes (double)w - x - 1.0 in double
 * (segms.py:37-40 on np.array(poly)).  out32 is the float32 rounding of THAT double -- what polys_to_mask_wrt_box sees after
 * np.array(poly, dtype=np.float32) -- not a float32 flip of a float32 point: at w = 640, x = 639.49 the two differ.  Points past the
 * last offset, y coordinates and images that are not flipped are copied (out32: the plain cast), so packing host-flipped lists equals
 * flipping the packed lists, padding included.
 * 1 <= B <= 65535, 0 <= PTS <= 65536, 0 <= NP <= 4096: DTC_EUNSUPPORTED beyond.  PTS = 0: nothing to do.  poly_xy and out64 8-byte
 * aligned. */
int dtc_flip_polygons(const double* poly_xy, const int32_t* poly_ptr, const int32_t* im_width, const int32_t* flipped, int batch,
                      int points_stride, int polys_stride, double* out64, float* out32, dtc_stream_t stream);

/* 4. COCO run lists mirrored without a bitmap: the reference's _flip_rle (decode column-major, mask[:, ::-1], encode).
 * Inputs: runs uint32 [N, R, runs_stride] and n_runs int32 [N, R], as dtc_mask_rle, dtc_poly_rle and pack_gt_masks leave them; counts
 * int32 [N] or NULL (all R rows; clamped to [0, R]); im_size float32 [N, 2] = (h, w), truncated to integers as in dtc_segm_iou (below
 * 1, NaN: 0); flipped int32 [N].
 * Outputs: out_runs uint32 [N, R, out_stride], which must not overlap runs (DTC_EINVAL); out_n_runs int32 [N, R]; need int32 [N, R],
 * the runs the row takes, written whatever the capacity.
 * A row below counts[n] of an image with flipped[n] != 0:
 *   n_runs < 0 or n_runs > runs_stride (a mask that did not fit upstream): out_n_runs = -1, need = 0;
 *   n_runs = 0 (pack_gt_masks' "no segmentation"): out_n_runs = 0, need = 0;
 *   runs that do not sum to exactly h w, or h w > 2^30: out_n_runs = -1, need = 0;
 *   otherwise the canonical COCO list of the mirrored bitmap: the runs alternate zeros and ones and start with zeros, only the first
 *   run may have length 0, the runs sum to h w -- also when the input carries zero-length runs anywhere; an image of 0 pixels gives the
 *   single run [0].  need = its length; out_n_runs = need when need <= out_stride, else -1 (runs of such a row hold no valid data).
 *   A flip can lengthen a list: the 3 x 4 mask with pixels (2, 1) and (0, 2) goes from [5, 2, 5] to [3, 1, 4, 1, 3]; never beyond
 *   3 n_runs + 1.
 * A row below counts[n] of an image that is not flipped is copied as it is: need = n_runs, out_n_runs = n_runs when it fits out_stride,
 * else -1; n_runs < 0 or > runs_stride: out_n_runs = -1, need = 0.  Rows past counts[n] are not written, in any output.
 * Nothing is written past a row's out_stride; out_runs past a row's out_n_runs are unspecified.
 * 1 <= N <= 65535, 0 <= R <= 65535, 1 <= runs_stride, out_stride <= 2^20: DTC_EUNSUPPORTED beyond.  R = 0: nothing to do.  h w <= 2^30
 * is the caller's to keep (im_size lives on the device): past it the row gets -1, never a wrong address.
 * One kernel node, one workgroup per (image, row), no sort.  A run [s, e) touches the columns c0 = s / h .. c1 = (e - 1) / h and
 * splits into at most three pieces: a head in c0, a block of whole columns c0 + 1 .. c1 - 1, which stays one piece when mirrored, and
 * a tail in c1 -- a background run over a thousand columns is three pieces.  A piece in column c at rows [y0, y1) moves to
 * (w - 1 - c) h + y0; pieces keep their order inside a column and the columns reverse.  Pass 1 walks the runs in chunks with
 * carried scans and leaves the pieces in the workspace in input order, each with the index at which its column group starts; pass 2
 * walks the output order -- piece T - 1 - o mirrored inside its group, the group's end from a carried scan over the group marks --,
 * merges neighbours of equal value and writes the differences of the starts that remain.
 * The workspace (dtc_flip_rle_workspace_bytes, 0 for an unsupported shape; 16-byte aligned; needs no initialisation) holds 3
 * runs_stride pieces of 8 bytes per row and must be exclusive to one in-flight call. */
size_t dtc_flip_rle_workspace_bytes(int batch, int rows_stride, int runs_stride);
int dtc_flip_rle(const uint32_t* runs, const int32_t* n_runs, const int32_t* counts, const float* im_size, const int32_t* flipped,
                 int batch, int rows_stride, int runs_stride, void* workspace, size_t workspace_bytes, uint32_t* out_runs,
                 int out_stride, int32_t* out_n_runs, int32_t* need, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_FLIP_HIP_H_ */
