/*
 * detectorch_grad_hip.h -- C ABI of libdetectorch_grad_hip.so: gradients of the region operators for the MI355X (gfx950 / CDNA4).
 * A fourth shared library next to libdetectorch_hip.so (include/detectorch_hip.h), libdetectorch_train_hip.so
 * (include/detectorch_train_hip.h) and libdetectorch_loss_hip.so (include/detectorch_loss_hip.h), whose export lists are pinned
 * and do not grow; the conventions are the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf).
 * Each entry cites the reference code it replaces (paths relative to the detectorch tree).
 */
#ifndef DETECTORCH_GRAD_HIP_H_
#define DETECTORCH_GRAD_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the gradient library ("gfx950"). */
const char* dtc_grad_target_arch(void);

/* One level of the gradient with respect to the feature maps: a dense float32 NCHW [batch, channels, height, width] map that
 * the call WRITES, 16-byte aligned.  spatial_scale is the level's scale of the forward call. */
typedef struct dtc_grad_level {
  float* grad;
  int32_t height, width;
  float spatial_scale;
  int32_t _pad;
} dtc_grad_level;

#define DTC_GRAD_MAX_POOLED 1024         /* 1 <= pooled_h, pooled_w <= 1024 */
#define DTC_GRAD_MAX_SAMPLING 1024       /* sampling_ratio <= 1024 (<= 0: adaptive) */
#define DTC_GRAD_MAX_ROIS 16777216       /* 0 <= n_rois <= 2^24 */
#define DTC_GRAD_MAX_BATCH 65536         /* 1 <= batch <= 65536 */
#define DTC_GRAD_MAX_EXTENT 1048576      /* 1 <= height, width <= 2^20 */
#define DTC_GRAD_MAX_GRID 32768          /* adaptive sampling grid of one RoI, per direction */

/* Bytes of workspace dtc_roi_align_backward needs: 8 bytes per (level, image) pair and 48 per RoI, whatever the channel count, the
 * pooled size and the maps' extents are.  Monotone in each argument; 0 for arguments the entry rejects. */
size_t dtc_roi_align_backward_workspace_bytes(int n_levels, int batch, int n_rois);

/* The gradient of multi-level RoIAlign with respect to its feature maps: what the reference computes with
 *   lib/model/roi_align.py:93-145                     RoIAlignFunction.backward
 *   lib/cppcuda/roi_align_backward_cpu.cpp:97-185     roi_align_backward_loop (the serial CPU loop)
 * one level at a time; here for up to DTC_MAX_LEVELS levels in one call, RoI r going to level roi_levels[r].
 * Inputs:
 *   levels       n_levels descriptors on the HOST (read during the call only): where each level's gradient is written
 *   rois         float32 [n_rois, roi_cols], roi_cols 5 = (batch index, x1, y1, x2, y2) or 4 = (x1, y1, x2, y2) for image 0,
 *                as dtc_roi_align_forward takes them
 *   roi_levels   int32 [n_rois], or NULL: every RoI on level 0
 *   grad_output  float32 [n_rois, channels, pooled_h, pooled_w], contiguous (4-byte aligned)
 * Output: EVERY element of every level's map is written on every call, exactly once: +0.0 where no RoI reaches.  The caller clears
 * nothing, and no memset node is enqueued.
 * Results.  Each element carries the BITS that the reference's serial loop produces when it is run per level on the RoIs of that
 * level in ascending index: the terms  top * w / count  in float32 (one rounding per operation, nothing contracted), added to the
 * element in the loop's order n, ph, pw, iy, ix, taps 1-4 -- the collapsed taps at the last row / column, where two taps of a
 * sample land on one pixel, included.  No atomics: every element is summed by ONE thread in that order, so the same inputs give
 * the same bits on every run, eagerly and under graph replay.  Denormal terms and sums are kept.
 * A batch index is converted as the reference converts it, truncated toward zero: every value in (-1, 1) is image 0, 1.999 is
 * image 1.  sampling_ratio <= 0, negative values included, is adaptive: ceil(roi size / pooled size) samples per bin and direction.
 * A grad_output that is not finite propagates exactly as the reference's four-tap add does: a valid sample adds all four of its
 * terms, the taps of weight zero included, so an infinite or NaN bin puts inf * 0 = NaN on the neighbouring pixels of its taps,
 * and an element whose only terms are -0.0 holds 0.f + -0.0 = +0.0.  (The payload of such a NaN is not part of the contract.)
 * Bad RoIs contribute nothing and are never used as an index (the reference has undefined behaviour for them):
 *   - a batch index that truncates to a value outside [0, batch), or is not finite,
 *   - a level outside [0, n_levels),
 *   - any non-finite coordinate; a scaled coordinate of magnitude 2^29 or more (beyond it the sample positions leave the int
 *     range the reference converts them to); with adaptive sampling a grid above DTC_GRAD_MAX_GRID in either direction (the
 *     reference's int sample count overflows from 46341 x 46341 on).
 * The result is the bits of the call without these rows.
 * The stream is the only place work goes: no host synchronisation, no allocation, no RoI value is read on the host.  Two kernel
 * nodes (the preparation pass that lists the valid RoIs of every (level, image) pair in ascending index with their geometry, then
 * the pass over the tiles of the maps).  Capturable in a hipGraph after one eager call; a replay after rois, roi_levels and
 * grad_output were rewritten in place gives the bits of an eager call on the new values.
 * Return codes, checked in this order, and on any of them nothing was launched and no byte was written:
 *   shapes     DTC_EINVAL: levels NULL, n_levels < 1, batch < 1, channels < 1, roi_cols not 4 or 5, n_rois < 0, pooled_h or
 *              pooled_w < 1, a level with height or width < 1 or a spatial_scale that is not finite
 *   limits     DTC_EUNSUPPORTED: n_levels > DTC_MAX_LEVELS, the DTC_GRAD_MAX_* above, channels > 2^23, or more than 2^31 - 1
 *              tiles of 4 x 16 elements over all levels and images
 *   pointers   DTC_EINVAL: a level's grad NULL or not 16-byte aligned; rois or grad_output NULL with n_rois > 0; rois,
 *              roi_levels or grad_output not 4-byte aligned; the workspace not 16-byte aligned
 *   workspace  DTC_EWORKSPACE: NULL, or smaller than dtc_roi_align_backward_workspace_bytes(n_levels, batch, n_rois)
 * n_rois == 0 is valid and gives all zeros.  The workspace needs no clearing and may hold anything; it belongs to ONE call in
 * flight at a time. */
int dtc_roi_align_backward(const dtc_grad_level* levels, int n_levels, int batch, int channels, const float* rois, int roi_cols,
                           const int32_t* roi_levels, int n_rois, int pooled_h, int pooled_w, int sampling_ratio,
                           const float* grad_output, void* workspace, size_t workspace_bytes, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_GRAD_HIP_H_ */
