/*
 * detectorch_aug_hip.h -- C ABI of libdetectorch_aug_hip.so: test-time augmentation on the batched path of the MI355X (gfx950 /
 * CDNA4).  The box-head outputs of several VIEWS of the same images -- mirrored and / or rescaled network inputs -- are merged into
 * one candidate set per image in original-image coordinates (entry 1), which dtc_postprocess_detections_ex2 takes through
 * decoded_boxes; the mask-head probabilities the views give for the final detections are combined into one map per detection (entry
 * 2), which dtc_mask_paste takes.  The reference has no test-time augmentation: the rule is the one of Detectron's core/test.py
 * (im_detect_bbox_aug, im_detect_bbox_hflip, im_detect_bbox_scale, im_detect_mask_aug and its flipped and scaled forms), restated in
 * tests/tta_ref.py; parity with Detectron itself is unpinned.
 * A thirteenth shared library next to libdetectorch_hip.so and the eleven other side libraries, whose export lists are pinned and do
 * not grow; no other library exports a name that starts with dtc_aug_.  The conventions are those of detectorch_mpost_hip.h:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside.  The two arrays that DESCRIBE the views (dtc_aug_view[],
 *     the pointer and flag arrays of entry 2) are HOST memory, read during the call only: their contents travel as kernel arguments,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers; a call that returns DTC_EINVAL or DTC_EUNSUPPORTED has enqueued nothing and written
 *     nothing; DTC_ELAUNCH is the runtime refusing a launch.  No entry takes a workspace, so none returns DTC_EWORKSPACE,
 *   - every entry is ONE kernel node and can be captured in a hipGraph after one eager call; a replay picks up inputs rewritten in
 *     place (heuristics, weights, flip flags and the views' pointers are baked into the captured kernel arguments),
 *   - EVERY output element is written exactly once on every call, the rows past a count included (zeros, -1 in out_src),
 *   - no count, class or coordinate read from the device is used as an address: counts are clamped to their strides, a class outside
 *     [0, K) selects nothing,
 *   - no atomics; float32 sums are taken in view order: the same bits on every run.
 */
#ifndef DETECTORCH_AUG_HIP_H_
#define DETECTORCH_AUG_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0. Build identification of the augmentation library ("gfx950"). */
const char* dtc_aug_target_arch(void);

#define DTC_AUG_MAX_VIEWS 8              /* T */
#define DTC_AUG_MAX_ROIS 4096            /* R, rows per view and image */
#define DTC_AUG_MAX_ROWS 32768           /* T R */
#define DTC_AUG_MAX_CLASSES 256          /* n_cls - 1 */
#define DTC_AUG_MAX_BATCH 65535          /* B */
#define DTC_AUG_MAX_MASK 64              /* M */
#define DTC_AUG_MAX_CHANNELS 1024        /* K */
#define DTC_AUG_MAX_MASK_ROWS (1 << 20)  /* B max_out */

#define DTC_AUG_UNION 0                  /* score_heur / coord_heur of dtc_aug_merge_boxes */
#define DTC_AUG_AVG 1
#define DTC_AUG_ID 2
#define DTC_AUG_SOFT_AVG 0               /* heur of dtc_aug_combine_masks */
#define DTC_AUG_SOFT_MAX 1
#define DTC_AUG_LOGIT_AVG 2

/* One view of the batch: the inputs dtc_postprocess_detections_ex2 would take for it.  rois5 float32 [B, R, 5] (batch index, x1,
 * y1, x2, y2) in the view's own scaled -- and, for a flipped view, mirrored -- coordinates; n_rois int32 [B] (clamped to [0, R]) or
 * NULL (all R rows); cls_score float32 [B, R, n_cls]; bbox_pred float32 [B, R, 4 n_cls]; scale float32 [B], the view's image scale
 * of each image; flipped: 0, or 1 for a mirrored view. */
typedef struct dtc_aug_view {
  const float* rois5;
  const int32_t* n_rois;
  const float* cls_score;
  const float* bbox_pred;
  const float* scale;
  int32_t flipped;
  int32_t _pad;
} dtc_aug_view;

/* 1. im_detect_bbox_aug's merge.  views: n_views = T descriptors (host); im_size float32 [B, 2] = the ORIGINAL (h, w); batch = B,
 * max_rois = R, n_cls; scores_are_logits: 0, or 1 when every view's cls_score holds the classifier's raw output; (wx, wy, ww, wh) =
 * bbox_reg_weights; score_heur, coord_heur.
 * Per view, row and class j (the background class 0 included, as bbox_transform decodes it):
 *   box = the view's rois5[r, 1:5] / scale[b] decoded with bbox_pred[r, 4 j : 4 j + 4] and clipped to im_size[b] -- the device code
 *   of dtc_postprocess_detections (csrc/box_decode.h: IEEE division, one float32 rounding per operation, exp evaluated in double and
 *   rounded once, fminf / fmaxf clip), shared with it and not restated;
 *   a flipped view then mirrors it:  x1' = (w - x2) - 1,  x2' = (w - x1) - 1  in float32, in that order, w = im_size[b, 1]
 *   (box_utils.flip_boxes after the clip, as im_detect_bbox_hflip has it);
 *   score = cls_score[r, j], or with scores_are_logits the softmax dtc_postprocess_detections_ex2 folds in: (float)(exp((double)l_j -
 *   max) / sum), the sum over j of exp((double)l_j - max) taken by slot j % 64 in increasing j and a 64 -> 1 halving tree
 *   (csrc/softmax_fold.h, shared with detections.hip).  Scores always come out as probabilities.
 * Outputs, with out_rows = T R under DTC_AUG_UNION and R otherwise: out_scores float32 [B, out_rows, n_cls]; out_boxes float32
 * [B, out_rows, 4 n_cls] (16-byte aligned); out_n int32 [B]; out_src int32 [B, out_rows].
 *   DTC_AUG_UNION (np.vstack): image b's rows are view 0's first n_rois rows, then view 1's, and so on, compacted; out_n[b] their
 *     total; out_src = view R + row.
 *   DTC_AUG_AVG: the views' rows are aligned, which needs equal n_rois[b] in every view (the caller's to keep; out_n[b] is the
 *     smallest); out = (v_0 + v_1 + ... + v_{T-1}) / (float)T, added in view order in float32, one IEEE division: np.mean(axis=0) of
 *     the stacked float32 arrays; out_src = row.
 *   DTC_AUG_ID: the last view's rows alone; out_n[b] = its n_rois; out_src = (T - 1) R + row.
 *   Rows at or past out_n[b]: +0.0 in out_scores and out_boxes, -1 in out_src.
 * Detectron allows separate heuristics for scores and coordinates but requires UNION for both or for neither: a pair of which
 * exactly one is DTC_AUG_UNION is DTC_EINVAL, as is a value outside 0 .. 2.  A pair of AVG and ID applies each to its own output.
 * Limits: 1 <= T <= 8, 1 <= R <= 4096, T R <= 32768, 2 <= n_cls <= 257, 1 <= B <= 65535: DTC_EUNSUPPORTED beyond, DTC_EINVAL below.
 * One kernel node, one wave per output row: the row's softmax statistics by a wave reduction, then one (box, score) per lane and
 * class step, the box stored as 16 bytes. */
int dtc_aug_merge_boxes(const dtc_aug_view* views, int n_views, const float* im_size, int batch, int max_rois, int n_cls,
                        int scores_are_logits, float wx, float wy, float ww, float wh, int score_heur, int coord_heur,
                        float* out_scores, float* out_boxes, int32_t* out_n, int32_t* out_src, dtc_stream_t stream);

/* 2. im_detect_mask_aug's combination.  masks: n_views = T device pointers (a host array), each float32 [B max_out, K, M, M]
 * probabilities of the SAME detections seen in view t, 16-byte aligned; flipped: T flags (a host array), 1 where the view's maps
 * are read mirrored along the last axis (masks_hf[:, :, :, ::-1]); det_count int32 [B] (clamped to [0, max_out]); mask_class int32
 * [B max_out] or NULL; heur.  Output: out float32 [B max_out, K, M, M], 16-byte aligned, no overlap with an input (DTC_EINVAL).
 *   DTC_AUG_SOFT_AVG   (v_0 + ... + v_{T-1}) / (float)T, float32, view order, one IEEE division (np.mean(axis=0))
 *   DTC_AUG_SOFT_MAX   the elementwise maximum (np.amax(axis=0): a NaN stays)
 *   DTC_AUG_LOGIT_AVG  l_t = -log((1 - y_t) / max(y_t, 1e-20)) with the subtraction, the maximum and the division in float32 and the
 *                      log evaluated in double and rounded once; m = the SOFT_AVG rule on l_t; out = 1 / (1 + exp(-m)), the exp
 *                      evaluated in double and rounded once, the sum and the division in float32.  y = 1 has the logit +inf and
 *                      gives exactly 1; no input in [0, 1] gives a NaN.
 * Every element of out is written exactly once.  Row r of image b with r >= det_count[b]: +0.0.  With mask_class, only channel
 * mask_class[b max_out + r] of a row is combined and its other channels are +0.0 (dtc_mask_paste with cls_specific_mask reads no
 * other; K times less traffic); a class outside [0, K) leaves the row +0.0.  With NULL every channel is combined.
 * Limits: 1 <= T <= 8, 1 <= M <= 64, 1 <= K <= 1024, 1 <= B <= 65535, 1 <= B max_out <= 2^20, and B max_out K M M < 2^39 elements (a
 * grid of one thread per element): DTC_EUNSUPPORTED beyond, DTC_EINVAL below.
 * One kernel node: a thread per four output elements with 16-byte loads and one 16-byte store where M is a multiple of 4 (a
 * mirrored group of four lies in the same row and is as aligned as the group itself), a thread per element otherwise. */
int dtc_aug_combine_masks(const float* const* masks, const int32_t* flipped, int n_views, const int32_t* det_count,
                          const int32_t* mask_class, int batch, int max_out, int n_cls, int M, int heur, float* out,
                          dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_AUG_HIP_H_ */
