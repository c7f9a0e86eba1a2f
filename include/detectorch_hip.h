/*
 * detectorch_hip.h -- C ABI of libdetectorch_hip.so: the MI355X (gfx950 / CDNA4) region-proposal hot path of detectorch.
 *
 * Plain pointers and sizes only; no torch / ATen / TH types cross this boundary.  Every entry point
 *   - takes DEVICE pointers (caller-owned; nothing is allocated or freed inside),
 *   - enqueues its kernels on the given hipStream_t and returns without synchronising,
 *   - returns DTC_OK (0) or a negative DTC_E* code (no exceptions, no printf), except the one entry that keeps the
 *     reference's own 1/0 convention (launch_roi_align_forward_hip).
 * Workspace is passed in by the caller; dtc_*_workspace_bytes() say how much.
 *
 * Each entry cites the reference interface it replaces (paths relative to the detectorch tree).
 */
#ifndef DETECTORCH_HIP_H_
#define DETECTORCH_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* dtc_stream_t; /* == hipStream_t */

enum { DTC_OK = 0, DTC_EINVAL = -1, DTC_ELAUNCH = -2, DTC_EWORKSPACE = -3, DTC_EUNSUPPORTED = -4 };
enum { DTC_F32 = 0, DTC_F16 = 1, DTC_U8 = 2 /* dtc_prep_images sources only */, DTC_BF16 = 3 /* RoIAlign features / output */ };

/* Library / build identification ("gfx950"); lets the host prove the native path is the one that is loaded. */
const char* dtc_version(void);
const char* dtc_target_arch(void);

/* ---------------------------------------------------------------------------------------------------------------
 * A1  RoIAlign forward
 * --------------------------------------------------------------------------------------------------------------- */

/* Drop-in for  int launch_roi_align_forward_cuda(...)  lib/cppcuda_cffi/src/cuda/roi_align_forward_cuda_kernel.h:7-19
 * (same argument list, cudaStream_t -> hipStream_t; returns 1 on success, 0 on error like the reference's launcher,
 * roi_align_forward_cuda_kernel.cu:161-201).  bottom_data float32 NCHW contiguous [B,C,H,W]; bottom_rois float32
 * [R,5] = (batch_idx, x1, y1, x2, y2); top_data float32 [R,C,PH,PW], R = outputElements / (C*PH*PW). */
int launch_roi_align_forward_hip(const int outputElements, const float* bottom_data, const float* bottom_rois,
                                 const float spatial_scale, const int channels, const int height, const int width,
                                 const int pooled_height, const int pooled_width, const int sampling_ratio,
                                 float* top_data, dtc_stream_t stream);

/* One feature map ("level").  Strides are in ELEMENTS, so NCHW-contiguous and channels_last (NHWC) tensors of the same
 * logical shape are both accepted without a copy. */
typedef struct dtc_feat_level {
  const void* data;
  int32_t height, width;
  float spatial_scale;
  int32_t _pad;
  int64_t stride_n, stride_c, stride_h, stride_w;
} dtc_feat_level;

#define DTC_MAX_LEVELS 8

/* Multi-level RoIAlign in ONE launch: replaces the per-level Python loop + torch.cat + index_select of
 * lib/model/detector.py:263-270 and lib/model/detector.py:101-106.  rois float32 [R,roi_cols] (roi_cols 5, or 4 =
 * batch 0 like lib/cppcuda/roi_align_cpu.cpp:143-147); roi_levels int32 [R] = index into levels[] (NULL: level 0);
 * out [R,C,PH,PW] contiguous, written in roi order.  in_dtype/out_dtype: DTC_F32, DTC_F16 or DTC_BF16 (always fp32 accumulate; f16 and bf16 do not mix). */
int dtc_roi_align_forward(const dtc_feat_level* levels, int n_levels, int channels, int in_dtype, const float* rois,
                          int roi_cols, const int32_t* roi_levels, int n_rois, int pooled_h, int pooled_w,
                          int sampling_ratio, void* out, int out_dtype, dtc_stream_t stream);

/* Same, with an explicit PROCESSING order: workgroup i pools RoI roi_order[i] (int32 [R], a permutation; NULL = identity).
 * The output row of a RoI does not change.  RoIs arrive in score order (spatially random); visiting them sorted by
 * (image, level, row) makes concurrently running workgroups read the same band of the feature map, so window re-reads
 * hit the XCD's L2 instead of HBM.  dtc_fpn_collect_distribute emits such an order. */
int dtc_roi_align_forward_ordered(const dtc_feat_level* levels, int n_levels, int channels, int in_dtype,
                                  const float* rois, int roi_cols, const int32_t* roi_levels, const int32_t* roi_order,
                                  int n_rois, int pooled_h, int pooled_w, int sampling_ratio, void* out, int out_dtype,
                                  dtc_stream_t stream);

/* Same, driven by packed descriptors: roi_desc float32 [R,8] = (batch, x1, y1, x2, y2, level, output_row, 0), one row per
 * workgroup in visiting order (level < 0: padding row, its output row is zero-filled on every call).  Saves the three dependent global
 * loads (order -> level -> roi) at the head of every workgroup.
 * Kernel selection (all produce bit-identical results): sampling_ratio 2 on NCHW maps -> cluster-stationary kernel; ONE level
 * whose whole map of 8 channels fits LDS (H*W <= ~4900 pixels: the C4 heads) with any other sampling ratio -> map-stationary
 * kernel, which stages the map of an image once per run of RoIs and therefore wants the descriptors IMAGE-MAJOR (what
 * dtc_fpn_collect_distribute emits; any order is correct, every change of image re-stages the map).  The plain entries take the
 * map-stationary kernel only for 4-column RoIs (one image). */
int dtc_roi_align_forward_packed(const dtc_feat_level* levels, int n_levels, int channels, int in_dtype,
                                 const float* roi_desc, int n_rois, int pooled_h, int pooled_w, int sampling_ratio, void* out,
                                 int out_dtype, dtc_stream_t stream);

/* dtc_roi_align_forward_packed with a caller-owned workspace (dtc_roi_align_workspace_bytes(n_rois) bytes, 16-byte aligned):
 * lets the map-stationary kernel (the C4 heads) form everything about a RoI that does not depend on the channels -- scaled box,
 * bin sizes, adaptive grid, the axis samples of lib/cppcuda_cffi/src/cpp/roi_align_cpu_loop.cpp:36-95 -- ONCE per launch in a
 * preparation kernel instead of once per (RoI, 8-channel workgroup).  Same results bit for bit; configurations that do not
 * take that kernel ignore the workspace (NULL is allowed: then this IS dtc_roi_align_forward_packed).  The workspace needs no
 * clearing: every call rewrites the records it reads, whatever another call over another RoI set left there. */
size_t dtc_roi_align_workspace_bytes(int n_rois);

/* Exactness switch of the adaptive-sampling (sampling_ratio <= 0) single-level path.  SEMANTICS: one process-wide value shared by
 * every thread and stream, read by the HOST at launch time and baked into the launch: a launch captured into a hipGraph keeps the
 * mode it was captured with (toggling later does not change replays), and two threads that want different modes must serialise
 * their launches around the switch themselves.  Leave it at 1 unless the whole process opts into the approximate mode.
 * exact = 1 (default): the reference's float32 operations in the reference's order (roi_align_cpu_loop.cpp:203-216): bit-identical.
 * exact = 0: with a workspace (dtc_roi_align_forward_packed_ws) the kernel may merge the gh x gw samples x 4 taps of a bin into
 * (gh + 1) x (gw + 1) taps with separable weight sums: the same sum in exact arithmetic, <= 1e-5 away in float32 on O(1) features
 * (BASELINE.json's tolerance for pooled features is 1e-4), about a quarter faster on the C4 heads. */
void dtc_roi_align_set_exact(int exact);
int dtc_roi_align_get_exact(void);
int dtc_roi_align_forward_packed_ws(const dtc_feat_level* levels, int n_levels, int channels, int in_dtype,
                                    const float* roi_desc, int n_rois, int pooled_h, int pooled_w, int sampling_ratio, void* out,
                                    int out_dtype, void* workspace, size_t workspace_bytes, dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * A5  Hard NMS
 * --------------------------------------------------------------------------------------------------------------- */

/* Drop-in for cython_nms.nms(dets, thresh)  lib/utils_cython/cython_nms.pyx:37-87 (entry lib/utils/boxes.py:332-336).
 * dets float32 [n,5] = (x1,y1,x2,y2,score) on the device; keep_out int64 [n] receives the ASCENDING ORIGINAL indices of
 * the survivors (np.where(suppressed == 0)[0], :87), keep_count int32 [1] their number.  Order inside the greedy loop is
 * (score descending, index ascending).  n <= 16384. */
size_t dtc_nms_workspace_bytes(int n);
int dtc_nms(const float* dets, int n, float thresh, void* workspace, size_t workspace_bytes, int64_t* keep_out,
            int32_t* keep_count, dtc_stream_t stream);

/* Segmented NMS over score-SORTED boxes: one launch for all (image, level) / (image, class) segments -- replaces the
 * per-level loop of lib/model/detector.py:252 + generate_proposals.py:115-117 and the 80-iteration loop of
 * lib/utils/result_utils.py:126-143.  boxes float32 [n_seg, n_stride, 4] sorted by score descending inside each
 * segment; counts int32 [n_seg] (NULL: all n_stride valid; a NEGATIVE count marks a segment that is already reduced: its
 * keep / keep_count are left untouched).  keep int32 [n_seg, keep_stride] receives the kept
 * POSITIONS in score order, at most max_keep (>0) of them (== keep[:post_nms_top_n]); keep_count int32 [n_seg].
 * keep_stride caps the kept positions when max_keep is 0 or larger than it: at most
 * cap = max_keep > 0 ? min(max_keep, keep_stride) : keep_stride positions are written per segment, the first cap of the greedy
 * walk, and keep_count <= cap; entries of keep past keep_count are left untouched.  The workspace needs no initialisation: no
 * word of it is read before this call has written it, whatever the counts. */
size_t dtc_nms_sorted_workspace_bytes(int n_seg, int n_stride);
int dtc_nms_sorted(const float* boxes, const int32_t* counts, int n_seg, int n_stride, float thresh, int max_keep,
                   void* workspace, size_t workspace_bytes, int32_t* keep, int keep_stride, int32_t* keep_count,
                   dtc_stream_t stream);

/* Segmented (score descending, index ascending) sort -- scores.argsort()[::-1] of cython_nms.pyx:45 with the canonical
 * tie rule.  scores [n_seg, n_stride] read with element stride score_stride_elems (5 for a dets array); optional
 * gather of boxes (element stride box_stride_elems between boxes) into sorted_boxes [n_seg, n_stride, 4]. */
int dtc_segment_sort_desc(const float* scores, int score_stride_elems, const float* boxes, int box_stride_elems,
                          const int32_t* counts, int n_seg, int n_stride, int32_t* order, float* sorted_boxes,
                          float* sorted_scores, dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * A2 + A3 + A4  RPN proposals: anchors, pre-NMS top-k, decode, clip, filter -- all images, all FPN levels
 * --------------------------------------------------------------------------------------------------------------- */

#define DTC_RPN_MAX_LEVELS 8
#define DTC_RPN_MAX_ANCHORS 16

/* One RPN head output (one FPN level, or the single C4 map) for a whole batch, in the conv's native layout:
 * cls_prob float32 [B, A, H, W] (post-sigmoid, lib/model/detector.py:125), bbox_pred float32 [B, 4A, H, W].
 * anchors = the A base anchors of generate_anchors(stride=feat_stride, ...) (lib/utils/generate_anchors.py:54-65),
 * row-major [A,4]; feat_stride = 1/spatial_scale (generate_proposals.py:130). pre_nms_top_n <= 0 means "all". */
typedef struct dtc_rpn_level {
  const float* cls_prob;
  const float* bbox_pred;
  int32_t num_anchors, height, width;
  int32_t pre_nms_top_n;
  float feat_stride;
  int32_t score_is_logit;   /* 0: cls_prob holds probabilities (the reference contract).  1: it holds the PRE-sigmoid logits
                             * of detector.py:125; ranking, tie-breaking and the emitted scores are those of
                             * sigmoid(logit) evaluated in double and rounded once -- the probability map is never
                             * materialised.  Field was padding before: zero-initialised callers are unchanged. */
  float anchors[DTC_RPN_MAX_ANCHORS * 4];
} dtc_rpn_level;

/* Steps 1-5 of GenerateProposals.forward (lib/model/generate_proposals.py:31-109) for every (image, level) segment
 * s = b * n_levels + l.  Outputs, per segment, in DESCENDING score order (ties: ascending (h,w,a) index):
 *   out_boxes float32 [B*L, k_stride, 4], out_scores float32 [B*L, k_stride], out_counts int32 [B*L]
 * i.e. exactly the `dets` the reference hands to NMS at :115.  k_stride >= max_l min(pre_nms_top_n_l, N_l) (0: that max).
 * (im_h, im_w) is the network input size (:100), min_size_scaled = rpn_min_size * scaling_factor (:154).
 * The workspace must be EXCLUSIVE to one in-flight call: it holds the histograms, tickets and block counts the kernels of the call
 * hand to each other (calls on different streams need different workspaces; calls on one stream may share one). */
size_t dtc_rpn_topk_decode_workspace_bytes(const dtc_rpn_level* levels, int n_levels, int batch, int k_stride);
int dtc_rpn_topk_decode(const dtc_rpn_level* levels, int n_levels, int batch, float im_h, float im_w,
                        float min_size_scaled, void* workspace, size_t workspace_bytes, float* out_boxes,
                        float* out_scores, int32_t* out_counts, int k_stride, dtc_stream_t stream);
/* dtc_rpn_topk_decode with a size per image: im_hw is a DEVICE float32 [batch, 2] array of (h_b, w_b), read by the kernels at run
 * time (a captured hipGraph picks up sizes written in place), or NULL: every image is (im_h, im_w), exactly dtc_rpn_topk_decode.
 * Image b of a padded batch then gives what a batch-1 call on its own (h_b, w_b) blob would: at each level only the anchor cells
 * y < ceil(h_b / feat_stride), x < ceil(w_b / feat_stride) take part, the per-segment top-n is min(pre_nms_top_n, A * H_b * W_b),
 * boxes are clipped to (w_b - 1, h_b - 1) and centre-filtered against (w_b, h_b).  Ties keep the ascending (h,w,a) order (row-major
 * order survives the crop).  Sizes above (im_h, im_w) are clamped to it and the cell extent to the map; h_b <= 0 or w_b <= 0 gives
 * count 0.  The level maps, k_stride and the workspace are those of the padded batch.
 * Rows past the count (both entries): out_boxes / out_scores rows >= out_counts[s] are unspecified (they may hold a previous call's
 * values); out_counts is rewritten on every call.  Anchor cells outside an image's extent are never read for that image's output. */
int dtc_rpn_topk_decode_sized(const dtc_rpn_level* levels, int n_levels, int batch, float im_h, float im_w, const float* im_hw,
                              float min_size_scaled, void* workspace, size_t workspace_bytes, float* out_boxes,
                              float* out_scores, int32_t* out_counts, int k_stride, dtc_stream_t stream);

/* proposals[keep] / scores[keep] of generate_proposals.py:119-120 for every segment: out_boxes [n_seg, keep_stride, 4],
 * out_scores [n_seg, keep_stride] (rows >= keep_count[s] untouched: they keep whatever the buffer held). */
int dtc_gather_kept(const float* sorted_boxes, const float* sorted_scores, int n_seg, int k_stride, const int32_t* keep,
                    const int32_t* keep_count, int keep_stride, float* out_boxes, float* out_scores,
                    dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * A7  FPN collect + distribute
 * --------------------------------------------------------------------------------------------------------------- */

/* collect() + distribute() of lib/model/collect_and_distribute_fpn_rpn_proposals.py:84-128 and
 * map_rois_to_fpn_levels of lib/utils/multilevel_rois.py:41-53, one workgroup per image.
 *   in_boxes float32 [B, n_in_levels, in_stride, 4], in_scores float32 [B, n_in_levels, in_stride] (post-NMS RPN
 *   proposals per level, rows >= in_counts[b,l] ignored).  in_scores == NULL: no sort, the rows are taken in the given
 *   order (add_multilevel_rois_for_test, lib/utils/multilevel_rois.py:19-39 -- the mask branch).
 * Outputs (post_nms_top_n rows per image; rows >= n_out[b] are padding with level -1):
 *   rois5 [B,topN,5] = (b,x1,y1,x2,y2) in collected (score) order; roi_scores [B,topN] (nullable);
 *   roi_levels int32 [B,topN] = level - k_min; n_out int32 [B];
 *   rois_by_level [B,topN,4] + level_counts int32 [B,k_max-k_min+1] = the reference's per-level lists, concatenated;
 *   idx_restore int32 [B,topN] = the reference's rois_idx_restore (:127);
 *   roi_order int32 [B,topN] (nullable) = global row ids b*topN + r sorted by (level, y centre): the visiting order for
 *   dtc_roi_align_forward_ordered (a performance hint, not part of the reference's semantics);
 *   roi_desc float32 [B,topN,8] (nullable) = the same rois packed in visiting order as (batch,x1,y1,x2,y2,level,row,0) for
 *   dtc_roi_align_forward_packed.
 * inputs_sorted != 0 promises that every input list is already in descending score order (true for NMS output): the
 * lists are then merged by rank instead of sorted.
 * Limits (DTC_EUNSUPPORTED): post_nms_top_n > 16384; with scores, n_in_levels * in_stride > 16384; and, for the shapes the merge
 * kernel does not take (post_nms_top_n > 2048, in_stride > 1024, n_in_levels * in_stride > 8192, its buffers past 150 KB, or
 * unsorted lists), whatever the general kernel's 144 KB of workgroup memory less its 616 bytes of tables cannot hold:
 *   with roi_order, 16 * max(4, next_pow2(post_nms_top_n)) bytes, i.e. post_nms_top_n > 8192;
 *   with sorted lists, 8 * post_nms_top_n + 4 * n_in_levels * in_stride + 16 bytes (16384 rows of input: post_nms_top_n > 10161).
 * Rewritten on every call, whatever the previous call left: n_out, level_counts, roi_levels (all topN rows: -1 past n_out),
 * roi_order (all topN rows: a permutation of b*topN + [0, topN)) and roi_desc (all topN rows: padding rows carry level -1, so
 * RoIAlign zero-fills their output rows).  Rows >= n_out[b] of rois5, roi_scores, rois_by_level and idx_restore are unspecified. */
int dtc_fpn_collect_distribute(const float* in_boxes, const float* in_scores, const int32_t* in_counts, int batch,
                               int n_in_levels, int in_stride, int post_nms_top_n, int k_min, int k_max, float* rois5,
                               float* roi_scores, int32_t* roi_levels, int32_t* n_out, float* rois_by_level,
                               int32_t* level_counts, int32_t* idx_restore, int32_t* roi_order, float* roi_desc,
                               int inputs_sorted, dtc_stream_t stream);

/* collect + distribute straight from the NMS output: list l of image b = rows keep[(b * L + l) * keep_stride + j], j < keep_count, of the
 * score-sorted pre-NMS arrays sorted_boxes / sorted_scores [B * L, k_stride, ...] (what dtc_rpn_topk_decode and dtc_nms_sorted leave
 * behind) -- proposals[keep], scores[keep] of generate_proposals.py:119-120 read in place, i.e. dtc_gather_kept +
 * dtc_fpn_collect_distribute(inputs_sorted = 1) in one launch, the same outputs bit for bit.  2 <= n_in_levels; shapes the merge
 * kernel does not hold (post_nms_top_n > 2048, keep_stride > 1024, n_in_levels * keep_stride > 8192) return DTC_EUNSUPPORTED: use the
 * two calls. */
int dtc_fpn_collect_distribute_kept(const float* sorted_boxes, const float* sorted_scores, int k_stride, const int32_t* keep,
                                    const int32_t* keep_count, int keep_stride, int batch, int n_in_levels, int post_nms_top_n,
                                    int k_min, int k_max, float* rois5, float* roi_scores, int32_t* roi_levels, int32_t* n_out,
                                    float* rois_by_level, int32_t* level_counts, int32_t* idx_restore, int32_t* roi_order,
                                    float* roi_desc, dtc_stream_t stream);

/* Precomputed (Fast R-CNN) proposals -> the rois of dtc_fpn_collect_distribute, one call for a batch: the test-time preprocessing of
 * lib/utils/preprocess_sample.py:35-45 -- scale by im_scale (:36), remove_dup_prop (:63-70), add_multilevel_rois_for_test for FPN
 * (lib/utils/multilevel_rois.py:19-53) -- on the device.
 *   boxes float32 [B, in_stride, 4] (16-byte aligned) in original-image coordinates; counts int32 [B] (device): rows >= counts[b]
 *   may hold any bits, NaN included, and are never used; im_scale float32 [B] (the reference's Python-float scale rounded to float32:
 *   numpy multiplies a float32 array by a Python float in float32); dedup_scale 0.0625 (remove_dup_proposals=True, spatial scale
 *   1/16) or 0 (no deduplication); k_min..k_max the FPN levels (2, 5), k_min == k_max for one level (C4: every row level 0);
 *   max_out >= in_stride rows per image in every output, so nothing overflows.
 * Semantics, per image (bit for bit inside the domain below):
 *   p = boxes * im_scale (one float32 multiply per coordinate); r = rint(p * dedup_scale) in float32 (np.round: half to even);
 *   hash = r.(1e3, 1e6, 1e9, 1e12) (exact as an integer); output rows = the unique hashes in ASCENDING order, each the scaled box p
 *   of its FIRST occurrence (np.unique(hash, return_index=True): :67-68, -0. kept).  dedup_scale 0: every row, in input order.
 *   Then exactly what dtc_fpn_collect_distribute(rows, in_scores = NULL, ...) writes for them: rois5, roi_levels, n_out,
 *   rois_by_level + level_counts (the reference's per-level blobs, concatenated), idx_restore (rois_idx_restore_int32), roi_order and
 *   roi_desc (the visiting order for dtc_roi_align_forward_packed[_ws]), with its rules for rows past n_out.
 *   src_index int32 [B, max_out] (nullable): np.unique's `index` of each output row (the input row it came from).
 * Domain: finite |p * dedup_scale| < 8192 (|p| < 131 072 px at 1/16), where the reference's float64 dot product is exact.  Finite rows
 * outside it have r clamped to +-8192 (deterministic, may merge rows the reference keeps apart); a row with a non-finite scaled
 * coordinate is dropped (it is neither hashed nor emitted; n_out counts the rows that remain).
 * Rewritten on every call: n_out, level_counts, roi_levels / roi_order / roi_desc on all max_out rows (as dtc_fpn_collect_distribute);
 * rows >= n_out[b] of rois5, rois_by_level, idx_restore and src_index are unspecified.
 * in_stride <= 2048 (DTC_EUNSUPPORTED beyond).  Two launches on `stream` (the deduplication, then dtc_fpn_collect_distribute), no
 * memset: graph-capturable, and a replay picks up boxes / counts / im_scale rewritten in place.  The workspace
 * (dtc_prepare_proposals_workspace_bytes, 16-byte aligned) holds the unique rows between the two launches: exclusive to one
 * in-flight call, no clearing needed. */
size_t dtc_prepare_proposals_workspace_bytes(int batch, int max_out);
int dtc_prepare_proposals(const float* boxes, const int32_t* counts, const float* im_scale, int batch, int in_stride,
                          float dedup_scale, int k_min, int k_max, int max_out, void* workspace, size_t workspace_bytes,
                          float* rois5, int32_t* roi_levels, int32_t* n_out, float* rois_by_level, int32_t* level_counts,
                          int32_t* idx_restore, int32_t* roi_order, float* roi_desc, int32_t* src_index, dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * A8  Detection post-processing
 * --------------------------------------------------------------------------------------------------------------- */

/* postprocess_output + box_results_with_nms_and_limit (hard NMS) of lib/utils/result_utils.py:76-168 for a batch.
 *   rois5 [B,R,5] (network-scale rois, column 0 ignored), n_rois int32 [B] (NULL: R), cls_score [B,R,n_cls] (softmax),
 *   bbox_pred [B,R,4*n_cls], scaling_factor float32 [B], im_size float32 [B,2] = original (h,w).
 *   (wx,wy,ww,wh) = bbox_reg_weights (10,10,5,5); score_thresh 0.05; nms_thresh 0.5; max_det 100 (0: unlimited).
 * Outputs: dets [B,max_out,6] = (x1,y1,x2,y2,score,class) ordered by class then by roi index (== np.vstack(cls_boxes),
 * :165); det_roi int32 [B,max_out] source roi; det_rois_scaled [B,max_out,4] = boxes * scaling_factor (nullable; the
 * rois of the mask branch, eval_mask_FPN.ipynb:249); det_count int32 [B] = true number (can exceed max_det on score
 * ties like the reference, :161; rows beyond max_out are dropped -- compare det_count with max_out). R <= 4096.
 * Cost model: the per-class NMS of a (class, image) segment runs inside ONE workgroup, n^2 / 2 pair tests for n candidates above the
 * score threshold -- microseconds for the 81-class heads this serves (tens of candidates per class), ~100 us at n = 1000, ~1.5 ms at
 * n = 4096: few-class models with low thresholds should expect the largest class segment to set the launch time.
 * Input rows r in [n_rois[b], R) of cls_score / bbox_pred must be addressable (the candidate scan loads them before it knows the
 * count) and may hold any bits, NaN included: they never reach an output.  Outputs: det_count is rewritten on every call; rows
 * d >= min(det_count[b], max_out) of dets / det_roi / det_rois_scaled are unspecified (they may hold a previous call's rows).
 * The same holds for every detection entry below. */
size_t dtc_postprocess_detections_workspace_bytes(int batch, int max_rois, int n_cls);
int dtc_postprocess_detections(const float* rois5, const int32_t* n_rois, const float* cls_score, const float* bbox_pred,
                               const float* scaling_factor, const float* im_size, int batch, int max_rois, int n_cls,
                               float wx, float wy, float ww, float wh, float score_thresh, float nms_thresh, int max_det,
                               void* workspace, size_t workspace_bytes, float* dets, int32_t* det_roi,
                               float* det_rois_scaled, int32_t* det_count, int max_out, dtc_stream_t stream);

/* Same with the box head's softmax folded in (lib/model/detector.py:281 F.softmax(cls_score) -> result_utils.py:76-94):
 * cls_logits [B,R,n_cls] is the raw output of the cls_score layer.  One wave per roi reduces (max, sum exp) -- 16 bytes per
 * roi in the workspace -- and the probability of a (roi, class) is formed where the class column is scanned:
 * float(exp(double(l) - max) / sum), rounded once (rel 1e-6 of torch's float32 softmax).  The [R,n_cls] probability
 * map is never written.  Everything else as dtc_postprocess_detections; same workspace size. */
int dtc_postprocess_detections_logits(const float* rois5, const int32_t* n_rois, const float* cls_logits,
                                      const float* bbox_pred, const float* scaling_factor, const float* im_size, int batch,
                                      int max_rois, int n_cls, float wx, float wy, float ww, float wh, float score_thresh,
                                      float nms_thresh, int max_det, void* workspace, size_t workspace_bytes, float* dets,
                                      int32_t* det_roi, float* det_rois_scaled, int32_t* det_count, int max_out,
                                      dtc_stream_t stream);

/* dtc_postprocess_detections[_logits] that ALSO emits the FPN level mapping of the detection rows for the mask branch
 * (add_multilevel_rois_for_test, lib/utils/multilevel_rois.py:19-39; call site eval_mask_FPN.ipynb:249) -- what a following
 * dtc_fpn_collect_distribute(det_rois_scaled, in_scores = NULL, det_count, batch, 1, max_out, max_out, k_min, k_max, ...) would
 * write, bit for bit, without that launch (the workgroup that finalises an image's detections has its <= ~100 rows in hand).
 * All of fpn's pointers are [B, max_out, ...] buffers as documented at dtc_fpn_collect_distribute (roi_order / roi_desc nullable);
 * det_rois_scaled is required; max_out <= 512 (DTC_EUNSUPPORTED beyond: use the separate call).  The fpn outputs are rewritten as
 * dtc_fpn_collect_distribute's: n_out = min(det_count, max_out), roi_levels -1 on every row past it, roi_desc padding rows level -1. */
typedef struct dtc_fpn_map_out {
  float* rois5; int32_t* roi_levels; int32_t* n_out; float* rois_by_level; int32_t* level_counts; int32_t* idx_restore;
  int32_t* roi_order; float* roi_desc;
  int32_t k_min, k_max;
} dtc_fpn_map_out;
int dtc_postprocess_detections_fpn(const float* rois5, const int32_t* n_rois, const float* cls_score, int scores_are_logits,
                                   const float* bbox_pred, const float* scaling_factor, const float* im_size, int batch,
                                   int max_rois, int n_cls, float wx, float wy, float ww, float wh, float score_thresh,
                                   float nms_thresh, int max_det, void* workspace, size_t workspace_bytes, float* dets,
                                   int32_t* det_roi, float* det_rois_scaled, int32_t* det_count, int max_out,
                                   const dtc_fpn_map_out* fpn, dtc_stream_t stream);

/* box_results_with_nms_and_limit (hard NMS) of lib/utils/result_utils.py:96-168 on ALREADY decoded + clipped boxes, for a
 * batch, in one pass on the device (the reference: 80 Python iterations, each a host NMS call):
 *   scores [B,R,n_cls], boxes [B,R,4*n_cls] (class j in columns 4j..4j+3), n_rois int32 [B] (NULL: R).
 * Per class j >= 1: score > score_thresh (:127), NMS at nms_thresh (:142); if more than max_det survive in total, those
 * with score >= the max_det-th largest (:159-163; max_det 0: unlimited).  Outputs as dtc_postprocess_detections (dets
 * [B,max_out,6] ordered by class then by row, det_roi = source row, det_count = true number).  Same workspace size. */
int dtc_box_results_nms_limit(const float* scores, const float* boxes, const int32_t* n_rois, int batch, int max_rois,
                              int n_cls, float score_thresh, float nms_thresh, int max_det, void* workspace,
                              size_t workspace_bytes, float* dets, int32_t* det_roi, int32_t* det_count, int max_out,
                              dtc_stream_t stream);

/* The reference's two optional test-time branches of box_results_with_nms_and_limit (lib/utils/result_utils.py:96-168),
 * Detectron's TEST.SOFT_NMS and TEST.BBOX_VOTE, on the batched device path.
 *   nms_method         0: cython_nms.nms (hard NMS, the other entries' behaviour); Soft-NMS (cython_nms.soft_nms,
 *                      :133-140): 1 linear, 2 gaussian, 3 hard.  Nt = nms_thresh.
 *   soft_sigma         gaussian sigma (0.5, :101); must be > 0 with method 2.
 *   soft_score_thresh  score floor of the Soft-NMS walk (0.0001, :138): a row decayed below it is discarded.
 *   bbox_vote          0/1: box_voting(nms_dets, dets_j, bbox_vote_thresh, 'ID') (:145-151); bbox_vote_thresh in (0, 1] (0.8).
 * Semantics: Soft-NMS works on dets_j in candidate order (roi ascending, :127-132); its rows of a class come out in selection
 * order with their DECAYED scores, which the max_det limit (:154-163, ties kept) uses.  Voting refines the post-NMS rows against
 * ALL of the class's candidates (undecayed weights); 'ID' scoring leaves the score.  Hard NMS keeps the roi-ascending order. */
typedef struct dtc_det_options {
  int32_t nms_method;
  float soft_sigma;
  float soft_score_thresh;
  int32_t bbox_vote;
  float bbox_vote_thresh;
} dtc_det_options;

/* Workspace of dtc_postprocess_detections_ex; opt == NULL (or hard NMS without voting): == dtc_postprocess_detections_workspace_bytes.
 * 0 for invalid arguments. */
size_t dtc_postprocess_detections_ex_workspace_bytes(int batch, int max_rois, int n_cls, const dtc_det_options* opt);

/* One entry for every form of the batched detection post-processing, with the options above:
 *   probabilities or logits (scores_are_logits, as dtc_postprocess_detections[_logits]); decoded_boxes [B,R,4*n_cls] already
 *   decoded + clipped boxes (as dtc_box_results_nms_limit: rois5 / bbox_pred / scaling_factor / im_size unused, det_rois_scaled
 *   must be NULL) or NULL (decode from rois5 + bbox_pred); fpn: the fused mask-branch mapping of dtc_postprocess_detections_fpn,
 *   or NULL.  opt == NULL, or nms_method 0 without voting: bit-identical to those entries (same launches).
 * Outputs as dtc_postprocess_detections; with Soft-NMS the rows of a class are in selection order and carry the decayed score;
 * with voting dets[:, :4] and det_rois_scaled hold the voted boxes, and the fpn mapping is computed from them.
 * DTC_EINVAL: an unknown nms_method, soft_sigma <= 0 with gaussian, bbox_vote not 0/1, bbox_vote_thresh outside (0, 1], and the
 * argument errors of the other entries.  R <= 4096 (DTC_EUNSUPPORTED beyond), n_cls - 1 <= 256.
 * Launches (fixed per option set, graph-capturable): the hard path's, + one per Soft-NMS (one wave per class and image: the
 * reference's sequential walk, O(n^2) in the class's candidates), + one for voting (one wave per emitted row), + one more with
 * voting AND fpn (the mapping of the voted boxes). */
int dtc_postprocess_detections_ex(const float* rois5, const int32_t* n_rois, const float* cls_score, int scores_are_logits,
                                  const float* bbox_pred, const float* decoded_boxes, const float* scaling_factor,
                                  const float* im_size, int batch, int max_rois, int n_cls, float wx, float wy, float ww,
                                  float wh, float score_thresh, float nms_thresh, int max_det, const dtc_det_options* opt,
                                  void* workspace, size_t workspace_bytes, float* dets, int32_t* det_roi,
                                  float* det_rois_scaled, int32_t* det_count, int max_out, const dtc_fpn_map_out* fpn,
                                  dtc_stream_t stream);

/* Scoring of the bbox vote (box_voting's scoring_method and beta, lib/utils/boxes.py:280-329; Detectron's
 * TEST.BBOX_VOTE.SCORING_METHOD / SCORING_METHOD_BETA).  'ID' keeps the score; every other method rewrites it from the scores of
 * the voters (the candidates of the row's class whose IoU with the row's box is >= bbox_vote_thresh, weighted as for the box):
 *   TEMP_AVG (mean of the temperature-smoothed two-way probabilities), AVG (mean), IOU_AVG (IoU-weighted mean),
 *   GENERALIZED_AVG (power mean, exponent beta), QUASI_SUM (sum / n^beta).  beta > 0 and finite (the reference's 1.0); taken
 *   as float32.  Numerics: numpy's float32 evaluation order (pairwise sums); ID, AVG, IOU_AVG, QUASI_SUM and GENERALIZED_AVG at
 *   beta 1 bit-exact; TEMP_AVG and GENERALIZED_AVG at beta != 1 evaluate log / exp / pow in double and round (numpy's float32
 *   routines differ by a few ulp): within 1e-6 relative. */
enum { DTC_VOTE_ID = 0, DTC_VOTE_TEMP_AVG, DTC_VOTE_AVG, DTC_VOTE_IOU_AVG, DTC_VOTE_GENERALIZED_AVG, DTC_VOTE_QUASI_SUM };
typedef struct dtc_vote_scoring {
  int32_t method;
  float beta;
} dtc_vote_scoring;

/* Workspace of dtc_postprocess_detections_ex2; scoring == NULL or DTC_VOTE_ID: == dtc_postprocess_detections_ex_workspace_bytes.
 * 0 for invalid arguments. */
size_t dtc_postprocess_detections_ex2_workspace_bytes(int batch, int max_rois, int n_cls, const dtc_det_options* opt,
                                                      const dtc_vote_scoring* scoring);

/* dtc_postprocess_detections_ex with the vote's scoring.  scoring == NULL or DTC_VOTE_ID: the same launches and bits as
 * dtc_postprocess_detections_ex.  Another method needs opt->bbox_vote == 1: since the scoring rewrites the score column and the
 * reference applies the max_det limit to the VOTED scores (:145-163), every kept row of every (class, image) segment is voted
 * BEFORE the limit -- one more launch ahead of the limit (grid (n_cls - 1, B): a workgroup stages its segment's candidates in
 * LDS, one wave per kept row), which replaces the kept row's score by its voted score; the limit then ranks those.  A row with
 * no voter keeps its score (cannot happen for the reference's call: every kept row votes for itself).  Row order within a class
 * as dtc_postprocess_detections_ex (roi ascending for hard NMS, selection order for Soft-NMS, whose voted score replaces the
 * decayed one); the boxes are voted after the limit as with 'ID'.
 * DTC_EINVAL: the errors of dtc_postprocess_detections_ex, a method outside 0..5, beta <= 0 or not finite, a method other than
 * DTC_VOTE_ID without opt->bbox_vote == 1.  R <= 4096 (DTC_EUNSUPPORTED beyond), n_cls - 1 <= 256.
 * Launches (fixed per option set, graph-capturable, no host synchronisation): dtc_postprocess_detections_ex's, + one with a
 * scoring other than DTC_VOTE_ID. */
int dtc_postprocess_detections_ex2(const float* rois5, const int32_t* n_rois, const float* cls_score, int scores_are_logits,
                                   const float* bbox_pred, const float* decoded_boxes, const float* scaling_factor,
                                   const float* im_size, int batch, int max_rois, int n_cls, float wx, float wy, float ww,
                                   float wh, float score_thresh, float nms_thresh, int max_det, const dtc_det_options* opt,
                                   const dtc_vote_scoring* scoring, void* workspace, size_t workspace_bytes, float* dets,
                                   int32_t* det_roi, float* det_rois_scaled, int32_t* det_count, int max_out,
                                   const dtc_fpn_map_out* fpn, dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * A9  Mask resize + binarise (+ paste geometry)
 * --------------------------------------------------------------------------------------------------------------- */

/* The per-detection body of segm_results, lib/utils/result_utils.py:182-214 (everything but the RLE encode).
 *   masks float32 [n_masks,n_cls,M,M] (mask-head output); mask_index int32 [B,max_out] row of each detection in masks
 *   (NULL: b*max_out + d); dets [B,max_out,6] / det_count [B] as produced above; im_size [B,2] original (h,w).
 * Outputs: mask_boxes int32 [B,max_out,4] expanded+truncated ref box (:183-184); mask_rects int32 [B,max_out,4] paste
 * rectangle (x_0,y_0,x_1,y_1) (:204-207); crops uint8 [B,per_image_capacity]: for detection d the binarised resized mask
 * restricted to its paste rectangle, row-major, at byte mask_offsets[b,d] of image b's region; mask_bytes int64 [B] =
 * bytes image b needs, whatever the capacity.  mask_offsets[b,d] is the sum of the rectangle areas of the image's detections in
 * front of d.  A detection is pasted iff mask_offsets[b,d] + area <= per_image_capacity (mask_bytes[b] > per_image_capacity: some
 * were not); the others are skipped, their rows of mask_boxes / mask_rects / mask_offsets are still written, and no byte outside
 * the pasted rectangles -- of this image's region, of another image's, or behind the last region -- is written.  mask_bytes is
 * rewritten on every call; rows d >= min(det_count[b], max_out) of mask_boxes / mask_rects / mask_offsets are unspecified; the
 * crop bytes outside the pasted rectangles keep what the caller left there.  masks rows of detections d >= min(det_count[b], max_out)
 * are never read.  cls_specific_mask 0: channel 0 of the detection's mask row, whatever its class (:192-195).  im_size is
 * truncated to integers.  M + 2 <= 64 (DTC_EINVAL beyond, and for M < 1). */
int dtc_mask_paste(const float* masks, const int32_t* mask_index, int n_cls, int M, const float* dets,
                   const int32_t* det_count, const float* im_size, int batch, int max_out, float thresh_binarize,
                   int cls_specific_mask, uint8_t* crops, long long per_image_capacity, int32_t* mask_boxes,
                   int32_t* mask_rects, long long* mask_offsets, long long* mask_bytes, dtc_stream_t stream);

/* COCO RLE of every pasted mask, on the device: what `mask_util.encode(np.array(im_mask[:, :, np.newaxis], order='F'))`
 * returns at lib/utils/result_utils.py:217-220 (pycocotools rleEncode + rleToString), computed from dtc_mask_paste's
 * crops / mask_rects / mask_offsets without materialising the (im_h, im_w) frame.  Per detection (b, d):
 *   rle_counts uint32 [B,max_out,runs_stride]  run lengths (column-major, first run = zeros), rle_n_runs int32 [B,max_out]
 *   rle_str    uint8  [B,max_out,str_stride]   the compressed "counts" string (ASCII, no terminator), rle_str_len int32
 * A detection whose runs do not fit runs_stride gets rle_n_runs = -(runs needed) and rle_str_len = -1 (the string is not formed,
 * so its length is not known: 7 bytes per run always suffice), and no valid data.  One whose runs fit and whose string does not
 * fit str_stride gets rle_n_runs = runs (> 0, rle_counts valid) and rle_str_len = -(bytes needed).  Either way: re-run with
 * larger strides or encode that one on the host.  A detection with mask_offsets[b,d] + area > per_image_capacity
 * (dtc_mask_paste skipped it) gets -1 / -1; a zero-area rectangle therefore gets -1 / -1 when its offset is above the capacity
 * and, like every empty rectangle that fits, one run of im_h * im_w zeros when its offset is at most the capacity.
 * d >= det_count[b]: 0 / 0, rewritten on every call.  Nothing is written past a row's runs_stride / str_stride, or to the rows
 * d >= det_count[b] of rle_counts / rle_str; rle_counts / rle_str past each row's length are unspecified. */
int dtc_mask_rle(const uint8_t* crops, long long per_image_capacity, const int32_t* mask_rects,
                 const long long* mask_offsets, const int32_t* det_count, const float* im_size, int batch, int max_out,
                 uint32_t* rle_counts, int runs_stride, int32_t* rle_n_runs, uint8_t* rle_str, int str_stride,
                 int32_t* rle_str_len, dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * (f)-4  bbox_overlaps / box_voting (the optional bbox-vote branch of the detection post-processing)
 * --------------------------------------------------------------------------------------------------------------- */

/* Drop-in for cython_bbox.bbox_overlaps(boxes, query_boxes)  lib/utils_cython/cython_bbox.pyx:32-72:
 * boxes float32 [n, box_cols>=4], query_boxes [k, query_cols>=4] (first four columns x1,y1,x2,y2) -> overlaps [n,k]. */
int dtc_bbox_overlaps(const float* boxes, int n, int box_cols, const float* query_boxes, int k, int query_cols,
                      float* overlaps, dtc_stream_t stream);

/* box_voting(top_dets, all_dets, thresh, scoring_method='ID')  lib/utils/boxes.py:280-329: top_dets [n_top,5],
 * all_dets [n_all,5] (x1,y1,x2,y2,score), n_all <= 8192 -> top_dets_out [n_top,5] with the boxes replaced by the
 * score-weighted average of the all_dets whose IoU with the top det is >= thresh (numpy's float32 evaluation order);
 * n_voters int32 [n_top] (optional) = number of voters (0: row copied unchanged; cannot happen for the reference's
 * call, where every top det is one of all_dets). */
int dtc_box_voting(const float* top_dets, int n_top, const float* all_dets, int n_all, float thresh,
                   float* top_dets_out, int32_t* n_voters, dtc_stream_t stream);

/* box_voting(top_dets, all_dets, thresh, scoring_method, beta): dtc_box_voting, and with a scoring other than DTC_VOTE_ID
 * (dtc_vote_scoring above) column 4 of top_dets_out holds the voted score (the top det's own score when nobody votes: the
 * reference raises ZeroDivisionError there, n_voters reports it).  scoring == NULL or DTC_VOTE_ID: dtc_box_voting itself.
 * One launch, one wave per top det; n_all <= 8192 (DTC_EUNSUPPORTED beyond).  DTC_EINVAL: the errors of dtc_box_voting, a
 * method outside 0..5, beta <= 0 or not finite. */
int dtc_box_voting_scored(const float* top_dets, int n_top, const float* all_dets, int n_all, float thresh,
                          const dtc_vote_scoring* scoring, float* top_dets_out, int32_t* n_voters, dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * OUTSIDE SURVEY section 8 (the region-proposal hot path): convolution epilogue of the backbone's inference form.
 * SURVEY 2 row 7 marks the backbone out of scope; this entry exists because detector.optimize_for_inference (round 3)
 * uses it.  It is frozen: no parity / roofline claim of this library rests on it, and a binding of the hot path does
 * not need it.
 * --------------------------------------------------------------------------------------------------------------- */

/* x [n,c,h,w] (dense NCHW, or dense channels_last when channels_last != 0; DTC_F32 / DTC_F16 / DTC_BF16), in place:
 *     x = act( x + bias[c] + residual )        float32 arithmetic, one rounding to x's type
 * bias float32 [c] or NULL; residual NULL, or a tensor of x's type and layout -- [n,c,h,w], or [n,c,h/2,w/2] read with
 * nearest-neighbour x2 upsampling when residual_up2 != 0 (h, w even); relu != 0: act = max(., 0) (NaN propagates).
 * One pass replaces what the reference's graph runs as separate ops after a convolution: the eval-mode BatchNorm /
 * AffineChannel of the ResNet body (detector.py:231; its scale folded into the weights, its shift = bias) + ReLU, the
 * bottleneck's `+ identity`, the FPN top-down `upsample(top) + lateral` (detector.py:45-46), the heads' bias + ReLU. */
int dtc_bias_act(void* x, const float* bias, const void* residual, int n, int c, int h, int w, int dtype,
                 int channels_last, int relu, int residual_up2, dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * (f)-3  Network-input preparation: prep_im_for_blob + im_list_to_blob  (lib/utils/blob.py:62-87, :27-59)
 * --------------------------------------------------------------------------------------------------------------- */

/* One source image: interleaved HWC, 3 channels in BGR order (as cv2.imread delivers), DTC_U8 or DTC_F32, on the device;
 * row_stride in elements (>= 3 * width). */
typedef struct dtc_image {
  const void* data;
  int32_t height, width, dtype, row_stride;
} dtc_image;

/* Host-side plan (no GPU work): per image the scale of blob.py:75-82 (target_size on the short side, capped so that the
 * long side stays <= max_size), the resized (h, w) cv2.resize(fx=fy=scale) produces, and the blob (H, W) of
 * im_list_to_blob: max over the batch, rounded up to pad_stride when pad_stride > 1 (fpn_on, :41-44).
 * im_scales double [batch], out_hw int32 [batch,2], blob_hw int32 [2] -- all host memory. */
int dtc_prep_plan(const int32_t* heights, const int32_t* widths, int batch, int target_size, int max_size, int pad_stride,
                  double* im_scales, int32_t* out_hw, int32_t* blob_hw);

/* blob float32 [batch,3,blob_h,blob_w] (device) = for every image: (image - pixel_means) resized bilinearly by
 * im_scales[b] to out_hw[b], zero padded, channels first.  images / pixel_means (3 doubles, BGR) / im_scales / out_hw are
 * HOST arrays (the plan above); batch <= 32 per call. */
int dtc_prep_images(const dtc_image* images, int batch, const double* pixel_means, const double* im_scales,
                    const int32_t* out_hw, float* blob, int blob_h, int blob_w, dtc_stream_t stream);

/* ---------------------------------------------------------------------------------------------------------------
 * A6  Soft-NMS  and  A4 (numpy flavour) box decode
 * --------------------------------------------------------------------------------------------------------------- */

/* Drop-in for cython_nms.soft_nms(boxes_in, sigma, Nt, threshold, method)  lib/utils_cython/cython_nms.pyx:98-203 (entry
 * lib/utils/boxes.py:339-356; method 0 hard / 1 linear / 2 gaussian).  dets float32 [n,5] on the device (not modified);
 * dets_out [n,5] and inds_out int64 [n] receive the N' surviving rows in SELECTION order, n_out int32 [1] = N'. n <= 6000.
 * Equal scores: the first maximum in row order is picked (:128-132).  NaN scores behave as in the reference's
 * `maxscore < boxes[pos, 4]` scan: the i-th pick is row i itself when its score is NaN, otherwise the first maximum of the
 * non-NaN scores; a NaN score is never below score_thresh, so such rows survive, with the NaN in dets_out. */
int dtc_soft_nms(const float* dets, int n, float sigma, float overlap_thresh, float score_thresh, int method,
                 float* dets_out, int64_t* inds_out, int32_t* n_out, dtc_stream_t stream);

/* bbox_transform (lib/utils/boxes.py:168-208) optionally followed by clip_tiled_boxes (:150-165): boxes [n,4],
 * deltas [n,4*n_cls] -> out [n,4*n_cls]. */
int dtc_bbox_transform(const float* boxes, const float* deltas, int n, int n_cls, float wx, float wy, float ww, float wh,
                       int do_clip, float im_h, float im_w, float* out, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_HIP_H_ */
