// dtc_aug_merge_boxes (include/detectorch_aug_hip.h, entry 1): the box-head outputs of up to eight views of a batch -> one candidate
// set per image in original-image coordinates, in ONE launch.  A wave owns one output row: it finds the (view, row) the row comes
// from (UNION: a walk over the <= 8 clamped counts of the image; AVG: the same row of every view; ID: the last view's), reduces the
// row's softmax statistics when the scores are logits, and then every lane takes one class per step: decode + clip with the device
// code of the detection stage (box_decode.h), the mirror for a flipped view, one 16-byte store for the box and one 4-byte store for
// the score.  The stream is ~ 5 n_cls floats per row in and 5 n_cls out: bandwidth-bound, nothing is staged (tests/README_tta.md has
// the measured time).
// Rows at or past out_n are written as zeros by the same wave, so every output element is written exactly once and no memset node
// is needed.  The view descriptors travel by value in the kernel arguments: no device copy of the host array exists.
#include "box_decode.h"
#include "dtc_common.h"
#include "softmax_fold.h"

#include "../../../include/detectorch_aug_hip.h"

namespace dtc {

constexpr int kAugThreads = 256;
constexpr int kAugWaves = kAugThreads / 64;

struct AugMergeParams {
  dtc_aug_view v[DTC_AUG_MAX_VIEWS];
  const float* im_size;
  int T, R, n_cls, logits, score_heur, coord_heur, out_rows;
  float wx, wy, ww, wh;
  float* out_scores;
  float* out_boxes;
  int32_t* out_n;
  int32_t* out_src;
};

__device__ __forceinline__ int aug_count(const dtc_aug_view& v, int b, int R) { return v.n_rois ? min(max(v.n_rois[b], 0), R) : R; }

// the box of (view t, row r, class j) of image b in original-image coordinates
__device__ __forceinline__ float4 aug_box(const AugMergeParams& p, int t, int b, int r, int j, float im_h, float im_w) {
  const dtc_aug_view& v = p.v[t];
  const size_t row = (size_t)b * p.R + r;
  const float* roi = v.rois5 + row * 5 + 1;
  const float* d = v.bbox_pred + row * 4 * p.n_cls + 4 * j;
  const float sf = v.scale[b];
  const float x1 = fdiv(roi[0], sf), y1 = fdiv(roi[1], sf), x2 = fdiv(roi[2], sf), y2 = fdiv(roi[3], sf);
  const float4 dl = *reinterpret_cast<const float4*>(d);          // 4 n_cls floats per row: every class's deltas are 16-byte aligned
  const float dv[4] = {dl.x, dl.y, dl.z, dl.w};
  float4 bx = decode_clip<true>(x1, y1, x2, y2, dv, p.wx, p.wy, p.ww, p.wh, im_h, im_w);
  if (v.flipped) {                                                  // box_utils.flip_boxes, after the clip
    const float nx1 = (im_w - bx.z) - 1.f, nx2 = (im_w - bx.x) - 1.f;
    bx.x = nx1; bx.z = nx2;
  }
  return bx;
}

__device__ __forceinline__ float aug_score(const AugMergeParams& p, int t, int b, int r, int j, const double* st) {
  const float s = p.v[t].cls_score[((size_t)b * p.R + r) * p.n_cls + j];
  return p.logits ? DTC_SOFTMAX_PROB(s, st) : s;
}

__global__ __launch_bounds__(kAugThreads) void aug_merge_kernel(AugMergeParams p) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int o = blockIdx.x * kAugWaves + (threadIdx.x >> 6);       // the wave's output row
  if (o >= p.out_rows) return;
  const bool uni = p.score_heur == DTC_AUG_UNION;
  // the image's counts (wave-uniform: every lane reads the same <= 8 words)
  int total = 0, src_t = -1, src_r = 0, n_min = p.R, n_last = 0;
  for (int t = 0; t < p.T; t++) {
    const int n = aug_count(p.v[t], b, p.R);
    if (uni && o >= total && o < total + n) { src_t = t; src_r = o - total; }
    total += n;
    n_min = min(n_min, n);
    n_last = n;
  }
  // (AVG and ID mixed: the rows every view has, which under AVG's contract of equal counts is all of them)
  const int out_n = uni ? total : (p.score_heur == DTC_AUG_ID && p.coord_heur == DTC_AUG_ID) ? n_last : n_min;
  if (o == 0 && lane == 0) p.out_n[b] = out_n;
  const size_t orow = (size_t)b * p.out_rows + o;
  float* os = p.out_scores + orow * p.n_cls;
  float4* ob = reinterpret_cast<float4*>(p.out_boxes + orow * 4 * p.n_cls);
  if (o >= out_n) {                                                 // padding: zeros, -1
    for (int j = lane; j < p.n_cls; j += 64) { os[j] = 0.f; ob[j] = make_float4(0.f, 0.f, 0.f, 0.f); }
    if (lane == 0) p.out_src[orow] = -1;
    return;
  }
  const float im_h = p.im_size[2 * b], im_w = p.im_size[2 * b + 1];
  if (uni) {
    double st[2] = {0.0, 1.0};
    if (p.logits) {
      float m;
      softmax_row_stats(p.v[src_t].cls_score + ((size_t)b * p.R + src_r) * p.n_cls, p.n_cls, lane, m, st[1]);
      st[0] = (double)m;
    }
    for (int j = lane; j < p.n_cls; j += 64) {
      os[j] = aug_score(p, src_t, b, src_r, j, st);
      ob[j] = aug_box(p, src_t, b, src_r, j, im_h, im_w);
    }
    if (lane == 0) p.out_src[orow] = src_t * p.R + src_r;
    return;
  }
  // AVG / ID, each output by its own heuristic: the same row o of the views
  const int last = p.T - 1;
  double st[DTC_AUG_MAX_VIEWS][2];
  if (p.logits) {
#pragma unroll
    for (int t = 0; t < DTC_AUG_MAX_VIEWS; t++) {                   // (constant bounds: st stays in registers)
      if (t >= p.T || (p.score_heur != DTC_AUG_AVG && t != last)) continue;
      float m;
      softmax_row_stats(p.v[t].cls_score + ((size_t)b * p.R + o) * p.n_cls, p.n_cls, lane, m, st[t][1]);
      st[t][0] = (double)m;
    }
  }
  const float fT = (float)p.T;
  for (int j = lane; j < p.n_cls; j += 64) {
    float s;
    if (p.score_heur == DTC_AUG_AVG) {                              // np.mean(axis=0): v0 + v1 + ... in view order, one division
      s = aug_score(p, 0, b, o, j, st[0]);
#pragma unroll
      for (int t = 1; t < DTC_AUG_MAX_VIEWS; t++)
        if (t < p.T) s = s + aug_score(p, t, b, o, j, st[t]);
      s = fdiv(s, fT);
    } else {
      s = 0.f;
#pragma unroll
      for (int t = 0; t < DTC_AUG_MAX_VIEWS; t++)
        if (t == last) s = aug_score(p, t, b, o, j, st[t]);
    }
    float4 bx;
    if (p.coord_heur == DTC_AUG_AVG) {
      bx = aug_box(p, 0, b, o, j, im_h, im_w);
      for (int t = 1; t < p.T; t++) {
        const float4 q = aug_box(p, t, b, o, j, im_h, im_w);
        bx.x = bx.x + q.x; bx.y = bx.y + q.y; bx.z = bx.z + q.z; bx.w = bx.w + q.w;
      }
      bx = make_float4(fdiv(bx.x, fT), fdiv(bx.y, fT), fdiv(bx.z, fT), fdiv(bx.w, fT));
    } else {
      bx = aug_box(p, last, b, o, j, im_h, im_w);
    }
    os[j] = s;
    ob[j] = bx;
  }
  if (lane == 0) p.out_src[orow] = p.score_heur == DTC_AUG_AVG ? o : last * p.R + o;
}

}  // namespace dtc

DTC_API const char* dtc_aug_target_arch(void) { return "gfx950"; }

DTC_API int dtc_aug_merge_boxes(const dtc_aug_view* views, int n_views, const float* im_size, int batch, int max_rois, int n_cls,
                                int scores_are_logits, float wx, float wy, float ww, float wh, int score_heur, int coord_heur,
                                float* out_scores, float* out_boxes, int32_t* out_n, int32_t* out_src, dtc_stream_t stream) {
  using namespace dtc;
  // shapes and parameters
  if (n_views < 1 || batch < 1 || max_rois < 1 || n_cls < 2) return DTC_EINVAL;
  if (score_heur < DTC_AUG_UNION || score_heur > DTC_AUG_ID || coord_heur < DTC_AUG_UNION || coord_heur > DTC_AUG_ID) return DTC_EINVAL;
  if ((score_heur == DTC_AUG_UNION) != (coord_heur == DTC_AUG_UNION)) return DTC_EINVAL;     // Detectron: UNION for both or for neither
  // limits
  if (n_views > DTC_AUG_MAX_VIEWS || max_rois > DTC_AUG_MAX_ROIS || n_views * max_rois > DTC_AUG_MAX_ROWS ||
      n_cls - 1 > DTC_AUG_MAX_CLASSES || batch > DTC_AUG_MAX_BATCH)
    return DTC_EUNSUPPORTED;
  // pointers
  if (!views || !im_size || !out_scores || !out_boxes || !out_n || !out_src) return DTC_EINVAL;
  if (reinterpret_cast<uintptr_t>(out_boxes) & 15) return DTC_EINVAL;
  AugMergeParams p;
  for (int t = 0; t < n_views; t++) {
    const dtc_aug_view& v = views[t];
    if (!v.rois5 || !v.cls_score || !v.bbox_pred || !v.scale || (v.flipped != 0 && v.flipped != 1)) return DTC_EINVAL;
    if (reinterpret_cast<uintptr_t>(v.bbox_pred) & 15) return DTC_EINVAL;
    p.v[t] = v;
  }
  for (int t = n_views; t < DTC_AUG_MAX_VIEWS; t++) p.v[t] = views[0];
  p.im_size = im_size;
  p.T = n_views; p.R = max_rois; p.n_cls = n_cls; p.logits = scores_are_logits != 0;
  p.score_heur = score_heur; p.coord_heur = coord_heur;
  p.out_rows = score_heur == DTC_AUG_UNION ? n_views * max_rois : max_rois;
  p.wx = wx; p.wy = wy; p.ww = ww; p.wh = wh;
  p.out_scores = out_scores; p.out_boxes = out_boxes; p.out_n = out_n; p.out_src = out_src;
  hipLaunchKernelGGL(aug_merge_kernel, dim3((unsigned)ceil_div(p.out_rows, kAugWaves), (unsigned)batch), dim3(kAugThreads), 0,
                     static_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
