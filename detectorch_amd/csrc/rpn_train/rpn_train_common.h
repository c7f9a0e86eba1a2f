// What the RPN training kernels share: the level plan (anchor numbering of include/detectorch_rpn_hip.h), the anchor of an index,
// and the validation of a level array.
#pragma once
#include <cmath>

#include "dtc_common.h"

#include "../../../include/detectorch_rpn_hip.h"

namespace dtc {

constexpr int kRpnThreads = 256;              // one anchor per thread: the workgroup of every per-anchor kernel
constexpr int kRpnSelThreads = 1024;          // the per-image selection kernels
constexpr int kRpnMaxGt = DTC_RPN_TRAIN_MAX_GT;
constexpr int kRpnMaxLevels = DTC_RPN_TRAIN_MAX_LEVELS;
constexpr int kRpnMaxSample = DTC_RPN_TRAIN_MAX_BATCH_PER_IM;

struct RpnTrainPlan {
  int n_levels, N;
  int off[kRpnMaxLevels + 1];                 // off[l]: the image-wide index of level l's first anchor; off[n_levels] = N
  int A[kRpnMaxLevels], H[kRpnMaxLevels], W[kRpnMaxLevels];
  float stride[kRpnMaxLevels];
};
struct RpnTrainAnchors { float a[kRpnMaxLevels][DTC_RPN_TRAIN_MAX_ANCHORS_PER_CELL * 4]; };

// shapes (DTC_EINVAL), then limits (DTC_EUNSUPPORTED); `anchors` may be NULL
inline int make_rpn_train_plan(const dtc_rpn_train_level* levels, int n_levels, RpnTrainPlan* plan, RpnTrainAnchors* anchors) {
  if (!levels || n_levels < 1) return DTC_EINVAL;
  for (int l = 0; l < n_levels && l < kRpnMaxLevels; l++) {
    const dtc_rpn_train_level& s = levels[l];
    if (s.num_anchors < 1 || s.height < 1 || s.width < 1 || !std::isfinite(s.feat_stride) || s.feat_stride <= 0.f) return DTC_EINVAL;
  }
  if (n_levels > kRpnMaxLevels) return DTC_EUNSUPPORTED;
  int64_t n = 0;
  plan->n_levels = n_levels;
  for (int l = 0; l < kRpnMaxLevels; l++) {
    const bool on = l < n_levels;
    if (on && levels[l].num_anchors > DTC_RPN_TRAIN_MAX_ANCHORS_PER_CELL) return DTC_EUNSUPPORTED;
    plan->off[l] = (int)n;
    plan->A[l] = on ? levels[l].num_anchors : 0;
    plan->H[l] = on ? levels[l].height : 0;
    plan->W[l] = on ? levels[l].width : 0;
    plan->stride[l] = on ? levels[l].feat_stride : 1.f;
    if (on) n += (int64_t)levels[l].num_anchors * levels[l].height * levels[l].width;
    if (n > DTC_RPN_TRAIN_MAX_ANCHORS) return DTC_EUNSUPPORTED;
    if (anchors)
      for (int i = 0; i < DTC_RPN_TRAIN_MAX_ANCHORS_PER_CELL * 4; i++)
        anchors->a[l][i] = on && i < 4 * levels[l].num_anchors ? levels[l].anchors[i] : 0.f;
  }
  plan->off[kRpnMaxLevels] = (int)n;
  for (int l = n_levels; l <= kRpnMaxLevels; l++) plan->off[l] = (int)n;
  plan->N = (int)n;
  return DTC_OK;
}

// the level of anchor i < N
__device__ __forceinline__ int rpn_level_of(const RpnTrainPlan& P, int i) {
  int l = 0;
#pragma unroll
  for (int q = 1; q < kRpnMaxLevels; q++) l += (q < P.n_levels && i >= P.off[q]) ? 1 : 0;
  return l;
}

struct RpnCell { int l, a, h, w; };
__device__ __forceinline__ RpnCell rpn_cell_of(const RpnTrainPlan& P, int i) {
  RpnCell c;
  c.l = rpn_level_of(P, i);
  const int r = i - P.off[c.l];
  c.w = r % P.W[c.l];
  const int t = r / P.W[c.l];
  c.h = t % P.H[c.l];
  c.a = t / P.H[c.l];
  return c;
}

// generate_proposals.py:130-148 in float32: base anchor + (w, h, w, h) * feat_stride
__device__ __forceinline__ float4 rpn_anchor_box(const RpnTrainPlan& P, const RpnTrainAnchors& K, const RpnCell& c) {
  const float sx = (float)c.w * P.stride[c.l], sy = (float)c.h * P.stride[c.l];
  const float* a = K.a[c.l] + 4 * c.a;
  return make_float4(a[0] + sx, a[1] + sy, a[2] + sx, a[3] + sy);
}

}  // namespace dtc
