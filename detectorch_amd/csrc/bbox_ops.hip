// The stand-alone box_utils drop-ins: bbox_overlaps and box_voting -- the IoU primitive and the optional bbox-vote refinement of
// the detection post-processing -- and bbox_transform + clip_tiled_boxes for all classes.  Reference:
// lib/utils_cython/cython_bbox.pyx:32-72 (bbox_overlaps), lib/utils/boxes.py:280-329 (box_voting, called from
// box_results_with_nms_and_limit, lib/utils/result_utils.py:147-153 when do_bbox_vote is set), :168-208 and :150-165 (the decode).
//
// Numerics (oracle/oracle.c:orc_bbox_overlaps has the derivation, pinned against the reference's own Cython build): every
// `a - b + 1` is (double)(a - b) + 1.0 -- the subtraction in float32, the +1 and span products in double -- rounded to float32
// where the reference stores into a DTYPE_t variable; iw*ih is a float32 product; the division is IEEE float32.
// box_voting reproduces numpy's evaluation order: the weighted coordinate sums add the voters in index order (axis-0
// reduction of the [m,4] product), the weight sum is numpy's pairwise float32 summation.
#include "box_decode.h"
#include "box_vote.h"
#include "dtc_common.h"

namespace dtc {

// span1 / iou_bbox / np_sum_f32 / box_vote_one: box_vote.h

__global__ __launch_bounds__(256) void bbox_overlaps_kernel(const float* __restrict__ boxes, int n, int box_stride,
                                                            const float* __restrict__ query, int k, int query_stride,
                                                            float* __restrict__ out, int vec_ok) {
  // thread <-> (row i, 4 consecutive queries): coalesced 16-byte stores of the row-major [n, k] matrix
  const long long total = (long long)n * ((k + 3) / 4);
  const int kq = (k + 3) / 4;
  for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long long)gridDim.x * blockDim.x) {
    const int i = (int)(t / kq), q0 = (int)(t - (long long)i * kq) * 4;
    const float* bp = boxes + (size_t)i * box_stride;
    const float4 B = make_float4(bp[0], bp[1], bp[2], bp[3]);
    float r[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int q = min(q0 + u, k - 1);
      const float* qp = query + (size_t)q * query_stride;
      r[u] = iou_bbox(B, make_float4(qp[0], qp[1], qp[2], qp[3]));
    }
    float* o = out + (size_t)i * k + q0;
    if (vec_ok) *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
    else
      for (int u = 0; u < 4 && q0 + u < k; u++) o[u] = r[u];
  }
}

constexpr int kVoteMax = 8192;     // all_dets per call (LDS voter list: 32 KB)

// one wave per top det.  kScored: scoring_method other than 'ID' -- the box as always (box_vote_one), the score by vote_score over
// the same voters; else the score stays (method / beta unused)
template <bool kScored>
__global__ __launch_bounds__(64) void box_voting_kernel(const float* __restrict__ top, int t, const float* __restrict__ all,
                                                        int a, float thresh, int method, float beta, float* __restrict__ out,
                                                        int32_t* __restrict__ n_voters) {
  __shared__ int vl[kVoteMax];
  const int k = blockIdx.x, lane = threadIdx.x;
  const float* tp = top + (size_t)k * 5;
  const float4 B = make_float4(tp[0], tp[1], tp[2], tp[3]);
  auto box = [&](int j) { const float* ap = all + (size_t)j * 5; return make_float4(ap[0], ap[1], ap[2], ap[3]); };
  auto score = [&](int j) { return all[(size_t)j * 5 + 4]; };
  int m = 0;
  const float v = box_vote_one(
      B, lane < 4 ? tp[lane] : 0.f, a, thresh, [](int) { return true; }, box, [&](int j, int c) { return all[(size_t)j * 5 + c]; },
      score, vl, lane, &m);
  float sc = tp[4];                                                                   // 'ID', or no voter: the score stays
  if constexpr (kScored) {
    __shared__ VoteScratch vs;
    if (m > 0) {
      vote_words(B, a, thresh, [](int) { return true; }, box, vs, lane);
      sc = vote_score(method, beta, vs, (a + 63) >> 6, m, score, [&](int j) { return iou_bbox(B, box(j)); }, lane);
    }
  }
  if (lane < 4) out[(size_t)k * 5 + lane] = v;                                         // :295 np.average
  if (lane == 4) out[(size_t)k * 5 + 4] = sc;                                          // :297-323
  if (lane == 5 && n_voters) n_voters[k] = m;
}

// A4 (numpy flavour)  bbox_transform + clip_tiled_boxes for ALL classes -- lib/utils/boxes.py:168-208 and :150-165.  The fused
// detection kernel decodes only the (roi, class) pairs that pass the score threshold; this entry exists for callers of the
// stand-alone box_utils functions.
__global__ void bbox_transform_kernel(const float* __restrict__ boxes, const float* __restrict__ deltas, int n, int n_cls,
                                      float wx, float wy, float ww, float wh, int do_clip, float im_h, float im_w,
                                      float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * n_cls) return;
  const int i = t / n_cls;
  const float* b = boxes + (size_t)i * 4;
  float4 v = decode_clip<false>(b[0], b[1], b[2], b[3], deltas + (size_t)t * 4, wx, wy, ww, wh, im_h, im_w);
  if (do_clip) v = clip_box(v, im_h, im_w);
  reinterpret_cast<float4*>(out)[t] = v;
}

}  // namespace dtc

DTC_API int dtc_bbox_overlaps(const float* boxes, int n, int box_cols, const float* query_boxes, int k, int query_cols,
                              float* overlaps, dtc_stream_t stream) {
  if (n < 0 || k < 0 || box_cols < 4 || query_cols < 4) return DTC_EINVAL;
  if (n == 0 || k == 0) return DTC_OK;
  if (!boxes || !query_boxes || !overlaps) return DTC_EINVAL;
  const long long total = (long long)n * ((k + 3) / 4);
  const int blocks = (int)((total + 255) / 256 < 65535 * 16 ? (total + 255) / 256 : 65535 * 16);
  hipLaunchKernelGGL(dtc::bbox_overlaps_kernel, dim3(blocks), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), boxes, n,
                     box_cols, query_boxes, k, query_cols, overlaps,
                     ((k & 3) == 0 && (reinterpret_cast<uintptr_t>(overlaps) & 15) == 0) ? 1 : 0);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}

// the argument check of both voting entries: DTC_OK with *run = whether there is anything to launch
static int box_voting_check(const float* top_dets, int n_top, const float* all_dets, int n_all, const float* top_dets_out, bool* run) {
  *run = false;
  if (n_top < 0 || n_all < 0) return DTC_EINVAL;
  if (n_top == 0) return DTC_OK;
  if (!top_dets || !top_dets_out || (n_all > 0 && !all_dets)) return DTC_EINVAL;
  if (n_all > dtc::kVoteMax) return DTC_EUNSUPPORTED;
  *run = true;
  return DTC_OK;
}

DTC_API int dtc_box_voting(const float* top_dets, int n_top, const float* all_dets, int n_all, float thresh,
                           float* top_dets_out, int32_t* n_voters, dtc_stream_t stream) {
  bool run;
  const int rc = box_voting_check(top_dets, n_top, all_dets, n_all, top_dets_out, &run);
  if (!run) return rc;
  hipLaunchKernelGGL(dtc::box_voting_kernel<false>, dim3(n_top), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), top_dets, n_top,
                     all_dets, n_all, thresh, 0, 0.f, top_dets_out, n_voters);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}

DTC_API int dtc_box_voting_scored(const float* top_dets, int n_top, const float* all_dets, int n_all, float thresh,
                                  const dtc_vote_scoring* scoring, float* top_dets_out, int32_t* n_voters, dtc_stream_t stream) {
  if (scoring && (scoring->method < dtc::kVoteID || scoring->method > dtc::kVoteQuasiSum || !(scoring->beta > 0.f) ||
                  !std::isfinite(scoring->beta)))
    return DTC_EINVAL;
  if (!scoring || scoring->method == dtc::kVoteID)
    return dtc_box_voting(top_dets, n_top, all_dets, n_all, thresh, top_dets_out, n_voters, stream);
  bool run;
  const int rc = box_voting_check(top_dets, n_top, all_dets, n_all, top_dets_out, &run);
  if (!run) return rc;
  hipLaunchKernelGGL(dtc::box_voting_kernel<true>, dim3(n_top), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), top_dets, n_top,
                     all_dets, n_all, thresh, scoring->method, scoring->beta, top_dets_out, n_voters);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}

// bbox_transform optionally followed by clip_tiled_boxes: boxes [n,4], deltas [n,4*n_cls] -> out [n,4*n_cls]
DTC_API int dtc_bbox_transform(const float* boxes, const float* deltas, int n, int n_cls, float wx, float wy, float ww,
                               float wh, int do_clip, float im_h, float im_w, float* out, dtc_stream_t stream) {
  if (n < 0 || n_cls < 1) return DTC_EINVAL;
  if (n == 0) return DTC_OK;
  if (!boxes || !deltas || !out) return DTC_EINVAL;
  const long long total = (long long)n * n_cls;
  hipLaunchKernelGGL(dtc::bbox_transform_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), boxes, deltas, n, n_cls, wx, wy, ww, wh, do_clip, im_h, im_w, out);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
