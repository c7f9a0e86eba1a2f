// COCOeval's evaluateImg on a given IoU matrix on gfx950 (include/detectorch_segm_hip.h has the contract): the walk of
// csrc/eval/eval_match.hip with the IoU of a pair read from iou [N, max_out, G] and a detection's own area read from det_area.
// One kernel node, one wave per (image, class); wave 0 of an image writes the rows that belong to no class.
//   1  the detection rows and the gt rows of the class, compacted in row order (ballots)
//   2  the rank of every detection: the number of detections of the class that precede it (score descending, then row)
//   3  per area range the gt order "not ignored first", stable, as a byte list in LDS
//   4  the match loop: the detections in rank order; the detection's IoUs with the class's gt are staged in LDS, every lane (a, t)
//      walks its own gt order; the matched-gt bitmask of every lane is four LDS words; a ballot per detection is its output word
#include "wave_ops.h"

#include "../../../include/detectorch_segm_hip.h"

namespace dtc {

constexpr int kSegmMatchWave = 64;
constexpr unsigned kSegmCrowdBit = 1u << 31;
constexpr long long kSegmPadKey = 0x7fffffffffffffffll;

struct SegmMatchParams {
  const float* dets; const int32_t* det_count; const double* iou; const int32_t* det_area; const int32_t* gt_classes;
  const int32_t* gt_is_crowd; const int32_t* gt_counts; const float* gt_area; const int32_t* gt_mask_area;
  int max_out, G, num_classes, T, A, max_det;
  const double* iou_thrs; const double* area_rngs;
  long long image_base;
  int32_t* dt_rank; uint64_t* dt_match; uint64_t* dt_ignore; int32_t* gt_ignore; int32_t* gt_match; int32_t* npig; long long* sort_key;
};

// the float32 score as an unsigned integer that decreases with it; -0 counts as +0
__device__ __forceinline__ uint32_t segm_score_key_desc(float s) {
  if (s == 0.f) s = 0.f;
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~u;
}

// the class of a detection row: 0 for anything outside 1 .. num_classes - 1 (NaN included)
__device__ __forceinline__ int segm_row_class(float c, int num_classes) { return (c >= 1.f && c < (float)num_classes) ? (int)c : 0; }

__global__ __launch_bounds__(kSegmMatchWave) void segm_match_kernel(SegmMatchParams p) {
  __shared__ int16_t s_drow[DTC_EVAL_MAX_OUT];              // the class's detection rows, in row order
  __shared__ float s_dscore[DTC_EVAL_MAX_OUT];
  __shared__ int16_t s_dord[DTC_EVAL_MAX_OUT];              // the rows by rank
  __shared__ int16_t s_grow[DTC_EVAL_MAX_GT];               // the class's gt rows, in row order
  __shared__ double s_iou[DTC_EVAL_MAX_GT];                 // the IoUs of the detection at hand with them
  __shared__ uint32_t s_gig[DTC_EVAL_MAX_GT];               // bit a: ignored in area range a; kSegmCrowdBit
  __shared__ uint8_t s_gord[DTC_EVAL_MAX_AREAS][DTC_EVAL_MAX_GT];   // per area range: the visiting order, as positions of s_grow
  __shared__ uint64_t s_gtm[DTC_EVAL_MAX_GT / 64][kSegmMatchWave];   // per lane: the gt matched so far

  const int lane = threadIdx.x, k = blockIdx.x, n = blockIdx.y;
  const int T = p.T, A = p.A, TA = T * A, K = p.num_classes - 1;
  const int nd = min(max(p.det_count[n], 0), p.max_out);
  const int ng = p.G > 0 ? min(max(p.gt_counts[n], 0), p.G) : 0;
  const float* dets = p.dets + (size_t)n * p.max_out * 6;
  const size_t drow0 = (size_t)n * p.max_out, grow0 = (size_t)n * p.G;

  if (k == 0) {                                            // the rows of no class
    for (int d = lane; d < p.max_out; d += kSegmMatchWave) {
      if (d < nd && segm_row_class(dets[d * 6 + 5], p.num_classes) != 0) continue;
      p.dt_rank[drow0 + d] = -1; p.dt_match[drow0 + d] = 0ull; p.dt_ignore[drow0 + d] = 0ull; p.sort_key[drow0 + d] = kSegmPadKey;
    }
    for (int g = 0; g < p.G; g++) {
      bool none = g >= ng;
      if (!none) { const int c = p.gt_classes[grow0 + g]; none = c < 1 || c > K; }
      if (!none) continue;
      if (lane == 0) p.gt_ignore[grow0 + g] = 0;
      if (lane < TA) p.gt_match[(grow0 + g) * TA + lane] = -1;
    }
    return;
  }

  // 1. the class's rows
  int D = 0;
  for (int d0 = 0; d0 < nd; d0 += kSegmMatchWave) {
    const int d = d0 + lane;
    const bool is = d < nd && segm_row_class(dets[d * 6 + 5], p.num_classes) == k;
    const uint64_t bal = __ballot(is);
    if (is) { const int at = D + lanes_below(bal, lane); s_drow[at] = (int16_t)d; s_dscore[at] = dets[d * 6 + 4]; }
    D += __builtin_popcountll(bal);
  }
  int Gk = 0;
  for (int g0 = 0; g0 < ng; g0 += kSegmMatchWave) {
    const int g = g0 + lane;
    const bool is = g < ng && p.gt_classes[grow0 + g] == k;
    const uint64_t bal = __ballot(is);
    if (is) s_grow[Gk + lanes_below(bal, lane)] = (int16_t)g;
    Gk += __builtin_popcountll(bal);
  }
  __syncthreads();
  for (int i = lane; i < Gk; i += kSegmMatchWave) {
    const int g = s_grow[i];
    const bool crowd = p.gt_is_crowd[grow0 + g] != 0;
    const double area = p.gt_area ? (double)p.gt_area[grow0 + g] : (double)p.gt_mask_area[grow0 + g];
    uint32_t ig = 0;
    for (int a = 0; a < A; a++)
      if (crowd || area < p.area_rngs[2 * a] || area > p.area_rngs[2 * a + 1]) ig |= 1u << a;
    p.gt_ignore[grow0 + g] = (int32_t)ig;
    s_gig[i] = ig | (crowd ? kSegmCrowdBit : 0u);
  }

  // 2. ranks, on the integer score keys: a total order whatever the bits, so the ranks are always a permutation
  for (int i = lane; i < D; i += kSegmMatchWave) {
    const uint32_t ki = segm_score_key_desc(s_dscore[i]);
    int rank = 0;
    for (int j = 0; j < D; j++) {
      const uint32_t kj = segm_score_key_desc(s_dscore[j]);
      rank += (kj < ki || (kj == ki && j < i)) ? 1 : 0;
    }
    const int row = s_drow[i];
    s_dord[rank] = (int16_t)row;
    const bool cut = rank >= p.max_det;
    p.dt_rank[drow0 + row] = cut ? -1 : rank;
    p.sort_key[drow0 + row] = cut ? kSegmPadKey
                                  : (long long)(((uint64_t)k << 53) | ((uint64_t)ki << 21) | (uint64_t)(p.image_base + n));
    if (cut) { p.dt_match[drow0 + row] = 0ull; p.dt_ignore[drow0 + row] = 0ull; }
  }
  __syncthreads();

  // 3. per area range: not ignored first, stable
  for (int a = 0; a < A; a++) {
    int nn = 0;
    for (int g0 = 0; g0 < Gk; g0 += kSegmMatchWave) {
      const int i = g0 + lane;
      nn += __builtin_popcountll(__ballot(i < Gk && !((s_gig[i] >> a) & 1u)));
    }
    int at_n = 0, at_i = nn;
    for (int g0 = 0; g0 < Gk; g0 += kSegmMatchWave) {
      const int i = g0 + lane;
      const bool in = i < Gk, ig = in && ((s_gig[i] >> a) & 1u);
      const uint64_t bn = __ballot(in && !ig), bi = __ballot(ig);
      if (in) s_gord[a][ig ? at_i + lanes_below(bi, lane) : at_n + lanes_below(bn, lane)] = (uint8_t)i;
      at_n += __builtin_popcountll(bn); at_i += __builtin_popcountll(bi);
    }
    if (lane == 0) p.npig[((size_t)n * K + (k - 1)) * A + a] = nn;
  }
  const bool active = lane < TA;
  const int a = active ? lane / T : 0, t = active ? lane % T : 0;
  if (active) {
    for (int i = 0; i < Gk; i++) p.gt_match[(grow0 + s_grow[i]) * TA + lane] = -1;     // the lane that may rewrite it below
  }
  for (int w = 0; w < DTC_EVAL_MAX_GT / 64; w++) s_gtm[w][lane] = 0ull;
  __syncthreads();

  // 4. the match loop
  const double thr = active ? fmin(p.iou_thrs[t], 1.0 - 1e-10) : 0.0;
  const double lo = active ? p.area_rngs[2 * a] : 0.0, hi = active ? p.area_rngs[2 * a + 1] : 0.0;
  const int Dm = min(D, p.max_det);
  for (int d = 0; d < Dm; d++) {
    const int row = s_dord[d];
    for (int i = lane; i < Gk; i += kSegmMatchWave) s_iou[i] = p.iou[(drow0 + row) * p.G + s_grow[i]];
    __syncthreads();
    bool matched = false, ign = false;
    if (active) {
      double best = thr;
      int m = -1;
      uint32_t m_ig = 0;
      for (int q = 0; q < Gk; q++) {
        const int i = s_gord[a][q];
        const uint32_t gi = s_gig[i];
        const bool crowd = (gi & kSegmCrowdBit) != 0, g_ig = ((gi >> a) & 1u) != 0;
        if (((s_gtm[i >> 6][lane] >> (i & 63)) & 1ull) && !crowd) continue;
        if (m >= 0 && !m_ig && g_ig) break;
        const double iou = s_iou[i];
        if (iou < best) continue;
        best = iou; m = i; m_ig = g_ig ? 1u : 0u;
      }
      if (m >= 0) {
        matched = true; ign = m_ig != 0;
        s_gtm[m >> 6][lane] |= 1ull << (m & 63);
        p.gt_match[(grow0 + s_grow[m]) * TA + lane] = row;
      } else {
        const double area = (double)p.det_area[drow0 + row];
        ign = area < lo || area > hi;
      }
    }
    const uint64_t bm = __ballot(matched), bi = __ballot(ign);
    if (lane == 0) { p.dt_match[drow0 + row] = bm; p.dt_ignore[drow0 + row] = bi; }
    __syncthreads();                                       // s_iou is rewritten for the next detection
  }
}

}  // namespace dtc

DTC_API int dtc_segm_match(const float* dets, const int32_t* det_count, const double* iou, const int32_t* det_area,
                           const int32_t* gt_classes, const int32_t* gt_is_crowd, const int32_t* gt_counts, const float* gt_area,
                           const int32_t* gt_mask_area, int batch, int max_out, int gt_stride, int num_classes, const double* iou_thrs,
                           int n_thrs, const double* area_rngs, int n_areas, int max_det, long long image_base, int32_t* dt_rank,
                           uint64_t* dt_match, uint64_t* dt_ignore, int32_t* gt_ignore, int32_t* gt_match, int32_t* npig,
                           long long* sort_key, dtc_stream_t stream) {
  // shapes and parameters, then limits
  if (batch < 1 || max_out < 1 || gt_stride < 0 || num_classes < 2 || n_thrs < 1 || n_areas < 1 || max_det < 1 || image_base < 0)
    return DTC_EINVAL;
  if (batch > DTC_EVAL_MAX_BATCH || max_out > DTC_EVAL_MAX_OUT || gt_stride > DTC_EVAL_MAX_GT || num_classes > DTC_EVAL_MAX_CLASSES ||
      n_areas > DTC_EVAL_MAX_AREAS || (long long)n_thrs * n_areas > DTC_EVAL_MAX_PAIRS || image_base > DTC_EVAL_MAX_IMAGES - batch)
    return DTC_EUNSUPPORTED;
  // pointers
  if (!dets || !det_count || !det_area || !iou_thrs || !area_rngs || !dt_rank || !dt_match || !dt_ignore || !npig || !sort_key)
    return DTC_EINVAL;
  if (gt_stride > 0 && (!iou || !gt_classes || !gt_is_crowd || !gt_counts || !gt_ignore || !gt_match || (!gt_area && !gt_mask_area)))
    return DTC_EINVAL;

  dtc::SegmMatchParams p{};
  p.dets = dets; p.det_count = det_count; p.iou = iou; p.det_area = det_area; p.gt_classes = gt_classes; p.gt_is_crowd = gt_is_crowd;
  p.gt_counts = gt_counts; p.gt_area = gt_area; p.gt_mask_area = gt_mask_area;
  p.max_out = max_out; p.G = gt_stride; p.num_classes = num_classes; p.T = n_thrs; p.A = n_areas; p.max_det = max_det;
  p.iou_thrs = iou_thrs; p.area_rngs = area_rngs; p.image_base = image_base;
  p.dt_rank = dt_rank; p.dt_match = dt_match; p.dt_ignore = dt_ignore; p.gt_ignore = gt_ignore; p.gt_match = gt_match; p.npig = npig;
  p.sort_key = sort_key;
  hipLaunchKernelGGL(dtc::segm_match_kernel, dim3(num_classes, batch), dim3(dtc::kSegmMatchWave), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
