// Precomputed proposals -> RoIAlign-ready rois for gfx950 -- the device form of the Fast R-CNN test-time preprocessing
//   scale        lib/utils/preprocess_sample.py:36        proposals = boxes * im_scale            (float32 array * Python float)
//   dedup        lib/utils/preprocess_sample.py:63-70     remove_dup_prop: np.round(p * 1/16) . (1e3, 1e6, 1e9, 1e12), np.unique
//   distribute   lib/utils/multilevel_rois.py:19-53       add_multilevel_rois_for_test (FPN), one level for C4
// Two launches: proposal_dedup_kernel (one workgroup per image) writes the unique rows in np.unique's order, then
// dtc_fpn_collect_distribute(in_scores = NULL) maps levels and emits the restore order and the RoIAlign descriptors -- those
// outputs are the pinned collect kernel's by construction.
#include <cmath>

#include "block_sort.h"
#include "dtc_common.h"
#include "wave_ops.h"

namespace dtc {

constexpr int kPrepThreads = 1024;
constexpr int kPrepMaxIn = 2048;          // two keys per thread through block_bitonic_sort
constexpr int kIdxBits = 11;              // row index < 2048
// The reference's hash divided by 1000 (every term is a multiple of 1e3): h = r1 + 1e3 r2 + 1e6 r3 + 1e9 r4 with |r| <= 8192,
// so |h| <= 8192 * 1001001001 < 2^43.  Key = (h + 2^43) << 11 | row: 55 bits, unique per row.  Ascending key = ascending hash,
// then ascending row, so the first key of every run of equal hashes is np.unique's return_index (the first occurrence).
constexpr int64_t kHashBias = 1ll << 43;
constexpr float kRMax = 8192.f;

struct PrepParams {
  const float* boxes;        // [B, in_stride, 4]
  const int32_t* counts;     // [B]
  const float* im_scale;     // [B]
  int in_stride, max_out;
  float dedup_scale;         // 0: no dedup (every finite row, input order)
  float* uniq;               // [B, max_out, 4]  unique scaled rows (workspace)
  int32_t* n_uniq;           // [B]              (workspace)
  int32_t* src_index;        // [B, max_out]     (nullable)
};

__device__ __forceinline__ float4 scaled_row(const PrepParams& p, int b, int i, float s) {
  const float4 v = reinterpret_cast<const float4*>(p.boxes)[(size_t)b * p.in_stride + i];
  return make_float4(v.x * s, v.y * s, v.z * s, v.w * s);        // one float32 multiply per coordinate
}

__device__ __forceinline__ int64_t grid_coord(float x, float ds) {
  const float r = rintf(x * ds);                                  // np.round: half to even, in float32
  return (int64_t)fminf(fmaxf(r, -kRMax), kRMax);                 // identity inside the exact domain
}

__global__ __launch_bounds__(kPrepThreads) void proposal_dedup_kernel(PrepParams p) {
  __shared__ uint64_t keys[kPrepMaxIn];
  __shared__ int wave_heads[kPrepThreads / 64];
  __shared__ int run_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n = min(max(p.counts[b], 0), p.in_stride);
  const float s = p.im_scale[b];
  const bool dedup = p.dedup_scale != 0.f;
  const int np2 = next_pow2(n);
  for (int i = tid; i < np2; i += kPrepThreads) {
    uint64_t k = kPadKey;
    if (i < n) {
      const float4 q = scaled_row(p, b, i, s);
      if (isfinite(q.x) && isfinite(q.y) && isfinite(q.z) && isfinite(q.w)) {       // non-finite rows are dropped
        int64_t h = i;                                                             // no dedup: every row unique, input order
        if (dedup) {
          const float ds = p.dedup_scale;
          h = grid_coord(q.x, ds) + 1000ll * grid_coord(q.y, ds) + 1000000ll * grid_coord(q.z, ds) +
              1000000000ll * grid_coord(q.w, ds);
        }
        k = ((uint64_t)(h + kHashBias) << kIdxBits) | (uint64_t)i;
      }
    }
    keys[i] = k;
  }
  block_bitonic_sort<kPrepThreads>(keys, np2);                     // barriers inside, before and after
  if (tid == 0) run_s = 0;
  __syncthreads();
  // sorted position j is the first occurrence of its hash when position j - 1 holds another hash; its unique rank is the number of
  // such heads before it (ballot per wave, wave totals through LDS, kPrepThreads positions per round)
  for (int j0 = 0; j0 < np2; j0 += kPrepThreads) {
    const int j = j0 + tid;
    bool head = false;
    uint64_t k = kPadKey;
    if (j < np2) {
      k = keys[j];
      head = k != kPadKey && (j == 0 || (k >> kIdxBits) != (keys[j - 1] >> kIdxBits));
    }
    const uint64_t m = __ballot(head);
    if (lane == 0) wave_heads[wv] = __builtin_popcountll(m);
    __syncthreads();
    int rank = run_s;
    for (int q = 0; q < wv; q++) rank += wave_heads[q];
    rank += lanes_below(m, lane);
    if (head && rank < p.max_out) {
      const int i = (int)(k & ((1u << kIdxBits) - 1u));
      reinterpret_cast<float4*>(p.uniq)[(size_t)b * p.max_out + rank] = scaled_row(p, b, i, s);
      if (p.src_index) p.src_index[(size_t)b * p.max_out + rank] = i;
    }
    __syncthreads();
    if (tid == 0) { int t = 0; for (int q = 0; q < kPrepThreads / 64; q++) t += wave_heads[q]; run_s += t; }
    __syncthreads();
  }
  if (tid == 0) p.n_uniq[b] = min(run_s, p.max_out);
}

// workspace layout: the unique rows between the two launches, and their number per image
struct PrepPlan { size_t uniq, n_uniq, total; };
static PrepPlan prep_plan(int batch, int max_out) {
  PrepPlan d;
  Carve w{16};
  d.uniq = w.take((size_t)batch * max_out * 4 * sizeof(float));
  d.n_uniq = w.take((size_t)(batch > 0 ? batch : 1) * sizeof(int32_t));
  d.total = w.end;
  return d;
}

}  // namespace dtc

DTC_API size_t dtc_prepare_proposals_workspace_bytes(int batch, int max_out) {
  if (batch < 0 || max_out < 1) return 0;
  return dtc::prep_plan(batch, max_out).total;
}

DTC_API int dtc_prepare_proposals(const float* boxes, const int32_t* counts, const float* im_scale, int batch, int in_stride,
                                  float dedup_scale, int k_min, int k_max, int max_out, void* workspace, size_t workspace_bytes,
                                  float* rois5, int32_t* roi_levels, int32_t* n_out, float* rois_by_level, int32_t* level_counts,
                                  int32_t* idx_restore, int32_t* roi_order, float* roi_desc, int32_t* src_index,
                                  dtc_stream_t stream) {
  if (batch < 0 || in_stride < 1 || max_out < in_stride || k_max < k_min || k_max - k_min + 1 > DTC_MAX_LEVELS ||
      !std::isfinite(dedup_scale) || dedup_scale < 0.f)
    return DTC_EINVAL;
  if (in_stride > dtc::kPrepMaxIn) return DTC_EUNSUPPORTED;
  if (batch == 0) return DTC_OK;
  if (!boxes || !counts || !im_scale || !rois5 || !roi_levels || !n_out || !rois_by_level || !level_counts || !idx_restore ||
      !workspace)
    return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0 || (reinterpret_cast<uintptr_t>(boxes) & 15) != 0) return DTC_EINVAL;
  const dtc::PrepPlan pl = dtc::prep_plan(batch, max_out);
  if (workspace_bytes < pl.total) return DTC_EWORKSPACE;
  dtc::PrepParams p;
  p.boxes = boxes; p.counts = counts; p.im_scale = im_scale; p.in_stride = in_stride; p.max_out = max_out;
  p.dedup_scale = dedup_scale;
  p.uniq = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + pl.uniq);
  p.n_uniq = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(workspace) + pl.n_uniq);
  p.src_index = src_index;
  hipLaunchKernelGGL(dtc::proposal_dedup_kernel, dim3(batch), dim3(dtc::kPrepThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  // one input list per image, no scores: rows taken in the given (np.unique) order; levels, restore order, visiting order
  return dtc_fpn_collect_distribute(p.uniq, nullptr, p.n_uniq, batch, 1, max_out, max_out, k_min, k_max, rois5, nullptr, roi_levels,
                                    n_out, rois_by_level, level_counts, idx_restore, roi_order, roi_desc, 0, stream);
}
