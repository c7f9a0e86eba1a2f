// maskApi.c:rleIou / rleArea on gfx950 for every (detection, gt) pair of one class, N images at once (include/detectorch_segm_hip.h
// has the contract).  Two kernel nodes, no bitmap:
//   1  segm_prepare_kernel: one wave per run list.  The runs become clipped run ENDS (64-bit prefix sums, min with h * w) in the
//      workspace; a gt's ends are paired with the ones accumulated up to each end, so that ones_g(x), the set pixels of g in front
//      of position x, is one binary search and one add.  The areas are the totals.  A row that takes part in nothing has n = 0.
//   2  segm_pair_kernel: one workgroup of four waves per detection row.  Thread g decides whether gt row g makes a pair with it (same
//      class, both taking part): no: it writes the 0; yes: g goes to a list in LDS.  Then one wave per pair of the list: the lanes
//      stride over the detection's one-runs [s, e) and add ones_g(e) - ones_g(s); the uint32 partial sums (at most 2^30 in all)
//      are reduced across the wave; lane 0 divides once, in float64.
// Nothing read from a run list or a run count is used as an address: counts are clamped to the stride, positions to h * w.
#include "wave_ops.h"

#include "../../../include/detectorch_segm_hip.h"

namespace dtc {

constexpr int kSegmWave = 64;
constexpr int kSegmPairWaves = 4;                            // waves of one workgroup of the pair kernel
static_assert(kSegmWave * kSegmPairWaves >= DTC_EVAL_MAX_GT, "one thread per gt row");

struct SegmIouParams {
  const float* dets; const int32_t* det_count; const uint32_t* det_runs; const int32_t* det_n_runs; const float* im_size;
  const uint32_t* gt_runs; const int32_t* gt_n_runs; const int32_t* gt_classes; const int32_t* gt_is_crowd; const int32_t* gt_counts;
  int max_out, det_stride, G, gt_stride, num_classes;
  uint32_t* det_ends;                                        // workspace [N, max_out, det_stride]: clipped run ends
  uint2* gt_tab;                                             // workspace [N, G, gt_stride]: (clipped run end, ones up to it)
  int32_t* det_n; int32_t* gt_n;                             // workspace [N, max_out], [N, G]: the runs in use, 0 on a row taking no part
  double* iou; int32_t* det_area; int32_t* gt_mask_area; int32_t* n_bad;
};

// the class of a detection row: 0 for anything outside 1 .. num_classes - 1 (NaN included)
__device__ __forceinline__ int segm_det_class(float c, int num_classes) { return (c >= 1.f && c < (float)num_classes) ? (int)c : 0; }

// one side of im_size as an integer: truncated; below 1, NaN: 0; above 2^30: 2^30
__device__ __forceinline__ long long segm_side(float v) {
  if (!(v >= 1.f)) return 0;
  return v >= (float)DTC_SEGM_MAX_PIXELS ? (long long)DTC_SEGM_MAX_PIXELS : (long long)(int)v;
}

__device__ __forceinline__ uint32_t segm_pixels(const float* im_size, int n) {
  const long long hw = segm_side(im_size[2 * n]) * segm_side(im_size[2 * n + 1]);
  return (uint32_t)(hw > DTC_SEGM_MAX_PIXELS ? DTC_SEGM_MAX_PIXELS : hw);
}

__global__ __launch_bounds__(kSegmWave) void segm_prepare_kernel(SegmIouParams p) {
  const int lane = threadIdx.x, n = blockIdx.y;
  const int row = blockIdx.x;                                // < max_out: a detection row; else gt row - max_out
  const bool is_gt = row >= p.max_out;
  const int r = is_gt ? row - p.max_out : row;
  const int K = p.num_classes - 1;
  const uint32_t hw = segm_pixels(p.im_size, n);

  const uint32_t* runs;
  int n_runs = 0;
  if (is_gt) {
    const int ng = min(max(p.gt_counts[n], 0), p.G);
    const size_t at = (size_t)n * p.G + r;
    if (r < ng) { const int c = p.gt_classes[at]; if (c >= 1 && c <= K) n_runs = min(max(p.gt_n_runs[at], 0), p.gt_stride); }
    runs = p.gt_runs + at * p.gt_stride;
  } else {
    const int nd = min(max(p.det_count[n], 0), p.max_out);
    const size_t at = (size_t)n * p.max_out + r;
    if (r < nd && segm_det_class(p.dets[at * 6 + 5], p.num_classes) != 0) n_runs = min(max(p.det_n_runs[at], 0), p.det_stride);
    runs = p.det_runs + at * p.det_stride;
  }
  uint32_t* ends = is_gt ? nullptr : p.det_ends + ((size_t)n * p.max_out + r) * p.det_stride;
  uint2* tab = is_gt ? p.gt_tab + ((size_t)n * p.G + r) * p.gt_stride : nullptr;

  long long pos = 0;                                         // the unclipped end of the runs in front of this chunk
  uint32_t prev_end = 0, ones = 0;                           // the clipped one, and the ones up to it
  for (int j0 = 0; j0 < n_runs; j0 += kSegmWave) {
    const int j = j0 + lane;
    const long long len = j < n_runs ? (long long)runs[j] : 0ll;
    const long long incl = pos + wave_incl_scan(len, lane);
    const uint32_t end = (uint32_t)(incl < (long long)hw ? incl : (long long)hw);
    uint32_t before = __shfl_up(end, 1, kSegmWave);
    if (lane == 0) before = prev_end;
    const uint32_t mine = (j < n_runs && (j & 1)) ? end - before : 0u;      // the pixels of a one-run that lie inside the image
    const uint32_t acc = ones + wave_incl_scan(mine, lane);
    if (j < n_runs) {
      if (is_gt) tab[j] = make_uint2(end, acc); else ends[j] = end;
    }
    pos = __shfl(incl, kSegmWave - 1, kSegmWave);
    prev_end = __shfl(end, kSegmWave - 1, kSegmWave);
    ones = __shfl(acc, kSegmWave - 1, kSegmWave);
  }
  if (lane == 0) {
    if (is_gt) { p.gt_n[(size_t)n * p.G + r] = n_runs; p.gt_mask_area[(size_t)n * p.G + r] = (int32_t)ones; }
    else { p.det_n[(size_t)n * p.max_out + r] = n_runs; p.det_area[(size_t)n * p.max_out + r] = (int32_t)ones; }
  }
}

// the set pixels of a gt in front of position x: tab holds n (end, ones up to the end) pairs with non-decreasing ends
__device__ __forceinline__ uint32_t segm_ones_before(const uint2* tab, int n, uint32_t x) {
  int lo = 0, hi = n;                                        // the first run whose end is above x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid].x > x) hi = mid; else lo = mid + 1;
  }
  if (lo == 0) return 0u;                                    // inside the leading zeros (or no runs at all)
  const uint2 before = tab[lo - 1];
  return before.y + ((lo < n && (lo & 1)) ? x - before.x : 0u);    // past the last run: zeros
}

__global__ __launch_bounds__(kSegmWave * kSegmPairWaves) void segm_pair_kernel(SegmIouParams p) {
  const int lane = threadIdx.x & (kSegmWave - 1), wave = threadIdx.x / kSegmWave;
  const int d = blockIdx.x, n = blockIdx.y;
  const int nd = min(max(p.det_count[n], 0), p.max_out);
  const size_t drow = (size_t)n * p.max_out + d;

  if (d == 0 && wave == 0) {                                 // the masks of this image that did not fit
    int bad = 0;
    for (int d0 = 0; d0 < nd; d0 += kSegmWave) {
      const int dd = d0 + lane;
      bad += __builtin_popcountll(__ballot(dd < nd && p.det_n_runs[(size_t)n * p.max_out + dd] < 0));
    }
    if (lane == 0) p.n_bad[n] = bad;
  }
  if (p.G == 0) return;

  const int ng = min(max(p.gt_counts[n], 0), p.G);
  const int cls = d < nd ? segm_det_class(p.dets[drow * 6 + 5], p.num_classes) : 0;
  const int n_d = cls ? p.det_n[drow] : 0;
  const uint32_t da = cls ? (uint32_t)p.det_area[drow] : 0u;
  const uint32_t* dends = p.det_ends + drow * p.det_stride;

  // thread g looks at gt row g (G <= 256 = the workgroup): no pair there: a zero, written coalesced; the pairs go to a list in LDS
  __shared__ int s_pairs[kSegmPairWaves];
  __shared__ int16_t s_g[DTC_EVAL_MAX_GT];
  const int tg = threadIdx.x;
  const bool pair = cls != 0 && tg < ng && p.gt_classes[(size_t)n * p.G + tg] == cls;
  if (tg < p.G && !pair) p.iou[drow * p.G + tg] = 0.0;
  const uint64_t bal = __ballot(pair);
  if (lane == 0) s_pairs[wave] = __builtin_popcountll(bal);
  __syncthreads();
  int at = 0, n_pairs = 0;
  for (int w = 0; w < kSegmPairWaves; w++) { if (w < wave) at += s_pairs[w]; n_pairs += s_pairs[w]; }
  if (pair) s_g[at + lanes_below(bal, lane)] = (int16_t)tg;
  __syncthreads();

  for (int i = wave; i < n_pairs; i += kSegmPairWaves) {     // one wave per pair
    const int g = s_g[i];
    const size_t grow = (size_t)n * p.G + g;
    const uint32_t ga = (uint32_t)p.gt_mask_area[grow];
    uint32_t inter = 0;
    if (da && ga) {
      const int n_g = p.gt_n[grow];
      const uint2* tab = p.gt_tab + grow * p.gt_stride;
      for (int j = 2 * lane + 1; j < n_d; j += 2 * kSegmWave) {         // the one-runs are the odd ones
        const uint32_t s = dends[j - 1], e = dends[j];
        if (e > s) inter += segm_ones_before(tab, n_g, e) - segm_ones_before(tab, n_g, s);
      }
#pragma unroll
      for (int off = kSegmWave / 2; off > 0; off >>= 1) inter += __shfl_xor(inter, off, kSegmWave);
    }
    double out = 0.0;
    if (inter) {
      const uint32_t u = p.gt_is_crowd[grow] != 0 ? da : da + ga - inter;
      out = (double)inter / (double)u;
    }
    if (lane == 0) p.iou[drow * p.G + g] = out;
  }
}

__host__ inline size_t segm_align16(size_t v) { return (v + 15) & ~(size_t)15; }

struct SegmLayout { size_t det_ends, gt_tab, det_n, gt_n, total; };

__host__ inline SegmLayout segm_layout(int batch, int max_out, int det_stride, int G, int gt_stride) {
  SegmLayout l;
  size_t at = 0;
  l.gt_tab = at; at += segm_align16((size_t)batch * G * gt_stride * sizeof(uint2));
  l.det_ends = at; at += segm_align16((size_t)batch * max_out * det_stride * sizeof(uint32_t));
  l.det_n = at; at += segm_align16((size_t)batch * max_out * sizeof(int32_t));
  l.gt_n = at; at += segm_align16((size_t)batch * G * sizeof(int32_t));
  l.total = at;
  return l;
}

__host__ inline int segm_iou_shape(int batch, int max_out, int det_stride, int G, int gt_stride) {
  if (batch < 1 || max_out < 1 || det_stride < 1 || G < 0 || gt_stride < 1) return DTC_EINVAL;
  if (batch > DTC_EVAL_MAX_BATCH || max_out > DTC_EVAL_MAX_OUT || G > DTC_EVAL_MAX_GT || det_stride > DTC_SEGM_MAX_RUNS ||
      gt_stride > DTC_SEGM_MAX_RUNS)
    return DTC_EUNSUPPORTED;
  return DTC_OK;
}

}  // namespace dtc

DTC_API const char* dtc_segm_target_arch(void) { return "gfx950"; }

DTC_API size_t dtc_segm_iou_workspace_bytes(int batch, int max_out, int det_runs_stride, int gt_stride, int gt_runs_stride) {
  if (dtc::segm_iou_shape(batch, max_out, det_runs_stride, gt_stride, gt_runs_stride) != DTC_OK) return 0;
  return dtc::segm_layout(batch, max_out, det_runs_stride, gt_stride, gt_runs_stride).total;
}

DTC_API int dtc_segm_iou(const float* dets, const int32_t* det_count, const uint32_t* det_runs, const int32_t* det_n_runs,
                         const float* im_size, const uint32_t* gt_runs, const int32_t* gt_n_runs, const int32_t* gt_classes,
                         const int32_t* gt_is_crowd, const int32_t* gt_counts, int batch, int max_out, int det_runs_stride,
                         int gt_stride, int gt_runs_stride, int num_classes, void* workspace, size_t workspace_bytes, double* iou,
                         int32_t* det_area, int32_t* gt_mask_area, int32_t* n_bad, dtc_stream_t stream) {
  // shapes and parameters, then limits
  const int shape = dtc::segm_iou_shape(batch, max_out, det_runs_stride, gt_stride, gt_runs_stride);
  if (shape == DTC_EINVAL || num_classes < 2) return DTC_EINVAL;
  if (shape != DTC_OK || num_classes > DTC_EVAL_MAX_CLASSES) return DTC_EUNSUPPORTED;
  // pointers
  const dtc::SegmLayout l = dtc::segm_layout(batch, max_out, det_runs_stride, gt_stride, gt_runs_stride);
  if (!dets || !det_count || !det_runs || !det_n_runs || !im_size || !det_area || !n_bad || !workspace) return DTC_EINVAL;
  if (gt_stride > 0 && (!gt_runs || !gt_n_runs || !gt_classes || !gt_is_crowd || !gt_counts || !iou || !gt_mask_area)) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0 || workspace_bytes < l.total) return DTC_EINVAL;

  char* ws = static_cast<char*>(workspace);
  dtc::SegmIouParams p{};
  p.dets = dets; p.det_count = det_count; p.det_runs = det_runs; p.det_n_runs = det_n_runs; p.im_size = im_size;
  p.gt_runs = gt_runs; p.gt_n_runs = gt_n_runs; p.gt_classes = gt_classes; p.gt_is_crowd = gt_is_crowd; p.gt_counts = gt_counts;
  p.max_out = max_out; p.det_stride = det_runs_stride; p.G = gt_stride; p.gt_stride = gt_runs_stride; p.num_classes = num_classes;
  p.det_ends = reinterpret_cast<uint32_t*>(ws + l.det_ends); p.gt_tab = reinterpret_cast<uint2*>(ws + l.gt_tab);
  p.det_n = reinterpret_cast<int32_t*>(ws + l.det_n); p.gt_n = reinterpret_cast<int32_t*>(ws + l.gt_n);
  p.iou = iou; p.det_area = det_area; p.gt_mask_area = gt_mask_area; p.n_bad = n_bad;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::segm_prepare_kernel, dim3(max_out + gt_stride, batch), dim3(dtc::kSegmWave), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::segm_pair_kernel, dim3(max_out, batch), dim3(dtc::kSegmWave * dtc::kSegmPairWaves), 0, s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
