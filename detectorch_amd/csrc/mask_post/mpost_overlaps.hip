// rle_masks_to_boxes and maskUtils.iou(a, b, iscrowd) on run lists (include/detectorch_mpost_hip.h, entries 1 and 2), no bitmap:
//   mpost_boxes_kernel    one wave per list: the one-runs' clipped [s, e) give the first and last position (x0, x1 = / h), the rows
//                         they touch (a run across a column boundary touches rows 0 and h - 1) and the area, by integer reductions.
//   mpost_prepare_kernel  one wave per list: a's runs become clipped run ENDS, b's (end, ones up to the end) pairs, so that ones_b(x),
//                         the set pixels of b in front of position x, is one binary search and one add.  The areas are the totals.
//   mpost_pair_kernel     one workgroup of four waves per row of a, one wave per pair: the lanes stride over a's one-runs [s, e) and
//                         add ones_b(e) - ones_b(s); lane 0 divides once, in float64.
#include "mpost_common.h"

namespace dtc {

constexpr int kMpostPairWaves = 4;

struct MpostBoxesParams {
  const uint32_t* runs; const int32_t* n_runs; const int32_t* counts; const float* im_size;
  int R, stride;
  int32_t* boxes; int32_t* area; int32_t* nonempty;
};

__global__ __launch_bounds__(kMpostWave) void mpost_boxes_kernel(MpostBoxesParams p) {
  const int lane = threadIdx.x, r = blockIdx.x, n = blockIdx.y;
  if (r >= mpost_count(p.counts, n, p.R)) return;            // rows past the count are not written
  const size_t row = (size_t)n * p.R + r;
  const uint32_t hw = mpost_pixels(p.im_size, n);
  const uint32_t h = (uint32_t)mpost_side(p.im_size[2 * n]);
  const int n_runs = min(max(p.n_runs[row], 0), p.stride);
  const uint32_t* runs = p.runs + row * p.stride;

  long long pos = 0;
  uint32_t prev_end = 0, first = 0xffffffffu, last = 0u, ymin = 0xffffffffu, ymax = 0u, ones = 0u;
  for (int j0 = 0; j0 < n_runs; j0 += kMpostWave) {
    uint32_t s, e;
    mpost_chunk_ends(runs, n_runs, j0, lane, hw, pos, prev_end, s, e);
    if (((j0 + lane) & 1) && e > s) {                        // a one-run with pixels inside the image (h >= 1: hw >= e > 0)
      const uint32_t c0 = s / h, c1 = (e - 1u) / h;
      first = min(first, s); last = max(last, e - 1u); ones += e - s;
      ymin = min(ymin, c1 > c0 ? 0u : s - c0 * h);
      ymax = max(ymax, c1 > c0 ? h - 1u : (e - 1u) - c1 * h);
    }
  }
  first = wave_min(first); last = wave_max(last); ymin = wave_min(ymin); ymax = wave_max(ymax); ones = wave_sum(ones);
  if (lane == 0) {
    int4 box = make_int4(0, 0, 0, 0);
    if (ones) box = make_int4((int)(first / h), (int)ymin, (int)(last / h), (int)ymax);
    reinterpret_cast<int4*>(p.boxes)[row] = box;
    p.area[row] = (int32_t)ones; p.nonempty[row] = ones ? 1 : 0;
  }
}

struct MpostOverlapsParams {
  const uint32_t* a_runs; const int32_t* a_n_runs; const int32_t* a_count; const uint32_t* b_runs; const int32_t* b_n_runs;
  const int32_t* b_count; const float* im_size;
  int Ra, a_stride, Rb, b_stride, crowd;
  uint32_t* a_ends;                                          // workspace [N, Ra, a_stride]: clipped run ends
  uint2* b_tab;                                              // workspace [N, Rb, b_stride]: (clipped run end, ones up to it)
  int32_t* a_n; int32_t* b_n;                                // workspace [N, Ra], [N, Rb]: the runs in use, 0 on a row past its count
  double* ovr; int32_t* a_area; int32_t* b_area;
};

__global__ __launch_bounds__(kMpostWave) void mpost_prepare_kernel(MpostOverlapsParams p) {
  const int lane = threadIdx.x, n = blockIdx.y;
  const bool is_b = (int)blockIdx.x >= p.Ra;
  const int r = is_b ? blockIdx.x - p.Ra : blockIdx.x;
  const int R = is_b ? p.Rb : p.Ra, stride = is_b ? p.b_stride : p.a_stride;
  const size_t row = (size_t)n * R + r;
  const uint32_t hw = mpost_pixels(p.im_size, n);
  const int cnt = mpost_count(is_b ? p.b_count : p.a_count, n, R);
  const int n_runs = r < cnt ? min(max((is_b ? p.b_n_runs : p.a_n_runs)[row], 0), stride) : 0;
  const uint32_t* runs = (is_b ? p.b_runs : p.a_runs) + row * stride;
  uint32_t* ends = is_b ? nullptr : p.a_ends + row * stride;
  uint2* tab = is_b ? p.b_tab + row * stride : nullptr;

  long long pos = 0;
  uint32_t prev_end = 0, ones = 0;
  for (int j0 = 0; j0 < n_runs; j0 += kMpostWave) {
    const int j = j0 + lane;
    uint32_t s, e;
    mpost_chunk_ends(runs, n_runs, j0, lane, hw, pos, prev_end, s, e);
    const uint32_t mine = (j < n_runs && (j & 1)) ? e - s : 0u;
    const uint32_t acc = ones + wave_incl_scan(mine, lane);
    if (j < n_runs) {
      if (is_b) tab[j] = make_uint2(e, acc); else ends[j] = e;
    }
    ones = __shfl(acc, kMpostWave - 1, kMpostWave);
  }
  if (lane == 0) {
    if (is_b) { p.b_n[row] = n_runs; p.b_area[row] = (int32_t)ones; }
    else { p.a_n[row] = n_runs; p.a_area[row] = (int32_t)ones; }
  }
}

// the set pixels of b in front of position x: tab holds n (end, ones up to the end) pairs with non-decreasing ends
__device__ __forceinline__ uint32_t mpost_ones_before(const uint2* tab, int n, uint32_t x) {
  int lo = 0, hi = n;                                        // the first run whose end is above x
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tab[mid].x > x) hi = mid; else lo = mid + 1;
  }
  if (lo == 0) return 0u;                                    // inside the leading zeros (or no runs at all)
  const uint2 before = tab[lo - 1];
  return before.y + ((lo < n && (lo & 1)) ? x - before.x : 0u);    // past the last run: zeros
}

__global__ __launch_bounds__(kMpostWave * kMpostPairWaves) void mpost_pair_kernel(MpostOverlapsParams p) {
  const int lane = threadIdx.x & (kMpostWave - 1), wave = threadIdx.x / kMpostWave;
  const int a = blockIdx.x, n = blockIdx.y;
  const size_t arow = (size_t)n * p.Ra + a;
  const int n_a = p.a_n[arow];                               // 0 past the count
  const uint32_t aa = (uint32_t)p.a_area[arow];
  const uint32_t* aends = p.a_ends + arow * p.a_stride;
  for (int b = wave; b < p.Rb; b += kMpostPairWaves) {       // one wave per pair
    const size_t brow = (size_t)n * p.Rb + b;
    const uint32_t ab = (uint32_t)p.b_area[brow];
    uint32_t inter = 0;
    if (aa && ab) {
      const int n_b = p.b_n[brow];
      const uint2* tab = p.b_tab + brow * p.b_stride;
      for (int j = 2 * lane + 1; j < n_a; j += 2 * kMpostWave) {          // the one-runs are the odd ones
        const uint32_t s = aends[j - 1], e = aends[j];
        if (e > s) inter += mpost_ones_before(tab, n_b, e) - mpost_ones_before(tab, n_b, s);
      }
      inter = wave_sum(inter);
    }
    double out = 0.0;
    if (inter) {
      const uint32_t u = p.crowd ? aa : aa + ab - inter;
      out = (double)inter / (double)u;
    }
    if (lane == 0) p.ovr[arow * p.Rb + b] = out;
  }
}

struct MpostOverlapsLayout { size_t a_ends, b_tab, a_n, b_n, total; };

__host__ inline MpostOverlapsLayout mpost_overlaps_layout(int batch, int Ra, int a_stride, int Rb, int b_stride) {
  Carve c{16};
  MpostOverlapsLayout l;
  l.b_tab = c.take((size_t)batch * Rb * b_stride * sizeof(uint2));
  l.a_ends = c.take((size_t)batch * Ra * a_stride * sizeof(uint32_t));
  l.a_n = c.take((size_t)batch * Ra * sizeof(int32_t));
  l.b_n = c.take((size_t)batch * Rb * sizeof(int32_t));
  l.total = c.end;
  return l;
}

}  // namespace dtc

DTC_API const char* dtc_mpost_target_arch(void) { return "gfx950"; }

DTC_API int dtc_mpost_boxes(const uint32_t* runs, const int32_t* n_runs, const int32_t* counts, const float* im_size, int batch,
                            int rows_stride, int runs_stride, int32_t* boxes, int32_t* area, int32_t* nonempty, dtc_stream_t stream) {
  // shapes, then limits
  const int shape = dtc::mpost_rows_shape(batch, rows_stride, runs_stride);
  if (shape != DTC_OK) return shape;
  // pointers
  if (!runs || !n_runs || !im_size || !boxes || !area || !nonempty) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(boxes) & 15) != 0) return DTC_EINVAL;       // a box is one 16-byte store
  dtc::MpostBoxesParams p{};
  p.runs = runs; p.n_runs = n_runs; p.counts = counts; p.im_size = im_size; p.R = rows_stride; p.stride = runs_stride;
  p.boxes = boxes; p.area = area; p.nonempty = nonempty;
  hipLaunchKernelGGL(dtc::mpost_boxes_kernel, dim3(rows_stride, batch), dim3(dtc::kMpostWave), 0, reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}

DTC_API size_t dtc_mpost_overlaps_workspace_bytes(int batch, int a_rows, int a_runs_stride, int b_rows, int b_runs_stride) {
  if (dtc::mpost_rows_shape(batch, a_rows, a_runs_stride) != DTC_OK || dtc::mpost_rows_shape(batch, b_rows, b_runs_stride) != DTC_OK) return 0;
  return dtc::mpost_overlaps_layout(batch, a_rows, a_runs_stride, b_rows, b_runs_stride).total;
}

DTC_API int dtc_mpost_overlaps(const uint32_t* a_runs, const int32_t* a_n_runs, const int32_t* a_count, const uint32_t* b_runs,
                               const int32_t* b_n_runs, const int32_t* b_count, const float* im_size, int batch, int a_rows,
                               int a_runs_stride, int b_rows, int b_runs_stride, int crowd, void* workspace, size_t workspace_bytes,
                               double* ovr, int32_t* a_area, int32_t* b_area, dtc_stream_t stream) {
  // shapes, then limits
  const int shape = dtc::mpost_worst(dtc::mpost_rows_shape(batch, a_rows, a_runs_stride), dtc::mpost_rows_shape(batch, b_rows, b_runs_stride));
  if (shape != DTC_OK) return shape;
  // pointers
  if (!a_runs || !a_n_runs || !a_count || !b_runs || !b_n_runs || !b_count || !im_size || !ovr || !a_area || !b_area) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return DTC_EINVAL;
  // workspace
  const dtc::MpostOverlapsLayout l = dtc::mpost_overlaps_layout(batch, a_rows, a_runs_stride, b_rows, b_runs_stride);
  if (!workspace || workspace_bytes < l.total) return DTC_EWORKSPACE;

  char* ws = static_cast<char*>(workspace);
  dtc::MpostOverlapsParams p{};
  p.a_runs = a_runs; p.a_n_runs = a_n_runs; p.a_count = a_count; p.b_runs = b_runs; p.b_n_runs = b_n_runs; p.b_count = b_count;
  p.im_size = im_size; p.Ra = a_rows; p.a_stride = a_runs_stride; p.Rb = b_rows; p.b_stride = b_runs_stride; p.crowd = crowd != 0;
  p.a_ends = reinterpret_cast<uint32_t*>(ws + l.a_ends); p.b_tab = reinterpret_cast<uint2*>(ws + l.b_tab);
  p.a_n = reinterpret_cast<int32_t*>(ws + l.a_n); p.b_n = reinterpret_cast<int32_t*>(ws + l.b_n);
  p.ovr = ovr; p.a_area = a_area; p.b_area = b_area;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::mpost_prepare_kernel, dim3(a_rows + b_rows, batch), dim3(dtc::kMpostWave), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::mpost_pair_kernel, dim3(a_rows, batch), dim3(dtc::kMpostWave * dtc::kMpostPairWaves), 0, s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
