// Boxes and polygons mirrored left to right per image (include/detectorch_flip_hip.h, entries 2 and 3).  One thread per group of four
// box columns / per polygon point; every thread reads what it writes before it writes, so the output may be the input itself.
#include "dtc_common.h"

#include "../../../include/detectorch_flip_hip.h"

namespace dtc {

// boxes f32 [B, R, cols]: thread <-> (b, r, group of four columns)
__global__ __launch_bounds__(256) void flip_boxes_kernel(const float* boxes, const int32_t* __restrict__ counts,
                                                         const int32_t* __restrict__ im_width, const int32_t* __restrict__ flipped,
                                                         int R, int groups, float* out) {
  const int b = blockIdx.y;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;        // (r, group)
  if (i >= (long long)R * groups) return;
  const int r = (int)(i / groups);
  const size_t at = ((size_t)b * R * groups + (size_t)i) * 4;
  float x1 = boxes[at], y1 = boxes[at + 1], x2 = boxes[at + 2], y2 = boxes[at + 3];
  const int n = counts ? min(max(counts[b], 0), R) : R;
  if (flipped[b] != 0 && r < n) {                              // roidb.py:114-117, float32, in this order
    const float w = (float)im_width[b];
    const float nx1 = w - x2 - 1.f, nx2 = w - x1 - 1.f;
    x1 = nx1; x2 = nx2;
  }
  out[at] = x1; out[at + 1] = y1; out[at + 2] = x2; out[at + 3] = y2;
}

// poly_xy f64 [B, PTS, 2]: thread <-> (b, point)
__global__ __launch_bounds__(256) void flip_polygons_kernel(const double* poly_xy, const int32_t* __restrict__ poly_ptr,
                                                            const int32_t* __restrict__ im_width, const int32_t* __restrict__ flipped,
                                                            int PTS, int NP, double* out64, float* __restrict__ out32) {
  const int b = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= PTS) return;
  const size_t at = ((size_t)b * PTS + i) * 2;
  double x = poly_xy[at];
  const double y = poly_xy[at + 1];
  if (flipped[b] != 0) {
    const int last = min(max(poly_ptr[(size_t)b * (NP + 1) + NP], 0), PTS);    // an offset is data: clamped before it is compared
    if (i < last) x = (double)im_width[b] - x - 1.0;           // segms.py:37-40, in double
  }
  if (out64) { out64[at] = x; out64[at + 1] = y; }
  if (out32) { out32[at] = (float)x; out32[at + 1] = (float)y; }   // the rounding of the double result
}

// the byte ranges [a, a + na) and [b, b + nb) share a byte
__host__ inline bool flip_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return na > 0 && nb > 0 && x < y + nb && y < x + na;
}

}  // namespace dtc

DTC_API int dtc_flip_boxes(const float* boxes, const int32_t* counts, const int32_t* im_width, const int32_t* flipped, int batch,
                           int rows_stride, int cols, float* out, dtc_stream_t stream) {
  const int R = rows_stride;
  if (batch < 1 || R < 0 || cols < 4 || cols % 4 != 0) return DTC_EINVAL;
  if (batch > DTC_FLIP_MAX_BATCH || R > DTC_FLIP_MAX_BOX_ROWS || cols > DTC_FLIP_MAX_BOX_COLS) return DTC_EUNSUPPORTED;
  if (!im_width || !flipped) return DTC_EINVAL;
  if (R == 0) return DTC_OK;
  if (!boxes || !out) return DTC_EINVAL;
  const size_t bytes = (size_t)batch * R * cols * sizeof(float);
  if (out != boxes && dtc::flip_overlap(boxes, bytes, out, bytes)) return DTC_EINVAL;
  const int groups = cols / 4;
  const long long per_image = (long long)R * groups;
  hipLaunchKernelGGL(dtc::flip_boxes_kernel, dim3((unsigned)((per_image + 255) / 256), batch), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), boxes, counts, im_width, flipped, R, groups, out);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}

DTC_API int dtc_flip_polygons(const double* poly_xy, const int32_t* poly_ptr, const int32_t* im_width, const int32_t* flipped, int batch,
                              int points_stride, int polys_stride, double* out64, float* out32, dtc_stream_t stream) {
  const int PTS = points_stride, NP = polys_stride;
  if (batch < 1 || PTS < 0 || NP < 0) return DTC_EINVAL;
  if (batch > DTC_FLIP_MAX_BATCH || PTS > DTC_FLIP_MAX_POINTS || NP > DTC_FLIP_MAX_POLYS) return DTC_EUNSUPPORTED;
  if (!im_width || !flipped || !poly_ptr || (!out64 && !out32)) return DTC_EINVAL;
  if (PTS == 0) return DTC_OK;
  if (!poly_xy) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(poly_xy) & 7) != 0 || (reinterpret_cast<uintptr_t>(out64) & 7) != 0 ||
      (reinterpret_cast<uintptr_t>(out32) & 3) != 0)
    return DTC_EINVAL;
  const size_t n = (size_t)batch * PTS * 2;
  if (out64 && out64 != poly_xy && dtc::flip_overlap(poly_xy, n * 8, out64, n * 8)) return DTC_EINVAL;
  if (out32 && dtc::flip_overlap(poly_xy, n * 8, out32, n * 4)) return DTC_EINVAL;
  if (out32 && out64 && dtc::flip_overlap(out64, n * 8, out32, n * 4)) return DTC_EINVAL;
  hipLaunchKernelGGL(dtc::flip_polygons_kernel, dim3((PTS + 255) / 256, batch), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     poly_xy, poly_ptr, im_width, flipped, PTS, NP, out64, out32);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
