// The greedy walk of rle_mask_nms on a given overlap matrix (include/detectorch_mpost_hip.h, entry 3).  One workgroup per image, one
// thread per row (R <= 512):
//   1  the rank of a row is the number of rows that come in front of it -- higher score; equal score and lower index; any number in
//      front of a NaN -- counted against the scores in LDS: a stable descending argsort without a sort.
//   2  the walk, one position per step: the first position alive is kept; every later position alive of the same class reads its own
//      value against the kept row and drops out unless value <= thresh.  One barrier per step.
// Comparisons only: the same bits on every run.
#include "mpost_common.h"

namespace dtc {

constexpr int kMpostNmsThreads = DTC_MPOST_MAX_ROWS;

struct MpostNmsParams {
  const float* dets; const int32_t* count; const double* ovr;
  int R, mode;
  double thresh;
  int32_t* keep; int32_t* keep_count;
};

// row a (score sa, index ia) is walked in front of row b
__device__ __forceinline__ bool mpost_nms_before(float sa, int ia, float sb, int ib) {
  const bool na = sa != sa, nb = sb != sb;
  if (na != nb) return nb;                                   // a number in front of a NaN
  if (!na && sa != sb) return sa > sb;
  return ia < ib;                                            // equal scores, two NaN: row order
}

__global__ __launch_bounds__(kMpostNmsThreads) void mpost_nms_kernel(MpostNmsParams p) {
  __shared__ float s_score[kMpostNmsThreads], s_cls[kMpostNmsThreads];
  __shared__ int s_order[kMpostNmsThreads], s_alive[kMpostNmsThreads];
  const int n = blockIdx.x, tid = threadIdx.x, R = p.R;
  const int cnt = min(max(p.count[n], 0), R);
  const float* dets = p.dets + (size_t)n * R * 6;
  const double* ovr = p.ovr + (size_t)n * R * R;
  int32_t* keep = p.keep + (size_t)n * R;

  if (tid < cnt) { s_score[tid] = dets[tid * 6 + 4]; s_cls[tid] = dets[tid * 6 + 5]; }
  s_alive[tid] = 1;
  __syncthreads();
  if (tid < cnt) {
    const float mine = s_score[tid];
    int rank = 0;
    for (int j = 0; j < cnt; j++) rank += mpost_nms_before(s_score[j], j, mine, tid) ? 1 : 0;
    s_order[rank] = tid;                                     // the ranks of cnt rows are 0 .. cnt - 1, each once
  }
  __syncthreads();

  const int j = tid < cnt ? s_order[tid] : 0;                // the row at this thread's position of the walk
  const float cj = s_cls[j];
  int kept = 0;
  for (int pos = 0; pos < cnt; pos++) {
    if (s_alive[pos]) {                                      // uniform: written before the barrier of an earlier step
      const int i = s_order[pos];
      if (tid == 0) keep[kept] = i;
      kept++;
      if (tid > pos && tid < cnt && s_alive[tid] && s_cls[i] == cj) {
        double v = ovr[(size_t)i * R + j];
        if (p.mode == DTC_MPOST_NMS_IOMA) {                  // np.maximum: NaN if either is
          const double w = ovr[(size_t)j * R + i];
          v = v != v ? v : (w != w ? w : (v > w ? v : w));
        }
        if (!(v <= p.thresh)) s_alive[tid] = 0;
      }
    }
    __syncthreads();
  }
  if (tid >= kept && tid < R) keep[tid] = -1;
  if (tid == 0) p.keep_count[n] = kept;
}

}  // namespace dtc

DTC_API int dtc_mpost_nms(const float* dets, const int32_t* count, const double* ovr, int batch, int rows_stride, double thresh, int mode,
                          int32_t* keep, int32_t* keep_count, dtc_stream_t stream) {
  // shapes and parameters, then limits
  const int shape = dtc::mpost_rows_shape(batch, rows_stride, 1);
  if (shape == DTC_EINVAL || mode < DTC_MPOST_NMS_IOU || mode > DTC_MPOST_NMS_CONTAINMENT) return DTC_EINVAL;
  if (shape != DTC_OK) return shape;
  // pointers
  if (!dets || !count || !ovr || !keep || !keep_count) return DTC_EINVAL;
  dtc::MpostNmsParams p{};
  p.dets = dets; p.count = count; p.ovr = ovr; p.R = rows_stride; p.mode = mode; p.thresh = thresh; p.keep = keep; p.keep_count = keep_count;
  hipLaunchKernelGGL(dtc::mpost_nms_kernel, dim3(batch), dim3(dtc::kMpostNmsThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
