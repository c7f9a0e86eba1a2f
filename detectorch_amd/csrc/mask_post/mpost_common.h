// What the kernels of libdetectorch_mpost_hip.so share (include/detectorch_mpost_hip.h has the contract): the sides of an image, the
// clipped run ends of a list, a workgroup scan.  Nothing read from a run list or a run count is used as an address: counts are
// clamped to the stride, positions to h * w.
#pragma once
#include "wave_ops.h"

#include "../../../include/detectorch_mpost_hip.h"

namespace dtc {

constexpr int kMpostWave = 64;

// one side of im_size as an integer: truncated; below 1, NaN: 0; above 2^30: 2^30 (dtc_segm_iou's rule)
__device__ __forceinline__ long long mpost_side(float v) {
  if (!(v >= 1.f)) return 0;
  return v >= (float)DTC_MPOST_MAX_PIXELS ? (long long)DTC_MPOST_MAX_PIXELS : (long long)(int)v;
}

// h * w clipped to 2^30
__device__ __forceinline__ uint32_t mpost_pixels(const float* im_size, int n) {
  const long long hw = mpost_side(im_size[2 * n]) * mpost_side(im_size[2 * n + 1]);
  return (uint32_t)(hw > DTC_MPOST_MAX_PIXELS ? DTC_MPOST_MAX_PIXELS : hw);
}

__device__ __forceinline__ int mpost_count(const int32_t* counts, int n, int R) { return counts ? min(max(counts[n], 0), R) : R; }

// One chunk of 64 runs of a list walked by one wave: run j = j0 + lane of n_runs.  -> this lane's clipped run start and end (equal
// where the run has no pixel inside the image or the lane is past the list); pos / prev_end carry the unclipped and the clipped end
// of the runs in front of the chunk.
__device__ __forceinline__ void mpost_chunk_ends(const uint32_t* runs, int n_runs, int j0, int lane, uint32_t hw, long long& pos,
                                                 uint32_t& prev_end, uint32_t& start, uint32_t& end) {
  const int j = j0 + lane;
  const long long len = j < n_runs ? (long long)runs[j] : 0ll;
  const long long incl = pos + wave_incl_scan(len, lane);
  end = (uint32_t)(incl < (long long)hw ? incl : (long long)hw);
  start = __shfl_up(end, 1, kMpostWave);
  if (lane == 0) start = prev_end;
  pos = __shfl(incl, kMpostWave - 1, kMpostWave);
  prev_end = __shfl(end, kMpostWave - 1, kMpostWave);
}

template <typename T> __device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = kMpostWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kMpostWave);
  return v;
}
__device__ __forceinline__ uint32_t wave_min(uint32_t v) {
#pragma unroll
  for (int off = kMpostWave / 2; off > 0; off >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, off, kMpostWave));
  return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int off = kMpostWave / 2; off > 0; off >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, off, kMpostWave));
  return v;
}

// the first run of n whose clipped end lies above position x (n: x is past the last run); ends are non-decreasing
__device__ __forceinline__ int mpost_run_at(const uint32_t* ends, int n, uint32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ends[mid] > x) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the shape of one side: images, rows per image, runs stride
__host__ inline int mpost_rows_shape(int batch, int R, int stride) {
  if (batch < 1 || R < 1 || stride < 1) return DTC_EINVAL;
  if (batch > DTC_MPOST_MAX_BATCH || R > DTC_MPOST_MAX_ROWS || stride > DTC_MPOST_MAX_RUNS) return DTC_EUNSUPPORTED;
  return DTC_OK;
}

// DTC_EINVAL in front of DTC_EUNSUPPORTED: shapes and parameters are checked before limits
__host__ inline int mpost_worst(int x, int y) { return (x == DTC_EINVAL || y == DTC_EINVAL) ? DTC_EINVAL : (x != DTC_OK ? x : y); }

__host__ inline bool mpost_overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb && y < x + na;
}

}  // namespace dtc
