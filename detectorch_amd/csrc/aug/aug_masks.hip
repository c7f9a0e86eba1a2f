// dtc_aug_combine_masks (include/detectorch_aug_hip.h, entry 2): the mask-head probabilities T views give for the same detections
// -> one [K, M, M] map per detection, in ONE launch.  A pure stream: T reads and one write per combined element, one write per
// element that is not combined (a row past det_count, a channel that is not the row's class).  Where M is a multiple of 4 a thread
// owns four neighbouring elements of one map row: 16-byte loads -- the mirrored group x .. x + 3 of a flipped view is M - 4 - x .. M -
// 1 - x of the same row, a multiple of 4 again, read as 16 bytes and reversed in registers -- and one 16-byte store.  Otherwise (odd
// and other widths) a thread owns one element.  The views' pointers and flags travel by value in the kernel arguments.
#include "dtc_common.h"

#include "../../../include/detectorch_aug_hip.h"

namespace dtc {

constexpr int kAugMaskThreads = 256;

struct AugMaskParams {
  const float* m[DTC_AUG_MAX_VIEWS];
  int flip[DTC_AUG_MAX_VIEWS];
  const int32_t* det_count;
  const int32_t* mask_class;
  int T, max_out, K, M, heur;
  size_t total;              // B max_out K M M
  float* out;
};

// logit(y) of im_detect_mask_aug: float32 but for the log, which is evaluated in double and rounded once
__device__ __forceinline__ float aug_logit(float y) {
  const float q = fdiv(1.0f - y, fmaxf(y, 1e-20f));
  return -(float)log((double)q);
}

// One element over the views, in view order.  kHeur is a template parameter: three streams, no per-element branch.
template <int kHeur> struct AugAcc {
  float a;
  __device__ __forceinline__ void first(float v) { a = kHeur == DTC_AUG_LOGIT_AVG ? aug_logit(v) : v; }
  __device__ __forceinline__ void next(float v) {
    if (kHeur == DTC_AUG_SOFT_MAX) a = (v > a || v != v) ? v : a;          // np.amax: a NaN stays
    else a = a + (kHeur == DTC_AUG_LOGIT_AVG ? aug_logit(v) : v);
  }
  __device__ __forceinline__ float done(float fT) const {
    if (kHeur == DTC_AUG_SOFT_MAX) return a;
    const float mean = fdiv(a, fT);
    if (kHeur == DTC_AUG_SOFT_AVG) return mean;
    return fdiv(1.0f, 1.0f + (float)exp((double)(-mean)));
  }
};

// is (row, channel) combined?  rows past the image's count and channels other than the row's class are zeros
__device__ __forceinline__ bool aug_mask_live(const AugMaskParams& p, size_t plane) {
  const int row = (int)(plane / (size_t)p.K), k = (int)(plane % (size_t)p.K);
  const int b = row / p.max_out, r = row % p.max_out;
  if (r >= min(max(p.det_count[b], 0), p.max_out)) return false;
  return !p.mask_class || p.mask_class[row] == k;
}

template <int kHeur>
__global__ __launch_bounds__(kAugMaskThreads) void aug_masks4_kernel(AugMaskParams p) {     // M % 4 == 0
  const size_t g = (size_t)blockIdx.x * kAugMaskThreads + threadIdx.x;                       // group of four elements
  if (g >= p.total / 4) return;
  const int gpr = p.M / 4;                                  // groups per map row
  const size_t line = g / gpr;                              // (plane, y)
  const int x = (int)(g % gpr) * 4;
  float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
  if (aug_mask_live(p, line / p.M)) {
    AugAcc<kHeur> a0, a1, a2, a3;
#pragma unroll
    for (int t = 0; t < DTC_AUG_MAX_VIEWS; t++) {
      if (t >= p.T) break;
      const float* src = p.m[t] + line * p.M;
      float4 v;
      if (p.flip[t]) {
        const float4 w = *reinterpret_cast<const float4*>(src + (p.M - 4 - x));
        v = make_float4(w.w, w.z, w.y, w.x);
      } else {
        v = *reinterpret_cast<const float4*>(src + x);
      }
      if (t == 0) { a0.first(v.x); a1.first(v.y); a2.first(v.z); a3.first(v.w); }
      else { a0.next(v.x); a1.next(v.y); a2.next(v.z); a3.next(v.w); }
    }
    const float fT = (float)p.T;
    o = make_float4(a0.done(fT), a1.done(fT), a2.done(fT), a3.done(fT));
  }
  *reinterpret_cast<float4*>(p.out + g * 4) = o;
}

template <int kHeur>
__global__ __launch_bounds__(kAugMaskThreads) void aug_masks1_kernel(AugMaskParams p) {     // any M
  const size_t i = (size_t)blockIdx.x * kAugMaskThreads + threadIdx.x;
  if (i >= p.total) return;
  const size_t line = i / p.M;
  const int x = (int)(i % p.M);
  float o = 0.f;
  if (aug_mask_live(p, line / p.M)) {
    AugAcc<kHeur> a;
#pragma unroll
    for (int t = 0; t < DTC_AUG_MAX_VIEWS; t++) {
      if (t >= p.T) break;
      const float v = p.m[t][line * p.M + (p.flip[t] ? p.M - 1 - x : x)];
      if (t == 0) a.first(v); else a.next(v);
    }
    o = a.done((float)p.T);
  }
  p.out[i] = o;
}

template <int kHeur> static int aug_masks_launch(const AugMaskParams& p, hipStream_t s) {
  if (p.M % 4 == 0) {
    const size_t groups = p.total / 4;
    hipLaunchKernelGGL(aug_masks4_kernel<kHeur>, dim3((unsigned)((groups + kAugMaskThreads - 1) / kAugMaskThreads)), dim3(kAugMaskThreads),
                       0, s, p);
  } else {
    hipLaunchKernelGGL(aug_masks1_kernel<kHeur>, dim3((unsigned)((p.total + kAugMaskThreads - 1) / kAugMaskThreads)), dim3(kAugMaskThreads),
                       0, s, p);
  }
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}

}  // namespace dtc

DTC_API int dtc_aug_combine_masks(const float* const* masks, const int32_t* flipped, int n_views, const int32_t* det_count,
                                  const int32_t* mask_class, int batch, int max_out, int n_cls, int M, int heur, float* out,
                                  dtc_stream_t stream) {
  using namespace dtc;
  // shapes and parameters
  if (n_views < 1 || batch < 1 || max_out < 1 || n_cls < 1 || M < 1) return DTC_EINVAL;
  if (heur < DTC_AUG_SOFT_AVG || heur > DTC_AUG_LOGIT_AVG) return DTC_EINVAL;
  // limits
  if (n_views > DTC_AUG_MAX_VIEWS || M > DTC_AUG_MAX_MASK || n_cls > DTC_AUG_MAX_CHANNELS || batch > DTC_AUG_MAX_BATCH ||
      (long long)batch * max_out > DTC_AUG_MAX_MASK_ROWS)
    return DTC_EUNSUPPORTED;
  // pointers
  if (!masks || !flipped || !det_count || !out || (reinterpret_cast<uintptr_t>(out) & 15)) return DTC_EINVAL;
  AugMaskParams p;
  p.total = (size_t)batch * max_out * n_cls * M * M;        // <= 2^20 2^10 2^12 = 2^42 elements; a grid of <= 2^32 / 4 blocks below
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), bytes = p.total * sizeof(float);
  for (int t = 0; t < n_views; t++) {
    const uintptr_t m0 = reinterpret_cast<uintptr_t>(masks[t]);
    if (!masks[t] || (m0 & 15) || (flipped[t] != 0 && flipped[t] != 1)) return DTC_EINVAL;
    if (m0 < o0 + bytes && o0 < m0 + bytes) return DTC_EINVAL;
    p.m[t] = masks[t]; p.flip[t] = flipped[t];
  }
  for (int t = n_views; t < DTC_AUG_MAX_VIEWS; t++) { p.m[t] = masks[0]; p.flip[t] = 0; }
  if ((p.total + kAugMaskThreads - 1) / kAugMaskThreads > 0x7fffffffull) return DTC_EUNSUPPORTED;   // one element per thread at most
  p.det_count = det_count; p.mask_class = mask_class;
  p.T = n_views; p.max_out = max_out; p.K = n_cls; p.M = M; p.heur = heur;
  p.out = out;
  hipStream_t s = static_cast<hipStream_t>(stream);
  switch (heur) {
    case DTC_AUG_SOFT_AVG: return aug_masks_launch<DTC_AUG_SOFT_AVG>(p, s);
    case DTC_AUG_SOFT_MAX: return aug_masks_launch<DTC_AUG_SOFT_MAX>(p, s);
    default: return aug_masks_launch<DTC_AUG_LOGIT_AVG>(p, s);
  }
}
