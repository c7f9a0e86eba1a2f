// The hard-NMS pair test of cython_nms.pyx:76-84, `inter / (iarea + areas[j] - inter) >= thresh` with an IEEE float32 division,
// decided WITHOUT dividing for all but about one pair in 10^6.
//
// Rounding is monotone, so the rounded quotient is >= thresh whenever the exact one is, and < thresh whenever the exact one is below
// thresh * (1 - 2^-24): the division itself is needed only if inter - thresh * u cannot be signed reliably.
// d = fl(inter - fl(thresh * u)) carries <= 2^-23 * pu of error, so outside the band |d| <= 2^-21 * pu its sign IS the answer: five
// instructions and ONE compare per pair, and that compare can be the ballot mask itself.  u <= 0 (degenerate boxes), thresh <= 0 and
// the band take the division, exactly like the reference; callers decide that per wavefront (a uniform branch).
//
// Users: det_candidates' in-workgroup NMS (detections.hip) calls iou_band; nms_mask_kernel (nms.hip) spells the same five operations
// out in its hand-unrolled row loop with v_min_f32 in inline assembly (it is written for instruction count) and points here.
#pragma once
#include "dtc_common.h"

namespace dtc {

__device__ __forceinline__ float box_area(float4 b) { return (b.z - b.x + 1.f) * (b.w - b.y + 1.f); }  // cython_nms.pyx:44

// u = union area, d = inter - thresh * u (returned: d > 0 <=> suppressed, when the answer is sure).  True: the pair is inside the
// band or u <= 0 -- decide it by fdiv(inter, u) >= thresh.
__device__ __forceinline__ bool iou_band(float inter, float u, float thresh, float& d) {
  const float pu = thresh * u;
  d = inter - pu;
  const float t = __builtin_fabsf(d) - pu * 4.76837158203125e-07f;         // 2^-21 (exact scaling)
  return !(fminf(t, u) > 0.f);
}

}  // namespace dtc
