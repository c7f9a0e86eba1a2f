// bbox_transform + clip_tiled_boxes of lib/utils/boxes.py (:168-208, :150-165) for one (box, class): the numpy flavour of the box
// decode, one float32 rounding per operation in the reference's order.  Used by the fused detection kernel (detections.hip, only
// for the candidates) and the stand-alone drop-in (bbox_ops.hip, every class).  proposals.hip keeps its own decode_box on purpose:
// the RPN path follows torch (NaN propagates through clamp), this one numpy (fminf / fmaxf drop a NaN operand).
#pragma once
#include "dtc_common.h"

namespace dtc {

// clip_tiled_boxes (:150-165) for one box: to the (im_h, im_w) image
__device__ __forceinline__ float4 clip_box(float4 b, float im_h, float im_w) {
  return make_float4(fmaxf(fminf(b.x, im_w - 1.f), 0.f), fmaxf(fminf(b.y, im_h - 1.f), 0.f),   // :158-164
                     fmaxf(fminf(b.z, im_w - 1.f), 0.f), fmaxf(fminf(b.w, im_h - 1.f), 0.f));
}

// bbox_transform (:168-208) for one (box, class).  (x1, y1, x2, y2): the box the deltas d[0..3] refer to; (wx, wy, ww, wh) =
// bbox_reg_weights; kClip: followed by clip_box.  (The clip is a template parameter and not an argument: a run-time flag that is
// constant at the call site still left det_candidates with another instruction schedule.)
template <bool kClip>
__device__ __forceinline__ float4 decode_clip(float x1, float y1, float x2, float y2, const float* d, float wx, float wy, float ww,
                                              float wh, float im_h, float im_w) {
  const float widths = x2 - x1 + 1.0f, heights = y2 - y1 + 1.0f;           // boxes.py:178-179
  const float ctr_x = x1 + 0.5f * widths, ctr_y = y1 + 0.5f * heights;     // :180-181
  const float dx = fdiv(d[0], wx), dy = fdiv(d[1], wy);                    // :184-185
  float dw = fdiv(d[2], ww), dh = fdiv(d[3], wh);                          // :186-187
  const float clipv = 4.135166556742356f;                                  // :73  np.log(1000. / 16.)
  dw = fminf(dw, clipv); dh = fminf(dh, clipv);                            // :190-191
  const float pcx = dx * widths + ctr_x, pcy = dy * heights + ctr_y;       // :193-194
  const float pw = fexp_cr(dw) * widths, ph = fexp_cr(dh) * heights;       // :195-196
  const float4 b = make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph,           // :200-202
                               pcx + 0.5f * pw - 1.f, pcy + 0.5f * ph - 1.f);  // :204-206
  if constexpr (kClip) return clip_box(b, im_h, im_w);
  return b;
}

}  // namespace dtc
