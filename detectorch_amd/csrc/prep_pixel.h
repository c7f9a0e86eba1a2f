// The per-pixel body of the network-input preparation, one text for its two kernels: csrc/prep_image.hip (dtc_prep_images, the
// image as it is) and csrc/flip/flip_prep.hip (dtc_flip_prep_images, images mirrored left to right where their flag says so).
// MAY_FLIP is a compile-time parameter: the no-flip form has no trace of the flag in its code.
//
// Reference: prep_im_for_blob + im_list_to_blob, lib/utils/blob.py:62-87 and :27-59; the mirror is image[:, ::-1, :] of
// lib/data/coco_dataset.py:51-53 in front of them.  The resize rule is restated in csrc/prep_image.hip's header.
#pragma once
#include "dtc_common.h"

namespace dtc {

struct PrepImage {
  const void* data;       // HWC, 3 channels (BGR), uint8 or float32
  int h, w, dtype, row_stride;   // row_stride in elements
  int oh, ow;             // resized size
  int flip;               // != 0: the source is read mirrored about the image's own width (read by the MAY_FLIP form only)
  float unused;           // (kept for alignment)
  double scale;           // im_scale (fx = fy)
};

constexpr int kPrepMaxBatch = 32;      // descriptor table travels as a kernel argument (~1.6 KB)

struct PrepParams {
  PrepImage im[kPrepMaxBatch];
  double mean[3];
  float* blob;            // [B, 3, Hb, Wb]
  int batch, Hb, Wb;
};

template <typename T>
__device__ __forceinline__ float px_minus_mean(const T* p, double mean) {
  return (float)((double)(*p) - mean);        // blob.py:72-73: float32 image -= float64 means (computed in double, stored float32)
}

// One destination pixel (x, y) of image b: thread <-> pixel, x fastest.  With MAY_FLIP and I.flip the taps and weights are those of
// the mirrored image -- destination x gives (sx, sx1, fx) exactly as without the flip -- and the source columns are w - 1 - sx and
// w - 1 - sx1: bit-equal to the no-flip form on image[:, ::-1, :].  The zero padding stays on the right.
template <bool MAY_FLIP>
__device__ __forceinline__ void prep_pixel(const PrepParams& p, int b, int x, int y) {
  const PrepImage& I = p.im[b];
  if (x >= p.Wb) return;
  float* out = p.blob + ((size_t)b * 3 * p.Hb + y) * p.Wb + x;
  const size_t plane = (size_t)p.Hb * p.Wb;
  if (y >= I.oh || x >= I.ow) {               // blob.py:45-49: zero padding
    out[0] = 0.f; out[plane] = 0.f; out[2 * plane] = 0.f;
    return;
  }
  const double inv = 1.0 / I.scale;           // cv::resize with fx given: scale_x = 1 / inv_scale_x
  float fy = (float)(((double)y + 0.5) * inv - 0.5);
  int sy = (int)floorf(fy); fy -= (float)sy;
  if (sy < 0) { sy = 0; fy = 0.f; }
  if (sy >= I.h - 1) { sy = I.h - 1; fy = 0.f; }
  const int sy1 = min(sy + 1, I.h - 1);
  float fx = (float)(((double)x + 0.5) * inv - 0.5);
  int sx = (int)floorf(fx); fx -= (float)sx;
  if (sx < 0) { sx = 0; fx = 0.f; }
  if (sx >= I.w - 1) { sx = I.w - 1; fx = 0.f; }
  int sx1 = min(sx + 1, I.w - 1);
  if (MAY_FLIP && I.flip) { sx = I.w - 1 - sx; sx1 = I.w - 1 - sx1; }
  const float ax0 = 1.f - fx, ay0 = 1.f - fy;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float v00, v01, v10, v11;
    if (I.dtype == DTC_U8) {
      const uint8_t* s = reinterpret_cast<const uint8_t*>(I.data);
      v00 = px_minus_mean(s + (size_t)sy * I.row_stride + sx * 3 + c, p.mean[c]);
      v01 = px_minus_mean(s + (size_t)sy * I.row_stride + sx1 * 3 + c, p.mean[c]);
      v10 = px_minus_mean(s + (size_t)sy1 * I.row_stride + sx * 3 + c, p.mean[c]);
      v11 = px_minus_mean(s + (size_t)sy1 * I.row_stride + sx1 * 3 + c, p.mean[c]);
    } else {
      const float* s = reinterpret_cast<const float*>(I.data);
      v00 = px_minus_mean(s + (size_t)sy * I.row_stride + sx * 3 + c, p.mean[c]);
      v01 = px_minus_mean(s + (size_t)sy * I.row_stride + sx1 * 3 + c, p.mean[c]);
      v10 = px_minus_mean(s + (size_t)sy1 * I.row_stride + sx * 3 + c, p.mean[c]);
      v11 = px_minus_mean(s + (size_t)sy1 * I.row_stride + sx1 * 3 + c, p.mean[c]);
    }
    const float r0 = v00 * ax0 + v01 * fx;    // horizontal pass
    const float r1 = v10 * ax0 + v11 * fx;
    out[c * plane] = r0 * ay0 + r1 * fy;      // vertical pass
  }
}

// The host side both entries share: the argument checks of dtc_prep_images and the descriptor table.  flipped: NULL (no image is
// mirrored) or a host array [batch].  -> DTC_OK, DTC_EINVAL or DTC_EUNSUPPORTED; nothing is enqueued here.
__host__ inline int prep_fill_params(const dtc_image* images, int batch, const double* pixel_means, const double* im_scales,
                                     const int32_t* out_hw, const int32_t* flipped, float* blob, int blob_h, int blob_w,
                                     PrepParams* p) {
  if (!images || batch < 1 || !pixel_means || !im_scales || !out_hw || !blob || blob_h < 1 || blob_w < 1) return DTC_EINVAL;
  if (batch > kPrepMaxBatch) return DTC_EUNSUPPORTED;
  for (int b = 0; b < batch; b++) {
    const dtc_image& s = images[b];
    if (!s.data || s.height < 1 || s.width < 1 || (s.dtype != DTC_U8 && s.dtype != DTC_F32) || s.row_stride < 3 * s.width ||
        out_hw[2 * b] > blob_h || out_hw[2 * b + 1] > blob_w)
      return DTC_EINVAL;
    PrepImage& d = p->im[b];
    d.data = s.data; d.h = s.height; d.w = s.width; d.dtype = s.dtype; d.row_stride = s.row_stride;
    d.oh = out_hw[2 * b]; d.ow = out_hw[2 * b + 1]; d.flip = flipped && flipped[b] ? 1 : 0; d.unused = 0.f; d.scale = im_scales[b];
  }
  for (int c = 0; c < 3; c++) p->mean[c] = pixel_means[c];
  p->blob = blob; p->batch = batch; p->Hb = blob_h; p->Wb = blob_w;
  return DTC_OK;
}

}  // namespace dtc
