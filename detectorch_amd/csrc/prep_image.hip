// Network-input preparation on the device (the caller side of the hot path).
//
// Reference: prep_im_for_blob + im_list_to_blob, lib/utils/blob.py:62-87 and :27-59 (driven by lib/utils/preprocess_sample.py:
// 25-34): BGR image -> float32, minus the per-channel pixel means (:72-73), cv2.resize(fx = fy = im_scale, INTER_LINEAR)
// (:84-85), zero-padded to the batch's max shape rounded up to the FPN stride (:38-47), HWC -> CHW (:55-57).
// The resize arithmetic is OpenCV's (third-party, absent, unpinned: "parity unpinned" like A9): restated from its
// documented rule -- dsize = round(src * scale); src coordinate of a destination pixel = (d + 0.5) / scale - 0.5; float32
// weights (1 - f, f); taps clamped at the borders (f forced to 0); horizontal pass first, then vertical -- exactly the
// restatement oracle/oracle.c:orc_prep_image checks this kernel against.
//
// One launch for the whole batch: thread <-> one destination pixel (x fastest: coalesced stores into the three channel
// planes), 4 taps x 3 channels gathered from the interleaved source.  HBM-bound: reads h*w*3 source bytes (u8) once through
// L2, writes 3*Hb*Wb floats.
#include "prep_pixel.h"

namespace dtc {

// the per-pixel body is csrc/prep_pixel.h's, shared with the mirrored launch of csrc/flip/flip_prep.hip: here its no-flip form
__global__ __launch_bounds__(256) void prep_image_kernel(const PrepParams p) {
  prep_pixel<false>(p, blockIdx.z, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}

}  // namespace dtc

// blob.py:75-82 -- the scale of one image; Python float (double) arithmetic, np.round = round half to even
static double prep_scale(int h, int w, int target_size, int max_size) {
  const int mn = h < w ? h : w, mx = h < w ? w : h;
  double s = (double)target_size / (double)mn;
  if (nearbyint(s * (double)mx) > (double)max_size) s = (double)max_size / (double)mx;
  return s;
}

DTC_API int dtc_prep_plan(const int32_t* heights, const int32_t* widths, int batch, int target_size, int max_size,
                          int pad_stride, double* im_scales, int32_t* out_hw, int32_t* blob_hw) {
  if (!heights || !widths || batch < 1 || target_size < 1 || max_size < 1 || !im_scales || !out_hw || !blob_hw)
    return DTC_EINVAL;
  int mh = 0, mw = 0;
  for (int b = 0; b < batch; b++) {
    if (heights[b] < 1 || widths[b] < 1) return DTC_EINVAL;
    const double s = prep_scale(heights[b], widths[b], target_size, max_size);
    im_scales[b] = s;
    // cv::resize: dsize = (saturate_cast<int>(w * fx), saturate_cast<int>(h * fy)) -- round half to even
    const int ow = (int)nearbyint((double)widths[b] * s), oh = (int)nearbyint((double)heights[b] * s);
    out_hw[2 * b] = oh < 1 ? 1 : oh; out_hw[2 * b + 1] = ow < 1 ? 1 : ow;
    if (out_hw[2 * b] > mh) mh = out_hw[2 * b];
    if (out_hw[2 * b + 1] > mw) mw = out_hw[2 * b + 1];
  }
  if (pad_stride > 1) {                       // blob.py:41-44
    mh = (mh + pad_stride - 1) / pad_stride * pad_stride;
    mw = (mw + pad_stride - 1) / pad_stride * pad_stride;
  }
  blob_hw[0] = mh; blob_hw[1] = mw;
  return DTC_OK;
}

DTC_API int dtc_prep_images(const dtc_image* images, int batch, const double* pixel_means, const double* im_scales,
                            const int32_t* out_hw, float* blob, int blob_h, int blob_w, dtc_stream_t stream) {
  dtc::PrepParams p;
  const int rc = dtc::prep_fill_params(images, batch, pixel_means, im_scales, out_hw, nullptr, blob, blob_h, blob_w, &p);
  if (rc != DTC_OK) return rc;
  hipLaunchKernelGGL(dtc::prep_image_kernel, dim3((blob_w + 255) / 256, blob_h, batch), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
