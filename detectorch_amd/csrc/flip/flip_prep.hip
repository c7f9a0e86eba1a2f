// The network input of a batch with mirrored images (include/detectorch_flip_hip.h, entry 1): csrc/prep_image.hip's launch with the
// flip form of the shared per-pixel body (csrc/prep_pixel.h).  The mirror costs nothing: it is folded into the tap addresses, so the
// launch reads and writes the bytes of the unflipped one.
#include "prep_pixel.h"

#include "../../../include/detectorch_flip_hip.h"

namespace dtc {

__global__ __launch_bounds__(256) void flip_prep_image_kernel(const PrepParams p) {
  prep_pixel<true>(p, blockIdx.z, blockIdx.x * blockDim.x + threadIdx.x, blockIdx.y);
}

}  // namespace dtc

DTC_API const char* dtc_flip_target_arch(void) { return "gfx950"; }

DTC_API int dtc_flip_prep_images(const dtc_image* images, int batch, const int32_t* flipped, const double* pixel_means,
                                 const double* im_scales, const int32_t* out_hw, float* blob, int blob_h, int blob_w,
                                 dtc_stream_t stream) {
  if (!flipped) return DTC_EINVAL;
  dtc::PrepParams p;
  const int rc = dtc::prep_fill_params(images, batch, pixel_means, im_scales, out_hw, flipped, blob, blob_h, blob_w, &p);
  if (rc != DTC_OK) return rc;
  hipLaunchKernelGGL(dtc::flip_prep_image_kernel, dim3((blob_w + 255) / 256, blob_h, batch), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
