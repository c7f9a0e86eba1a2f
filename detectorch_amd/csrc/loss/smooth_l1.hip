// lib/model/loss.py:13-20 smooth_L1(pred, targets, alpha_in, alpha_out, beta) with any weights, and its gradient, for gfx950.
// One pass over the FLAT arrays in 16-byte pieces (the row structure only sets the divisor), the < 4 left-over elements by the
// first threads; every element in double (loss_common.h).  The loss: a double per thread, block_sum, one partial result per
// workgroup, summed in index order by a second, one-workgroup node.  No atomics.
#include <algorithm>

#include "loss_common.h"

namespace dtc {

struct SmoothL1Params {
  const float* pred; const float* targets; const float* alpha_in; const float* alpha_out; const float* upstream;
  size_t total;
  int n;
  float beta;
  double* partial; float* grad;
};

__global__ __launch_bounds__(kLossThreads) void smooth_l1_kernel(SmoothL1Params p) {
  __shared__ double sh_d[kLossWaves];
  const double beta = (double)p.beta;
  const double gscale = (p.upstream ? (double)p.upstream[0] : 1.0) / (double)p.n;
  const size_t n4 = p.total >> 2, step = (size_t)gridDim.x * kLossThreads, first = (size_t)blockIdx.x * kLossThreads + threadIdx.x;
  double acc = 0.0;
  for (size_t i = first; i < n4; i += step) {
    const float4 a = reinterpret_cast<const float4*>(p.pred)[i], t = reinterpret_cast<const float4*>(p.targets)[i];
    const float4 wi = reinterpret_cast<const float4*>(p.alpha_in)[i], wo = reinterpret_cast<const float4*>(p.alpha_out)[i];
    double sx, sy, sz, sw;
    acc += smooth_l1_term(a.x, t.x, wi.x, wo.x, beta, &sx);
    acc += smooth_l1_term(a.y, t.y, wi.y, wo.y, beta, &sy);
    acc += smooth_l1_term(a.z, t.z, wi.z, wo.z, beta, &sz);
    acc += smooth_l1_term(a.w, t.w, wi.w, wo.w, beta, &sw);
    if (p.grad)
      reinterpret_cast<float4*>(p.grad)[i] =
          make_float4((float)(sx * gscale), (float)(sy * gscale), (float)(sz * gscale), (float)(sw * gscale));
  }
  const size_t j = 4 * n4 + first;                                      // the left-over elements: threads 0 .. 2 of workgroup 0
  if (j < p.total) {
    double sl;
    acc += smooth_l1_term(p.pred[j], p.targets[j], p.alpha_in[j], p.alpha_out[j], beta, &sl);
    if (p.grad) p.grad[j] = (float)(sl * gscale);
  }
  if (!p.partial) return;
  const double b = block_sum(acc, sh_d);
  if (threadIdx.x == 0) p.partial[blockIdx.x] = b;
}

__global__ __launch_bounds__(kLossThreads) void smooth_l1_sum_kernel(const double* partial, int n_partial, int n, float* loss) {
  __shared__ double sh_d[kLossWaves];
  double t = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += kLossThreads) t += partial[i];
  t = block_sum(t, sh_d);
  if (threadIdx.x == 0) loss[0] = (float)(t / (double)n);               // :20  / pred.size(0)
}

constexpr size_t kSmoothL1WsBytes = (size_t)kLossMaxBlocks * sizeof(double);

}  // namespace dtc

DTC_API size_t dtc_smooth_l1_workspace_bytes(int n, int w) {
  if (n < 1 || w < 1 || (int64_t)n * w > DTC_LOSS_MAX_ELEMS) return 0;
  return dtc::kSmoothL1WsBytes;
}

DTC_API int dtc_smooth_l1(const float* pred, const float* targets, const float* alpha_in, const float* alpha_out, int n, int w,
                          float beta, const float* upstream, void* workspace, size_t workspace_bytes, float* loss, float* grad_pred,
                          dtc_stream_t stream) {
  // shapes and parameters
  if (n < 1 || w < 1 || !std::isfinite(beta) || beta <= 0.f) return DTC_EINVAL;
  // limits
  if ((int64_t)n * w > DTC_LOSS_MAX_ELEMS) return DTC_EUNSUPPORTED;
  // pointers
  if (!pred || !targets || !alpha_in || !alpha_out || (!loss && !grad_pred)) return DTC_EINVAL;
  const uintptr_t al = reinterpret_cast<uintptr_t>(pred) | reinterpret_cast<uintptr_t>(targets) | reinterpret_cast<uintptr_t>(alpha_in) |
                       reinterpret_cast<uintptr_t>(alpha_out) | reinterpret_cast<uintptr_t>(grad_pred);
  if ((al & 15) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0) return DTC_EINVAL;
  if (loss && (!workspace || workspace_bytes < dtc::kSmoothL1WsBytes)) return DTC_EWORKSPACE;

  const size_t total = (size_t)n * (size_t)w;
  dtc::SmoothL1Params p{pred, targets, alpha_in, alpha_out, upstream, total, n, beta,
                        loss ? static_cast<double*>(workspace) : nullptr, grad_pred};
  const int blocks = (int)std::min<size_t>(std::max<size_t>((total / 4 + dtc::kLossThreads - 1) / dtc::kLossThreads, 1), dtc::kLossMaxBlocks);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::smooth_l1_kernel, dim3(blocks), dim3(dtc::kLossThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  if (loss) {
    hipLaunchKernelGGL(dtc::smooth_l1_sum_kernel, dim3(1), dim3(dtc::kLossThreads), 0, s, static_cast<const double*>(workspace), blocks, n,
                       loss);
    DTC_CHECK_LAUNCH();
  }
  return DTC_OK;
}
