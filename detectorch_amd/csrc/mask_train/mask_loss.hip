// The class-specific sigmoid cross-entropy of the mask branch fused with its dense gradient for gfx950
// (include/detectorch_mask_hip.h has the contract).  Kernel nodes, nb = min(Rm, kMaskLossMaxBlocks) workgroups, workgroup x takes
// the rows x, x + nb, ...:
//   1  mask_loss_count   the valid elements of the workgroup's rows -> one integer per workgroup: the divisor of every gradient
//                        element has to be known before the dense pass writes its first one
//   2  mask_loss_dense   the nb integers in index order -> n_valid; per row, the loss terms of the class channel (one element per
//                        thread and round, added per lane in double, block_sum, one partial result per workgroup), then the row's
//                        K * M * M gradient elements as ONE flat range: 16-byte stores between the first and the last 16-byte
//                        boundary of the range whatever M * M is, single words at its two ends; a vector that does not touch the
//                        class channel is four zeros without a load -- the store is the byte floor of the call
//   3  mask_loss_final   one workgroup: the partial results in index order, the loss, n_valid
// The loss terms never depend on the gradient pointer or its alignment, so a loss-only call gives the bits of the fused call.
#include <algorithm>

#include "loss/loss_common.h"

#include "../../../include/detectorch_mask_hip.h"

namespace dtc {

constexpr int kMaskLossMaxBlocks = 1024;      // workgroups of nodes 1 and 2 = partial results for the last sum

struct MaskLossWs {
  int32_t* ctrl;         // [0] n_valid
  double* part;          // [nb]
  int32_t* cnt;          // [nb]
  static size_t bytes(int nb) { return 16 + (size_t)nb * 16; }
  MaskLossWs() = default;
  MaskLossWs(void* ws, int nb) : ctrl(static_cast<int32_t*>(ws)), part(reinterpret_cast<double*>(static_cast<char*>(ws) + 16)),
                                 cnt(reinterpret_cast<int32_t*>(static_cast<char*>(ws) + 16 + (size_t)nb * 8)) {}
};

struct MaskLossParams {
  const float* logits; const int32_t* masks; const int32_t* cls; const float* upstream;
  int Rm, K, MM;
  MaskLossWs ws;
  float* loss; int32_t* n_valid; float* grad;
};

__device__ __forceinline__ bool mask_target_valid(int t) { return t == 0 || t == 1; }

__global__ __launch_bounds__(kLossThreads) void mask_loss_count_kernel(MaskLossParams p) {
  __shared__ int sh_i[kLossWaves];
  int c = 0;
  for (int r = blockIdx.x; r < p.Rm; r += gridDim.x) {
    const int k = p.cls[r];
    if (k < 0 || k >= p.K) continue;
    const int32_t* t = p.masks + (size_t)r * p.MM;
    for (int e = threadIdx.x; e < p.MM; e += kLossThreads) c += mask_target_valid(t[e]) ? 1 : 0;
  }
  c = block_sum(c, sh_i);
  if (threadIdx.x == 0) p.ws.cnt[blockIdx.x] = c;
}

// sigmoid(x) - t and the loss term of one valid element, in double
__device__ __forceinline__ double mask_term(float xf, int t, double* slope) {
  const double x = (double)xf, y = (double)t;
  const double e = exp(-fabs(x));
  *slope = (x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e)) - y;
  return (fmax(x, 0.0) - x * y) + log1p(e);
}

__global__ __launch_bounds__(kLossThreads) void mask_loss_dense_kernel(MaskLossParams p) {
  __shared__ double sh_d[kLossWaves];
  __shared__ int sh_i[kLossWaves];
  const int tid = threadIdx.x, MM = p.MM;
  int nv = 0;
  for (int q = tid; q < (int)gridDim.x; q += kLossThreads) nv += p.ws.cnt[q];
  nv = block_sum(nv, sh_i);
  const double scale = (p.upstream ? (double)p.upstream[0] : 1.0) / (double)max(nv, 1);
  const size_t row_elems = (size_t)p.K * MM;
  double acc = 0.0;
  for (int r = blockIdx.x; r < p.Rm; r += gridDim.x) {
    const int k = p.cls[r];
    const bool on = k >= 0 && k < p.K;
    const int32_t* t = p.masks + (size_t)r * MM;
    const float* x = p.logits + (size_t)r * row_elems + (size_t)(on ? k : 0) * MM;
    if (on) {
      for (int e = tid; e < MM; e += kLossThreads) {
        const int te = t[e];
        double slope;
        if (mask_target_valid(te)) acc += mask_term(x[e], te, &slope);
      }
    }
    if (!p.grad) continue;
    float* g = p.grad + (size_t)r * row_elems;
    const size_t c0 = on ? (size_t)k * MM : row_elems, c1 = c0 + (on ? MM : 0);       // the class channel inside the flat range
    auto value = [&](size_t f) -> float {                                           // the gradient element at flat index f
      if (f < c0 || f >= c1) return 0.f;
      const int e = (int)(f - c0), te = t[e];
      if (!mask_target_valid(te)) return 0.f;
      double slope;
      mask_term(x[e], te, &slope);
      return (float)(slope * scale);
    };
    const size_t to16 = ((16 - (reinterpret_cast<uintptr_t>(g) & 15)) & 15) >> 2;     // words before the first 16-byte boundary
    const size_t head = to16 < row_elems ? to16 : row_elems;
    const size_t n4 = (row_elems - head) >> 2, tail = head + 4 * n4;
    if ((size_t)tid < head) g[tid] = value(tid);
    if ((size_t)tid < row_elems - tail) g[tail + tid] = value(tail + tid);
    for (size_t v = tid; v < n4; v += kLossThreads) {
      const size_t f = head + 4 * v;
      float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
      if (f + 4 > c0 && f < c1) o = make_float4(value(f), value(f + 1), value(f + 2), value(f + 3));
      store_stream16(g + f, o);
    }
  }
  acc = block_sum(acc, sh_d);
  if (tid == 0) p.ws.part[blockIdx.x] = acc;
  if (tid == 0 && blockIdx.x == 0) p.ws.ctrl[0] = nv;
}

__global__ __launch_bounds__(kLossThreads) void mask_loss_final_kernel(MaskLossParams p, int nb) {
  __shared__ double sh_d[kLossWaves];
  double s = 0.0;
  for (int q = threadIdx.x; q < nb; q += kLossThreads) s += p.ws.part[q];
  s = block_sum(s, sh_d);
  if (threadIdx.x == 0) {
    const int nv = p.ws.ctrl[0];
    p.loss[0] = nv > 0 ? (float)(s / (double)nv) : 0.f;
    p.n_valid[0] = nv;
  }
}

static int mask_loss_blocks(int rows) { return std::min(rows, kMaskLossMaxBlocks); }

static int mask_loss_shapes(int rows, int K, int M) {
  if (rows < 1 || K < 1 || M < 1) return DTC_EINVAL;
  if (rows > DTC_MASK_MAX_LOSS_ROWS || K > DTC_MASK_MAX_CLASSES || M > DTC_MASK_MAX_M) return DTC_EUNSUPPORTED;
  return DTC_OK;
}

}  // namespace dtc

DTC_API size_t dtc_mask_loss_workspace_bytes(int rows, int K, int M) {
  if (dtc::mask_loss_shapes(rows, K, M) != DTC_OK) return 0;
  return dtc::MaskLossWs::bytes(dtc::mask_loss_blocks(rows));
}

DTC_API int dtc_mask_loss(const float* mask_logits, const int32_t* masks, const int32_t* mask_class, int rows, int K, int M,
                          const float* upstream, void* workspace, size_t workspace_bytes, float* loss, int32_t* n_valid,
                          float* grad_mask_logits, dtc_stream_t stream) {
  // shapes, then limits
  const int rc = dtc::mask_loss_shapes(rows, K, M);
  if (rc != DTC_OK) return rc;
  // pointers
  if (!mask_logits || !masks || !mask_class || !loss || !n_valid) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0 || (reinterpret_cast<uintptr_t>(grad_mask_logits) & 3) != 0) return DTC_EINVAL;
  // workspace
  const int nb = dtc::mask_loss_blocks(rows);
  if (!workspace || workspace_bytes < dtc::MaskLossWs::bytes(nb)) return DTC_EWORKSPACE;

  dtc::MaskLossParams p{};
  p.logits = mask_logits; p.masks = masks; p.cls = mask_class; p.upstream = upstream;
  p.Rm = rows; p.K = K; p.MM = M * M;
  p.ws = dtc::MaskLossWs(workspace, nb);
  p.loss = loss; p.n_valid = n_valid; p.grad = grad_mask_logits;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::mask_loss_count_kernel, dim3(nb), dim3(dtc::kLossThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::mask_loss_dense_kernel, dim3(nb), dim3(dtc::kLossThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::mask_loss_final_kernel, dim3(1), dim3(dtc::kLossThreads), 0, s, p, nb);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
