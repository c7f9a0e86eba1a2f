// The two RPN losses fused with their dense gradient maps for gfx950 (include/detectorch_rpn_hip.h has the contract), read from the
// outputs of dtc_rpn_targets.  Kernel nodes:
//   1  rpn_loss_count   one workgroup: n_valid = sum_b (n_fg_b + n_bg_b) -- the divisor of every gradient element has to be known
//                       before the dense pass writes its first one
//   2  rpn_loss_dense   one anchor per thread and round over [B, N]: the label decides; a logit is read only where the label is 0 or 1
//                       (256 of the ~10^5 anchors of an image), every element of grad_cls_logits and -- as +0.0 -- of grad_bbox_pred
//                       is written; the cross-entropy terms add up per lane in double, block_sum, one partial result per workgroup
//   3  rpn_loss_rows    one workgroup: smooth-L1 over the <= B * F sampled foreground rows (the four predictions of a row are
//                       gathered through fg_index, its four gradient elements written over the zeros of node 2), then the partial
//                       results of node 2 in index order, and the two losses
// No float atomics and no arrival counters: the order of every sum is fixed by the launch shape, which depends on (N, B) alone, so a
// loss-only call gives the bits of the fused call.
#include <algorithm>

#include "loss/loss_common.h"
#include "rpn_train_common.h"

namespace dtc {

constexpr int kRpnLossMaxBlocks = 512;        // workgroups per image of the dense pass

struct RpnLossLevels {
  const float* cls[kRpnMaxLevels]; const float* box[kRpnMaxLevels]; float* g_cls[kRpnMaxLevels]; float* g_box[kRpnMaxLevels];
};

struct RpnLossWs {
  int32_t* ctrl;        // [0] n_valid
  double* part;         // [B * blocks per image]
  static size_t bytes(int B, int nb) { return 16 + (size_t)B * nb * 8; }
  RpnLossWs() = default;
  explicit RpnLossWs(void* ws) : ctrl(static_cast<int32_t*>(ws)), part(reinterpret_cast<double*>(static_cast<char*>(ws) + 16)) {}
};

struct RpnLossParams {
  RpnTrainPlan plan;
  RpnLossLevels lv;
  const int32_t* labels; const int32_t* fg_index; const float* fg_targets; const int32_t* n_fg; const int32_t* n_bg;
  const float* upstream;
  int B, F, want_g_cls, want_g_box;
  float beta;
  RpnLossWs ws;
  float* losses; int32_t* n_valid;
};

__device__ __forceinline__ int rpn_rows_fg(const RpnLossParams& p, int b) { return min(max(p.n_fg[b], 0), p.F); }
__device__ __forceinline__ int rpn_rows_valid(const RpnLossParams& p, int b) { return rpn_rows_fg(p, b) + max(p.n_bg[b], 0); }

__global__ __launch_bounds__(kLossThreads) void rpn_loss_count_kernel(RpnLossParams p) {
  __shared__ int sh_i[kLossWaves];
  int c = 0;
  for (int b = threadIdx.x; b < p.B; b += kLossThreads) c += rpn_rows_valid(p, b);
  c = block_sum(c, sh_i);
  if (threadIdx.x == 0) { p.ws.ctrl[0] = c; p.n_valid[0] = c; }
}

__global__ __launch_bounds__(kLossThreads) void rpn_loss_dense_kernel(RpnLossParams p) {
  __shared__ double sh_d[kLossWaves];
  const int b = blockIdx.y, N = p.plan.N;
  const int n_valid = p.ws.ctrl[0];
  const double scale = (p.upstream ? (double)p.upstream[0] : 1.0) / (double)max(n_valid, 1);
  double acc = 0.0;
  for (int i = blockIdx.x * kLossThreads + threadIdx.x; i < N; i += gridDim.x * kLossThreads) {
    const int label = p.labels[(size_t)b * N + i];
    const RpnCell c = rpn_cell_of(p.plan, i);
    const size_t hw = (size_t)p.plan.H[c.l] * p.plan.W[c.l];
    const size_t cell = (size_t)c.h * p.plan.W[c.l] + c.w;
    const size_t at = ((size_t)b * p.plan.A[c.l] + c.a) * hw + cell;          // [B, A, H, W]
    float g = 0.f;
    if (label == 0 || label == 1) {
      const double x = (double)p.lv.cls[c.l][at], y = (double)label;
      const double e = exp(-fabs(x));
      acc += (fmax(x, 0.0) - x * y) + log1p(e);
      const double sig = x >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
      g = (float)((sig - y) * scale);
    }
    if (p.want_g_cls) p.lv.g_cls[c.l][at] = g;
    if (p.want_g_box) {
      float* dst = p.lv.g_box[c.l] + ((size_t)b * 4 * p.plan.A[c.l] + 4 * c.a) * hw + cell;   // [B, 4A, H, W], channel 4a + k
#pragma unroll
      for (int k = 0; k < 4; k++) dst[k * hw] = 0.f;
    }
  }
  acc = block_sum(acc, sh_d);
  if (threadIdx.x == 0) p.ws.part[(size_t)b * gridDim.x + blockIdx.x] = acc;
}

__global__ __launch_bounds__(kLossThreads) void rpn_loss_rows_kernel(RpnLossParams p, int n_part) {
  __shared__ double sh_d[kLossWaves];
  const int N = p.plan.N, tid = threadIdx.x;
  const double up = p.upstream ? (double)p.upstream[1] : 1.0, beta = (double)p.beta;
  double acc = 0.0;
  for (int64_t r = tid; r < (int64_t)p.B * p.F; r += kLossThreads) {
    const int b = (int)(r / p.F), j = (int)(r % p.F);
    if (j >= rpn_rows_fg(p, b)) continue;
    const int i = p.fg_index[r];
    if (i < 0 || i >= N) continue;                                            // never an address
    const RpnCell c = rpn_cell_of(p.plan, i);
    const size_t hw = (size_t)p.plan.H[c.l] * p.plan.W[c.l];
    const size_t at = ((size_t)b * 4 * p.plan.A[c.l] + 4 * c.a) * hw + (size_t)c.h * p.plan.W[c.l] + c.w;
    const double div = (double)max(rpn_rows_valid(p, b), 1);
    const float* t = p.fg_targets + 4 * r;
    double row = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      double slope;
      row += smooth_l1_term(p.lv.box[c.l][at + k * hw], t[k], 1.f, 1.f, beta, &slope);
      if (p.want_g_box) p.lv.g_box[c.l][at + k * hw] = (float)(slope * up / (div * (double)p.B));
    }
    acc += row / div;
  }
  const double t_box = block_sum(acc, sh_d);
  double t_cls = 0.0;
  for (int q = tid; q < n_part; q += kLossThreads) t_cls += p.ws.part[q];
  t_cls = block_sum(t_cls, sh_d);
  if (tid == 0) {
    p.losses[0] = (float)(t_cls / (double)max(p.ws.ctrl[0], 1));
    p.losses[1] = (float)(t_box / (double)p.B);
  }
}

static int rpn_loss_blocks(int N) { return std::min(ceil_div(N, kLossThreads), kRpnLossMaxBlocks); }

}  // namespace dtc

DTC_API size_t dtc_rpn_loss_workspace_bytes(const dtc_rpn_train_level* levels, int n_levels, int batch) {
  dtc::RpnTrainPlan plan;
  if (batch < 1 || batch > 65535 || dtc::make_rpn_train_plan(levels, n_levels, &plan, nullptr) != DTC_OK) return 0;
  return dtc::RpnLossWs::bytes(batch, dtc::rpn_loss_blocks(plan.N));
}

DTC_API int dtc_rpn_loss(const dtc_rpn_train_level* levels, int n_levels, int batch, const int32_t* labels, const int32_t* fg_index,
                         const float* fg_targets, const int32_t* n_fg, const int32_t* n_bg, int fg_stride, float beta,
                         const float* upstream, void* workspace, size_t workspace_bytes, float* losses, int32_t* n_valid,
                         dtc_stream_t stream) {
  // shapes and parameters, then limits
  if (batch < 1 || fg_stride < 0 || !std::isfinite(beta) || beta <= 0.f || !levels || n_levels < 1) return DTC_EINVAL;
  dtc::RpnLossParams p{};
  const int rc = dtc::make_rpn_train_plan(levels, n_levels, &p.plan, nullptr);
  if (rc != DTC_OK) return rc;
  if (batch > 65535 || fg_stride > DTC_RPN_TRAIN_MAX_BATCH_PER_IM) return DTC_EUNSUPPORTED;
  // pointers
  if (!labels || !n_fg || !n_bg || !losses || !n_valid || (fg_stride > 0 && (!fg_index || !fg_targets))) return DTC_EINVAL;
  int n_g_cls = 0, n_g_box = 0;
  for (int l = 0; l < n_levels; l++) {
    const dtc_rpn_train_level& s = levels[l];
    if (!s.cls_logits || !s.bbox_pred) return DTC_EINVAL;
    n_g_cls += s.grad_cls_logits != nullptr;
    n_g_box += s.grad_bbox_pred != nullptr;
    p.lv.cls[l] = s.cls_logits; p.lv.box[l] = s.bbox_pred; p.lv.g_cls[l] = s.grad_cls_logits; p.lv.g_box[l] = s.grad_bbox_pred;
  }
  if ((n_g_cls != 0 && n_g_cls != n_levels) || (n_g_box != 0 && n_g_box != n_levels)) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return DTC_EINVAL;
  // workspace
  const int nb = dtc::rpn_loss_blocks(p.plan.N);
  if (!workspace || workspace_bytes < dtc::RpnLossWs::bytes(batch, nb)) return DTC_EWORKSPACE;

  p.labels = labels; p.fg_index = fg_index; p.fg_targets = fg_targets; p.n_fg = n_fg; p.n_bg = n_bg; p.upstream = upstream;
  p.B = batch; p.F = fg_stride; p.want_g_cls = n_g_cls != 0; p.want_g_box = n_g_box != 0;
  p.beta = beta;
  p.ws = dtc::RpnLossWs(workspace);
  p.losses = losses; p.n_valid = n_valid;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::rpn_loss_count_kernel, dim3(1), dim3(dtc::kLossThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::rpn_loss_dense_kernel, dim3(nb, batch), dim3(dtc::kLossThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::rpn_loss_rows_kernel, dim3(1), dim3(dtc::kLossThreads), 0, s, p, nb * batch);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
