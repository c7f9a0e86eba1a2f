// The Fast R-CNN head losses with their gradients for gfx950, read from the compact targets of dtc_fast_rcnn_targets:
//   train_fast.py:147  cross_entropy(cls_score, cls_labels)          train_fast.py:148  smooth_L1(...)  (lib/model/loss.py:13-20)
//   train_fast.py:151  accuracy(cls_score, cls_labels)  (lib/model/loss.py:22-26)      train_fast.py:158  loss.backward()
// Two kernel nodes:
//   1  loss_count_kernel: one workgroup counts the rows with label >= 0 (the divisor of every gradient element has to be known
//      before the pass writes its first one) and clears the arrival counter of the pass.
//   2  fast_rcnn_loss_kernel<E>: ONE pass.  A row of C logits belongs to L = 1, 2, .. 64 neighbouring lanes of a wavefront
//      (the least power of two with 4 L >= C, 64 at the most: two rows per wavefront at C = 81), lane `sub` holding the columns
//      sub, sub + L, .. in registers (E = 4 of them, 16 for C > 256).  Row maximum with its lowest index, sum of exponentials
//      and the label's logit travel by xor butterflies inside the L lanes, so that every lane of a row ends with the same bits;
//      the exponentials stay in the registers and leave as the gradient: cls_score is read once, 4 bytes per lane and
//      instruction, neighbouring lanes neighbouring addresses (rows are 4-byte aligned only; nothing wider is assumed).
//      Lane 0 of the row reads the five compact targets and the 16 selected bytes of bbox_pred; the row's W gradient floats
//      leave as 16-byte stores from its L lanes, the zeros of the unselected classes included.
//      Sums over rows: per lane in double, block_sum, one partial result per workgroup; the last workgroup to arrive (one
//      agent-scope counter add per workgroup, nobody waits) sums the partial results in index order.
// No float atomics: the same bits on every run.
#include <algorithm>

#include "loss_common.h"

namespace dtc {

constexpr int kCountThreads = 1024;

// the workspace: [0] arrival counter, [1] n_valid, 16 bytes in all; then the partial results of the pass
struct LossWorkspace {
  int32_t* ctrl; double* part_cls; double* part_box; int32_t* part_ok;
  static constexpr size_t kBytes = 16 + (size_t)kLossMaxBlocks * (8 + 8 + 4);
  explicit LossWorkspace(void* ws) {
    char* b = static_cast<char*>(ws);
    ctrl = reinterpret_cast<int32_t*>(b);
    part_cls = reinterpret_cast<double*>(b + 16);
    part_box = part_cls + kLossMaxBlocks;
    part_ok = reinterpret_cast<int32_t*>(part_box + kLossMaxBlocks);
  }
};

struct LossParams {
  const float* cls_score; const int32_t* labels; const float* bbox_pred; const float* targets5; const float* upstream;
  int n, c, w, L;
  float beta;
  LossWorkspace ws;
  float* losses; float* grad_cls; float* grad_box;
};

__global__ __launch_bounds__(kCountThreads) void loss_count_kernel(const int32_t* labels, int n, int32_t* ctrl) {
  __shared__ int part[kCountThreads / 64];
  int cnt = 0;
  for (int i = threadIdx.x; i < n; i += kCountThreads) cnt += labels[i] >= 0 ? 1 : 0;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < kCountThreads / 64; w++) t += part[w];
    ctrl[1] = t;
    ctrl[0] = 0;
  }
}

template <int E>
__global__ __launch_bounds__(kLossThreads) void fast_rcnn_loss_kernel(LossParams p) {
  __shared__ double sh_d[kLossWaves];
  __shared__ int sh_i[kLossWaves];
  __shared__ int sh_last;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = p.L, sub = lane & (L - 1), lead = lane & ~(L - 1);         // lead: lane 0 of this lane's row
  const int rows_per_wave = 64 / L, rows_per_block = rows_per_wave * kLossWaves;
  const int row_in_block = wave * rows_per_wave + lead / L;
  const bool want_loss = p.losses != nullptr, want_grad = p.grad_cls != nullptr, has_box = p.bbox_pred != nullptr;
  const int n_valid = p.ws.ctrl[1];
  const float up_cls = p.upstream ? p.upstream[0] : 1.f;
  const double up_box = p.upstream ? (double)p.upstream[1] : 1.0;
  const float scale_cls = n_valid > 0 ? fdiv(up_cls, (float)n_valid) : 0.f;
  const double scale_box = n_valid > 0 ? up_box / (double)n_valid : 0.0;
  const double beta = (double)p.beta;
  const int C = p.c, W4 = p.w >> 2;
  const bool agnostic = p.w == 8;

  double acc_cls = 0.0, acc_box = 0.0;
  int acc_ok = 0;
  for (int base = blockIdx.x * rows_per_block; base < p.n; base += gridDim.x * rows_per_block) {
    const int row = base + row_in_block;
    const bool in = row < p.n;
    const int label = in ? p.labels[row] : -1;
    const bool row_ok = label >= 0, cls_ok = row_ok && label < C;      // the lanes of a row agree on both

    // ---- cross-entropy and accuracy.  A row without a usable label is never read: its lanes hold -inf and are masked below.
    float x[E];
    float m = -INFINITY;
    int am = 0x7fffffff;
    const float* src = p.cls_score + (size_t)row * C;
#pragma unroll
    for (int e = 0; e < E; e++) {
      const int j = e * L + sub;
      x[e] = (cls_ok && j < C) ? src[j] : -INFINITY;
      if (x[e] > m) { m = x[e]; am = j; }                               // ascending j: the lowest index of the lane's maximum
    }
    for (int off = L >> 1; off > 0; off >>= 1) {
      const float om = __shfl_xor(m, off, 64);
      const int oi = __shfl_xor(am, off, 64);
      if (om > m || (om == m && oi < am)) { m = om; am = oi; }
    }
    float xl = 0.f;                                                     // the label's logit: column label = le * L + ls
    const int le = label / L, ls = label & (L - 1);
#pragma unroll
    for (int e = 0; e < E; e++) xl = e == le ? x[e] : xl;
    xl = __shfl(xl, lead + ls, 64);
    const float mm = cls_ok ? m : 0.f;
    float s = 0.f;
#pragma unroll
    for (int e = 0; e < E; e++) { x[e] = expf(x[e] - mm); s += x[e]; }
    for (int off = L >> 1; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (cls_ok && sub == 0) {
      acc_cls += ((double)m - (double)xl) + (double)logf(s);            // logsumexp(row) - row[label]
      acc_ok += am == label ? 1 : 0;
    }
    if (want_grad && in) {                                              // (softmax - onehot) * upstream[0] / n_valid, zeros elsewhere
      float* dst = p.grad_cls + (size_t)row * C;
#pragma unroll
      for (int e = 0; e < E; e++) {
        const int j = e * L + sub;
        if (j < C) dst[j] = cls_ok ? (fdiv(x[e], s) - (j == label ? 1.f : 0.f)) * scale_cls : 0.f;
      }
    }

    // ---- smooth-L1 on the four columns the TARGET class selects
    if (has_box) {
      int k = -1;
      float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
      if (row_ok && sub == 0) {
        const float* t = p.targets5 + (size_t)row * 5;
        const float tc = t[0];
        if (tc > 0.f && tc < (float)C && tc == floorf(tc)) {             // an integer in (0, C): never an index otherwise
          k = agnostic ? 1 : (int)tc;
          const float4 pr = *reinterpret_cast<const float4*>(p.bbox_pred + (size_t)row * p.w + 4 * k);
          double sx, sy, sz, sw;
          acc_box += smooth_l1_term(pr.x, t[1], 1.f, 1.f, beta, &sx);
          acc_box += smooth_l1_term(pr.y, t[2], 1.f, 1.f, beta, &sy);
          acc_box += smooth_l1_term(pr.z, t[3], 1.f, 1.f, beta, &sz);
          acc_box += smooth_l1_term(pr.w, t[4], 1.f, 1.f, beta, &sw);
          g = make_float4((float)(sx * scale_box), (float)(sy * scale_box), (float)(sz * scale_box), (float)(sw * scale_box));
        }
      }
      if (want_grad) {
        k = __shfl(k, lead, 64);
        g.x = __shfl(g.x, lead, 64); g.y = __shfl(g.y, lead, 64); g.z = __shfl(g.z, lead, 64); g.w = __shfl(g.w, lead, 64);
        if (in) {
          float4* dst = reinterpret_cast<float4*>(p.grad_box + (size_t)row * p.w);
          for (int q = sub; q < W4; q += L) dst[q] = q == k ? g : make_float4(0.f, 0.f, 0.f, 0.f);
        }
      }
    }
  }
  if (!want_loss) return;

  // ---- one partial result per workgroup; the last workgroup to arrive sums them in index order
  const double b_cls = block_sum(acc_cls, sh_d);
  const double b_box = block_sum(acc_box, sh_d);
  const int b_ok = block_sum(acc_ok, sh_i);
  if (tid == 0) {
    // write-through stores, drained, then the counter: the payload is in memory before the arrival can be seen
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p.ws.part_cls + blockIdx.x), (unsigned long long)__double_as_longlong(b_cls),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p.ws.part_box + blockIdx.x), (unsigned long long)__double_as_longlong(b_box),
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(p.ws.part_ok + blockIdx.x, b_ok, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const int arrived = __hip_atomic_fetch_add(p.ws.ctrl, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    sh_last = arrived == (int)gridDim.x - 1 ? 1 : 0;
  }
  __syncthreads();
  if (!sh_last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  double t_cls = 0.0, t_box = 0.0;
  int t_ok = 0;
  for (int i = tid; i < (int)gridDim.x; i += kLossThreads) {             // loads that bypass this CU's L1
    t_cls += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(p.ws.part_cls + i),
                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    t_box += __longlong_as_double((long long)__hip_atomic_load(reinterpret_cast<unsigned long long*>(p.ws.part_box + i),
                                                                __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    t_ok += __hip_atomic_load(p.ws.part_ok + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  t_cls = block_sum(t_cls, sh_d);
  t_box = block_sum(t_box, sh_d);
  t_ok = block_sum(t_ok, sh_i);
  if (tid == 0) {
    const double nv = (double)n_valid;
    p.losses[0] = n_valid > 0 ? (float)(t_cls / nv) : 0.f;
    p.losses[1] = n_valid > 0 ? (float)(t_box / nv) : 0.f;
    p.losses[2] = n_valid > 0 ? (float)((double)t_ok / nv) : 0.f;
    p.losses[3] = (float)n_valid;
  }
}

// lanes per row: the least power of two with 4 * L >= C, 64 at the most (then E = 16 columns per lane hold C <= 1024)
inline int lanes_per_row(int c) {
  int L = 1;
  while (L < 64 && 4 * L < c) L <<= 1;
  return L;
}

}  // namespace dtc

DTC_API const char* dtc_loss_target_arch(void) { return "gfx950"; }

DTC_API size_t dtc_fast_rcnn_loss_workspace_bytes(int n, int c) {
  if (n < 1 || n > DTC_LOSS_MAX_ROWS || c < 2 || c > DTC_LOSS_MAX_CLASSES) return 0;
  return dtc::LossWorkspace::kBytes;
}

DTC_API int dtc_fast_rcnn_loss(const float* cls_score, const int32_t* labels, const float* bbox_pred, const float* bbox_targets5, int n,
                               int c, int bbox_width, float beta, const float* upstream, void* workspace, size_t workspace_bytes,
                               float* losses, float* grad_cls_score, float* grad_bbox_pred, dtc_stream_t stream) {
  // shapes and parameters
  if (n < 1 || c < 2 || !std::isfinite(beta) || beta <= 0.f) return DTC_EINVAL;
  const bool has_box = bbox_pred != nullptr;
  if (has_box && bbox_width != 8 && (int64_t)bbox_width != 4 * (int64_t)c) return DTC_EINVAL;
  // limits
  if (c > DTC_LOSS_MAX_CLASSES || n > DTC_LOSS_MAX_ROWS) return DTC_EUNSUPPORTED;
  // pointers
  if (!cls_score || !labels || (bbox_pred != nullptr) != (bbox_targets5 != nullptr)) return DTC_EINVAL;
  if (!losses && !grad_cls_score) return DTC_EINVAL;
  if (grad_bbox_pred && (!grad_cls_score || !has_box)) return DTC_EINVAL;
  if (grad_cls_score && has_box && !grad_bbox_pred) return DTC_EINVAL;
  if (((reinterpret_cast<uintptr_t>(bbox_pred) | reinterpret_cast<uintptr_t>(grad_bbox_pred) | reinterpret_cast<uintptr_t>(workspace)) & 15) != 0)
    return DTC_EINVAL;
  if (!workspace || workspace_bytes < dtc::LossWorkspace::kBytes) return DTC_EWORKSPACE;

  dtc::LossParams p{cls_score, labels, bbox_pred, bbox_targets5, upstream, n, c, has_box ? bbox_width : 0, dtc::lanes_per_row(c),
                    beta, dtc::LossWorkspace(workspace), losses, grad_cls_score, grad_bbox_pred};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::loss_count_kernel, dim3(1), dim3(dtc::kCountThreads), 0, s, labels, n, p.ws.ctrl);
  DTC_CHECK_LAUNCH();
  const int rows_per_block = 64 / p.L * dtc::kLossWaves;
  const dim3 grid(std::min(dtc::ceil_div(n, rows_per_block), dtc::kLossMaxBlocks));
  if (c <= 256)
    hipLaunchKernelGGL(dtc::fast_rcnn_loss_kernel<4>, grid, dim3(dtc::kLossThreads), 0, s, p);
  else
    hipLaunchKernelGGL(dtc::fast_rcnn_loss_kernel<16>, grid, dim3(dtc::kLossThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
