// Gradient clipping by the global norm fused with momentum SGD for gfx950: train_fast.py:165-166 (clip_grad_norm + the step of
// torch.optim.SGD) as two kernel nodes over a table of tensors (include/detectorch_optim_hip.h holds the contract).
//
// The host cuts every tensor into chunks (dtc_sgd_plan: pure host code), one workgroup per chunk in both kernels:
//   sgd_norm_kernel    sums g^2 of its chunk in double, the workgroup's sum in a fixed order, one double per chunk to the workspace;
//   sgd_update_kernel  every workgroup sums the K partials itself in one fixed order (thread t takes t, t + 256, ..., then the
//                      workgroup sum): the same bits everywhere, K * 8 bytes of L2 reads per workgroup, no arrival counter and no
//                      waiting on another workgroup.  It derives total_norm and coef, streams its chunk, and workgroup 0 reports.
// 24 bytes per element in all: 4 read by the norm pass, 12 read and 8 written by the update pass.  The gradients are never
// written.  16-byte accesses when the three arrays of a chunk are misaligned alike (a head of up to 3 elements, the body, a tail
// of up to 3), dword accesses otherwise.
#include <algorithm>
#include <cmath>
#include <vector>

#include "loss/loss_common.h"

#include "../../../include/detectorch_optim_hip.h"

namespace dtc {

constexpr int kSgdThreads = kLossThreads;         // block_sum (loss/loss_common.h) is written for this many
constexpr int kSgdMaxChunks = DTC_SGD_MAX_TENSORS + DTC_SGD_BODY_CHUNKS;

struct SgdTensorDev {                             // the plan's tensor record
  float* p;
  const float* g;
  float* buf;
  uint32_t n;
  int32_t group;
};
static_assert(sizeof(SgdTensorDev) == 32, "the plan holds 32 bytes per tensor");

struct SgdChunk {                                 // the plan's chunk record: elements [offset, offset + count) of `tensor`
  uint32_t tensor, offset, count, _pad;
};
static_assert(sizeof(SgdChunk) == 16, "the plan holds 16 bytes per chunk");

// The plan's pointers come out of memory, so the compiler cannot know their address space and would use flat accesses: they are
// device memory by contract (header), and are accessed as such.
typedef __attribute__((address_space(1))) float gf32;
typedef __attribute__((address_space(1))) f32x4 gf32x4;
__device__ __forceinline__ gf32* global(float* a) { return (gf32*)a; }
__device__ __forceinline__ const gf32* global(const float* a) { return (const gf32*)a; }

__device__ __forceinline__ uint32_t word_phase(const gf32* a) { return (uint32_t)((uintptr_t)a >> 2) & 3u; }
__device__ __forceinline__ double square(float v) { return (double)v * (double)v; }

__global__ __launch_bounds__(kSgdThreads) void sgd_norm_kernel(const SgdTensorDev* __restrict__ tensors,
                                                               const SgdChunk* __restrict__ chunks, double* __restrict__ partials) {
  __shared__ double sh[kLossWaves];
  const SgdChunk c = chunks[blockIdx.x];
  const gf32* g = global(tensors[c.tensor].g) + c.offset;
  const uint32_t n = c.count, t = threadIdx.x;
  const uint32_t head = min(n, (4u - word_phase(g)) & 3u);            // elements in front of the first 16-byte boundary
  const uint32_t nv = (n - head) >> 2;
  const gf32x4* gv = (const gf32x4*)(g + head);
  double acc = t < head ? square(g[t]) : 0.0;
#pragma unroll 4
  for (uint32_t i = t; i < nv; i += kSgdThreads) {
    const f32x4 v = gv[i];
    acc += square(v.x); acc += square(v.y); acc += square(v.z); acc += square(v.w);
  }
  const uint32_t tail = head + 4u * nv + t;
  if (tail < n) acc += square(g[tail]);
  const double total = block_sum(acc, sh);
  if (t == 0) partials[blockIdx.x] = total;
}

// One element of the step (header: four operations, one rounding each; nothing is contracted in this library).
__device__ __forceinline__ void sgd_element(float& p, float g, float& buf, float coef, float lr, float wd, float momentum) {
  const float gc = g * coef;
  const float d = gc + wd * p;
  buf = momentum * buf + d;
  p = p - lr * buf;
}

__global__ __launch_bounds__(kSgdThreads) void sgd_update_kernel(const SgdTensorDev* __restrict__ tensors,
                                                                 const SgdChunk* __restrict__ chunks,
                                                                 const double* __restrict__ partials, int n_chunks,
                                                                 const float* __restrict__ hyper, float momentum, float max_norm,
                                                                 int flags, float* __restrict__ stats) {
  __shared__ double sh[kLossWaves];
  const uint32_t t = threadIdx.x;
  double acc = 0.0;
  for (int k = t; k < n_chunks; k += kSgdThreads) acc += partials[k];
  const float total_norm = (float)sqrt(block_sum(acc, sh));
  const float q = fdiv(max_norm, total_norm + 1e-6f);
  const float coef = q > 1.0f ? 1.0f : q;                             // min(1, q) that keeps a NaN
  const bool nonfinite = !(fabsf(total_norm) <= 3.402823466e38f);     // NaN or inf
  if (blockIdx.x == 0 && t == 0) {
    stats[0] = total_norm; stats[1] = coef; stats[2] = nonfinite ? 1.0f : 0.0f; stats[3] = 0.0f;
  }
  if (nonfinite && (flags & DTC_SGD_SKIP_NONFINITE)) return;          // the whole grid alike: the bits are the same everywhere

  const SgdChunk c = chunks[blockIdx.x];
  const SgdTensorDev T = tensors[c.tensor];
  const float lr = hyper[2 * T.group], wd = hyper[2 * T.group + 1];
  gf32* p = global(T.p) + c.offset;
  const gf32* g = global(T.g) + c.offset;
  gf32* buf = global(T.buf) + c.offset;
  const uint32_t n = c.count;
  const uint32_t phase = word_phase(p);
  if (phase != word_phase(g) || phase != word_phase(buf)) {           // misaligned differently: dwords
#pragma unroll 4
    for (uint32_t i = t; i < n; i += kSgdThreads) {
      float pv = p[i], bv = buf[i];
      sgd_element(pv, g[i], bv, coef, lr, wd, momentum);
      buf[i] = bv; p[i] = pv;
    }
    return;
  }
  const uint32_t head = min(n, (4u - phase) & 3u);
  const uint32_t nv = (n - head) >> 2;
  const uint32_t edge = t < head ? t : 4u * nv + t;                   // threads [0, head): the head; the next (< 4): the tail
  if (edge < n) {
    float pv = p[edge], bv = buf[edge];
    sgd_element(pv, g[edge], bv, coef, lr, wd, momentum);
    buf[edge] = bv; p[edge] = pv;
  }
  gf32x4* p4 = (gf32x4*)(p + head);
  const gf32x4* g4 = (const gf32x4*)(g + head);
  gf32x4* b4 = (gf32x4*)(buf + head);
#pragma unroll 4
  for (uint32_t i = t; i < nv; i += kSgdThreads) {
    const f32x4 p0 = p4[i], g0 = g4[i], b0 = b4[i];
    f32x4 pv, bv;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      float pe = p0[e], be = b0[e];
      sgd_element(pe, g0[e], be, coef, lr, wd, momentum);
      pv[e] = pe; bv[e] = be;
    }
    b4[i] = bv; p4[i] = pv;
  }
}

// ---- the plan (host) -----------------------------------------------------------------------------------------------------------
// The chunk size of a call with `total` elements: DTC_SGD_CHUNK << k, the least k with ceil(total / chunk) <= DTC_SGD_BODY_CHUNKS.
inline int64_t sgd_chunk_elems(int64_t total) {
  int64_t chunk = DTC_SGD_CHUNK;
  while ((total + chunk - 1) / chunk > DTC_SGD_BODY_CHUNKS) chunk <<= 1;
  return chunk;
}

// -> the number of chunks of tensors with the given counts, or -1 when a count, their number or their total is outside its limit.
// *bound_out: what dtc_sgd_plan_bytes sizes the table for (header: monotone, never below the count).
template <typename Count> inline int64_t sgd_count_chunks(int n_tensors, Count count, int64_t* chunk_out, int64_t* bound_out) {
  if (n_tensors < 1 || n_tensors > DTC_SGD_MAX_TENSORS) return -1;
  int64_t total = 0;
  for (int i = 0; i < n_tensors; i++) {
    const int64_t n = count(i);
    if (n < 1 || n > DTC_SGD_MAX_ELEMENTS) return -1;
    total += n;
  }
  if (total > DTC_SGD_MAX_TOTAL) return -1;
  const int64_t chunk = sgd_chunk_elems(total);
  int64_t k = 0;
  for (int i = 0; i < n_tensors; i++) k += (count(i) + chunk - 1) / chunk;
  *chunk_out = chunk;
  *bound_out = n_tensors + std::min<int64_t>((total + DTC_SGD_CHUNK - 1) / DTC_SGD_CHUNK, DTC_SGD_BODY_CHUNKS);
  return k;
}

inline size_t sgd_plan_size(int n_tensors, int64_t n_chunks) {
  return sizeof(SgdTensorDev) * (size_t)n_tensors + sizeof(SgdChunk) * (size_t)n_chunks;
}

}  // namespace dtc

DTC_API const char* dtc_optim_target_arch(void) { return "gfx950"; }

DTC_API size_t dtc_sgd_plan_bytes(int n_tensors, const int64_t* counts) {
  if (!counts) return 0;
  int64_t chunk, bound;
  const int64_t k = dtc::sgd_count_chunks(n_tensors, [&](int i) { return counts[i]; }, &chunk, &bound);
  return k < 0 ? 0 : dtc::sgd_plan_size(n_tensors, bound);
}

DTC_API int dtc_sgd_plan(const dtc_sgd_tensor* records, int n_tensors, int n_groups, void* plan_out, size_t plan_bytes,
                         int* n_chunks) {
  using namespace dtc;
  // shapes
  if (!records || !n_chunks || n_tensors < 1 || n_groups < 1) return DTC_EINVAL;
  for (int i = 0; i < n_tensors; i++)
    if (records[i].n < 1 || records[i].group < 0 || records[i].group >= n_groups) return DTC_EINVAL;
  // limits
  int64_t chunk, bound;
  const int64_t k = sgd_count_chunks(n_tensors, [&](int i) { return records[i].n; }, &chunk, &bound);
  if (k < 0 || n_groups > DTC_SGD_MAX_GROUPS) return DTC_EUNSUPPORTED;
  // pointers
  std::vector<std::pair<uintptr_t, uintptr_t>> spans;                 // [begin, end) of every array
  spans.reserve(3 * (size_t)n_tensors);
  for (int i = 0; i < n_tensors; i++)
    for (const void* a : {(const void*)records[i].p, (const void*)records[i].g, (const void*)records[i].buf}) {
      const uintptr_t at = reinterpret_cast<uintptr_t>(a);
      if (!a || (at & 3) != 0) return DTC_EINVAL;
      spans.emplace_back(at, at + 4 * (uintptr_t)records[i].n);
    }
  std::sort(spans.begin(), spans.end());
  for (size_t i = 1; i < spans.size(); i++)
    if (spans[i].first < spans[i - 1].second) return DTC_EINVAL;
  if (!plan_out) return DTC_EINVAL;
  // workspace
  if (plan_bytes < sgd_plan_size(n_tensors, bound)) return DTC_EWORKSPACE;

  SgdTensorDev* tensors = static_cast<SgdTensorDev*>(plan_out);
  SgdChunk* chunks = reinterpret_cast<SgdChunk*>(tensors + n_tensors);
  for (int i = 0; i < n_tensors; i++) {
    tensors[i] = SgdTensorDev{records[i].p, records[i].g, records[i].buf, (uint32_t)records[i].n, records[i].group};
    for (int64_t off = 0; off < records[i].n; off += chunk)
      *chunks++ = SgdChunk{(uint32_t)i, (uint32_t)off, (uint32_t)std::min<int64_t>(chunk, records[i].n - off), 0u};
  }
  *n_chunks = (int)k;
  return DTC_OK;
}

DTC_API size_t dtc_sgd_workspace_bytes(int n_chunks) {
  if (n_chunks < 1 || n_chunks > dtc::kSgdMaxChunks) return 0;
  return dtc::align_up(sizeof(double) * (size_t)n_chunks, 16);
}

DTC_API int dtc_sgd_step(const void* plan_dev, size_t plan_bytes, int n_tensors, int n_chunks, const float* group_hyper_dev,
                         int n_groups, float momentum, float max_norm, int flags, void* workspace, size_t workspace_bytes,
                         float* stats, dtc_stream_t stream) {
  using namespace dtc;
  // shapes
  if (n_tensors < 1 || n_chunks < n_tensors || n_groups < 1 || plan_bytes != sgd_plan_size(n_tensors, n_chunks) ||
      !(max_norm > 0.0f) || !(momentum >= 0.0f && momentum < 1.0f) || (flags & ~DTC_SGD_SKIP_NONFINITE) != 0)
    return DTC_EINVAL;
  // limits
  if (n_tensors > DTC_SGD_MAX_TENSORS || n_chunks > n_tensors + DTC_SGD_BODY_CHUNKS || n_groups > DTC_SGD_MAX_GROUPS)
    return DTC_EUNSUPPORTED;
  // pointers
  if (!plan_dev || !group_hyper_dev || !stats) return DTC_EINVAL;
  if (((reinterpret_cast<uintptr_t>(plan_dev) | reinterpret_cast<uintptr_t>(workspace)) & 15) != 0 ||
      ((reinterpret_cast<uintptr_t>(group_hyper_dev) | reinterpret_cast<uintptr_t>(stats)) & 3) != 0)
    return DTC_EINVAL;
  // workspace
  if (!workspace || workspace_bytes < dtc_sgd_workspace_bytes(n_chunks)) return DTC_EWORKSPACE;

  const SgdTensorDev* tensors = static_cast<const SgdTensorDev*>(plan_dev);
  const SgdChunk* chunks = reinterpret_cast<const SgdChunk*>(tensors + n_tensors);
  double* partials = static_cast<double*>(workspace);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(sgd_norm_kernel, dim3(n_chunks), dim3(kSgdThreads), 0, s, tensors, chunks, partials);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(sgd_update_kernel, dim3(n_chunks), dim3(kSgdThreads), 0, s, tensors, chunks, partials, n_chunks,
                     group_hyper_dev, momentum, max_norm, flags, stats);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
