// The RPN training minibatch for gfx950 (include/detectorch_rpn_hip.h has the contract): labels for every anchor of every image,
// the sample of batch_size_per_im of them, box targets of the sampled foreground.  Eight kernel nodes on the stream, none of whose
// workgroups waits for another:
//   0  zero            the per-gt maxima, the two key histograms per image and the list counters
//   1  rpn_overlap     one anchor per thread, gt in LDS: inside test, max / first argmax over the non-crowd gt, and the per-gt
//                      maximum as an INTEGER maximum on the bits of the non-negative IoU (LDS, then one global atomic per gt and
//                      workgroup): order-independent
//   2  rpn_group       fg / bg / ignored per anchor (an anchor whose maximum reaches a gt's best overlap recomputes that IoU) and
//                      the 256-bin histogram of the top 8 bits of rand_key per image and group: the workgroup adds up in LDS, then
//                      one global integer add per bin it touched; on maps of 65 536 anchors or more a workgroup takes 2048 anchors
//   3  rpn_select_bin  one workgroup per image: group sizes, n_fg / n_bg, and the histogram bin that holds the last taken key
//   4  rpn_gather      the anchors of that bin go to a candidate list (fg from the front, bg from the back of one [N] array)
//   5  rpn_threshold   one workgroup per (image, group): MSB-first radix select of the remaining 44 bits of (rand_key, index) among
//                      the candidates -> the exact threshold key.  (rand_key << 20 | index) is unique per anchor, so "taken" is a
//                      comparison and the set does not depend on the order the list was filled in
//   6  rpn_finalize    final labels, the expanded blobs, and the taken fg keys into a list of at most 4096
//   7  rpn_fg_rows     one workgroup per image: bitonic sort of the taken fg keys, then fg_index / fg_targets / fg_gt in sampling order
// Selecting the k smallest keys runs on select_digit (radix_select.h: the k-th LARGEST) over the complemented key.
#include <algorithm>

#include "block_sort.h"
#include "box_vote.h"
#include "radix_select.h"
#include "rpn_train_common.h"

namespace dtc {

constexpr int kRpnKeyBins = 256;                          // top 8 bits of rand_key
constexpr int kRpnIdxBits = 20;                           // i < 2^20
constexpr uint64_t kRpnKeyMax = (1ull << 52) - 1ull;      // rand_key << 20 | i
constexpr int kRpnDigitBins = 2048;                       // the four 11-bit digits below the bin
constexpr int kRpnDigitBits = 11;
constexpr int kRpnGroupPer = 8;                           // anchors per thread of rpn_group on large maps: 2048 per workgroup share one
constexpr int kRpnGroupPerFrom = 1 << 16;                 // LDS histogram; below this N one per thread (few workgroups: latency counts)
enum { kSelNone = 0, kSelAll = 1, kSelBin = 2 };

// per image: group 0 = fg, 1 = bg
struct RpnSel { int32_t mode[2], bin[2], rem[2], take[2]; };

struct RpnTargetsWs {
  uint32_t* gtmax;      // [B, G]           zeroed
  uint32_t* hist;       // [B, 2, 256]      zeroed
  int32_t* cnt;         // [B, 4]           zeroed: candidates of group 0 / 1, taken fg listed
  RpnSel* sel;          // [B]
  uint64_t* bound;      // [B, 2]           taken <=> key < bound
  float* ov;            // [B, N]
  int32_t* arg;         // [B, N]           first argmax among the gt rows; -1: no gt; -2: not inside
  uint64_t* cand;       // [B, N]
  uint64_t* fgkeys;     // [B, 4096]
  size_t zero_bytes, bytes;
  RpnTargetsWs() = default;
  RpnTargetsWs(void* ws, int B, int G, int N) {
    Carve c{256};
    const size_t o_gtmax = c.take((size_t)B * G * 4), o_hist = c.take((size_t)B * 2 * kRpnKeyBins * 4), o_cnt = c.take((size_t)B * 16);
    zero_bytes = c.end;
    const size_t o_sel = c.take((size_t)B * sizeof(RpnSel)), o_bound = c.take((size_t)B * 16), o_ov = c.take((size_t)B * N * 4),
                 o_arg = c.take((size_t)B * N * 4), o_cand = c.take((size_t)B * N * 8), o_fg = c.take((size_t)B * kRpnMaxSample * 8);
    bytes = c.end;
    char* b = static_cast<char*>(ws);
    gtmax = reinterpret_cast<uint32_t*>(b + o_gtmax); hist = reinterpret_cast<uint32_t*>(b + o_hist);
    cnt = reinterpret_cast<int32_t*>(b + o_cnt); sel = reinterpret_cast<RpnSel*>(b + o_sel);
    bound = reinterpret_cast<uint64_t*>(b + o_bound); ov = reinterpret_cast<float*>(b + o_ov);
    arg = reinterpret_cast<int32_t*>(b + o_arg); cand = reinterpret_cast<uint64_t*>(b + o_cand);
    fgkeys = reinterpret_cast<uint64_t*>(b + o_fg);
  }
};

struct RpnTargetsParams {
  RpnTrainPlan plan;
  const float* gt_boxes; const int32_t* gt_is_crowd; const int32_t* gt_counts; const float* im_scale; const float* im_hw;
  const uint32_t* rand_keys;
  int G, R, F, group_per;
  float pos, neg, st;
  RpnTargetsWs ws;
  int32_t* labels; int32_t* fg_index; float* fg_targets; int32_t* fg_gt; int32_t* n_fg; int32_t* n_bg;
  float* max_overlaps; float* gt_max; float* targets; float* inside; float* outside;
};

__device__ __forceinline__ int rpn_gt_count(const RpnTargetsParams& p, int b) {
  return p.G > 0 ? min(max(p.gt_counts[b], 0), p.G) : 0;
}
// row g of image b in blob coordinates: one float32 multiply per coordinate
__device__ __forceinline__ float4 rpn_scaled_gt(const RpnTargetsParams& p, int b, int g) {
  const float4 q = reinterpret_cast<const float4*>(p.gt_boxes)[(size_t)b * p.G + g];
  const float s = p.im_scale[b];
  return make_float4(q.x * s, q.y * s, q.z * s, q.w * s);
}
// the image's gt rows -> LDS (every thread of a kRpnThreads workgroup calls; G <= kRpnThreads); ok: a non-crowd row below the count
__device__ __forceinline__ void rpn_stage_gt(const RpnTargetsParams& p, int b, int n_g, float4* g_box, int* g_ok) {
  const int t = threadIdx.x;
  if (t < n_g) {
    g_box[t] = rpn_scaled_gt(p, b, t);
    g_ok[t] = p.gt_is_crowd[(size_t)b * p.G + t] == 0 ? 1 : 0;
  }
}
__device__ __forceinline__ uint64_t rpn_key(uint32_t rand_key, int i) { return ((uint64_t)rand_key << kRpnIdxBits) | (uint32_t)i; }
__device__ __forceinline__ int rpn_key_bin(uint32_t rand_key) { return kRpnKeyBins - 1 - (int)(rand_key >> 24); }   // complemented

// bbox_transform_inv (boxes.py:224-238) with weights (1, 1, 1, 1): float32, one rounding per operation; the logarithm in double
__device__ __forceinline__ float4 rpn_deltas(float4 box, float4 gt) {
  const float ew = (box.z - box.x) + 1.f, eh = (box.w - box.y) + 1.f;
  const float ecx = box.x + 0.5f * ew, ecy = box.y + 0.5f * eh;
  const float gw = (gt.z - gt.x) + 1.f, gh = (gt.w - gt.y) + 1.f;
  const float gcx = gt.x + 0.5f * gw, gcy = gt.y + 0.5f * gh;
  return make_float4(fdiv(gcx - ecx, ew), fdiv(gcy - ecy, eh), (float)log((double)fdiv(gw, ew)), (float)log((double)fdiv(gh, eh)));
}

__global__ __launch_bounds__(kRpnThreads) void rpn_overlap_kernel(RpnTargetsParams p, RpnTrainAnchors K) {
  __shared__ float4 g_box[kRpnMaxGt];
  __shared__ int g_ok[kRpnMaxGt];
  __shared__ uint32_t g_max[kRpnMaxGt];
  const int b = blockIdx.y, tid = threadIdx.x, N = p.plan.N;
  const int n_g = rpn_gt_count(p, b);
  rpn_stage_gt(p, b, n_g, g_box, g_ok);
  g_max[tid] = 0u;
  __syncthreads();
  const int i = blockIdx.x * kRpnThreads + tid;
  if (i < N) {
    const float4 box = rpn_anchor_box(p.plan, K, rpn_cell_of(p.plan, i));
    const float h_b = p.im_hw[2 * b], w_b = p.im_hw[2 * b + 1];
    const bool inside = p.st < 0.f || (box.x >= -p.st && box.y >= -p.st && box.z < w_b + p.st && box.w < h_b + p.st);
    float best = 0.f;
    int arg = inside ? -1 : -2;
    if (inside) {
      for (int j = 0; j < n_g; j++) {
        if (!g_ok[j]) continue;
        const float v = iou_bbox(box, g_box[j]);
        if (arg < 0 || v > best) { best = v; arg = j; }                       // the first maximum
        if (v > 0.f && __float_as_uint(v) > g_max[j]) atomicMax(&g_max[j], __float_as_uint(v));
      }
    }
    p.ws.ov[(size_t)b * N + i] = best;
    p.ws.arg[(size_t)b * N + i] = arg;
    if (p.max_overlaps) p.max_overlaps[(size_t)b * N + i] = best;
  }
  __syncthreads();
  if (tid < n_g && g_max[tid] > 0u) atomicMax(&p.ws.gtmax[(size_t)b * p.G + tid], g_max[tid]);
}

__global__ __launch_bounds__(kRpnThreads) void rpn_group_kernel(RpnTargetsParams p, RpnTrainAnchors K) {
  __shared__ float4 g_box[kRpnMaxGt];
  __shared__ int g_ok[kRpnMaxGt];
  __shared__ uint32_t g_max[kRpnMaxGt];
  __shared__ uint32_t l_hist[2 * kRpnKeyBins];
  const int b = blockIdx.y, tid = threadIdx.x, N = p.plan.N;
  const int n_g = rpn_gt_count(p, b);
  rpn_stage_gt(p, b, n_g, g_box, g_ok);
  g_max[tid] = tid < n_g ? p.ws.gtmax[(size_t)b * p.G + tid] : 0u;
  for (int q = tid; q < 2 * kRpnKeyBins; q += kRpnThreads) l_hist[q] = 0u;
  if (p.gt_max && blockIdx.x == 0 && tid < p.G) p.gt_max[(size_t)b * p.G + tid] = __uint_as_float(g_max[tid]);
  __syncthreads();
  for (int k = 0; k < p.group_per; k++) {
    const int i = (blockIdx.x * p.group_per + k) * kRpnThreads + tid;
    if (i >= N) break;
    const int arg = p.ws.arg[(size_t)b * N + i];
    int grp = -1;
    if (arg != -2) {
      const float m = p.ws.ov[(size_t)b * N + i];
      bool fg = m >= p.pos;
      if (!fg && m > 0.f) {                                                   // ties a gt's best overlap?  (ov(i, j) <= m for every j)
        const uint32_t mb = __float_as_uint(m);
        const float4 box = rpn_anchor_box(p.plan, K, rpn_cell_of(p.plan, i));
        for (int j = 0; j < n_g && !fg; j++) {
          const uint32_t gm = g_max[j];
          if (!g_ok[j] || gm == 0u || gm > mb) continue;
          fg = __float_as_uint(iou_bbox(box, g_box[j])) == gm;
        }
      }
      grp = fg ? 1 : (m < p.neg ? 0 : -1);
    }
    p.labels[(size_t)b * N + i] = grp;                                        // provisional: rpn_finalize drops what is not taken
    if (grp >= 0) atomicAdd(&l_hist[(grp == 1 ? 0 : 1) * kRpnKeyBins + rpn_key_bin(p.rand_keys[(size_t)b * N + i])], 1u);
  }
  __syncthreads();
  for (int q = tid; q < 2 * kRpnKeyBins; q += kRpnThreads)                    // one global add per bin the workgroup touched
    if (l_hist[q] != 0u) atomicAdd(&p.ws.hist[(size_t)b * 2 * kRpnKeyBins + q], l_hist[q]);
}

__global__ __launch_bounds__(256) void rpn_select_bin_kernel(RpnTargetsParams p) {
  __shared__ uint32_t sh[2];
  __shared__ uint32_t wsum[2][4];
  const int b = blockIdx.x, tid = threadIdx.x;
  uint32_t total[2];
  for (int s = 0; s < 2; s++) {
    const uint32_t* h = p.ws.hist + ((size_t)b * 2 + s) * kRpnKeyBins;
    uint32_t c = 0;
    for (int q = tid; q < kRpnKeyBins; q += 256) c += h[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((tid & 63) == 0) wsum[s][tid >> 6] = c;
  }
  __syncthreads();
  for (int s = 0; s < 2; s++) total[s] = wsum[s][0] + wsum[s][1] + wsum[s][2] + wsum[s][3];
  int take[2];
  take[0] = (int)min((uint32_t)p.F, total[0]);
  take[1] = (int)min((uint32_t)(p.R - take[0]), total[1]);
  RpnSel r;
  for (int s = 0; s < 2; s++) {
    r.take[s] = take[s]; r.bin[s] = 0; r.rem[s] = 0;
    r.mode[s] = take[s] == 0 ? kSelNone : (uint32_t)take[s] == total[s] ? kSelAll : kSelBin;
    if (r.mode[s] == kSelBin) {                                               // uniform in the workgroup
      select_digit(p.ws.hist + ((size_t)b * 2 + s) * kRpnKeyBins, kRpnKeyBins, (uint32_t)take[s], sh);
      r.bin[s] = (int)sh[0];
      r.rem[s] = (int)sh[1];
      __syncthreads();
    }
  }
  if (tid == 0) { p.ws.sel[b] = r; p.n_fg[b] = take[0]; p.n_bg[b] = take[1]; }
}

__global__ __launch_bounds__(kRpnThreads) void rpn_gather_kernel(RpnTargetsParams p) {
  const int b = blockIdx.y, N = p.plan.N, i = blockIdx.x * kRpnThreads + threadIdx.x;
  if (i >= N) return;
  const int grp = p.labels[(size_t)b * N + i];
  if (grp < 0) return;
  const int s = grp == 1 ? 0 : 1;
  const RpnSel& r = p.ws.sel[b];
  if (r.mode[s] != kSelBin) return;
  const uint32_t rk = p.rand_keys[(size_t)b * N + i];
  if (rpn_key_bin(rk) != r.bin[s]) return;
  const int slot = atomicAdd(&p.ws.cnt[4 * b + s], 1);                        // < N: fg and bg anchors are disjoint
  p.ws.cand[(size_t)b * N + (s == 0 ? slot : N - 1 - slot)] = rpn_key(rk, i);
}

__global__ __launch_bounds__(kRpnSelThreads) void rpn_threshold_kernel(RpnTargetsParams p) {
  __shared__ __attribute__((aligned(16))) uint32_t h[kRpnDigitBins];
  __shared__ uint32_t sh[2];
  const int s = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, N = p.plan.N;
  const RpnSel& r = p.ws.sel[b];
  const int mode = r.mode[s];
  if (mode != kSelBin) {
    if (tid == 0) p.ws.bound[2 * b + s] = mode == kSelAll ? kRpnKeyMax + 1ull : 0ull;
    return;
  }
  const int n_c = min(max(p.ws.cnt[4 * b + s], 0), N);
  const uint64_t* cand = p.ws.cand + (size_t)b * N;
  uint64_t prefix = (uint64_t)r.bin[s];                                       // of the complemented key: its top 8 bits
  uint32_t k = (uint32_t)r.rem[s];
  for (int shift = 3 * kRpnDigitBits; shift >= 0; shift -= kRpnDigitBits) {
    for (int q = tid; q < kRpnDigitBins; q += kRpnSelThreads) h[q] = 0u;
    __syncthreads();
    for (int e = tid; e < n_c; e += kRpnSelThreads) {
      const uint64_t ck = kRpnKeyMax - cand[s == 0 ? e : N - 1 - e];
      if ((ck >> (shift + kRpnDigitBits)) == prefix) atomicAdd(&h[(uint32_t)(ck >> shift) & (kRpnDigitBins - 1)], 1u);
    }
    __syncthreads();
    select_digit(h, kRpnDigitBins, k, sh);
    prefix = (prefix << kRpnDigitBits) | sh[0];
    k = sh[1];
    __syncthreads();
  }
  if (tid == 0) p.ws.bound[2 * b + s] = (kRpnKeyMax - prefix) + 1ull;          // the threshold key itself is taken
}

__global__ __launch_bounds__(kRpnThreads) void rpn_finalize_kernel(RpnTargetsParams p, RpnTrainAnchors K) {
  const int b = blockIdx.y, N = p.plan.N, i = blockIdx.x * kRpnThreads + threadIdx.x;
  if (i >= N) return;
  const int grp = p.labels[(size_t)b * N + i];
  int label = -1;
  uint64_t key = 0;
  if (grp >= 0) {
    key = rpn_key(p.rand_keys[(size_t)b * N + i], i);
    if (key < p.ws.bound[2 * b + (grp == 1 ? 0 : 1)]) label = grp;
  }
  p.labels[(size_t)b * N + i] = label;
  if (label == 1) {
    const int slot = atomicAdd(&p.ws.cnt[4 * b + 2], 1);
    if (slot < kRpnMaxSample) p.ws.fgkeys[(size_t)b * kRpnMaxSample + slot] = key;
  }
  if (p.targets) {
    const RpnCell c = rpn_cell_of(p.plan, i);
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    const int g = label == 1 ? p.ws.arg[(size_t)b * N + i] : -1;             // (-1: fg without a gt, positive_overlap <= 0)
    if (g >= 0 && g < p.G) d = rpn_deltas(rpn_anchor_box(p.plan, K, c), rpn_scaled_gt(p, b, g));
    const RpnSel& r = p.ws.sel[b];
    const float in = label == 1 ? 1.f : 0.f;
    const float out = label >= 0 ? fdiv(1.f, (float)(r.take[0] + r.take[1])) : 0.f;
    const size_t hw = (size_t)p.plan.H[c.l] * p.plan.W[c.l];
    const size_t at = (size_t)b * 4 * N + 4 * (size_t)p.plan.off[c.l] + (size_t)(4 * c.a) * hw + (size_t)c.h * p.plan.W[c.l] + c.w;
    const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      p.targets[at + k * hw] = dv[k];
      p.inside[at + k * hw] = in;
      p.outside[at + k * hw] = out;
    }
  }
}

__global__ __launch_bounds__(kRpnSelThreads) void rpn_fg_rows_kernel(RpnTargetsParams p, RpnTrainAnchors K) {
  __shared__ uint64_t keys[kRpnMaxSample];
  const int b = blockIdx.x, tid = threadIdx.x, N = p.plan.N;
  const int n = min(p.ws.sel[b].take[0], kRpnMaxSample);
  const int np2 = next_pow2(n);
  for (int j = tid; j < np2; j += kRpnSelThreads) keys[j] = j < n ? p.ws.fgkeys[(size_t)b * kRpnMaxSample + j] : kPadKey;
  block_bitonic_sort<kRpnSelThreads>(keys, np2);                             // barriers inside, before and after
  for (int j = tid; j < p.F; j += kRpnSelThreads) {
    int idx = -1, g = -1;
    float4 d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (j < n) {
      idx = (int)(keys[j] & ((1u << kRpnIdxBits) - 1u));
      g = idx < N ? p.ws.arg[(size_t)b * N + idx] : -1;                       // (idx < N by construction: never an address otherwise)
      if (g >= p.G) g = -1;
      if (g >= 0) d = rpn_deltas(rpn_anchor_box(p.plan, K, rpn_cell_of(p.plan, idx)), rpn_scaled_gt(p, b, g));
      else g = -1;
    }
    const size_t row = (size_t)b * p.F + j;
    p.fg_index[row] = idx;
    p.fg_gt[row] = g;
    reinterpret_cast<float4*>(p.fg_targets)[row] = d;
  }
}

}  // namespace dtc

DTC_API const char* dtc_rpn_train_target_arch(void) { return "gfx950"; }

static int rpn_targets_shapes(const dtc_rpn_train_level* levels, int n_levels, int batch, int gt_stride, dtc::RpnTrainPlan* plan,
                              dtc::RpnTrainAnchors* anchors) {
  if (batch < 0 || gt_stride < 0) return DTC_EINVAL;
  const int rc = dtc::make_rpn_train_plan(levels, n_levels, plan, anchors);
  if (rc != DTC_OK) return rc;
  if (gt_stride > DTC_RPN_TRAIN_MAX_GT || batch > 65535) return DTC_EUNSUPPORTED;
  return DTC_OK;
}

DTC_API size_t dtc_rpn_targets_workspace_bytes(const dtc_rpn_train_level* levels, int n_levels, int batch, int gt_stride) {
  dtc::RpnTrainPlan plan;
  if (batch < 1 || rpn_targets_shapes(levels, n_levels, batch, gt_stride, &plan, nullptr) != DTC_OK) return 0;
  return dtc::RpnTargetsWs(nullptr, batch, gt_stride, plan.N).bytes;
}

DTC_API int dtc_rpn_targets(const dtc_rpn_train_level* levels, int n_levels, int batch, const float* gt_boxes, const int32_t* gt_is_crowd,
                            const int32_t* gt_counts, int gt_stride, const float* im_scale, const float* im_hw, const uint32_t* rand_keys,
                            const dtc_rpn_train_params* params, void* workspace, size_t workspace_bytes, int32_t* labels,
                            int32_t* fg_index, float* fg_targets, int32_t* fg_gt, int32_t* n_fg, int32_t* n_bg, float* max_overlaps,
                            float* gt_max, float* bbox_targets, float* bbox_inside_weights, float* bbox_outside_weights,
                            dtc_stream_t stream) {
  // shapes and parameters
  if (batch < 0 || gt_stride < 0 || !params || !levels || n_levels < 1) return DTC_EINVAL;
  const dtc_rpn_train_params& q = *params;
  if (q.batch_size_per_im < 1 || !std::isfinite(q.fg_fraction) || q.fg_fraction < 0.0 || q.fg_fraction > 1.0 ||
      !std::isfinite(q.positive_overlap) || !std::isfinite(q.negative_overlap) || !std::isfinite(q.straddle_thresh) ||
      q.negative_overlap > q.positive_overlap)
    return DTC_EINVAL;
  dtc::RpnTargetsParams p{};
  dtc::RpnTrainAnchors anchors;
  // ... and limits
  const int rc = rpn_targets_shapes(levels, n_levels, batch, gt_stride, &p.plan, &anchors);
  if (rc != DTC_OK) return rc;
  if (q.batch_size_per_im > DTC_RPN_TRAIN_MAX_BATCH_PER_IM) return DTC_EUNSUPPORTED;
  if (batch == 0) return DTC_OK;
  p.G = gt_stride; p.R = q.batch_size_per_im;
  p.group_per = p.plan.N >= dtc::kRpnGroupPerFrom ? dtc::kRpnGroupPer : 1;
  p.F = (int)(q.fg_fraction * (double)q.batch_size_per_im);
  // pointers
  if (gt_stride > 0 && (!gt_boxes || !gt_is_crowd || !gt_counts)) return DTC_EINVAL;
  if (!im_scale || !im_hw || !rand_keys || !labels || !n_fg || !n_bg) return DTC_EINVAL;
  if (p.F > 0 && (!fg_index || !fg_targets || !fg_gt)) return DTC_EINVAL;
  const int n_exp = (bbox_targets != nullptr) + (bbox_inside_weights != nullptr) + (bbox_outside_weights != nullptr);
  if (n_exp != 0 && n_exp != 3) return DTC_EINVAL;
  if (((reinterpret_cast<uintptr_t>(gt_boxes) | reinterpret_cast<uintptr_t>(fg_targets) | reinterpret_cast<uintptr_t>(workspace)) & 15) != 0)
    return DTC_EINVAL;
  // workspace
  const dtc::RpnTargetsWs ws(workspace, batch, gt_stride, p.plan.N);
  if (!workspace || workspace_bytes < ws.bytes) return DTC_EWORKSPACE;

  p.gt_boxes = gt_boxes; p.gt_is_crowd = gt_is_crowd; p.gt_counts = gt_counts; p.im_scale = im_scale; p.im_hw = im_hw;
  p.rand_keys = rand_keys;
  p.pos = q.positive_overlap; p.neg = q.negative_overlap; p.st = q.straddle_thresh;
  p.ws = ws;
  p.labels = labels; p.fg_index = fg_index; p.fg_targets = fg_targets; p.fg_gt = fg_gt; p.n_fg = n_fg; p.n_bg = n_bg;
  p.max_overlaps = max_overlaps; p.gt_max = gt_max; p.targets = bbox_targets; p.inside = bbox_inside_weights;
  p.outside = bbox_outside_weights;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 per_anchor(dtc::ceil_div(p.plan.N, dtc::kRpnThreads), batch), block(dtc::kRpnThreads);
  if (dtc::zero_async(workspace, ws.zero_bytes, s) != DTC_OK) return DTC_ELAUNCH;
  hipLaunchKernelGGL(dtc::rpn_overlap_kernel, per_anchor, block, 0, s, p, anchors);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::rpn_group_kernel, dim3(dtc::ceil_div(p.plan.N, dtc::kRpnThreads * p.group_per), batch), block, 0, s, p, anchors);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::rpn_select_bin_kernel, dim3(batch), dim3(256), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::rpn_gather_kernel, per_anchor, block, 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::rpn_threshold_kernel, dim3(2, batch), dim3(dtc::kRpnSelThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::rpn_finalize_kernel, per_anchor, block, 0, s, p, anchors);
  DTC_CHECK_LAUNCH();
  if (p.F > 0) {
    hipLaunchKernelGGL(dtc::rpn_fg_rows_kernel, dim3(batch), dim3(dtc::kRpnSelThreads), 0, s, p, anchors);
    DTC_CHECK_LAUNCH();
  }
  return DTC_OK;
}
