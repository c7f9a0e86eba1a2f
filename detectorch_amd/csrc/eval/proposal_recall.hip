// The reference's evaluate_box_proposals (lib/utils/json_dataset_evaluator.py:238-319) for a batch on gfx950
// (include/detectorch_eval_hip.h has the contract).  One kernel node, one workgroup of kPropThreads per image:
//   - the gt taking part, compacted in row order;
//   - every gt column caches its best remaining proposal as one 64-bit key (overlap bits << 32 | ~proposal: the maximum is the
//     largest overlap and then the smallest proposal); a column is (re)scanned by the whole workgroup, kPropThreads proposals per
//     pass, only when it is new or its cached proposal was retired;
//   - a round takes the maximum of (overlap bits << 32 | ~gt) over the live columns, records it and retires the pair.
// The overlap is iou_bbox of box_vote.h (the element of cython_bbox.bbox_overlaps, pinned to the Cython build); it is >= 0 on finite
// boxes, so its float32 bits order as unsigned integers.
#include "box_vote.h"

#include "../../../include/detectorch_eval_hip.h"

namespace dtc {

constexpr int kPropThreads = 256;
constexpr int kPropWaves = kPropThreads / 64;

struct PropRecallParams {
  const float* proposals; const int32_t* prop_counts; const float* gt_boxes; const int32_t* gt_classes; const int32_t* gt_is_crowd;
  const int32_t* gt_counts; const float* gt_area;
  int P, G, limit;
  const double* area_rng;
  double* gt_overlaps; int32_t* n_pos; int32_t* n_overlaps;
};

// the maximum of v over the workgroup, in every thread; sh: kPropWaves words
__device__ __forceinline__ uint64_t block_max_u64(uint64_t v, uint64_t* sh) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
    const uint64_t o = ((uint64_t)hi << 32) | lo;
    v = o > v ? o : v;
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  uint64_t r = sh[0];
#pragma unroll
  for (int w = 1; w < kPropWaves; w++) r = sh[w] > r ? sh[w] : r;
  return r;
}

__global__ __launch_bounds__(kPropThreads) void eval_proposal_recall_kernel(PropRecallParams p) {
  __shared__ float4 s_gbox[DTC_EVAL_MAX_GT];
  __shared__ uint64_t s_col[DTC_EVAL_MAX_GT];                 // the column's best remaining proposal; 0: the column is retired
  __shared__ uint8_t s_scan[DTC_EVAL_MAX_GT];                 // the column has to be scanned
  __shared__ double s_val[DTC_EVAL_MAX_GT];                   // the overlap recorded by round j
  __shared__ uint32_t s_retired[DTC_EVAL_MAX_PROPOSALS / 32];
  __shared__ uint64_t s_red[kPropWaves];
  __shared__ int s_wave_n[kPropWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, n = blockIdx.x;
  int Pc = min(max(p.prop_counts[n], 0), p.P);
  if (p.limit > 0) Pc = min(Pc, p.limit);
  const int ng = p.G > 0 ? min(max(p.gt_counts[n], 0), p.G) : 0;
  const size_t grow0 = (size_t)n * p.G;
  const float4* props = reinterpret_cast<const float4*>(p.proposals) + (size_t)n * p.P;

  // the gt taking part (G <= kPropThreads: one per thread), compacted in row order
  bool take = false;
  float4 gb = make_float4(0.f, 0.f, 0.f, 0.f);
  if (tid < ng) {
    gb = reinterpret_cast<const float4*>(p.gt_boxes)[grow0 + tid];
    const double area = p.gt_area ? (double)p.gt_area[grow0 + tid]
                                  : (((double)gb.z - (double)gb.x) + 1.0) * (((double)gb.w - (double)gb.y) + 1.0);
    take = p.gt_is_crowd[grow0 + tid] == 0 && p.gt_classes[grow0 + tid] > 0 && area >= p.area_rng[0] && area <= p.area_rng[1];
  }
  const uint64_t bal = __ballot(take);
  if (lane == 0) s_wave_n[wave] = __builtin_popcountll(bal);
  for (int w = tid; w < (Pc + 31) / 32; w += kPropThreads) s_retired[w] = 0u;
  __syncthreads();
  int before = 0, Gv = 0;
  for (int w = 0; w < kPropWaves; w++) { if (w < wave) before += s_wave_n[w]; Gv += s_wave_n[w]; }
  if (take) { const int at = before + lanes_below(bal, lane); s_gbox[at] = gb; }
  if (tid < DTC_EVAL_MAX_GT) { s_scan[tid] = tid < Gv ? 1 : 0; s_col[tid] = 0ull; }
  __syncthreads();

  const int rounds = min(Pc, Gv);
  for (int j = 0; j < rounds; j++) {
    for (int g = 0; g < Gv; g++) {
      if (!s_scan[g]) continue;                               // the same for every thread
      const float4 Q = s_gbox[g];
      uint64_t best = 0ull;
      for (int q = tid; q < Pc; q += kPropThreads) {
        if ((s_retired[q >> 5] >> (q & 31)) & 1u) continue;
        const uint64_t key = ((uint64_t)__float_as_uint(iou_bbox(props[q], Q)) << 32) | (uint32_t)~(uint32_t)q;
        best = key > best ? key : best;
      }
      best = block_max_u64(best, s_red);
      if (tid == 0) { s_col[g] = best; s_scan[g] = 0; }
    }
    __syncthreads();
    uint64_t mine = 0ull;
    if (tid < Gv && s_col[tid] != 0ull) mine = (s_col[tid] & 0xffffffff00000000ull) | (uint32_t)~(uint32_t)tid;
    const uint64_t sel = block_max_u64(mine, s_red);
    const int g_sel = (int)~(uint32_t)sel;
    const uint32_t p_sel = ~(uint32_t)s_col[g_sel];
    __syncthreads();
    if (tid == 0) {
      s_val[j] = (double)__uint_as_float((uint32_t)(sel >> 32));
      s_retired[p_sel >> 5] |= 1u << (p_sel & 31);
      s_col[g_sel] = 0ull;
    }
    if (tid < Gv && tid != g_sel && s_col[tid] != 0ull && ~(uint32_t)s_col[tid] == p_sel) s_scan[tid] = 1;
    __syncthreads();
  }

  for (int g = tid; g < p.G; g += kPropThreads) p.gt_overlaps[grow0 + g] = g < rounds ? s_val[g] : 0.0;
  if (tid == 0) { p.n_pos[n] = Gv; p.n_overlaps[n] = Pc > 0 ? Gv : 0; }
}

}  // namespace dtc

DTC_API int dtc_eval_proposal_recall(const float* proposals, const int32_t* prop_counts, const float* gt_boxes, const int32_t* gt_classes,
                                     const int32_t* gt_is_crowd, const int32_t* gt_counts, const float* gt_area, int batch,
                                     int proposal_stride, int gt_stride, const double* area_rng, int limit, double* gt_overlaps,
                                     int32_t* n_pos, int32_t* n_overlaps, dtc_stream_t stream) {
  if (batch < 1 || proposal_stride < 1 || gt_stride < 0 || limit < 0) return DTC_EINVAL;
  if (batch > DTC_EVAL_MAX_BATCH || proposal_stride > DTC_EVAL_MAX_PROPOSALS || gt_stride > DTC_EVAL_MAX_GT) return DTC_EUNSUPPORTED;
  if (!proposals || !prop_counts || !area_rng || !n_pos || !n_overlaps) return DTC_EINVAL;
  if (gt_stride > 0 && (!gt_boxes || !gt_classes || !gt_is_crowd || !gt_counts || !gt_overlaps)) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(proposals) & 15) != 0 || (reinterpret_cast<uintptr_t>(gt_boxes) & 15) != 0) return DTC_EINVAL;

  dtc::PropRecallParams p{};
  p.proposals = proposals; p.prop_counts = prop_counts; p.gt_boxes = gt_boxes; p.gt_classes = gt_classes; p.gt_is_crowd = gt_is_crowd;
  p.gt_counts = gt_counts; p.gt_area = gt_area; p.P = proposal_stride; p.G = gt_stride; p.limit = limit; p.area_rng = area_rng;
  p.gt_overlaps = gt_overlaps; p.n_pos = n_pos; p.n_overlaps = n_overlaps;
  hipLaunchKernelGGL(dtc::eval_proposal_recall_kernel, dim3(batch), dim3(dtc::kPropThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
