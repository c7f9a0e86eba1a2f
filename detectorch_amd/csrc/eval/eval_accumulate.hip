// COCOeval's accumulate on gfx950 (include/detectorch_eval_hip.h has the contract).  Two kernel nodes:
//   1  eval_counts      counts[k, a] = the sum of npig over the images, one thread per (k, a)
//   2  eval_accumulate  one wave per (class, m), one lane per (a, t).  The class's rows are one segment of the sorted order (two
//                       binary searches on the keys).  The segment goes through LDS in tiles of kAccTile rows, loaded by the lanes
//                       side by side and then walked by every lane on its own bit: forward for the totals of tp and fp, then
//                       backward, where the running maximum of the precision is at hand when a recall threshold is first met.
//                       tp and fp are integers (exact as float64), so walking back from the totals gives the forward cumsum's values.
#include "wave_ops.h"

#include "../../../include/detectorch_eval_hip.h"

namespace dtc {

constexpr int kAccWave = 64;
constexpr int kAccTile = 256;          // rows of the segment staged at a time
constexpr uint64_t kAccPadKey = 0x7fffffffffffffffull;     // sort_key of a row that takes part in nothing (dt_rank -1)

struct EvalAccParams {
  const int32_t* dt_rank; const uint64_t* dt_match; const uint64_t* dt_ignore; const long long* sort_key; const int32_t* order;
  long long rows;
  const int32_t* npig; int images, K, T, A;
  const double* rec_thrs; int R; const int32_t* max_dets; int M;
  double* precision; double* recall; int32_t* counts;
};

__global__ __launch_bounds__(256) void eval_counts_kernel(EvalAccParams p) {
  const int KA = p.K * p.A, idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= KA) return;
  int c = 0;
  for (int i = 0; i < p.images; i++) c += p.npig[(size_t)i * KA + idx];
  p.counts[idx] = c;
}

// the first sorted position whose key is >= bound (keys compared as unsigned: the padding key is the largest)
__device__ __forceinline__ long long first_at_least(const EvalAccParams& p, uint64_t bound) {
  long long lo = 0, hi = p.rows;
  while (lo < hi) {
    const long long mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)p.sort_key[p.order[mid]] < bound) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(kAccWave) void eval_accumulate_kernel(EvalAccParams p) {
  __shared__ int32_t s_rank[kAccTile];
  __shared__ uint64_t s_match[kAccTile];
  __shared__ uint64_t s_ignore[kAccTile];
  const int lane = threadIdx.x, k = blockIdx.x, m = blockIdx.y;
  const int T = p.T, A = p.A, K = p.K, M = p.M, R = p.R;
  const bool active = lane < T * A;
  const int a = active ? lane / T : 0, t = active ? lane % T : 0;
  const int md = p.max_dets[m];
  // the segment ends before the next class and before the padding keys: at num_classes = 1024 the last class's upper bound
  // (k + 2) << 53 is 2^63, beyond the padding key, which must stay outside every segment
  const uint64_t next_class = (uint64_t)(k + 2) << 53;
  const long long seg_lo = first_at_least(p, (uint64_t)(k + 1) << 53),
                  seg_hi = first_at_least(p, next_class < kAccPadKey ? next_class : kAccPadKey);
  const int count = active ? p.counts[k * A + a] : 0;
  const bool live = active && count > 0;

  auto stage = [&](long long base) {
    __syncthreads();
    for (int e = lane; e < kAccTile; e += kAccWave) {
      const long long i = base + e;
      if (i < seg_hi) {
        const int row = p.order[i];
        s_rank[e] = p.dt_rank[row]; s_match[e] = p.dt_match[row]; s_ignore[e] = p.dt_ignore[row];
      }
    }
    __syncthreads();
  };
  const long long n_tiles = (seg_hi - seg_lo + kAccTile - 1) / kAccTile;

  // forward: the totals
  int tp = 0, fp = 0;
  for (long long ti = 0; ti < n_tiles; ti++) {
    const long long base = seg_lo + ti * kAccTile;
    stage(base);
    const int cnt = (int)min((long long)kAccTile, seg_hi - base);
    for (int e = 0; e < cnt; e++) {
      if (s_rank[e] < 0 || s_rank[e] >= md || ((s_ignore[e] >> lane) & 1ull)) continue;
      const int mt = (int)((s_match[e] >> lane) & 1ull);
      tp += mt; fp += 1 - mt;
    }
  }

  const size_t rc_at = (((size_t)t * K + k) * A + a) * M + m;
  auto pr_at = [&](int r) { return ((((size_t)t * R + r) * K + k) * A + a) * M + m; };
  const double npos = (double)count;
  int r = R - 1;
  double best = 0.0;                    // the reverse running maximum of the precision (every precision is >= 0)
  if (active && !live) {
    p.recall[rc_at] = -1.0;
    for (int q = 0; q < R; q++) p.precision[pr_at(q)] = -1.0;
  }
  if (live) {
    const double rc_end = (double)tp / npos;
    p.recall[rc_at] = rc_end;
    while (r >= 0 && p.rec_thrs[r] > rc_end) { p.precision[pr_at(r)] = 0.0; r--; }       // past the end
  }

  // backward: (tp, fp) are the counts up to and including the row at hand
  for (long long ti = n_tiles - 1; ti >= 0; ti--) {
    const long long base = seg_lo + ti * kAccTile;
    stage(base);
    if (!live) continue;
    const int cnt = (int)min((long long)kAccTile, seg_hi - base);
    for (int e = cnt - 1; e >= 0; e--) {
      if (s_rank[e] < 0 || s_rank[e] >= md || ((s_ignore[e] >> lane) & 1ull)) continue;
      const double dtp = (double)tp, dfp = (double)fp;
      best = fmax(best, dtp / ((dfp + dtp) + 2.220446049250313e-16));
      if ((s_match[e] >> lane) & 1ull) {
        tp--;
        const double rc_prev = (double)tp / npos;        // the recall before this row: thresholds above it are first met here
        while (r >= 0 && p.rec_thrs[r] > rc_prev) { p.precision[pr_at(r)] = best; r--; }
      } else {
        fp--;
      }
    }
  }
  if (live) {
    while (r >= 0) { p.precision[pr_at(r)] = best; r--; }     // thresholds met at the first row
  }
}

}  // namespace dtc

DTC_API int dtc_eval_accumulate(const int32_t* dt_rank, const uint64_t* dt_match, const uint64_t* dt_ignore, const long long* sort_key,
                                const int32_t* order, long long rows, const int32_t* npig, int images, int num_classes, int n_thrs,
                                int n_areas, const double* rec_thrs, int n_rec, const int32_t* max_dets, int n_max_dets,
                                double* precision, double* recall, int32_t* counts, dtc_stream_t stream) {
  if (rows < 1 || images < 1 || num_classes < 2 || n_thrs < 1 || n_areas < 1 || n_rec < 1 || n_max_dets < 1) return DTC_EINVAL;
  if (rows > DTC_EVAL_MAX_ROWS || num_classes > DTC_EVAL_MAX_CLASSES || n_areas > DTC_EVAL_MAX_AREAS ||
      (long long)n_thrs * n_areas > DTC_EVAL_MAX_PAIRS || n_rec > DTC_EVAL_MAX_REC_THRS || n_max_dets > DTC_EVAL_MAX_MAX_DETS ||
      images > DTC_EVAL_MAX_IMAGES)
    return DTC_EUNSUPPORTED;
  if (!dt_rank || !dt_match || !dt_ignore || !sort_key || !order || !npig || !rec_thrs || !max_dets || !precision || !recall || !counts)
    return DTC_EINVAL;

  dtc::EvalAccParams p{};
  p.dt_rank = dt_rank; p.dt_match = dt_match; p.dt_ignore = dt_ignore; p.sort_key = sort_key; p.order = order; p.rows = rows;
  p.npig = npig; p.images = images; p.K = num_classes - 1; p.T = n_thrs; p.A = n_areas;
  p.rec_thrs = rec_thrs; p.R = n_rec; p.max_dets = max_dets; p.M = n_max_dets;
  p.precision = precision; p.recall = recall; p.counts = counts;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::eval_counts_kernel, dim3(dtc::ceil_div(p.K * p.A, 256)), dim3(256), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::eval_accumulate_kernel, dim3(p.K, n_max_dets), dim3(dtc::kAccWave), 0, s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
