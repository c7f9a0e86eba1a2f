// rle_mask_voting on run lists (include/detectorch_mpost_hip.h, entry 4), no h x w frame.  Two kernel nodes:
//   1  mpost_vote_prepare_kernel: one wave per voter list: its clipped run ENDS go to the workspace, with the runs in use and the span
//      [first one, behind the last one) of its set pixels.
//   2  mpost_vote_kernel: one workgroup per (image, top).  The uniform ways out first (a list that did not fit, a top of area 0, fewer
//      than two voters: the row is copied); then the voters go to LDS in index order with their support slices and inside weights,
//      and the pixels are walked in chunks of one per thread: every thread looks its position up in each voter's run ends (a binary
//      search), adds num and den in voter order in float64 and divides once.  A pixel that differs from the one in front of it starts
//      a run; a scan carried across the chunks numbers the starts, and the differences of the starts are the runs.  A chunk in which
//      no voter has a pixel is off without a lookup, and when the pixel in front of it is off too the walk jumps to where the
//      nearest run of any voter starts.
// No atomics, the float64 sums in one order: the same bits on every run.
#include <climits>

#include "mpost_common.h"

namespace dtc {

constexpr int kVoteThreads = 256;
constexpr double kVoteFloor = 1e-5;                          // np.maximum(mask_weights, 1e-5)

struct MpostVoteParams {
  const uint32_t* top_runs; const int32_t* top_n_runs; const int32_t* top_count;
  const uint32_t* all_runs; const int32_t* all_n_runs; const float* all_dets; const int32_t* all_count;
  const double* ovr; const float* im_size;
  int T, top_stride, A, all_stride, dets_stride, method, out_stride;
  double iou_thresh, binarize_thresh;
  uint32_t* all_ends;                                        // workspace [N, A, all_stride]: clipped run ends
  int32_t* all_n;                                            // workspace [N, A]: the runs in use, 0 past the count
  uint2* all_span;                                           // workspace [N, A]: (first set position, behind the last one); none: (2^32 - 1, 0)
  uint32_t* out_runs; int32_t* out_n_runs; int32_t* need;
};

__global__ __launch_bounds__(kMpostWave) void mpost_vote_prepare_kernel(MpostVoteParams p) {
  const int lane = threadIdx.x, k = blockIdx.x, n = blockIdx.y;
  const size_t row = (size_t)n * p.A + k;
  const uint32_t hw = mpost_pixels(p.im_size, n);
  const int n_runs = k < mpost_count(p.all_count, n, p.A) ? min(max(p.all_n_runs[row], 0), p.all_stride) : 0;
  const uint32_t* runs = p.all_runs + row * p.all_stride;
  uint32_t* ends = p.all_ends + row * p.all_stride;
  long long pos = 0;
  uint32_t prev_end = 0, first = 0xffffffffu, last = 0u;
  for (int j0 = 0; j0 < n_runs; j0 += kMpostWave) {
    const int j = j0 + lane;
    uint32_t s, e;
    mpost_chunk_ends(runs, n_runs, j0, lane, hw, pos, prev_end, s, e);
    if (j < n_runs) ends[j] = e;
    if ((j & 1) && e > s) { first = min(first, s); last = max(last, e); }
  }
  first = wave_min(first); last = wave_max(last);
  if (lane == 0) { p.all_n[row] = n_runs; p.all_span[row] = make_uint2(first, last); }
}

struct VoteAdd { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct VoteMax { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct VoteMin { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; } };

// EXCLUSIVE scan of v under op over the threads of the workgroup (ident in front of thread 0), and the total; ws: kVoteThreads / 64
// slots of 8 bytes.  Two barriers; ws may be used again on return.
template <typename T, typename Op>
__device__ __forceinline__ T vote_block_scan(T v, Op op, T ident, unsigned long long* ws_raw, T* total) {
  T* ws = reinterpret_cast<T*>(ws_raw);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const T o = __shfl_up(incl, off, 64); if (lane >= off) incl = op(o, incl); }
  T excl = __shfl_up(incl, 1, 64);
  if (lane == 0) excl = ident;
  if (lane == 63) ws[wv] = incl;
  __syncthreads();
  T before = ident, tot = ident;
#pragma unroll
  for (int k = 0; k < kVoteThreads / 64; k++) { const T c = ws[k]; if (k < wv) before = op(before, c); tot = op(tot, c); }
  __syncthreads();
  *total = tot;
  return op(before, excl);
}

// astype(np.int32) of a box coordinate: truncated toward zero; NaN: 0; saturated past the int32 range
__device__ __forceinline__ long long vote_trunc(float v) {
  if (v != v) return 0;
  if (v <= -2147483648.f) return (long long)INT_MIN;
  if (v >= 2147483648.f) return (long long)INT_MAX;
  return (long long)(int)v;
}

// the numpy slice [max(lo, 0) : min(hi + 1, size)] of an axis of `size` as [start, stop): a negative stop counts from the far edge
__device__ __forceinline__ void vote_slice(long long lo, long long hi, long long size, int* start, int* stop) {
  const long long a = lo > 0 ? lo : 0;
  long long b = hi + 1 < size ? hi + 1 : size;
  if (b < 0) { b += size; if (b < 0) b = 0; }
  *start = (int)(a < size ? a : size); *stop = (int)b;
}

__global__ __launch_bounds__(kVoteThreads) void mpost_vote_kernel(MpostVoteParams p) {
  __shared__ unsigned long long scan_s[kVoteThreads / 64];
  __shared__ uint32_t bl_s[kVoteThreads];
  __shared__ int val_s[kVoteThreads];
  __shared__ int v_idx[DTC_MPOST_MAX_ROWS], v_n[DTC_MPOST_MAX_ROWS];
  __shared__ int4 v_box[DTC_MPOST_MAX_ROWS];                 // the support slice: columns [x, y), rows [z, w)
  __shared__ double v_win[DTC_MPOST_MAX_ROWS];               // the weight inside the support
  const int t = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  if (t >= mpost_count(p.top_count, n, p.T)) return;         // rows past the count are not written
  const size_t row = (size_t)n * p.T + t;
  const int m = p.top_n_runs[row];
  const uint32_t* in = p.top_runs + row * p.top_stride;
  uint32_t* out = p.out_runs + row * p.out_stride;
  auto finish = [&](int n_runs, int need) { if (tid == 0) { p.out_n_runs[row] = n_runs; p.need[row] = need; } };
  auto copy = [&]() {                                        // copied as it is
    const bool fits = m <= p.out_stride;
    if (fits) for (int k = tid; k < m; k += kVoteThreads) out[k] = in[k];
    finish(fits ? m : -1, m);
  };

  // every branch up to the pixel walk is uniform over the workgroup
  if (m < 0 || m > p.top_stride) { finish(-1, 0); return; }  // did not fit upstream
  const long long h = mpost_side(p.im_size[2 * n]), w = mpost_side(p.im_size[2 * n + 1]);
  if (h * w > DTC_MPOST_MAX_PIXELS) { finish(-1, 0); return; }
  const uint32_t hw = (uint32_t)(h * w), H = (uint32_t)h;

  // the top's area: is any pixel of a one-run inside the image
  {
    unsigned long long pos = 0;
    int has = 0;
    for (int base = 0; base < m && pos < hw; base += kVoteThreads) {
      const int k = base + tid;
      const unsigned long long len = k < m ? (unsigned long long)in[k] : 0ull;
      unsigned long long len_tot;
      const unsigned long long s = pos + vote_block_scan(len, VoteAdd(), 0ull, scan_s, &len_tot);
      has |= ((k & 1) && len > 0 && s < hw) ? 1 : 0;
      pos += len_tot;
    }
    if (!__syncthreads_or(has)) { copy(); return; }
  }

  // the voters, in index order
  const int n_all = mpost_count(p.all_count, n, p.A);
  const double* ovr = p.ovr + row * p.A;
  int nv = 0;
  for (int base = 0; base < p.A; base += kVoteThreads) {
    const int k = base + tid;
    const int is = (k < n_all && ovr[k] >= p.iou_thresh) ? 1 : 0;
    int tot;
    const int at = nv + vote_block_scan(is, VoteAdd(), 0, scan_s, &tot);
    if (is) v_idx[at] = k;
    nv += tot;
  }
  __syncthreads();
  if (nv < 2) { copy(); return; }

  uint32_t lo = 0xffffffffu, hi = 0u;
  for (int i = tid; i < nv; i += kVoteThreads) {
    const size_t arow = (size_t)n * p.A + v_idx[i];
    const float* d = p.all_dets + arow * p.dets_stride;
    int4 box;
    vote_slice(vote_trunc(d[0]), vote_trunc(d[2]), w, &box.x, &box.y);
    vote_slice(vote_trunc(d[1]), vote_trunc(d[3]), h, &box.z, &box.w);
    const double s = (double)d[4];
    v_box[i] = box; v_win[i] = s != s ? s : (s > kVoteFloor ? s : kVoteFloor);
    v_n[i] = p.all_n[arow];
    const uint2 span = p.all_span[arow];
    lo = min(lo, span.x); hi = max(hi, span.y);
  }
  {
    uint32_t tot;
    vote_block_scan(lo, VoteMin(), 0xffffffffu, scan_s, &tot); lo = tot;
    vote_block_scan(hi, VoteMax(), 0u, scan_s, &tot); hi = tot;   // (its barriers also publish the voters' LDS)
  }
  const bool avg = p.method == DTC_MPOST_VOTE_AVG;
  const double bt = p.binarize_thresh;
  if (avg && bt < 0.0) { lo = 0u; hi = hw; }                 // 0 / den > a negative threshold: a pixel no voter has is on
  else if (lo >= hi) { lo = 0u; hi = 0u; }                   // no voter has a pixel: nothing is on
  else hi = min(hi + 1u, hw);                                // one pixel past the last: it ends the last run of ones
  const uint32_t* all_ends = p.all_ends + (size_t)n * p.A * p.all_stride;

  int nb = 0, prev_val = 0;                                  // nb: run starts so far; the pixel in front of the walk is off
  uint32_t prev_start = 0u;
  const bool can_skip = !(avg && bt < 0.0);                   // a chunk no voter has a pixel in is off
  for (uint32_t base = lo; base < hi; base += kVoteThreads) {
    bool empty = false;
    if (can_skip) {                                          // thread i looks voter i up at the front of the chunk
      const uint32_t chunk_end = min(base + (uint32_t)kVoteThreads, hi);
      uint32_t next = hi;                                    // where the nearest run behind the chunk starts
      int has = 0;
      for (int i = tid; i < nv; i += kVoteThreads) {
        const int nk = v_n[i];
        const uint32_t* ends = all_ends + (size_t)v_idx[i] * p.all_stride;
        const int r = mpost_run_at(ends, nk, base);
        if (r < nk) {
          const uint32_t e = ends[r];                        // base is in a one-run, or in zeros that end at e
          if ((r & 1) || e < chunk_end) has = 1; else next = min(next, e);
        }
      }
      empty = !__syncthreads_or(has);
      if (empty && prev_val == 0) {                          // nothing to end, nothing to start: on to where a run may start
        uint32_t next_tot;
        vote_block_scan(next, VoteMin(), 0xffffffffu, scan_s, &next_tot);
        base = min(next_tot, hi) - (uint32_t)kVoteThreads;   // (next_tot >= chunk_end: the loop moves forward)
        continue;
      }
    }
    const uint32_t x = base + tid;
    const bool act = x < hi;
    int val = 0;
    if (act && !empty) {
      const int c = (int)(x / H), y = (int)(x - (uint32_t)c * H);
      double num = 0.0, den = 0.0;
      bool any = false;
      for (int i = 0; i < nv; i++) {
        const int nk = v_n[i];
        const int r = mpost_run_at(all_ends + (size_t)v_idx[i] * p.all_stride, nk, x);
        const bool on = r < nk && (r & 1);
        any |= on;
        if (avg) {
          const int4 box = v_box[i];
          const double wt = (c >= box.x && c < box.y && y >= box.z && y < box.w) ? v_win[i] : kVoteFloor;
          num = num + wt * (on ? 1.0 : 0.0);
          den = den + wt;
        }
      }
      val = avg ? (num / den > bt ? 1 : 0) : (any ? 1 : 0);
    }
    val_s[tid] = val;
    __syncthreads();
    const bool is_start = act && val != (tid ? val_s[tid - 1] : prev_val);
    int st_tot;
    const int q = vote_block_scan(is_start ? 1 : 0, VoteAdd(), 0, scan_s, &st_tot);
    if (is_start) bl_s[q] = x;
    __syncthreads();
    if (tid < st_tot) {                                      // the run that ends at this start
      const int idx = nb + tid;
      if (idx < p.out_stride) out[idx] = bl_s[tid] - (tid ? bl_s[tid - 1] : prev_start);
    }
    const int next_val = val_s[min((uint32_t)kVoteThreads, hi - base) - 1u];
    const uint32_t next_start = st_tot ? bl_s[st_tot - 1] : prev_start;
    __syncthreads();
    prev_val = next_val; prev_start = next_start; nb += st_tot;
  }
  const int total = nb + 1;
  if (tid == 0 && nb < p.out_stride) out[nb] = hw - prev_start;
  finish(total <= p.out_stride ? total : -1, total);
}

struct MpostVoteLayout { size_t ends, n, span, total; };

__host__ inline MpostVoteLayout mpost_vote_layout(int batch, int A, int all_stride) {
  Carve c{16};
  MpostVoteLayout l;
  l.ends = c.take((size_t)batch * A * all_stride * sizeof(uint32_t));
  l.n = c.take((size_t)batch * A * sizeof(int32_t));
  l.span = c.take((size_t)batch * A * sizeof(uint2));
  l.total = c.end;
  return l;
}

}  // namespace dtc

DTC_API size_t dtc_mpost_vote_workspace_bytes(int batch, int all_rows, int all_runs_stride) {
  if (dtc::mpost_rows_shape(batch, all_rows, all_runs_stride) != DTC_OK) return 0;
  return dtc::mpost_vote_layout(batch, all_rows, all_runs_stride).total;
}

DTC_API int dtc_mpost_vote(const uint32_t* top_runs, const int32_t* top_n_runs, const int32_t* top_count, const uint32_t* all_runs,
                           const int32_t* all_n_runs, const float* all_dets, const int32_t* all_count, const double* ovr,
                           const float* im_size, int batch, int top_rows, int top_runs_stride, int all_rows, int all_runs_stride,
                           int dets_stride, double iou_thresh, double binarize_thresh, int method, void* workspace,
                           size_t workspace_bytes, uint32_t* out_runs, int out_stride, int32_t* out_n_runs, int32_t* need,
                           dtc_stream_t stream) {
  // shapes and parameters, then limits
  const int shape = dtc::mpost_worst(dtc::mpost_worst(dtc::mpost_rows_shape(batch, top_rows, top_runs_stride),
                                                      dtc::mpost_rows_shape(batch, all_rows, all_runs_stride)),
                                     dtc::mpost_rows_shape(1, 1, out_stride));
  if (shape == DTC_EINVAL || dets_stride < 5 || (method != DTC_MPOST_VOTE_AVG && method != DTC_MPOST_VOTE_UNION)) return DTC_EINVAL;
  if (shape != DTC_OK) return shape;
  // pointers
  if (!top_runs || !top_n_runs || !top_count || !all_runs || !all_n_runs || !all_dets || !all_count || !ovr || !im_size || !out_runs ||
      !out_n_runs || !need)
    return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return DTC_EINVAL;
  {
    const size_t no = (size_t)batch * top_rows * out_stride * 4;
    if (dtc::mpost_overlap(out_runs, no, top_runs, (size_t)batch * top_rows * top_runs_stride * 4) ||
        dtc::mpost_overlap(out_runs, no, all_runs, (size_t)batch * all_rows * all_runs_stride * 4))
      return DTC_EINVAL;                                     // out_runs must not overlap an input list
  }
  // workspace
  const dtc::MpostVoteLayout l = dtc::mpost_vote_layout(batch, all_rows, all_runs_stride);
  if (!workspace || workspace_bytes < l.total) return DTC_EWORKSPACE;

  char* ws = static_cast<char*>(workspace);
  dtc::MpostVoteParams p{};
  p.top_runs = top_runs; p.top_n_runs = top_n_runs; p.top_count = top_count; p.all_runs = all_runs; p.all_n_runs = all_n_runs;
  p.all_dets = all_dets; p.all_count = all_count; p.ovr = ovr; p.im_size = im_size;
  p.T = top_rows; p.top_stride = top_runs_stride; p.A = all_rows; p.all_stride = all_runs_stride; p.dets_stride = dets_stride;
  p.method = method; p.out_stride = out_stride; p.iou_thresh = iou_thresh; p.binarize_thresh = binarize_thresh;
  p.all_ends = reinterpret_cast<uint32_t*>(ws + l.ends); p.all_n = reinterpret_cast<int32_t*>(ws + l.n);
  p.all_span = reinterpret_cast<uint2*>(ws + l.span);
  p.out_runs = out_runs; p.out_n_runs = out_n_runs; p.need = need;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::mpost_vote_prepare_kernel, dim3(all_rows, batch), dim3(dtc::kMpostWave), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::mpost_vote_kernel, dim3(top_rows, batch), dim3(dtc::kVoteThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
