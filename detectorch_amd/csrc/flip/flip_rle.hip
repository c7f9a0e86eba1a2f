// COCO run lists mirrored left to right without a bitmap (include/detectorch_flip_hip.h, entry 4, has the contract and the
// formulation).  One kernel node, one workgroup per (image, row), two passes with a workgroup barrier in between:
//   1  the runs in chunks of kFlipThreads, one run per thread: carried scans give every run its start, its pieces (head, block of
//      whole columns, tail) their index in input order, and every piece the index at which its column group starts.  The pieces go
//      to the workspace as (new start << 2 | starts a group << 1 | value); zero-length runs leave no piece, so the pieces tile the
//      image.
//   2  the output order in chunks: output piece o is input piece T - 1 - o mirrored inside its column group [gs, ge); ge comes from
//      a carried min-scan over the group marks, walked downwards.  A piece whose value differs from the one in front of it starts
//      a run; the differences of those starts are the runs.
// Integers only, no atomics: the same bits on every run.
#include <climits>

#include "dtc_common.h"

#include "../../../include/detectorch_flip_hip.h"

namespace dtc {

constexpr int kFlipThreads = 256;
constexpr int kFlipPiecesPerRun = 3;

struct FlipRleParams {
  const uint32_t* runs; const int32_t* n_runs; const int32_t* counts; const float* im_size; const int32_t* flipped;
  int R, runs_stride, out_stride;
  uint32_t* rec;                               // workspace [N, R, 3 runs_stride]: the pieces in input order
  uint32_t* gs;                                // workspace [N, R, 3 runs_stride]: the first piece of the piece's column group
  uint32_t* out_runs; int32_t* out_n_runs; int32_t* need;
};

// one side of im_size as an integer: truncated; below 1, NaN: 0; above 2^30: 2^30 (dtc_segm_iou's rule)
__device__ __forceinline__ long long flip_side(float v) {
  if (!(v >= 1.f)) return 0;
  return v >= (float)DTC_FLIP_MAX_PIXELS ? (long long)DTC_FLIP_MAX_PIXELS : (long long)(int)v;
}

struct FlipAdd { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct FlipMax { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a > b ? a : b; } };
struct FlipMin { template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a < b ? a : b; } };

// EXCLUSIVE scan of v under op over the threads of the workgroup (ident in front of thread 0), and the total; ws: kFlipThreads / 64
// slots of 8 bytes.  Two barriers; ws may be used again on return.
template <typename T, typename Op>
__device__ __forceinline__ T flip_block_scan(T v, Op op, T ident, unsigned long long* ws_raw, T* total) {
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
  for (int k = 0; k < kFlipThreads / 64; k++) { const T c = ws[k]; if (k < wv) before = op(before, c); tot = op(tot, c); }
  __syncthreads();
  *total = tot;
  return op(before, excl);
}

__global__ __launch_bounds__(kFlipThreads) void flip_rle_kernel(FlipRleParams p) {
  __shared__ unsigned long long scan_s[kFlipThreads / 64];
  __shared__ uint32_t bl_s[kFlipThreads];
  __shared__ int val_s[kFlipThreads];
  const int r = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const int cnt = p.counts ? min(max(p.counts[n], 0), p.R) : p.R;
  if (r >= cnt) return;                        // rows past the count are not written
  const size_t row = (size_t)n * p.R + r;
  const int m = p.n_runs[row];
  const uint32_t* in = p.runs + row * p.runs_stride;
  uint32_t* out = p.out_runs + row * p.out_stride;
  auto finish = [&](int n_runs, int need) { if (tid == 0) { p.out_n_runs[row] = n_runs; p.need[row] = need; } };

  // every branch up to pass 2 is uniform over the workgroup
  if (m < 0 || m > p.runs_stride) { finish(-1, 0); return; }   // did not fit upstream
  if (p.flipped[n] == 0) {                     // copied as it is
    const bool fits = m <= p.out_stride;
    if (fits) for (int k = tid; k < m; k += kFlipThreads) out[k] = in[k];
    finish(fits ? m : -1, m);
    return;
  }
  if (m == 0) { finish(0, 0); return; }        // no segmentation
  const long long h = flip_side(p.im_size[2 * n]), w = flip_side(p.im_size[2 * n + 1]);
  if (h * w > DTC_FLIP_MAX_PIXELS) { finish(-1, 0); return; }
  const unsigned long long hw = (unsigned long long)(h * w);
  const uint32_t H = (uint32_t)h, W = (uint32_t)w;
  uint32_t* rec = p.rec + row * kFlipPiecesPerRun * p.runs_stride;
  uint32_t* gsa = p.gs + row * kFlipPiecesPerRun * p.runs_stride;

  // ---- pass 1: the pieces in input order.  Piece indices stay below 3 m <= 3 runs_stride.
  unsigned long long pos = 0;                  // the pixels in front of the chunk
  int T = 0, glast = -1;                       // the pieces in front of the chunk; the last group start among them
  for (int base = 0; base < m && pos <= hw; base += kFlipThreads) {
    const int k = base + tid;
    const unsigned long long len = k < m ? (unsigned long long)in[k] : 0ull;
    unsigned long long len_tot;
    const unsigned long long s = pos + flip_block_scan(len, FlipAdd(), 0ull, scan_s, &len_tot), e = s + len;
    uint32_t c0 = 0, c1 = 0, y0 = 0;
    int np = 0;
    if (len > 0 && e <= hw) {                  // (H >= 1 here: hw >= e > 0)
      c0 = (uint32_t)s / H; y0 = (uint32_t)s - c0 * H; c1 = ((uint32_t)e - 1u) / H;
      np = 1 + (c1 > c0 ? 1 : 0) + (c1 > c0 + 1u ? 1 : 0);
    }
    int np_tot, g_tot;
    const int pb = T + flip_block_scan(np, FlipAdd(), 0, scan_s, &np_tot);
    const bool head_starts = y0 == 0;          // nothing of this column in front of the head
    const int my_last = np == 0 ? -1 : np == 1 ? (head_starts ? pb : -1) : pb + np - 1;
    const int g_before = max(glast, flip_block_scan(my_last, FlipMax(), -1, scan_s, &g_tot));
    if (np > 0) {
      const uint32_t v = (uint32_t)k & 1u;
      rec[pb] = (((W - 1u - c0) * H + y0) << 2) | (head_starts ? 2u : 0u) | v;
      gsa[pb] = (uint32_t)(head_starts ? pb : g_before);
      int j = pb + 1;
      if (c1 > c0 + 1u) { rec[j] = (((W - c1) * H) << 2) | 2u | v; gsa[j] = (uint32_t)j; j++; }    // columns c0 + 1 .. c1 - 1
      if (c1 > c0) { rec[j] = (((W - 1u - c1) * H) << 2) | 2u | v; gsa[j] = (uint32_t)j; }
    }
    pos += len_tot; T += np_tot; glast = max(glast, g_tot);
  }
  if (pos != hw) { finish(-1, 0); return; }    // the runs do not sum to h w
  __syncthreads();                             // the pieces are in the workspace for every thread
  if (T == 0) {                                // an image of 0 pixels
    if (tid == 0) out[0] = 0u;
    finish(1, 1);
    return;
  }

  // ---- pass 2: the output order
  int ge_carry = INT_MAX, nb = 0, prev_val = -1, lead = 0;     // nb: run starts so far; lead: 1 when the first pixel is set
  uint32_t prev_start = 0u;
  for (int base = 0; base < T; base += kFlipThreads) {
    const int o = base + tid, ip = T - 1 - o;
    const bool act = o < T;
    int cand = INT_MAX;                        // the nearest group start behind piece ip, as far as this thread sees
    if (act) cand = ip + 1 == T ? T : ((rec[ip + 1] & 2u) ? ip + 1 : INT_MAX);
    int cand_tot;
    const int cand_before = flip_block_scan(cand, FlipMin(), INT_MAX, scan_s, &cand_tot);
    const int ge = min(ge_carry, min(cand_before, cand));
    uint32_t start = 0u;
    int val = -2;
    if (act) {
      const int src = min(max((int)gsa[ip] + ge - 1 - ip, 0), T - 1);
      const uint32_t rc = rec[src];
      start = rc >> 2; val = (int)(rc & 1u);
    }
    val_s[tid] = val;
    __syncthreads();
    const bool is_start = act && val != (tid ? val_s[tid - 1] : prev_val);
    if (base == 0) lead = val_s[0];
    int st_tot;
    const int q = flip_block_scan(is_start ? 1 : 0, FlipAdd(), 0, scan_s, &st_tot);
    if (is_start) bl_s[q] = start;
    __syncthreads();
    if (tid < st_tot && nb + tid > 0) {        // the run that ends at this start
      const int idx = nb + tid - 1 + lead;
      if (idx < p.out_stride) out[idx] = bl_s[tid] - (tid ? bl_s[tid - 1] : prev_start);
    }
    const int next_val = val_s[min(kFlipThreads, T - base) - 1];
    const uint32_t next_start = st_tot ? bl_s[st_tot - 1] : prev_start;
    __syncthreads();
    prev_val = next_val; prev_start = next_start; nb += st_tot; ge_carry = min(ge_carry, cand_tot);
  }
  const int total = nb + lead;
  if (tid == 0) {
    if (lead) out[0] = 0u;                     // (out_stride >= 1)
    if (total - 1 < p.out_stride) out[total - 1] = (uint32_t)hw - prev_start;
  }
  finish(total <= p.out_stride ? total : -1, total);
}

struct FlipLayout { size_t rec, gs, total; };

__host__ inline FlipLayout flip_layout(int batch, int R, int runs_stride) {
  Carve c{16};
  FlipLayout l;
  const size_t pieces = (size_t)batch * R * kFlipPiecesPerRun * runs_stride;
  l.rec = c.take(pieces * sizeof(uint32_t));
  l.gs = c.take(pieces * sizeof(uint32_t));
  l.total = c.end;
  return l;
}

__host__ inline int flip_rle_shape(int batch, int R, int runs_stride) {
  if (batch < 1 || R < 0 || runs_stride < 1) return DTC_EINVAL;
  if (batch > DTC_FLIP_MAX_BATCH || R > DTC_FLIP_MAX_ROWS || runs_stride > DTC_FLIP_MAX_RUNS) return DTC_EUNSUPPORTED;
  return DTC_OK;
}

}  // namespace dtc

DTC_API size_t dtc_flip_rle_workspace_bytes(int batch, int rows_stride, int runs_stride) {
  if (dtc::flip_rle_shape(batch, rows_stride, runs_stride) != DTC_OK) return 0;
  return dtc::flip_layout(batch, rows_stride, runs_stride).total + 16;        // (never 0 for a supported shape, R = 0 included)
}

DTC_API int dtc_flip_rle(const uint32_t* runs, const int32_t* n_runs, const int32_t* counts, const float* im_size, const int32_t* flipped,
                         int batch, int rows_stride, int runs_stride, void* workspace, size_t workspace_bytes, uint32_t* out_runs,
                         int out_stride, int32_t* out_n_runs, int32_t* need, dtc_stream_t stream) {
  // shapes and parameters, then limits
  const int R = rows_stride;
  const int shape = dtc::flip_rle_shape(batch, R, runs_stride);
  if (shape == DTC_EINVAL || out_stride < 1) return DTC_EINVAL;
  if (shape != DTC_OK || out_stride > DTC_FLIP_MAX_RUNS) return DTC_EUNSUPPORTED;
  // pointers
  if (!im_size || !flipped) return DTC_EINVAL;
  if (R > 0 && (!runs || !n_runs || !out_runs || !out_n_runs || !need)) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return DTC_EINVAL;
  {
    const uintptr_t a = reinterpret_cast<uintptr_t>(runs), b = reinterpret_cast<uintptr_t>(out_runs);
    const size_t na = (size_t)batch * R * runs_stride * 4, nb = (size_t)batch * R * out_stride * 4;
    if (R > 0 && a < b + nb && b < a + na) return DTC_EINVAL;                  // out_runs must not overlap runs
  }
  // workspace
  const dtc::FlipLayout l = dtc::flip_layout(batch, R, runs_stride);
  if (!workspace || workspace_bytes < l.total + 16) return DTC_EWORKSPACE;
  if (R == 0) return DTC_OK;                   // no row: no output element

  char* ws = static_cast<char*>(workspace);
  dtc::FlipRleParams p{};
  p.runs = runs; p.n_runs = n_runs; p.counts = counts; p.im_size = im_size; p.flipped = flipped;
  p.R = R; p.runs_stride = runs_stride; p.out_stride = out_stride;
  p.rec = reinterpret_cast<uint32_t*>(ws + l.rec); p.gs = reinterpret_cast<uint32_t*>(ws + l.gs);
  p.out_runs = out_runs; p.out_n_runs = out_n_runs; p.need = need;
  hipLaunchKernelGGL(dtc::flip_rle_kernel, dim3(R, batch), dim3(dtc::kFlipThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
