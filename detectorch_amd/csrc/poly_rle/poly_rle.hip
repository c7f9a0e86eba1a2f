// annToRLE of polygon annotations for gfx950 (include/detectorch_poly_hip.h has the contract): the polygons of one gt row at image
// size, straight to COCO's run list, no bitmap.  Kernel nodes, one workgroup per (image, gt row) each:
//   1  poly_events   validates the row's polygons and traces their edges: one edge per thread, and one edge per wavefront -- its
//                    lanes over the pixel columns -- where an edge spans more than kPolyLongSpan columns; per column the closed form
//                    when dx >= dy and a bisection on the monotone trace when dx < dy (csrc/mask_train/mask_targets.hip's
//                    mask_edge_events with M split into h and w).  The events go to the workspace as keys (polygon << 32 | position)
//                    in the order of an LDS counter; the count goes there too (-1: a row that takes part in nothing).
//   2  poly_runs     sorts the keys in LDS (block_sort.h's LSD radix sort, the digits in use only); event r of a polygon whose first
//                    event is at s starts a span when r - s is even and ends one when it is odd; the keys (position << 1 | end) are
//                    sorted again; a scan of +1 / -1 gives the coverage in front of every event; the last event of every position
//                    compares the coverage in front of the position's first event with the one behind itself: where exactly one of
//                    them is 0, the position is a boundary; the differences of the boundaries are the runs.
// Positions are below 2^30 and fit 32 bits; i * h + j is formed in 64 bits.  Integer LDS atomics only, and nothing after the sorts
// depends on the order of the first node's stores: the same bits on every run.
#include <cmath>

#include "block_sort.h"
#include "wave_ops.h"

#include "../../../include/detectorch_poly_hip.h"

namespace dtc {

constexpr int kPolyGenThreads = 256;          // node 1
constexpr int kPolyLongSpan = 32;             // an edge over more pixel columns is traced by a wavefront
constexpr int kPolyKeysPerThread = 8;         // node 2: its workgroup sorts kPolyKeysPerThread keys per thread at the most
constexpr int kPolyMaxEvents = 8192;
static_assert(kPolyMaxEvents == DTC_POLY_MAX_EVENTS && kPolyMaxEvents == 1024 * kPolyKeysPerThread, "the largest workgroup sorts them all");
constexpr double kPolyCoordLimit = 67108864.0;   // 2^26: 5 x + 0.5 stays far inside an int

struct PolyParams {
  const double* poly_xy; const int32_t* poly_ptr; const int32_t* gt_poly_ptr; const int32_t* gt_counts; const float* im_size;
  int G, PTS, NP, events_stride, runs_stride;
  uint64_t* keys;                              // workspace [N, G, events_stride]
  int32_t* count;                              // workspace [N, G]: the events of the row, -1: the row takes part in nothing
  uint32_t* runs; int32_t* n_runs; int32_t* area; int32_t* need;
};

// one side of im_size as an integer: truncated; below 1, NaN: 0; above 2^30: 2^30 (dtc_segm_iou's rule)
__device__ __forceinline__ long long poly_side(float v) {
  if (!(v >= 1.f)) return 0;
  return v >= (float)DTC_POLY_MAX_PIXELS ? (long long)DTC_POLY_MAX_PIXELS : (long long)(int)v;
}

// C's (int): the arguments stay below 2^30 in magnitude
__device__ __forceinline__ int poly_trunc(double v) { return (int)v; }
__device__ __forceinline__ int poly_floor_div5(int a) { return a >= 0 ? a / 5 : -((4 - a) / 5); }

// an edge on the 5x grid, ready to be asked for the event of a pixel column: the ends swapped so that the major coordinate increases
struct PolyEdge {
  int xs, ys, len;                             // the start, and dx (shallow) or dy (steep)
  double s;                                    // the slope per step of the major coordinate
  int u0, u1;                                  // steep: the first and the last u of the trace
  int i_lo, i_hi;                              // the pixel columns whose centre line 5 i + 2 the trace can cross (none: i_lo > i_hi)
  bool shallow;
};

// |coordinates| < 2^26 * 5 + 1: dx, dy < 2^30 and every 5 i + 2 below is inside an int, i_hi being at most xe / 5
__device__ __forceinline__ PolyEdge poly_edge(int xs, int ys, int xe, int ye, int w) {
  PolyEdge e;
  const int dx = abs(xe - xs), dy = abs(ye - ys);
  e.shallow = dx >= dy;
  e.u0 = e.u1 = 0;
  if (dx == 0 && dy == 0) { e.xs = xs; e.ys = ys; e.len = 0; e.s = 0.0; e.i_lo = 0; e.i_hi = -1; return e; }
  if (e.shallow) {
    if (xs > xe) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    e.s = (double)(ye - ys) / (double)dx;
    e.len = dx;
    // pairs (t, t + 1), t = 0 .. dx - 1: us = xs + t = 5 i + 2
    e.i_lo = max(0, poly_floor_div5(xs - 2 + 4));
    e.i_hi = min(w - 1, poly_floor_div5(xe - 1 - 2));
  } else {
    if (ys > ye) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    e.s = (double)(xe - xs) / (double)dy;
    e.len = dy;
    e.u0 = poly_trunc((double)xs + e.s * 0.0 + 0.5);
    e.u1 = poly_trunc((double)xs + e.s * (double)dy + 0.5);
    const int lo = min(e.u0, e.u1), hi = max(e.u0, e.u1);
    e.i_lo = max(0, poly_floor_div5(lo - 2 + 4));
    e.i_hi = min(w - 1, poly_floor_div5(hi - 1 - 2));
  }
  e.xs = xs; e.ys = ys;
  return e;
}

// the event of pixel column i_lo <= i <= i_hi of the edge: false, or the smaller v of its pair of trace points
__device__ __forceinline__ bool poly_edge_column(const PolyEdge& e, int i, int* vs) {
  const int c = 5 * i + 2;
  if (e.shallow) {
    const int t = c - e.xs;
    const int va = poly_trunc((double)e.ys + e.s * (double)t + 0.5), vb = poly_trunc((double)e.ys + e.s * (double)(t + 1) + 0.5);
    *vs = min(va, vb);
    return true;
  }
  auto u_of = [&](int t) { return poly_trunc((double)e.xs + e.s * (double)t + 0.5); };   // monotone in t
  const bool rising = e.u0 < e.u1;
  int a = 0, z = e.len;                        // rising: u(a) <= c < u(z); falling: u(a) > c >= u(z)
  while (z - a > 1) {
    const int m = a + ((z - a) >> 1);
    const bool left = rising ? u_of(m) <= c : u_of(m) > c;
    if (left) a = m; else z = m;
  }
  *vs = e.ys + a;                              // us = min(u) = c; vs = min(v) = ys + a
  return (rising ? u_of(a) : u_of(z)) == c;
}

__global__ __launch_bounds__(kPolyGenThreads) void poly_events_kernel(PolyParams p) {
  __shared__ unsigned int count_s;
  const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const size_t row = (size_t)n * p.G + g;
  const long long h = poly_side(p.im_size[2 * n]), w = poly_side(p.im_size[2 * n + 1]);
  const long long hw = h * w > DTC_POLY_MAX_PIXELS ? (long long)DTC_POLY_MAX_PIXELS : h * w;
  const int ng = min(max(p.gt_counts[n], 0), p.G);
  int q0 = 0, q1 = 0;
  bool live = g < ng && hw > 0 && p.NP > 0 && p.PTS > 0;
  if (live) {
    const int32_t* gp = p.gt_poly_ptr + (size_t)n * (p.G + 1);
    q0 = gp[g]; q1 = gp[g + 1];
    live = q0 >= 0 && q1 <= p.NP && q0 <= q1;
  }
  if (!live) {                                 // uniform
    if (tid == 0) p.count[row] = -1;
    return;
  }
  if (tid == 0) count_s = 0u;
  const double* pts = p.poly_xy + (size_t)n * p.PTS * 2;
  const int32_t* pp = p.poly_ptr + (size_t)n * (p.NP + 1);
  uint64_t* keys = p.keys + row * p.events_stride;
  const unsigned int cap = (unsigned int)p.events_stride;
  const double hd = (double)h;

  auto emit = [&](uint64_t poly, int i, int vs) {
    const double yd = fmin(fmax(((double)vs + 0.5) / 5.0 - 0.5, 0.0), hd);
    const long long pos = (long long)i * h + (long long)ceil(yd);
    if (pos < hw) {
      const unsigned int slot = atomicAdd(&count_s, 1u);
      if (slot < cap) keys[slot] = (poly << 32) | (uint64_t)pos;
    }
  };
  auto vertex = [&](int i, int* X, int* Y) {
    *X = poly_trunc(5.0 * pts[2 * (size_t)i] + 0.5);
    *Y = poly_trunc(5.0 * pts[2 * (size_t)i + 1] + 0.5);
  };

  int n_valid = 0;                             // the same in every thread
  for (int q = q0; q < q1; q++) {
    const int ps = pp[q], pe = pp[q + 1];      // offsets are data and never become an address unchecked
    if (!(ps >= 0 && pe <= p.PTS && ps <= pe - 3)) continue;
    bool bad = false, big = false;
    for (int i = ps + tid; i < pe; i += kPolyGenThreads) {
      const double x = pts[2 * (size_t)i], y = pts[2 * (size_t)i + 1];
      bad |= !(isfinite(x) && isfinite(y));
      big |= !(fabs(x) < kPolyCoordLimit && fabs(y) < kPolyCoordLimit);
    }
    if (__syncthreads_or(bad ? 1 : 0)) continue;               // (also: count_s is initialised)
    n_valid++;
    if (__syncthreads_or(big ? 1 : 0)) continue;
    const int np = pe - ps;
    const uint64_t poly = (uint64_t)(q - q0);
    const int wi = (int)w;
    for (int k = tid; k < np; k += kPolyGenThreads) {          // one edge per thread: those over few columns
      int xs, ys, xe, ye;
      vertex(ps + k, &xs, &ys);
      vertex(ps + (k + 1 == np ? 0 : k + 1), &xe, &ye);
      const PolyEdge e = poly_edge(xs, ys, xe, ye, wi);
      if (e.i_hi - e.i_lo >= kPolyLongSpan) continue;
      for (int i = e.i_lo; i <= e.i_hi; i++) {
        int vs;
        if (poly_edge_column(e, i, &vs)) emit(poly, i, vs);
      }
    }
    for (int k = wv; k < np; k += kPolyGenThreads / 64) {      // one edge per wavefront, the lanes over its columns: the others
      int xs, ys, xe, ye;
      vertex(ps + k, &xs, &ys);
      vertex(ps + (k + 1 == np ? 0 : k + 1), &xe, &ye);
      const PolyEdge e = poly_edge(xs, ys, xe, ye, wi);
      if (e.i_hi - e.i_lo < kPolyLongSpan) continue;           // wave-uniform
      for (int i = e.i_lo + lane; i <= e.i_hi; i += 64) {
        int vs;
        if (poly_edge_column(e, i, &vs)) emit(poly, i, vs);
      }
    }
  }
  __syncthreads();
  if (tid == 0) p.count[row] = n_valid > 0 ? (int32_t)min(count_s, 0x7fffffffu) : -1;
}

// exclusive prefix sum of v over the threads of the workgroup, and the total; ws: THREADS / 64 words
template <int THREADS>
__device__ __forceinline__ int poly_block_scan(int v, int* ws, int* total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int incl = wave_incl_scan(v, lane);
  if (lane == 63) ws[wv] = incl;
  __syncthreads();
  int before = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < THREADS / 64; k++) { const int c = ws[k]; before += k < wv ? c : 0; tot += c; }
  __syncthreads();                             // ws may be written again
  *total = tot;
  return before + incl - v;
}

// the first index in the ascending keys[0 .. n) whose key is at least `target`
__device__ __forceinline__ int poly_lower_bound(const uint64_t* keys, int n, uint64_t target) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// the digits (8 bits each) in which keys whose OR is `any` can differ
__device__ __forceinline__ uint32_t poly_digit_mask(uint64_t any) {
  uint32_t m = 0;
#pragma unroll
  for (int d = 0; d < 8; d++) m |= ((any >> (8 * d)) & 255ull) ? 1u << d : 0u;
  return m;
}

// node 2's LDS, all of it dynamic (a static variable in front of the dynamic region would take the 64-bit keys off their alignment):
// two key buffers, the radix sort's counters per wavefront and digit bases, 16 words for the scans and 4 single words
__host__ __device__ constexpr size_t poly_runs_lds_bytes(int threads) {
  return (size_t)2 * 8 * threads * kPolyKeysPerThread + (size_t)(threads / 64) * 256 * 4 + 256 * 4 + (16 + 4) * 4;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void poly_runs_kernel(PolyParams p) {
  constexpr int CAP = THREADS * kPolyKeysPerThread, NW = THREADS / 64;
  extern __shared__ __attribute__((aligned(16))) unsigned char poly_smem[];
  uint64_t* buf_a = reinterpret_cast<uint64_t*>(poly_smem);
  uint64_t* buf_b = buf_a + CAP;
  uint32_t* rcnt = reinterpret_cast<uint32_t*>(buf_b + CAP);   // [NW * 256]
  uint32_t* dig = rcnt + NW * 256;                             // [256]
  int* scan_s = reinterpret_cast<int*>(dig + 256);             // [16 >= NW]
  uint32_t& any_lo_s = dig[256 + 16];
  uint32_t& any_hi_s = dig[256 + 17];
  uint32_t& area_s = dig[256 + 18];
  const int g = blockIdx.x, n = blockIdx.y, tid = threadIdx.x;
  const size_t row = (size_t)n * p.G + g;
  const int n_ev = p.count[row];
  uint32_t* runs = p.runs + row * p.runs_stride;

  if (n_ev < 0 || n_ev > min(p.events_stride, CAP)) {          // uniform: takes part in nothing, or the events did not fit
    if (tid == 0) {
      p.n_runs[row] = n_ev < 0 ? 0 : -1;
      p.area[row] = 0;
      p.need[2 * row] = max(n_ev, 0);
      p.need[2 * row + 1] = n_ev < 0 ? 0 : -1;
    }
    return;
  }
  const long long hh = poly_side(p.im_size[2 * n]), ww = poly_side(p.im_size[2 * n + 1]);
  const uint32_t hw = (uint32_t)(hh * ww > DTC_POLY_MAX_PIXELS ? (long long)DTC_POLY_MAX_PIXELS : hh * ww);

  // ---- 1: the keys (polygon, position), sorted
  if (tid == 0) { any_lo_s = 0u; any_hi_s = 0u; area_s = 0u; }
  __syncthreads();
  {
    const uint64_t* src = p.keys + row * p.events_stride;
    uint64_t any = 0;
    for (int i = tid; i < n_ev; i += THREADS) { const uint64_t k = src[i]; buf_a[i] = k; any |= k; }
    if ((uint32_t)any) atomicOr(&any_lo_s, (uint32_t)any);
    if ((uint32_t)(any >> 32)) atomicOr(&any_hi_s, (uint32_t)(any >> 32));
  }
  __syncthreads();
  const uint32_t any_lo = any_lo_s, any_hi = any_hi_s;
  uint64_t* sorted = block_radix_sort_u64<THREADS, kPolyKeysPerThread>(buf_a, buf_b, rcnt, dig, n_ev,
                                                                        poly_digit_mask(((uint64_t)any_hi << 32) | any_lo));
  uint64_t* other = sorted == buf_a ? buf_b : buf_a;

  // ---- 2: the parity of an event's rank within its polygon makes it the start or the end of a span; sorted by position
  for (int r = tid; r < n_ev; r += THREADS) {
    const uint64_t k = sorted[r];
    const int first = poly_lower_bound(sorted, n_ev, k & 0xffffffff00000000ull);
    other[r] = ((k & 0xffffffffull) << 1) | (uint64_t)((r - first) & 1);
  }
  sorted = block_radix_sort_u64<THREADS, kPolyKeysPerThread>(other, sorted, rcnt, dig, n_ev, poly_digit_mask(((uint64_t)any_lo << 1) | 1ull));
  other = sorted == buf_a ? buf_b : buf_a;
  int32_t* cover = reinterpret_cast<int32_t*>(other);          // [CAP] the coverage in front of every event
  uint32_t* bnd = reinterpret_cast<uint32_t*>(other) + CAP;    // [CAP] the boundaries, ascending

  // ---- 3: the coverage: thread tid owns the events [r0, r1)
  const int per = (n_ev + THREADS - 1) / THREADS;              // <= kPolyKeysPerThread
  const int r0 = min(tid * per, n_ev), r1 = min(r0 + per, n_ev);
  int sum = 0, total;
  for (int r = r0; r < r1; r++) sum += (sorted[r] & 1ull) ? -1 : 1;
  int c = poly_block_scan<THREADS>(sum, scan_s, &total);
  for (int r = r0; r < r1; r++) { cover[r] = c; c += (sorted[r] & 1ull) ? -1 : 1; }
  __syncthreads();

  // ---- 4: the last event of every position: a boundary where the coverage passes between 0 and at least 1 over the position
  uint32_t flags = 0;
  for (int r = r0; r < r1; r++) {
    const uint64_t k = sorted[r];
    const uint64_t pos = k >> 1;
    if (r + 1 < n_ev && (sorted[r + 1] >> 1) == pos) continue;
    const int first = poly_lower_bound(sorted, n_ev, pos << 1);
    const bool before = cover[first] > 0, after = cover[r] + ((k & 1ull) ? -1 : 1) > 0;
    if (before != after) flags |= 1u << (r - r0);
  }
  int n_bnd;
  int at = poly_block_scan<THREADS>(__builtin_popcount(flags), scan_s, &n_bnd);
  for (int r = r0; r < r1; r++)
    if ((flags >> (r - r0)) & 1u) bnd[at++] = (uint32_t)(sorted[r] >> 1);
  __syncthreads();

  // ---- 5: the runs: the differences of the boundaries, and what is left of the image behind the last one
  const int n_runs = n_bnd + 1;
  const bool fits = n_runs <= p.runs_stride;
  if (fits) {
    uint32_t ones = 0;
    for (int k = tid; k < n_runs; k += THREADS) {
      const uint32_t from = k > 0 ? bnd[k - 1] : 0u, to = k < n_bnd ? bnd[k] : hw;
      runs[k] = to - from;
      ones += (k & 1) ? to - from : 0u;
    }
    if (ones) atomicAdd(&area_s, ones);
  }
  __syncthreads();
  if (tid == 0) {
    p.n_runs[row] = fits ? n_runs : -1;
    p.area[row] = fits ? (int32_t)area_s : 0;
    p.need[2 * row] = n_ev;
    p.need[2 * row + 1] = n_runs;
  }
}

struct PolyLayout { size_t keys, count, total; };

__host__ inline PolyLayout poly_layout(int batch, int G, int events_stride) {
  Carve c{16};
  PolyLayout l;
  l.keys = c.take((size_t)batch * G * events_stride * sizeof(uint64_t));
  l.count = c.take((size_t)batch * G * sizeof(int32_t));
  l.total = c.end;
  return l;
}

__host__ inline int poly_rle_shape(int batch, int G, int PTS, int NP, int events_stride) {
  if (batch < 1 || G < 0 || PTS < 0 || NP < 0 || events_stride < 1) return DTC_EINVAL;
  if (batch > DTC_POLY_MAX_BATCH || G > DTC_POLY_MAX_GT || PTS > DTC_POLY_MAX_POINTS || NP > DTC_POLY_MAX_POLYS ||
      events_stride > DTC_POLY_MAX_EVENTS)
    return DTC_EUNSUPPORTED;
  return DTC_OK;
}

}  // namespace dtc

DTC_API const char* dtc_poly_target_arch(void) { return "gfx950"; }

DTC_API size_t dtc_poly_rle_workspace_bytes(int batch, int gt_stride, int points_stride, int polys_stride, int events_stride) {
  if (dtc::poly_rle_shape(batch, gt_stride, points_stride, polys_stride, events_stride) != DTC_OK) return 0;
  return dtc::poly_layout(batch, gt_stride, events_stride).total + 16;     // (never 0 for a supported shape, G = 0 included)
}

DTC_API int dtc_poly_rle(const double* poly_xy, const int32_t* poly_ptr, const int32_t* gt_poly_ptr, const int32_t* gt_counts,
                         const float* im_size, int batch, int gt_stride, int points_stride, int polys_stride, int events_stride,
                         void* workspace, size_t workspace_bytes, uint32_t* runs, int runs_stride, int32_t* n_runs, int32_t* area,
                         int32_t* need, dtc_stream_t stream) {
  // shapes and parameters, then limits
  const int G = gt_stride, PTS = points_stride, NP = polys_stride;
  const int shape = dtc::poly_rle_shape(batch, G, PTS, NP, events_stride);
  if (shape == DTC_EINVAL || runs_stride < 1) return DTC_EINVAL;
  if (shape != DTC_OK || runs_stride > DTC_POLY_MAX_RUNS) return DTC_EUNSUPPORTED;
  // pointers
  if (!im_size) return DTC_EINVAL;
  if (G > 0 && (!gt_poly_ptr || !gt_counts || !runs || !n_runs || !area || !need)) return DTC_EINVAL;
  if (G > 0 && NP > 0 && PTS > 0 && (!poly_xy || !poly_ptr)) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(poly_xy) & 7) != 0 || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return DTC_EINVAL;
  // workspace
  const dtc::PolyLayout l = dtc::poly_layout(batch, G, events_stride);
  if (!workspace || workspace_bytes < l.total + 16) return DTC_EWORKSPACE;
  if (G == 0) return DTC_OK;                   // no row: no output element

  char* ws = static_cast<char*>(workspace);
  dtc::PolyParams p{};
  p.poly_xy = poly_xy; p.poly_ptr = poly_ptr; p.gt_poly_ptr = gt_poly_ptr; p.gt_counts = gt_counts; p.im_size = im_size;
  p.G = G; p.PTS = PTS; p.NP = NP; p.events_stride = events_stride; p.runs_stride = runs_stride;
  p.keys = reinterpret_cast<uint64_t*>(ws + l.keys); p.count = reinterpret_cast<int32_t*>(ws + l.count);
  p.runs = runs; p.n_runs = n_runs; p.area = area; p.need = need;
  if (dtc::raise_lds_once<dtc::poly_runs_kernel<256>, dtc::poly_runs_kernel<512>, dtc::poly_runs_kernel<1024>>(152 * 1024) != DTC_OK)
    return DTC_ELAUNCH;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(G, batch);
  hipLaunchKernelGGL(dtc::poly_events_kernel, grid, dim3(dtc::kPolyGenThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  // the smallest workgroup whose sort holds events_stride keys: 2048, 4096 or 8192
  if (events_stride <= 256 * dtc::kPolyKeysPerThread)
    hipLaunchKernelGGL(dtc::poly_runs_kernel<256>, grid, dim3(256), dtc::poly_runs_lds_bytes(256), s, p);
  else if (events_stride <= 512 * dtc::kPolyKeysPerThread)
    hipLaunchKernelGGL(dtc::poly_runs_kernel<512>, grid, dim3(512), dtc::poly_runs_lds_bytes(512), s, p);
  else
    hipLaunchKernelGGL(dtc::poly_runs_kernel<1024>, grid, dim3(1024), dtc::poly_runs_lds_bytes(1024), s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
