// Mask targets of a Mask R-CNN minibatch for gfx950 (include/detectorch_mask_hip.h has the contract): Detectron's add_mask_rcnn_blobs
// on the compact output of dtc_fast_rcnn_targets.  Kernel nodes:
//   1  mask_rows     one workgroup per image: the foreground rows in row order (or the fallback row), the poly-box of every eligible
//                    gt (one wavefront per gt, its lanes over the points), the matching of every mask row (one row per thread against
//                    the poly-boxes in LDS); writes every per-row output and, for node 2, the matched gt and the box of every row
//   2  mask_raster   one workgroup per mask row: per polygon of the matched gt, the events of every edge (one edge per thread and
//                    round; closed form per pixel column when dx >= dy, a bisection on the monotone trace per column when dx < dy, so
//                    no loop is as long as a coordinate) toggle bits in LDS, a prefix parity over the M * M column-major positions
//                    turns them into the polygon's pixels, which are ORed into the row's mask
// Integer LDS atomics only (xor commutes): the same bits on every run.
#include <cmath>

#include "box_vote.h"
#include "fpn_map.h"
#include "wave_ops.h"

#include "../../../include/detectorch_mask_hip.h"

namespace dtc {

constexpr int kMaskThreads = 256;             // both kernels
constexpr int kMaskWaves = kMaskThreads / 64;
constexpr int kMaskMaxM = DTC_MASK_MAX_M;
constexpr int kMaskMaxGt = DTC_MASK_MAX_GT;
constexpr int kMaskMaxRows = DTC_MASK_MAX_ROWS;
constexpr int kMaskMaxPos = kMaskMaxM * kMaskMaxM;
constexpr int kMaskChunk = (kMaskMaxPos + kMaskThreads - 1) / kMaskThreads;   // positions per thread of the parity scan, at the most
static_assert(kMaskChunk * kMaskThreads >= kMaskMaxPos, "every position has an owner");
constexpr float kMaskCoordLimit = 67108864.f; // 2^26: 5 x + 0.5 stays far inside an int

struct MaskTargetsWs {
  int32_t* row_gt;       // [B * Fm] the matched gt, -1: the row matches nothing (or lies past n_mask)
  float4* row_box;       // [B * Fm] the row's box, original coordinates
  static size_t bytes(int B, int Fm) { Carve c{256}; c.take((size_t)B * Fm * 4); c.take((size_t)B * Fm * 16); return c.end; }
  MaskTargetsWs() = default;
  MaskTargetsWs(void* ws, int B, int Fm) {
    Carve c{256};
    char* base = static_cast<char*>(ws);
    row_gt = reinterpret_cast<int32_t*>(base + c.take((size_t)B * Fm * 4));
    row_box = reinterpret_cast<float4*>(base + c.take((size_t)B * Fm * 16));
  }
};

struct MaskTargetsParams {
  const int32_t* labels; const int32_t* keep_inds; const int32_t* n_rois;
  const float* gt_boxes; const int32_t* gt_classes; const int32_t* gt_is_crowd; const int32_t* gt_counts;
  const float* proposals; const float* im_scale; const float* poly_xy; const int32_t* poly_ptr; const int32_t* gt_poly_ptr;
  int B, R, G, P, PTS, NP, M, k_min, k_max, Fm;
  MaskTargetsWs ws;
  float* mask_rois; int32_t* masks; int32_t* mask_class; int32_t* mask_roi_levels; int32_t* roi_has_mask; int32_t* n_mask;
  int32_t* mask_gt;
};

__device__ __forceinline__ bool finite4(float4 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w); }

// the point range of polygon q < NP of image b, or false: offsets are data and never become an address unchecked
__device__ __forceinline__ bool poly_range(const MaskTargetsParams& p, int b, int q, int* ps, int* pe) {
  const int32_t* pp = p.poly_ptr + (size_t)b * (p.NP + 1);
  *ps = pp[q]; *pe = pp[q + 1];
  return *ps >= 0 && *pe <= p.PTS && *ps <= *pe - 3;
}

// the polygon range of gt g < G of image b, or false
__device__ __forceinline__ bool gt_poly_range(const MaskTargetsParams& p, int b, int g, int* q0, int* q1) {
  const int32_t* gp = p.gt_poly_ptr + (size_t)b * (p.G + 1);
  *q0 = gp[g]; *q1 = gp[g + 1];
  return *q0 >= 0 && *q1 <= p.NP && *q0 <= *q1;
}

__global__ __launch_bounds__(kMaskThreads) void mask_rows_kernel(MaskTargetsParams p) {
  __shared__ float4 g_box[kMaskMaxGt];        // poly-boxes
  __shared__ int g_ok[kMaskMaxGt];            // eligible
  __shared__ int rows_s[kMaskMaxRows];        // the minibatch row of every mask row
  __shared__ int cnt_s[kMaskWaves];
  __shared__ int first_bg_s, n_fg_s;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int R = p.R, Fm = p.Fm;
  const int n_r = min(max(p.n_rois[b], 0), R);
  const int n_g = p.G > 0 ? min(max(p.gt_counts[b], 0), p.G) : 0;
  const bool has_polys = p.G > 0 && p.NP > 0 && p.PTS > 0;
  const int32_t* labels = p.labels + (size_t)b * R;

  // ---- 1: how many foreground rows, and the first background row
  if (tid == 0) { first_bg_s = R; n_fg_s = 0; }
  __syncthreads();
  {
    int c = 0, fb = R;
    for (int r = tid; r < n_r; r += kMaskThreads) {
      const int l = labels[r];
      c += l > 0 ? 1 : 0;
      if (l == 0) fb = min(fb, r);
    }
    if (c) atomicAdd(&n_fg_s, c);
    if (fb < R) atomicMin(&first_bg_s, fb);
  }
  __syncthreads();
  const int n_fg = n_fg_s, first_bg = first_bg_s;
  const bool fallback = n_fg == 0 && first_bg < R;
  const int n_m = fallback ? 1 : min(n_fg, Fm);

  // ---- 2: the foreground rows in row order -> rows_s, and roi_has_mask on every row
  int taken = 0;                                // the same in every thread
  for (int base = 0; base < R; base += kMaskThreads) {
    const int r = base + tid;
    const bool fg = r < n_r && labels[r] > 0;
    const uint64_t m = __ballot(fg);
    if (lane == 0) cnt_s[wv] = __builtin_popcountll(m);
    __syncthreads();
    int before = taken, total = 0;
#pragma unroll
    for (int w = 0; w < kMaskWaves; w++) { before += w < wv ? cnt_s[w] : 0; total += cnt_s[w]; }
    const int slot = before + lanes_below(m, lane);
    const bool take = fg && slot < Fm;
    if (take) rows_s[slot] = r;
    if (p.roi_has_mask && r < R) p.roi_has_mask[(size_t)b * R + r] = (take || (fallback && r == first_bg)) ? 1 : 0;
    taken += total;
    __syncthreads();
  }
  if (fallback && tid == 0) rows_s[0] = first_bg;

  // ---- 3: eligible gt and their poly-boxes: wavefront wv takes gt wv, wv + 4, ...
  for (int g = tid; g < kMaskMaxGt; g += kMaskThreads) g_ok[g] = 0;
  __syncthreads();
  for (int g = wv; g < n_g; g += kMaskWaves) {
    const size_t at = (size_t)b * p.G + g;
    int q0, q1;
    if (!has_polys || p.gt_classes[at] <= 0 || p.gt_is_crowd[at] != 0 || !gt_poly_range(p, b, g, &q0, &q1)) continue;   // wave-uniform
    const float inf = __builtin_inff();
    float lo_x = inf, lo_y = inf, hi_x = -inf, hi_y = -inf;
    int n_valid = 0;
    for (int q = q0; q < q1; q++) {
      int ps, pe;
      if (!poly_range(p, b, q, &ps, &pe)) continue;
      const float2* pts = reinterpret_cast<const float2*>(p.poly_xy) + (size_t)b * p.PTS;
      float ax = inf, ay = inf, bx = -inf, by = -inf;
      bool bad = false;
      for (int i = ps + lane; i < pe; i += 64) {
        const float2 v = pts[i];
        bad |= !(isfinite(v.x) && isfinite(v.y));
        ax = fminf(ax, v.x); ay = fminf(ay, v.y); bx = fmaxf(bx, v.x); by = fmaxf(by, v.y);
      }
      if (__ballot(bad) != 0ull) continue;
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        ax = fminf(ax, __shfl_xor(ax, off, 64)); ay = fminf(ay, __shfl_xor(ay, off, 64));
        bx = fmaxf(bx, __shfl_xor(bx, off, 64)); by = fmaxf(by, __shfl_xor(by, off, 64));
      }
      lo_x = fminf(lo_x, ax); lo_y = fminf(lo_y, ay); hi_x = fmaxf(hi_x, bx); hi_y = fmaxf(hi_y, by);
      n_valid++;
    }
    if (lane == 0 && n_valid > 0) { g_box[g] = make_float4(lo_x, lo_y, hi_x, hi_y); g_ok[g] = 1; }
  }
  __syncthreads();

  // ---- 4: one mask row per thread and round
  const float scale = p.im_scale[b];
  for (int t = tid; t < Fm; t += kMaskThreads) {
    const size_t row = (size_t)b * Fm + t;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f), sb = box;
    int cls = 0, lvl = 0, match = -1;
    if (t < n_m) {
      const int r = rows_s[t];
      cls = fallback ? 0 : labels[r];
      const int c = p.keep_inds[(size_t)b * R + r];
      bool have = false;
      if (c >= 0 && c < n_g) { box = reinterpret_cast<const float4*>(p.gt_boxes)[(size_t)b * p.G + c]; have = true; }
      else if (c >= n_g && c - n_g < p.P) { box = reinterpret_cast<const float4*>(p.proposals)[(size_t)b * p.P + (c - n_g)]; have = true; }
      sb = make_float4(box.x * scale, box.y * scale, box.z * scale, box.w * scale);
      lvl = p.k_min == p.k_max ? 0 : fpn_level(sb.x, sb.y, sb.z, sb.w, p.k_min, p.k_max) - p.k_min;
      if (have && !fallback && finite4(box)) {
        float best = 0.f;
        for (int g = 0; g < n_g; g++) {
          if (!g_ok[g]) continue;
          const float v = iou_bbox(box, g_box[g]);                          // bbox_overlaps(boxes = rois, query = poly-boxes)
          if (match < 0 || v > best) { best = v; match = g; }               // np.argmax: the first maximum
        }
      }
    }
    float* r5 = p.mask_rois + row * 5;
    r5[0] = t < n_m ? (float)b : 0.f; r5[1] = sb.x; r5[2] = sb.y; r5[3] = sb.z; r5[4] = sb.w;
    p.mask_class[row] = cls;
    p.mask_roi_levels[row] = lvl;
    if (p.mask_gt) p.mask_gt[row] = match;
    p.ws.row_gt[row] = match;
    p.ws.row_box[row] = box;
  }
  if (tid == 0) p.n_mask[b] = n_m;
}

// C's (int): the arguments stay below 2^30 in magnitude
__device__ __forceinline__ int trunc_i(double v) { return (int)v; }
__device__ __forceinline__ int floor_div5(int a) { return a >= 0 ? a / 5 : -((4 - a) / 5); }

// the event of column i at the pair of trace points whose smaller v is vs
__device__ __forceinline__ void mask_toggle(int* tog, int i, int vs, int M) {
  const double yd = fmin(fmax(((double)vs + 0.5) / 5.0 - 0.5, 0.0), (double)M);
  const int pos = i * M + (int)ceil(yd);
  if (pos < M * M) atomicXor(&tog[pos], 1);
}

// every event of the edge (xs, ys) -> (xe, ye) on the 5x grid
__device__ __forceinline__ void mask_edge_events(int* tog, int xs, int ys, int xe, int ye, int M) {
  const int dx = abs(xe - xs), dy = abs(ye - ys);
  if (dx == 0 && dy == 0) return;
  if (dx >= dy) {
    if (xs > xe) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    const double s = (double)(ye - ys) / (double)dx;
    // pairs (t, t + 1), t = 0 .. dx - 1: us = xs + t = 5 i + 2
    const int i_lo = max(0, floor_div5(xs - 2 + 4)), i_hi = min(M - 1, floor_div5(xe - 1 - 2));
    for (int i = i_lo; i <= i_hi; i++) {
      const int t = 5 * i + 2 - xs;
      const int va = trunc_i((double)ys + s * (double)t + 0.5), vb = trunc_i((double)ys + s * (double)(t + 1) + 0.5);
      mask_toggle(tog, i, min(va, vb), M);
    }
  } else {
    if (ys > ye) { int t = xs; xs = xe; xe = t; t = ys; ys = ye; ye = t; }
    const double s = (double)(xe - xs) / (double)dy;
    auto u_of = [&](int t) { return trunc_i((double)xs + s * (double)t + 0.5); };     // monotone in t: every operation is
    const int u0 = u_of(0), u1 = u_of(dy);
    const int lo = min(u0, u1), hi = max(u0, u1);
    const int i_lo = max(0, floor_div5(lo - 2 + 4)), i_hi = min(M - 1, floor_div5(hi - 1 - 2));
    for (int i = i_lo; i <= i_hi; i++) {
      const int c = 5 * i + 2;                 // lo <= c < hi: the trace passes from c to beyond it exactly once
      int a = 0, z = dy;                       // rising: u(a) <= c < u(z); falling: u(a) > c >= u(z)
      const bool rising = u0 < u1;
      while (z - a > 1) {
        const int m = a + ((z - a) >> 1);
        const bool left = rising ? u_of(m) <= c : u_of(m) > c;
        if (left) a = m; else z = m;
      }
      if ((rising ? u_of(a) : u_of(z)) == c) mask_toggle(tog, i, ys + a, M);   // us = min(u) = c; vs = min(v) = ys + a
    }
  }
}

__global__ __launch_bounds__(kMaskThreads) void mask_raster_kernel(MaskTargetsParams p) {
  __shared__ int tog[kMaskMaxPos + 1];
  __shared__ int acc[kMaskMaxPos];
  __shared__ int par_s[kMaskWaves];
  const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int M = p.M, MM = M * M;
  const size_t row = (size_t)b * p.Fm + t;
  int32_t* out = p.masks + row * MM;
  const int g = p.ws.row_gt[row];
  int q0 = 0, q1 = 0;
  if (g < 0 || g >= p.G || !gt_poly_range(p, b, g, &q0, &q1)) {               // wave-uniform: nothing to match, or past n_mask
    for (int i = tid; i < MM; i += kMaskThreads) out[i] = -1;
    return;
  }
  const float4 box = p.ws.row_box[row];
  const float w = fmaxf(box.z - box.x, 1.f), h = fmaxf(box.w - box.y, 1.f), fm = (float)M;   // segms.py:99-103
  for (int i = tid; i < MM; i += kMaskThreads) { tog[i] = 0; acc[i] = 0; }
  const float2* pts = reinterpret_cast<const float2*>(p.poly_xy) + (size_t)b * p.PTS;
  auto norm = [&](float2 v) { return make_float2(fdiv((v.x - box.x) * fm, w), fdiv((v.y - box.y) * fm, h)); };   // :108-109
  const int chunk = (MM + kMaskThreads - 1) / kMaskThreads;
  for (int q = q0; q < q1; q++) {
    int ps, pe;
    if (!poly_range(p, b, q, &ps, &pe)) continue;
    bool bad = false;
    for (int i = ps + tid; i < pe; i += kMaskThreads) {
      const float2 v = pts[i], nv = norm(v);
      bad |= !(isfinite(v.x) && isfinite(v.y) && fabsf(nv.x) < kMaskCoordLimit && fabsf(nv.y) < kMaskCoordLimit);   // NaN: false
    }
    if (__syncthreads_or(bad ? 1 : 0)) continue;                              // (also: tog and acc are initialised)
    const int n = pe - ps;
    for (int e = tid; e < n; e += kMaskThreads) {
      const float2 a = norm(pts[ps + e]), z = norm(pts[ps + (e + 1 == n ? 0 : e + 1)]);
      mask_edge_events(tog, trunc_i(5.0 * (double)a.x + 0.5), trunc_i(5.0 * (double)a.y + 0.5), trunc_i(5.0 * (double)z.x + 0.5),
                       trunc_i(5.0 * (double)z.y + 0.5), M);
    }
    __syncthreads();
    // prefix parity: thread tid owns the positions [tid * chunk, tid * chunk + chunk)
    const int p0 = min(tid * chunk, MM), p1 = min(p0 + chunk, MM);
    int par = 0;
    for (int i = p0; i < p1; i++) par ^= tog[i];
    const uint64_t m = __ballot(par != 0);
    if (lane == 0) par_s[wv] = __builtin_popcountll(m) & 1;
    __syncthreads();
    int run = lanes_below(m, lane) & 1;
#pragma unroll
    for (int k = 0; k < kMaskWaves; k++) run ^= k < wv ? par_s[k] : 0;
    for (int i = p0; i < p1; i++) {
      run ^= tog[i];
      tog[i] = 0;                                                            // clean for the next polygon
      if (run) acc[(i % M) * M + i / M] = 1;                                 // column-major position -> row-major pixel
    }
    __syncthreads();
  }
  __syncthreads();
  for (int i = tid; i < MM; i += kMaskThreads) out[i] = acc[i];
}

}  // namespace dtc

DTC_API const char* dtc_mask_train_target_arch(void) { return "gfx950"; }

static int mask_targets_shapes(int batch, int R, int G, int P, int PTS, int NP, int M, int k_min, int k_max, int Fm) {
  if (batch < 1 || R < 1 || G < 0 || P < 0 || G + (long long)P < 1 || PTS < 0 || NP < 0 || M < 1 || Fm < 1 || k_min < 0 || k_max > 15 ||
      k_min > k_max)
    return DTC_EINVAL;
  if (batch > 65535 || R > DTC_MASK_MAX_ROIS || G > DTC_MASK_MAX_GT || P > DTC_MASK_MAX_PROPOSALS || PTS > DTC_MASK_MAX_POINTS ||
      NP > DTC_MASK_MAX_POLYS || M > DTC_MASK_MAX_M || Fm > DTC_MASK_MAX_ROWS)
    return DTC_EUNSUPPORTED;
  return DTC_OK;
}

DTC_API size_t dtc_mask_targets_workspace_bytes(int batch, int mask_rows) {
  if (batch < 1 || batch > 65535 || mask_rows < 1 || mask_rows > DTC_MASK_MAX_ROWS) return 0;
  return dtc::MaskTargetsWs::bytes(batch, mask_rows);
}

DTC_API int dtc_mask_targets(const int32_t* labels, const int32_t* keep_inds, const int32_t* n_rois, int batch, int rois_per_image,
                             const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_is_crowd, const int32_t* gt_counts,
                             int gt_stride, const float* proposals, int proposal_stride, const float* im_scale, const float* poly_xy,
                             const int32_t* poly_ptr, const int32_t* gt_poly_ptr, int points_stride, int polys_stride, int M, int k_min,
                             int k_max, int mask_rows, void* workspace, size_t workspace_bytes, float* mask_rois, int32_t* masks,
                             int32_t* mask_class, int32_t* mask_roi_levels, int32_t* roi_has_mask, int32_t* n_mask, int32_t* mask_gt,
                             dtc_stream_t stream) {
  // shapes and parameters, then limits
  const int G = gt_stride, P = proposal_stride, PTS = points_stride, NP = polys_stride;
  const int rc = mask_targets_shapes(batch, rois_per_image, G, P, PTS, NP, M, k_min, k_max, mask_rows);
  if (rc != DTC_OK) return rc;
  // pointers
  if (!labels || !keep_inds || !n_rois || !im_scale || !mask_rois || !masks || !mask_class || !mask_roi_levels || !n_mask) return DTC_EINVAL;
  if (G > 0 && (!gt_boxes || !gt_classes || !gt_is_crowd || !gt_counts || !gt_poly_ptr)) return DTC_EINVAL;
  if (P > 0 && !proposals) return DTC_EINVAL;
  if (G > 0 && NP > 0 && PTS > 0 && (!poly_xy || !poly_ptr)) return DTC_EINVAL;
  if (((reinterpret_cast<uintptr_t>(gt_boxes) | reinterpret_cast<uintptr_t>(proposals) | reinterpret_cast<uintptr_t>(workspace)) & 15) != 0 ||
      (reinterpret_cast<uintptr_t>(poly_xy) & 7) != 0)
    return DTC_EINVAL;
  // workspace
  if (!workspace || workspace_bytes < dtc::MaskTargetsWs::bytes(batch, mask_rows)) return DTC_EWORKSPACE;

  dtc::MaskTargetsParams p{};
  p.labels = labels; p.keep_inds = keep_inds; p.n_rois = n_rois; p.gt_boxes = gt_boxes; p.gt_classes = gt_classes;
  p.gt_is_crowd = gt_is_crowd; p.gt_counts = gt_counts; p.proposals = proposals; p.im_scale = im_scale; p.poly_xy = poly_xy;
  p.poly_ptr = poly_ptr; p.gt_poly_ptr = gt_poly_ptr;
  p.B = batch; p.R = rois_per_image; p.G = G; p.P = P; p.PTS = PTS; p.NP = NP; p.M = M; p.k_min = k_min; p.k_max = k_max; p.Fm = mask_rows;
  p.ws = dtc::MaskTargetsWs(workspace, batch, mask_rows);
  p.mask_rois = mask_rois; p.masks = masks; p.mask_class = mask_class; p.mask_roi_levels = mask_roi_levels; p.roi_has_mask = roi_has_mask;
  p.n_mask = n_mask; p.mask_gt = mask_gt;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dtc::mask_rows_kernel, dim3(batch), dim3(dtc::kMaskThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(dtc::mask_raster_kernel, dim3(mask_rows, batch), dim3(dtc::kMaskThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
