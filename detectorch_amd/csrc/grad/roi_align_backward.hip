// RoIAlign backward for gfx950: lib/cppcuda/roi_align_backward_cpu.cpp:97-185 (roi_align_backward_loop) for up to 8 levels in one
// call, bit for bit, without atomics (include/detectorch_grad_hip.h holds the contract).
//
// Owner-computes.  A workgroup owns a kTileH x kTileW tile of ONE (level, image) map for a block of kBwdThreads channels; a thread
// owns one channel's copy of the tile in LDS, laid out [pixel][thread] (pitch kBwdThreads + 1).  In the accumulation the pixel is
// the same in every lane and the lanes are consecutive words: no bank conflict, and no two threads ever touch one word, so
// there are no LDS atomics and no barrier before the write-out.  The thread walks the valid RoIs of its (level, image) in
// ascending index and runs the reference's loops ph, pw, iy, ix, taps 1-4 on each, adding the taps that fall into its tile: every
// element's sum has the serial loop's order, and every output byte is written exactly once (zeros included) by the write-out.
// The geometry (sample positions, weights before the product with top) is the same in every lane.
//
// A preparation kernel lists, per (level, image), the valid RoIs in ascending index with their scaled box, grid and the pixel
// range their taps can reach (exact: the sample positions are monotone in ph and iy), so that a tile skips the RoIs, bins and
// sample rows that cannot touch it.  The lists hold n_rois records in all.
#include <cmath>

#include "roi_align_common.h"

#include "../../../include/detectorch_grad_hip.h"

namespace dtc {

constexpr int kBwdThreads = 256;                  // channels per workgroup (the channel block)
constexpr int kTileH = 4, kTileW = 16;            // 64 pixels: 64 * 257 * 4 B = 65 792 B of LDS, two workgroups per CU
constexpr int kTilePixels = kTileH * kTileW;
constexpr int kTilePitch = kBwdThreads + 1;       // [pixel][thread] + 1: the write-out reads 16 pixels x 4 channels per wave
constexpr float kMaxScaled = 536870912.f;         // 2^29: scaled coordinates stay below it (header: bad RoIs)

// One valid RoI in the list of its (level, image): what roi_align_backward_cpu.cpp:104-142 derives before its sample loops.
struct BwdRec {
  float sw, sh, bin_w, bin_h;                     // :112-113 scaled start, :124-125 bin sizes
  int gh, gw, r;                                  // :135-139 sampling grid; the RoI's row in grad_output
  float count;                                    // :142
  int x0, x1, y0, y1;                             // inclusive pixel range of the taps of all its samples
};
static_assert(sizeof(BwdRec) == 48, "the workspace holds 48 bytes per RoI");

struct BwdLevel {
  float* grad;
  int height, width, tiles_x, tiles;              // tiles: tiles_y * tiles_x of one image
  float spatial_scale;
  int first;                                      // the level's first work item (tiles of all images of the levels before it)
};

struct BwdParams {
  BwdLevel lv[DTC_MAX_LEVELS];
  const float* rois;
  const int32_t* roi_levels;
  const float* top;
  int2* groups;                                   // [n_levels * batch] (offset into recs, count)
  BwdRec* recs;                                   // [n_rois]
  int n_levels, batch, channels, roi_cols, n_rois, pooled_h, pooled_w, sampling_ratio;
};

// The (level, image) pair of RoI i as level * batch + image, or -1 for a bad RoI (header); *rec: its record, when rec != nullptr.
__device__ __forceinline__ int bwd_classify(const BwdParams& p, int i, BwdRec* rec) {
  const int lvl = p.roi_levels ? p.roi_levels[i] : 0;
  if (lvl < 0 || lvl >= p.n_levels) return -1;
  const float* roi = p.rois + (size_t)i * p.roi_cols;
  int b = 0;
  if (p.roi_cols == 5) {                                                  // :105-109
    const float bf = roi[0];
    if (!(bf > -1.f && bf < (float)p.batch)) return -1;                   // (int)bf outside [0, batch), or NaN
    b = (int)bf;
    roi++;
  }
  const float x1 = roi[0], y1 = roi[1], x2 = roi[2], y2 = roi[3];
  if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2))) return -1;
  float s = 1.f;
  int H = 1, W = 1;
#pragma unroll
  for (int l = 0; l < DTC_MAX_LEVELS; l++)
    if (l == lvl) { s = p.lv[l].spatial_scale; H = p.lv[l].height; W = p.lv[l].width; }
  const float sw = x1 * s, sh = y1 * s, ew = x2 * s, eh = y2 * s;         // :112-115 (no rounding)
  if (!(fabsf(sw) < kMaxScaled && fabsf(sh) < kMaxScaled && fabsf(ew) < kMaxScaled && fabsf(eh) < kMaxScaled)) return -1;
  const float rw = fmaxf(ew - sw, 1.f), rh = fmaxf(eh - sh, 1.f);         // :122-123
  const float bin_h = fdiv(rh, (float)p.pooled_h), bin_w = fdiv(rw, (float)p.pooled_w);   // :124-125
  int gh = p.sampling_ratio, gw = p.sampling_ratio;
  if (p.sampling_ratio <= 0) {                                            // :135-139
    const float fh = ceilf(fdiv(rh, (float)p.pooled_h)), fw = ceilf(fdiv(rw, (float)p.pooled_w));
    if (fh > (float)DTC_GRAD_MAX_GRID || fw > (float)DTC_GRAD_MAX_GRID) return -1;
    gh = (int)fh; gw = (int)fw;
  }
  if (rec) {
    rec->sw = sw; rec->sh = sh; rec->bin_w = bin_w; rec->bin_h = bin_h;
    rec->gh = gh; rec->gw = gw; rec->r = i;
    rec->count = (float)(gh * gw);                                        // :142
    // the sample positions are monotone in (p, i): the first and the last sample bound every tap of the RoI
    rec->y0 = make_axis(sh, bin_h, 0, 0, gh, H).lo;
    rec->y1 = make_axis(sh, bin_h, p.pooled_h - 1, gh - 1, gh, H).hi;
    rec->x0 = make_axis(sw, bin_w, 0, 0, gw, W).lo;
    rec->x1 = make_axis(sw, bin_w, p.pooled_w - 1, gw - 1, gw, W).hi;
  }
  return lvl * p.batch + b;
}

// One workgroup per (level, image) pair g: the valid RoIs of g, in ascending index, go to recs[offset .. offset + count), where
// offset is the number of valid RoIs of the pairs before g.  Integer counts only: the result does not depend on any order.
__global__ __launch_bounds__(kBwdThreads) void roi_align_bwd_prep_kernel(BwdParams p) {
  __shared__ int sh_before[kBwdThreads / 64], sh_wave[kBwdThreads / 64];
  const int g = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int before = 0;
  for (int i = tid; i < p.n_rois; i += kBwdThreads) {
    const int key = bwd_classify(p, i, nullptr);
    before += (key >= 0 && key < g) ? 1 : 0;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
  if (lane == 0) sh_before[wave] = before;
  __syncthreads();
  int base = 0;
#pragma unroll
  for (int w = 0; w < kBwdThreads / 64; w++) base += sh_before[w];
  const int offset = base;
  for (int i0 = 0; i0 < p.n_rois; i0 += kBwdThreads) {
    const int i = i0 + tid;
    BwdRec rec;
    const bool mine = i < p.n_rois && bwd_classify(p, i, &rec) == g;
    const uint64_t mask = __ballot(mine);
    __syncthreads();                                 // (sh_wave may still be read from the chunk before)
    if (lane == 0) sh_wave[wave] = __builtin_popcountll(mask);
    __syncthreads();
    int slot = base + lanes_below(mask, lane), all = 0;
#pragma unroll
    for (int w = 0; w < kBwdThreads / 64; w++) {
      if (w < wave) slot += sh_wave[w];
      all += sh_wave[w];
    }
    if (mine) p.recs[slot] = rec;
    base += all;
  }
  if (tid == 0) p.groups[g] = make_int2(offset, base - offset);
}

// acc[pixel] += top * w / count (:171-181) for one tap, when the tap lies in the tile.
__device__ __forceinline__ void bwd_tap(float* acc, int y, int x, int ty0, int tx0, float t, float w, float count, float inv_count) {
  const unsigned dy = (unsigned)(y - ty0), dx = (unsigned)(x - tx0);
  if (dy >= (unsigned)kTileH || dx >= (unsigned)kTileW) return;
  const float tw = t * w;
  const float g = inv_count != 0.f ? tw * inv_count : fdiv(tw, count);      // count a power of two: the same quotient
  float* a = acc + (dy * kTileW + dx) * kTilePitch;
  *a = *a + g;
}

__global__ __launch_bounds__(kBwdThreads) void roi_align_bwd_tile_kernel(BwdParams p) {
  extern __shared__ float tile[];                    // [kTilePixels][kTilePitch]
  const int tid = threadIdx.x;
  // which tile: level, image, tile row and column (the same in every lane)
  const int item = blockIdx.x;
  int l = 0;
#pragma unroll
  for (int k = 1; k < DTC_MAX_LEVELS; k++)
    if (k < p.n_levels && item >= p.lv[k].first) l = k;
  BwdLevel lv = p.lv[0];
#pragma unroll
  for (int k = 1; k < DTC_MAX_LEVELS; k++)
    if (k == l) lv = p.lv[k];
  const int local = item - lv.first;
  const int b = local / lv.tiles, t_in = local - b * lv.tiles;
  const int ty0 = (t_in / lv.tiles_x) * kTileH, tx0 = (t_in % lv.tiles_x) * kTileW;
  const int H = lv.height, W = lv.width;
  const int c0 = blockIdx.y * kBwdThreads, c = c0 + tid;
  const bool live = c < p.channels;

  float* acc = tile + tid;
#pragma unroll 8
  for (int px = 0; px < kTilePixels; px++) acc[px * kTilePitch] = 0.f;

  const int2 grp = p.groups[l * p.batch + b];
  const int PH = p.pooled_h, PW = p.pooled_w;
  for (int k = 0; k < grp.y; k++) {
    const BwdRec rec = p.recs[grp.x + k];
    if (rec.y1 < ty0 || rec.y0 >= ty0 + kTileH || rec.x1 < tx0 || rec.x0 >= tx0 + kTileW) continue;
    const float* top = p.top + ((size_t)rec.r * p.channels + (live ? c : c0)) * ((size_t)PH * PW);
    const int gg = rec.gh * rec.gw;
    const float inv_count = ((gg & (gg - 1)) == 0) ? fdiv(1.f, rec.count) : 0.f;
    for (int ph = 0; ph < PH; ph++) {
      // the rows this bin's samples can reach: from its first sample's low row to its last sample's high row
      if (make_axis(rec.sh, rec.bin_h, ph, rec.gh - 1, rec.gh, H).hi < ty0) continue;
      if (make_axis(rec.sh, rec.bin_h, ph, 0, rec.gh, H).lo >= ty0 + kTileH) break;
      for (int pw = 0; pw < PW; pw++) {
        if (make_axis(rec.sw, rec.bin_w, pw, rec.gw - 1, rec.gw, W).hi < tx0) continue;
        if (make_axis(rec.sw, rec.bin_w, pw, 0, rec.gw, W).lo >= tx0 + kTileW) break;
        const float t = top[ph * PW + pw];                                  // :132
        for (int iy = 0; iy < rec.gh; iy++) {
          const AxisEntry ay = make_axis(rec.sh, rec.bin_h, ph, iy, rec.gh, H);
          if (ay.hi < ty0) continue;
          if (ay.lo >= ty0 + kTileH) break;
          if (ay.l == 0.f && ay.h == 0.f) continue;                         // :26-31 an empty sample (valid ones have h = 1 - l)
          for (int ix = 0; ix < rec.gw; ix++) {
            const AxisEntry ax = make_axis(rec.sw, rec.bin_w, pw, ix, rec.gw, W);
            if (ax.hi < tx0) continue;
            if (ax.lo >= tx0 + kTileW) break;
            if (ax.l == 0.f && ax.h == 0.f) continue;
            const float w1 = ay.h * ax.h, w2 = ay.h * ax.l, w3 = ay.l * ax.h, w4 = ay.l * ax.l;   // :68
            bwd_tap(acc, ay.lo, ax.lo, ty0, tx0, t, w1, rec.count, inv_count);                    // :178-181, in this order
            bwd_tap(acc, ay.lo, ax.hi, ty0, tx0, t, w2, rec.count, inv_count);
            bwd_tap(acc, ay.hi, ax.lo, ty0, tx0, t, w3, rec.count, inv_count);
            bwd_tap(acc, ay.hi, ax.hi, ty0, tx0, t, w4, rec.count, inv_count);
          }
        }
      }
    }
  }
  __syncthreads();

  // write-out: every element of the tile that lies inside the map, once
  float* out = lv.grad + ((size_t)b * p.channels + c0) * ((size_t)H * W);
  const int n_ch = min(kBwdThreads, p.channels - c0);
  if ((W & 3) == 0) {
    // 16-byte stores: 4 lanes cover a row of the tile (64 B), 16 lanes one channel's four rows
    for (int i = tid; i < kBwdThreads * kTileH * (kTileW / 4); i += kBwdThreads) {
      const int q = i & 3, row = (i >> 2) & 3, ch = i >> 4;
      const int y = ty0 + row, x = tx0 + 4 * q;
      if (ch >= n_ch || y >= H || x >= W) continue;
      const float* s = tile + (row * kTileW + 4 * q) * kTilePitch + ch;
      store_stream16(out + ((size_t)ch * H + y) * W + x, make_float4(s[0], s[kTilePitch], s[2 * kTilePitch], s[3 * kTilePitch]));
    }
  } else {
    for (int i = tid; i < kBwdThreads * kTilePixels; i += kBwdThreads) {
      const int px = i & (kTilePixels - 1), ch = i >> 6;
      const int y = ty0 + px / kTileW, x = tx0 + px % kTileW;
      if (ch >= n_ch || y >= H || x >= W) continue;
      out[((size_t)ch * H + y) * W + x] = tile[px * kTilePitch + ch];
    }
  }
}

constexpr size_t kBwdLdsBytes = (size_t)kTilePixels * kTilePitch * sizeof(float);
static_assert(2 * kBwdLdsBytes <= (size_t)kCuLdsBytes, "two workgroups per CU");
static_assert(kTilePixels == 64 && kTileH == 4 && kTileW == 16, "the write-out's index arithmetic");

struct BwdLayout { size_t groups, recs, end; };
inline BwdLayout bwd_layout(int n_levels, int batch, int n_rois) {
  Carve cv{16};
  BwdLayout o;
  o.groups = cv.take((size_t)n_levels * batch * sizeof(int2));
  o.recs = cv.take((size_t)(n_rois > 0 ? n_rois : 1) * sizeof(BwdRec));
  o.end = cv.end;
  return o;
}

inline bool bwd_counts_ok(int n_levels, int batch, int n_rois) {
  return n_levels >= 1 && n_levels <= DTC_MAX_LEVELS && batch >= 1 && batch <= DTC_GRAD_MAX_BATCH && n_rois >= 0 &&
         n_rois <= DTC_GRAD_MAX_ROIS;
}

}  // namespace dtc

DTC_API const char* dtc_grad_target_arch(void) { return "gfx950"; }

DTC_API size_t dtc_roi_align_backward_workspace_bytes(int n_levels, int batch, int n_rois) {
  if (!dtc::bwd_counts_ok(n_levels, batch, n_rois)) return 0;
  return dtc::bwd_layout(n_levels, batch, n_rois).end;
}

DTC_API int dtc_roi_align_backward(const dtc_grad_level* levels, int n_levels, int batch, int channels, const float* rois, int roi_cols,
                                   const int32_t* roi_levels, int n_rois, int pooled_h, int pooled_w, int sampling_ratio,
                                   const float* grad_output, void* workspace, size_t workspace_bytes, dtc_stream_t stream) {
  using namespace dtc;
  // shapes
  if (!levels || n_levels < 1 || batch < 1 || channels < 1 || (roi_cols != 4 && roi_cols != 5) || n_rois < 0 || pooled_h < 1 ||
      pooled_w < 1)
    return DTC_EINVAL;
  for (int l = 0; l < n_levels && l < DTC_MAX_LEVELS; l++)
    if (levels[l].height < 1 || levels[l].width < 1 || !std::isfinite(levels[l].spatial_scale)) return DTC_EINVAL;
  // limits
  if (!bwd_counts_ok(n_levels, batch, n_rois) || pooled_h > DTC_GRAD_MAX_POOLED || pooled_w > DTC_GRAD_MAX_POOLED ||
      sampling_ratio > DTC_GRAD_MAX_SAMPLING || channels > (1 << 23))
    return DTC_EUNSUPPORTED;
  BwdParams p{};
  int64_t items = 0;
  for (int l = 0; l < n_levels; l++) {
    if (levels[l].height > DTC_GRAD_MAX_EXTENT || levels[l].width > DTC_GRAD_MAX_EXTENT) return DTC_EUNSUPPORTED;
    BwdLevel& v = p.lv[l];
    v.grad = levels[l].grad; v.height = levels[l].height; v.width = levels[l].width; v.spatial_scale = levels[l].spatial_scale;
    v.tiles_x = ceil_div(v.width, kTileW);
    const int64_t tiles = (int64_t)ceil_div(v.height, kTileH) * v.tiles_x;
    if (tiles * batch > INT32_MAX) return DTC_EUNSUPPORTED;
    v.tiles = (int)tiles;
    v.first = (int)items;
    items += tiles * batch;
    if (items > INT32_MAX) return DTC_EUNSUPPORTED;
  }
  // pointers
  for (int l = 0; l < n_levels; l++)
    if (!levels[l].grad || (reinterpret_cast<uintptr_t>(levels[l].grad) & 15) != 0) return DTC_EINVAL;
  if (n_rois > 0 && (!rois || !grad_output)) return DTC_EINVAL;
  if (((reinterpret_cast<uintptr_t>(rois) | reinterpret_cast<uintptr_t>(roi_levels) | reinterpret_cast<uintptr_t>(grad_output)) & 3) != 0 ||
      (reinterpret_cast<uintptr_t>(workspace) & 15) != 0)
    return DTC_EINVAL;
  // workspace
  const BwdLayout lay = bwd_layout(n_levels, batch, n_rois);
  if (!workspace || workspace_bytes < lay.end) return DTC_EWORKSPACE;

  p.rois = rois; p.roi_levels = roi_levels; p.top = grad_output;
  p.groups = reinterpret_cast<int2*>(static_cast<char*>(workspace) + lay.groups);
  p.recs = reinterpret_cast<BwdRec*>(static_cast<char*>(workspace) + lay.recs);
  p.n_levels = n_levels; p.batch = batch; p.channels = channels; p.roi_cols = roi_cols; p.n_rois = n_rois;
  p.pooled_h = pooled_h; p.pooled_w = pooled_w; p.sampling_ratio = sampling_ratio;
  if (raise_lds_once<roi_align_bwd_tile_kernel>() != DTC_OK) return DTC_ELAUNCH;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(roi_align_bwd_prep_kernel, dim3(n_levels * batch), dim3(kBwdThreads), 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(roi_align_bwd_tile_kernel, dim3((unsigned)items, ceil_div(channels, kBwdThreads)), dim3(kBwdThreads), kBwdLdsBytes,
                     s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
