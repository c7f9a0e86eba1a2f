// dtc_kps_heatmaps_to_keypoints (include/detectorch_kps_hip.h): K heatmaps of S x S logits per detection -> K keypoints (x, y, logit,
// prob), Detectron's heatmaps_to_keypoints with cv2.resize(INTER_CUBIC), in THREE launches of a fixed shape.  The resized map (up to
// 4096 x 4096 per keypoint) is never stored: kps_band_kernel<false> finds each band's maximum and first position, kps_band_kernel<true>
// recomputes the values against the map's maximum and sums the exp terms, kps_finish_kernel folds the bands and writes the outputs.
//
// Work split.  A map is cut into row BANDS of max(ceil(Hr / 8), 32) resized rows, one workgroup of four wavefronts each, so the grid is
// 8 workgroups per map whatever the boxes hold; the workgroups of bands a small map does not have, and of rows that are not live,
// return at once.  A workgroup stages only the source rows its band reads.  Inside a band the wavefronts take 64-column STRIPS in
// turn; a lane owns one column, computes its four column taps and weights once per strip and walks down the band: the four horizontal
// results of the current source rows stay in registers and move up by one when the source row advances (the usual case when a map is
// enlarged), so a resized value costs one vertical combination and, every Hr / S rows, one horizontal one.  Consecutive lanes read
// consecutive or equal LDS words.
#include "dtc_common.h"

#include "../../../include/detectorch_kps_hip.h"

namespace dtc {

constexpr int kKpsThreads = 256, kKpsWaves = kKpsThreads / DTC_WAVE;
constexpr int kKpsMapWords = DTC_KPS_MAX_MAP * DTC_KPS_MAX_MAP + 2 * DTC_KPS_MAX_MAP;   // two spare rows: no tap address leaves the array
constexpr float kKpsA = -0.75f;                    // OpenCV's INTER_CUBIC
constexpr float kKpsExpFloor = -104.0f;            // exp(x) < 2^-150 below ln(2^-150) = -103.97: rounds to +0.0f

struct KpsParams {
  const float* heatmaps;
  const float* dets;
  const int32_t* det_count;
  int max_out, K, S, person_class, min_size;
  int n_rows;                // B max_out
  float2* band_max;          // [n_rows K, DTC_KPS_BANDS] (value, position bits)
  double* band_sum;          // [n_rows K, DTC_KPS_BANDS]
  float* keyps;
  int32_t* kp_status;
};

// ---- a detection row: live (1), not a row (0) or refused (-1), and the resized size -----------------------------------------------------
struct KpsRow {
  int status, Wr, Hr;
  float x1, y1, wc, hc;
};

__device__ __forceinline__ KpsRow kps_row(const KpsParams& p, int row) {
  KpsRow r;
  r.status = 0; r.Wr = r.Hr = 1; r.x1 = r.y1 = 0.f; r.wc = r.hc = 1.f;
  const int b = row / p.max_out, d = row % p.max_out;
  if (d >= min(max(p.det_count[b], 0), p.max_out)) return r;
  const float* q = p.dets + (size_t)row * 6;
  if (p.person_class >= 0 && q[5] != (float)p.person_class) return r;
  const float x1 = q[0], y1 = q[1], x2 = q[2], y2 = q[3];
  r.status = -1;
  if (!(isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2))) return r;
  const float w = fmaxf(x2 - x1, 1.0f), h = fmaxf(y2 - y1, 1.0f);
  float cw = ceilf(w), ch = ceilf(h);
  if (p.min_size > 0) { cw = fmaxf(cw, (float)p.min_size); ch = fmaxf(ch, (float)p.min_size); }
  if (!(cw <= (float)DTC_KPS_MAX_SIDE && ch <= (float)DTC_KPS_MAX_SIDE)) return r;    // before the casts: an inf or 1e30 side stops here
  r.status = 1;
  r.Wr = (int)cw; r.Hr = (int)ch;
  r.x1 = x1; r.y1 = y1;
  r.wc = fdiv(w, (float)r.Wr); r.hc = fdiv(h, (float)r.Hr);
  return r;
}

__device__ __forceinline__ int kps_band_rows(int Hr) { return max(ceil_div(Hr, DTC_KPS_BANDS), DTC_KPS_MIN_BAND); }

// ---- the cubic taps of one destination index -------------------------------------------------------------------------------------------
struct KpsTaps {
  int s;                     // floor of the source coordinate: taps s-1 .. s+2
  float c0, c1, c2, c3;
};

__device__ __forceinline__ KpsTaps kps_taps(int d, double scale) {
  KpsTaps k;
  const float f = (float)(((double)d + 0.5) * scale - 0.5);
  const float fl = floorf(f);
  k.s = (int)fl;
  const float t = f - fl, t1 = t + 1.0f, u = 1.0f - t;
  constexpr float A = kKpsA;
  k.c0 = ((A * t1 - 5.0f * A) * t1 + 8.0f * A) * t1 - 4.0f * A;
  k.c1 = ((A + 2.0f) * t - (A + 3.0f)) * t * t + 1.0f;
  k.c2 = ((A + 2.0f) * u - (A + 3.0f)) * u * u + 1.0f;
  k.c3 = 1.0f - k.c0 - k.c1 - k.c2;
  return k;
}

__device__ __forceinline__ int kps_clamp(int i, int S) { return min(max(i, 0), S - 1); }

// ---- the maximum with np.argmax's order: a NaN beats a number, then the larger value, then the smaller position ------------------------
__device__ __forceinline__ bool kps_better(float v, int i, float bv, int bi) {
  const bool vn = v != v, bn = bv != bv;
  if (vn != bn) return vn;
  if (vn) return i < bi;
  return v > bv || (v == bv && i < bi);
}

// One band of one map.  kSum = false: (maximum, first position) of the band -> band_max.  kSum = true: the band's sum of the exp terms
// against the map's maximum (folded from band_max) -> band_sum.
template <bool kSum>
__global__ __launch_bounds__(kKpsThreads) void kps_band_kernel(KpsParams p) {
  __shared__ float map[kKpsMapWords];
  __shared__ float red_v[kKpsWaves];
  __shared__ int red_i[kKpsWaves];
  __shared__ double red_s[kKpsWaves];
  const int band = blockIdx.x % DTC_KPS_BANDS;
  const int m = blockIdx.x / DTC_KPS_BANDS;                  // map = row K + k
  const KpsRow r = kps_row(p, m / p.K);                      // the same for every thread of the workgroup; the grid is exact
  if (r.status != 1) return;
  const int rows = kps_band_rows(r.Hr);
  const int y0 = band * rows, y1 = min(y0 + rows, r.Hr);
  if (y0 >= r.Hr) return;
  const int S = p.S;
  const double sx = (double)S / (double)r.Wr, sy = (double)S / (double)r.Hr;
  // the source rows this band reads: f is monotonic in the destination index
  const int q_lo = kps_clamp(kps_taps(y0, sy).s - 1, S), q_hi = kps_clamp(kps_taps(y1 - 1, sy).s + 2, S);
  const float* src = p.heatmaps + ((size_t)m * S + q_lo) * S;
  for (int i = threadIdx.x; i < (q_hi - q_lo + 1) * S; i += kKpsThreads) map[i] = src[i];
  float top = 0.f;
  if (kSum) {                                                // the map's maximum: the bands in increasing order
    const int n_bands = ceil_div(r.Hr, rows);
    const float2* bm = p.band_max + (size_t)m * DTC_KPS_BANDS;
    int ti = __float_as_int(bm[0].y);
    top = bm[0].x;
    for (int c = 1; c < n_bands; c++)
      if (kps_better(bm[c].x, __float_as_int(bm[c].y), top, ti)) { top = bm[c].x; ti = __float_as_int(bm[c].y); }
  }
  __syncthreads();
  const int lane = threadIdx.x % DTC_WAVE, wave = threadIdx.x / DTC_WAVE;
  float bv = -INFINITY;
  int bi = 0x7fffffff;
  double sum = 0.0;
  const int n_strips = ceil_div(r.Wr, DTC_WAVE);
  for (int st = wave; st < n_strips; st += kKpsWaves) {
    const int x = st * DTC_WAVE + lane;
    const bool active = x < r.Wr;
    const KpsTaps tx = kps_taps(active ? x : r.Wr - 1, sx);
    const int a0 = kps_clamp(tx.s - 1, S), a1 = kps_clamp(tx.s, S), a2 = kps_clamp(tx.s + 1, S), a3 = kps_clamp(tx.s + 2, S);
    auto hrow = [&](int q) {                                 // the horizontal result of source row q at this lane's column
      const float* l = map + (kps_clamp(q, S) - q_lo) * S;
      return ((l[a0] * tx.c0 + l[a1] * tx.c1) + l[a2] * tx.c2) + l[a3] * tx.c3;
    };
    float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f;
    int s_have = -100;                                       // kps_taps gives s >= -1
    for (int y = y0; y < y1; y++) {
      const KpsTaps ty = kps_taps(y, sy);                    // the same in every lane
      if (ty.s != s_have) {
        if (ty.s == s_have + 1) { h0 = h1; h1 = h2; h2 = h3; h3 = hrow(ty.s + 2); }
        else { h0 = hrow(ty.s - 1); h1 = hrow(ty.s); h2 = hrow(ty.s + 1); h3 = hrow(ty.s + 2); }
        s_have = ty.s;
      }
      const float v = ((h0 * ty.c0 + h1 * ty.c1) + h2 * ty.c2) + h3 * ty.c3;
      if (!active) continue;
      if (kSum) {
        const float e = v - top;
        if (!(e < kKpsExpFloor)) sum += (double)fexp_cr(e);
      } else {
        const int i = y * r.Wr + x;
        if (kps_better(v, i, bv, bi)) { bv = v; bi = i; }
      }
    }
  }
  if (kSum) {
#pragma unroll
    for (int o = DTC_WAVE / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, DTC_WAVE);
    if (lane == 0) red_s[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = red_s[0];
      for (int w = 1; w < kKpsWaves; w++) t += red_s[w];
      p.band_sum[(size_t)m * DTC_KPS_BANDS + band] = t;
    }
  } else {
#pragma unroll
    for (int o = DTC_WAVE / 2; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o, DTC_WAVE);
      const int oi = __shfl_xor(bi, o, DTC_WAVE);
      if (kps_better(ov, oi, bv, bi)) { bv = ov; bi = oi; }
    }
    if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int w = 1; w < kKpsWaves; w++)
        if (kps_better(red_v[w], red_i[w], bv, bi)) { bv = red_v[w]; bi = red_i[w]; }
      p.band_max[(size_t)m * DTC_KPS_BANDS + band] = make_float2(bv, __int_as_float(bi));
    }
  }
}

// One thread per map: fold the bands, write the four values of keypoint k of the row; the thread of k = 0 writes the row's status.
__global__ __launch_bounds__(kKpsThreads) void kps_finish_kernel(KpsParams p) {
  const size_t m = (size_t)blockIdx.x * kKpsThreads + threadIdx.x;
  if (m >= (size_t)p.n_rows * p.K) return;
  const int row = (int)(m / p.K), k = (int)(m % p.K);
  const KpsRow r = kps_row(p, row);
  float x = 0.f, y = 0.f, logit = 0.f, prob = 0.f;
  if (r.status == 1) {
    const int n_bands = ceil_div(r.Hr, kps_band_rows(r.Hr));
    const float2* bm = p.band_max + m * DTC_KPS_BANDS;
    const double* bs = p.band_sum + m * DTC_KPS_BANDS;
    int pos = __float_as_int(bm[0].y);
    logit = bm[0].x;
    double sum = bs[0];
    for (int c = 1; c < n_bands; c++) {
      if (kps_better(bm[c].x, __float_as_int(bm[c].y), logit, pos)) { logit = bm[c].x; pos = __float_as_int(bm[c].y); }
      sum += bs[c];
    }
    const int xi = pos % r.Wr, yi = pos / r.Wr;
    x = (float)(((double)xi + 0.5) * (double)r.wc + (double)r.x1);
    y = (float)(((double)yi + 0.5) * (double)r.hc + (double)r.y1);
    prob = (float)(1.0 / sum);
  }
  float* o = p.keyps + (size_t)row * 4 * p.K + k;
  o[0] = x; o[p.K] = y; o[2 * p.K] = logit; o[3 * p.K] = prob;
  if (k == 0) p.kp_status[row] = r.status;
}

struct KpsLayout {
  size_t band_max, band_sum, bytes;
  KpsLayout(int batch, int max_out, int K) {
    Carve c{16};
    const size_t n = (size_t)batch * max_out * K * DTC_KPS_BANDS;
    band_sum = c.take(n * sizeof(double));
    band_max = c.take(n * sizeof(float2));
    bytes = c.end;
  }
};

// shapes and parameters, then limits: DTC_OK, or the code the entry returns
static int kps_check_shape(int batch, int max_out, int K) {
  if (batch < 1 || max_out < 1 || K < 1) return DTC_EINVAL;
  if (batch > DTC_KPS_MAX_BATCH || max_out > DTC_KPS_MAX_OUT || K > DTC_KPS_MAX_KEYPOINTS ||
      (long long)batch * max_out * K > DTC_KPS_MAX_MAPS)
    return DTC_EUNSUPPORTED;
  return DTC_OK;
}

}  // namespace dtc

DTC_API const char* dtc_kps_target_arch(void) { return "gfx950"; }

DTC_API size_t dtc_kps_workspace_bytes(int batch, int max_out, int K) {
  using namespace dtc;
  return kps_check_shape(batch, max_out, K) == DTC_OK ? KpsLayout(batch, max_out, K).bytes : 0;
}

DTC_API int dtc_kps_heatmaps_to_keypoints(const float* heatmaps, const float* dets, const int32_t* det_count, int batch, int max_out,
                                          int K, int S, int person_class, int min_size, void* workspace, size_t workspace_bytes,
                                          float* keyps, int32_t* kp_status, dtc_stream_t stream) {
  using namespace dtc;
  // shapes and parameters
  if (batch < 1 || max_out < 1 || K < 1 || S < 1 || person_class < -1 || min_size < 0) return DTC_EINVAL;
  // limits
  if (S > DTC_KPS_MAX_MAP || min_size > DTC_KPS_MAX_SIDE) return DTC_EUNSUPPORTED;
  if (const int rc = kps_check_shape(batch, max_out, K)) return rc;
  // pointers
  if (!heatmaps || !dets || !det_count || !keyps || !kp_status || !workspace) return DTC_EINVAL;
  if ((reinterpret_cast<uintptr_t>(keyps) & 15) || (reinterpret_cast<uintptr_t>(workspace) & 15)) return DTC_EINVAL;
  // workspace
  const KpsLayout lay(batch, max_out, K);
  if (workspace_bytes < lay.bytes) return DTC_EWORKSPACE;
  KpsParams p;
  p.heatmaps = heatmaps; p.dets = dets; p.det_count = det_count;
  p.max_out = max_out; p.K = K; p.S = S; p.person_class = person_class; p.min_size = min_size;
  p.n_rows = batch * max_out;                                   // <= 2^20
  char* ws = static_cast<char*>(workspace);
  p.band_max = reinterpret_cast<float2*>(ws + lay.band_max);
  p.band_sum = reinterpret_cast<double*>(ws + lay.band_sum);
  p.keyps = keyps; p.kp_status = kp_status;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const unsigned maps = (unsigned)(p.n_rows * K);               // <= 2^20: 2^23 workgroups, 2^31 threads
  const dim3 grid(maps * DTC_KPS_BANDS), block(kKpsThreads);
  hipLaunchKernelGGL(kps_band_kernel<false>, grid, block, 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kps_band_kernel<true>, grid, block, 0, s, p);
  DTC_CHECK_LAUNCH();
  hipLaunchKernelGGL(kps_finish_kernel, dim3(ceil_div((int)maps, kKpsThreads)), block, 0, s, p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
