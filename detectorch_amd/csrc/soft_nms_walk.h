// The Soft-NMS walk of cython_nms.soft_nms (lib/utils_cython/cython_nms.pyx:98-203) by ONE wavefront on LDS arrays -- shared by the
// single-segment drop-in dtc_soft_nms (nms.hip) and the batched detection post-processing (det_soft_nms_kernel, detections.hip), so
// that the two are bit-identical by construction.
//
// The reference's in-place array algorithm: per pick a wave-wide argmax (first maximum, :128-132), the swap (:135-148), a
// lane-parallel decay of the rest (:159-187) and, only when some score fell below the threshold, lane 0 replays the reference's
// swap-with-last loop (:191-199) on the precomputed flags.  Mixed precision exactly as the Cython compiles: `x2 - x1 + 1` etc. are
// float differences promoted to DOUBLE by the literal 1.0 (see oracle/oracle.c orc_soft_nms).
#pragma once
#include "dtc_common.h"

namespace dtc {

// X1..S / I / dead: LDS arrays of n rows (I is carried along with its row, dead is scratch); the caller's workgroup is ONE
// wavefront.  method 0 hard, 1 linear, 2 gaussian (lib/utils/boxes.py:346).  Returns N': rows [0, N') hold the survivors in
// selection order.
__device__ __forceinline__ int soft_nms_walk(float* X1, float* Y1, float* X2, float* Y2, float* S, int32_t* I,
                                             unsigned char* dead, int n, float sigma, float Nt, float threshold, int method,
                                             int lane) {
  int N = n;
  for (int i = 0; i < N; i++) {
    // ---- argmax over [i, N): first maximum in scan order (strict <)  :128-132
    // NaN scores as the reference's `maxscore < boxes[pos, 4]` treats them: the scan starts from row i and a compare with a NaN is
    // false either way, so a NaN at row i stays the pick and a NaN anywhere else is never picked.  Here: NaN candidates are skipped
    // (a lane without candidates keeps the sentinel, so bs is never NaN in the butterfly), and a NaN at row i overrides the result.
    const float si = S[i];
    float bs = -INFINITY; int bp = 0x7fffffff;
    for (int pos = i + lane; pos < N; pos += 64) {
      const float s = S[pos];
      if (s == s && (bp == 0x7fffffff || s > bs)) { bs = s; bp = pos; }   // within a lane positions ascend: keep the first max
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float os = __shfl_xor(bs, off, 64);
      const int op = __shfl_xor(bp, off, 64);
      const bool take = (op != 0x7fffffff) && (bp == 0x7fffffff || os > bs || (os == bs && op < bp));
      if (take) { bs = os; bp = op; }
    }
    const int maxpos = si == si ? bp : i;
    // ---- swap rows i and maxpos  :135-148
    if (lane == 0 && maxpos != i) {
      float t;
      t = X1[i]; X1[i] = X1[maxpos]; X1[maxpos] = t;
      t = Y1[i]; Y1[i] = Y1[maxpos]; Y1[maxpos] = t;
      t = X2[i]; X2[i] = X2[maxpos]; X2[maxpos] = t;
      t = Y2[i]; Y2[i] = Y2[maxpos]; Y2[maxpos] = t;
      t = S[i]; S[i] = S[maxpos]; S[maxpos] = t;
      const int ti = I[i]; I[i] = I[maxpos]; I[maxpos] = ti;
    }
    __syncthreads();
    const float tx1 = X1[i], ty1 = Y1[i], tx2 = X2[i], ty2 = Y2[i];
    // ---- decay the rest  :159-187
    bool any_dead = false;
    for (int pos = i + 1 + lane; pos < N; pos += 64) {
      const float x1 = X1[pos], y1 = Y1[pos], x2 = X2[pos], y2 = Y2[pos];
      const float area = (float)(((double)(x2 - x1) + 1.0) * ((double)(y2 - y1) + 1.0));      // :166
      const float iw = (float)((double)(fminf(tx2, x2) - fmaxf(tx1, x1)) + 1.0);              // :167
      bool d = false;
      if (iw > 0.f) {
        const float ih = (float)((double)(fminf(ty2, y2) - fmaxf(ty1, y1)) + 1.0);            // :169
        if (ih > 0.f) {
          const float ua = (float)(((((double)(tx2 - tx1) + 1.0) * ((double)(ty2 - ty1) + 1.0)) + (double)area) -
                                   (double)(iw * ih));                                       // :171
          const float ov = fdiv(iw * ih, ua);                                                 // :172
          float weight;
          if (method == 1) weight = ov > Nt ? (float)(1.0 - (double)ov) : 1.f;                // :174-178
          else if (method == 2) weight = (float)exp((double)fdiv(-(ov * ov), sigma));         // :180
          else weight = ov > Nt ? 0.f : 1.f;                                                  // :182-185
          const float ns = weight * S[pos];                                                   // :187
          S[pos] = ns;
          d = ns < threshold;                                                                 // :191
        }
      }
      dead[pos] = d ? 1 : 0;
      any_dead |= d;
    }
    any_dead = __any(any_dead);
    __syncthreads();
    // ---- discard by swap-with-last, replayed sequentially on the flags  :191-199
    if (any_dead) {
      if (lane == 0) {
        int pos = i + 1;
        while (pos < N) {
          if (dead[pos]) {
            X1[pos] = X1[N - 1]; Y1[pos] = Y1[N - 1]; X2[pos] = X2[N - 1]; Y2[pos] = Y2[N - 1]; S[pos] = S[N - 1];
            I[pos] = I[N - 1]; dead[pos] = dead[N - 1];
            N = N - 1; pos = pos - 1;
          }
          pos = pos + 1;
        }
      }
      N = __shfl(N, 0, 64);
      __syncthreads();
    }
  }
  return N;
}

// LDS bytes of a walk over n rows (the layout of soft_nms_lds_arrays)
__host__ __device__ __forceinline__ size_t soft_nms_lds_bytes(int n) { return (size_t)n * (6 * 4 + 1) + 16; }

struct SoftNmsLds { float *X1, *Y1, *X2, *Y2, *S; int32_t* I; unsigned char* dead; };
__device__ __forceinline__ SoftNmsLds soft_nms_lds_arrays(unsigned char* smem, int n) {
  SoftNmsLds a;
  a.X1 = reinterpret_cast<float*>(smem);
  a.Y1 = a.X1 + n; a.X2 = a.Y1 + n; a.Y2 = a.X2 + n; a.S = a.Y2 + n;
  a.I = reinterpret_cast<int32_t*>(a.S + n);
  a.dead = reinterpret_cast<unsigned char*>(a.I + n);
  return a;
}

}  // namespace dtc
