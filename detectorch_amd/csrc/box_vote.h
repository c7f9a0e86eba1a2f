// The IoU primitive of cython_bbox.bbox_overlaps and the numpy-order body of box_voting with 'ID' scoring (lib/utils/boxes.py:280-329)
// as device functions -- shared by the single-segment drop-ins of bbox_ops.hip (dtc_bbox_overlaps, dtc_box_voting) and the batched
// detection post-processing (det_vote_kernel, detections.hip), so that the two are bit-identical by construction.
//
// Numerics (oracle/oracle.c:orc_bbox_overlaps has the derivation, pinned against the reference's own Cython build): every
// `a - b + 1` is (double)(a - b) + 1.0 -- the subtraction in float32, the +1 and span products in double -- rounded to float32
// where the reference stores into a DTYPE_t variable; iw*ih is a float32 product; the division is IEEE float32.
// box_voting reproduces numpy's evaluation order: the weighted coordinate sums add the voters in index order (axis-0
// reduction of the [m,4] product), the weight sum is numpy's pairwise float32 summation.
#pragma once
#include "dtc_common.h"

namespace dtc {

__device__ __forceinline__ double span1(float hi, float lo) { return (double)(hi - lo) + 1.0; }

// one element of bbox_overlaps: box B vs query Q (cython_bbox.pyx:54-74)
__device__ __forceinline__ float iou_bbox(float4 B, float4 Q) {
  const float box_area = (float)(span1(Q.z, Q.x) * span1(Q.w, Q.y));          // :54-57
  const float iw = (float)span1(fminf(B.z, Q.z), fmaxf(B.x, Q.x));            // :59-62
  if (!(iw > 0.f)) return 0.f;
  const float ih = (float)span1(fminf(B.w, Q.w), fmaxf(B.y, Q.y));            // :64-67
  if (!(ih > 0.f)) return 0.f;
  const float ua = (float)(span1(B.z, B.x) * span1(B.w, B.y) + (double)box_area - (double)(iw * ih));   // :69-73
  return fdiv(iw * ih, ua);                                                   // :74
}

// numpy float32 pairwise add-reduce over W(0 .. n-1) (see oracle/oracle.c:np_pairwise_sum_f32), explicit stack instead of
// recursion: blocks of <= 128 elements, split at n/2 rounded down to a multiple of 8.
template <typename WF> __device__ float np_sum_f32(WF W, int n) {
  auto leaf = [&](int s, int m) {
    if (m < 8) {
      float r = 0.f;
      for (int i = 0; i < m; i++) r += W(s + i);
      return r;
    }
    float r0 = W(s), r1 = W(s + 1), r2 = W(s + 2), r3 = W(s + 3), r4 = W(s + 4), r5 = W(s + 5), r6 = W(s + 6), r7 = W(s + 7);
    int i = 8;
    for (; i < m - (m % 8); i += 8) {
      r0 += W(s + i); r1 += W(s + i + 1); r2 += W(s + i + 2); r3 += W(s + i + 3);
      r4 += W(s + i + 4); r5 += W(s + i + 5); r6 += W(s + i + 6); r7 += W(s + i + 7);
    }
    float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
    for (; i < m; i++) res += W(s + i);
    return res;
  };
  int fs[16], fn[16], fstage[16];
  float val[16];
  int sp = 0, vp = 0;
  fs[0] = 0; fn[0] = n; fstage[0] = 0; sp = 1;
  while (sp > 0) {
    const int s = fs[sp - 1], m = fn[sp - 1];
    if (m <= 128) { val[vp++] = leaf(s, m); sp--; continue; }
    int n2 = m / 2; n2 -= n2 % 8;
    if (fstage[sp - 1] == 0) { fstage[sp - 1] = 1; fs[sp] = s; fn[sp] = n2; fstage[sp] = 0; sp++; }
    else if (fstage[sp - 1] == 1) { fstage[sp - 1] = 2; fs[sp] = s + n2; fn[sp] = m - n2; fstage[sp] = 0; sp++; }
    else { const float b = val[--vp]; const float a = val[--vp]; val[vp++] = a + b; sp--; }
  }
  return val[0];
}

// box_voting(top, all, thresh, 'ID') for ONE top box B by one wavefront (lib/utils/boxes.py:287-296).  The voters are the rows
// j < a of all_dets with cand(j) (a sparse row set: the batched caller's candidate bitmap) and IoU(B, box(j)) >= thresh, in
// increasing j; coord(j, c) is column c < 4 of row j, score(j) its weight.  vl: the wave's LDS voter list, capacity >= a.
// Returns, in lane c < 4, coordinate c of the voted box (the top box's own coordinate `top_c` when nobody votes); other lanes 0.
template <typename CandF, typename BoxF, typename CoordF, typename ScoreF>
__device__ __forceinline__ float box_vote_one(float4 B, float top_c, int a, float thresh, CandF cand, BoxF box, CoordF coord,
                                              ScoreF score, int* vl, int lane, int* n_voters) {
  int m = 0;
  for (int j0 = 0; j0 < a; j0 += 64) {
    const int j = j0 + lane;
    bool vote = false;
    if (j < a && cand(j)) vote = iou_bbox(B, box(j)) >= thresh;                   // boxes.py:292
    const uint64_t bal = __ballot(vote);
    if (vote) vl[m + __builtin_popcountll(bal & ((1ull << lane) - 1ull))] = j;
    m += __builtin_popcountll(bal);
  }
  __syncthreads();
  float res = 0.f;
  if (lane < 4) {            // weighted coordinate sums: voters in index order (axis-0 reduce of boxes * ws[:, None])
    float acc = 0.f;
    for (int i = 0; i < m; i++) {
      const int j = vl[i];
      const float prod = coord(j, lane) * score(j);
      acc = i == 0 ? prod : acc + prod;
    }
    res = acc;
  }
  float scl = 0.f;
  if (lane == 4 && m > 0) scl = np_sum_f32([&](int i) { return score(vl[i]); }, m);   // ws.sum(): numpy pairwise
  scl = __shfl(scl, 4, 64);
  *n_voters = m;
  return lane < 4 ? (m > 0 ? fdiv(res, scl) : top_c) : 0.f;                          // :295 np.average
}

}  // namespace dtc
