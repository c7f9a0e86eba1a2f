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
#include "wave_ops.h"

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

// one leaf (a block of m <= 128 elements) of numpy's float32 pairwise sum; NX() yields the block's elements in order
template <typename NX> __device__ __forceinline__ float np_leaf_f32(NX nx, int m) {
  if (m < 8) {
    float r = 0.f;
    for (int i = 0; i < m; i++) r += nx();
    return r;
  }
  float r0 = nx(), r1 = nx(), r2 = nx(), r3 = nx(), r4 = nx(), r5 = nx(), r6 = nx(), r7 = nx();   // declarators: in order
  int i = 8;
  for (; i < m - (m % 8); i += 8) {
    r0 += nx(); r1 += nx(); r2 += nx(); r3 += nx();
    r4 += nx(); r5 += nx(); r6 += nx(); r7 += nx();
  }
  float res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < m; i++) res += nx();
  return res;
}

// numpy's pairwise tree over n elements, explicit stack instead of recursion: blocks of <= 128 elements, split at n/2 rounded
// down to a multiple of 8.  leaf(s, m) is called for the leaves in increasing s; their values are combined in the tree's order.
template <typename LF> __device__ float np_pairwise_tree(LF leaf, int n) {
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

// numpy float32 pairwise add-reduce over W(0 .. n-1) (see oracle/oracle.c:np_pairwise_sum_f32), by one lane
template <typename WF> __device__ float np_sum_f32(WF W, int n) {
  return np_pairwise_tree([&](int s, int m) { int i = s; return np_leaf_f32([&]() { return W(i++); }, m); }, n);
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
    if (vote) vl[m + lanes_below(bal, lane)] = j;
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


// ---- scoring_method other than 'ID' (boxes.py:297-323): the voted score of ONE top box by one wavefront ------------------------------
// Method codes of dtc_vote_scoring (include/detectorch_hip.h).
enum { kVoteID = 0, kVoteTempAvg = 1, kVoteAvg = 2, kVoteIouAvg = 3, kVoteGeneralizedAvg = 4, kVoteQuasiSum = 5 };
constexpr int kVoteWordsMax = 128;   // voter words of a top box: n_all <= 8192 (single segment), R <= 4096 (batched: 64)

// The wave's LDS scratch of vote_score: the voter set as ballot words and their popcount prefix, one float per pairwise leaf.
struct VoteScratch {
  uint64_t w[kVoteWordsMax];
  int pre[kVoteWordsMax + 1];
  float leaf[kVoteWordsMax];       // the pairwise tree of n <= 8192 elements has <= 128 leaves (every leaf of n > 128 holds >= 64)
};

// numpy's float32 pairwise sum of V(k) over the voters k of vs (in increasing k), by one wave: the tree's leaves are independent
// blocks -> one lane each (leaf i on lane i % 64, the voters walked from the ballot words); lane 0 combines them in the tree's order.
// Every lane returns the sum.
template <typename VF> __device__ float wave_voter_sum(VF V, VoteScratch& vs, int nw, int n, int lane) {
  auto walk = [&](int s, int m) {                      // the leaf [s, s + m) of voters, walked from the ballot words
    int lo = 0, hi = nw;                               // the word holding voter s: the last word with pre[wi] <= s
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (vs.pre[mid] <= s) lo = mid; else hi = mid; }
    int wi = lo;
    uint64_t cur = vs.w[wi];
    for (int t = s - vs.pre[wi]; t > 0; t--) cur &= cur - 1ull;
    return np_leaf_f32([&]() {
      while (cur == 0ull) cur = vs.w[++wi];
      const int k = wi * 64 + __builtin_ctzll(cur);
      cur &= cur - 1ull;
      return V(k);
    }, m);
  };
  if (n <= 128) {                                      // the tree is one leaf (the usual class segment): no walk, no exchange
    float r = 0.f;
    if (lane == 0) r = walk(0, n);
    return __shfl(r, 0, 64);
  }
  int s0 = 0, m0 = 0, s1 = 0, m1 = 0;                  // this lane's leaves: number lane and lane + 64
  int nl = 0;
  np_pairwise_tree([&](int s, int m) {                 // uniform: every lane walks the same tree and keeps the leaves it owns
    if (nl == lane) { s0 = s; m0 = m; }
    if (nl == lane + 64) { s1 = s; m1 = m; }
    nl++;
    return 0.f;
  }, n);
  if (m0 > 0) vs.leaf[lane] = walk(s0, m0);
  if (m1 > 0) vs.leaf[lane + 64] = walk(s1, m1);
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  float r = 0.f;
  if (lane == 0) { int li = 0; r = np_pairwise_tree([&](int, int) { return vs.leaf[li++]; }, n); }
  return __shfl(r, 0, 64);
}

// The score of box_voting's scoring_method for one top box, in numpy's float32 order; vs.w[0 .. nw) holds the voter set (bit k of
// word k / 64: candidate k votes, as box_vote_one selects them), n > 0 voters.  ws(k): the voter's score, iou(k): its IoU with the top
// box (top_to_all_overlaps[k]).  The wave's lanes all return the score.
//   AVG              ws.mean(): the pairwise float32 sum, divided by the count in double (np.mean divides by an intp), rounded
//   IOU_AVG          np.average(ws, weights=iou): pairwise sum of the float32 products over the pairwise sum of the IoUs
//   QUASI_SUM        ws.sum() / float(n) ** beta: the power in double (Python), the division in float32 (numpy 2 scalar rules)
//   GENERALIZED_AVG  np.mean(ws ** beta) ** (1.0 / beta): exact at beta 1 (pow(x, 1) = x); else powers evaluated in double, rounded
//   TEMP_AVG         per voter p = ws, q = 1 - ws, x = log(y / max(p, q)), e = exp(x / beta), t = e_p / (e_p + e_q); then mean(t);
//                    log / exp in double, rounded (numpy's float32 SIMD routines differ by a few ulp: not bit-exact)
template <typename WF, typename IF>
__device__ float vote_score(int method, float beta, VoteScratch& vs, int nw, int n, WF ws, IF iou, int lane) {
  {                                                    // popcount prefix of the words: two shuffle scans of 64 words
    int carry = 0;
    for (int w0 = 0; w0 < nw; w0 += 64) {
      const int w = w0 + lane;
      const int pc = w < nw ? __builtin_popcountll(vs.w[w]) : 0;
      const int incl = wave_incl_scan(pc, lane);
      if (w < nw) vs.pre[w] = carry + incl - pc;
      carry += __shfl(incl, 63, 64);
    }
    if (lane == 0) vs.pre[nw] = carry;
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  }
  const double dn = (double)n;
  switch (method) {
    case kVoteAvg: {
      const float s = wave_voter_sum(ws, vs, nw, n, lane);
      return (float)((double)s / dn);
    }
    case kVoteIouAvg: {
      const float num = wave_voter_sum([&](int k) { return ws(k) * iou(k); }, vs, nw, n, lane);
      const float den = wave_voter_sum(iou, vs, nw, n, lane);
      return fdiv(num, den);
    }
    case kVoteQuasiSum: {
      const float s = wave_voter_sum(ws, vs, nw, n, lane);
      return fdiv(s, (float)pow(dn, (double)beta));
    }
    case kVoteGeneralizedAvg: {
      const bool one = beta == 1.f;
      const float s = wave_voter_sum([&](int k) { return one ? ws(k) : (float)pow((double)ws(k), (double)beta); }, vs, nw, n, lane);
      const float mean = (float)((double)s / dn);
      return one ? mean : (float)pow((double)mean, (double)(float)(1.0 / (double)beta));
    }
    default: {                                          // kVoteTempAvg
      const float s = wave_voter_sum([&](int k) {
        const float p = ws(k), q = 1.f - p, mx = fmaxf(p, q);
        const float ep = (float)exp((double)fdiv((float)log((double)fdiv(p, mx)), beta));
        const float eq = (float)exp((double)fdiv((float)log((double)fdiv(q, mx)), beta));
        return fdiv(ep, ep + eq);
      }, vs, nw, n, lane);
      return (float)((double)s / dn);
    }
  }
}

// The voter set of top box B as ballot words into vs.w[0 .. ceil(a / 64)): candidate j < a votes iff cand(j) and
// iou_bbox(B, box(j)) >= thresh (box_vote_one's selection).  Returns the number of voters.
template <typename CandF, typename BoxF>
__device__ __forceinline__ int vote_words(float4 B, int a, float thresh, CandF cand, BoxF box, VoteScratch& vs, int lane) {
  int m = 0;
  for (int j0 = 0; j0 < a; j0 += 64) {
    const int j = j0 + lane;
    bool vote = false;
    if (j < a && cand(j)) vote = iou_bbox(B, box(j)) >= thresh;
    const uint64_t bal = __ballot(vote);
    if (lane == 0) vs.w[j0 >> 6] = bal;
    m += __builtin_popcountll(bal);
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  return m;
}

}  // namespace dtc
