// A8  Detection post-processing for gfx950 -- replaces postprocess_output (lib/utils/result_utils.py:76-94) and
// box_results_with_nms_and_limit (:96-168, hard-NMS branch), which run on the host: 3 D2H copies, numpy decode of all
// R x 81 boxes, an 80-iteration Python loop calling Cython NMS, np.sort for the per-image limit.
//
//   det_candidates   grid (class, image): score > thresh (:127) -> ordered compaction (dets_j order), class-specific box
//                    decode with weights (10,10,5,5) (lib/utils/boxes.py:168-208) ONLY for the candidates, clip to the
//                    original image (:150-165), (score desc, index asc) sort in LDS -> NMS input
//                    and the segment's hard NMS (cython_nms.pyx:37-87) in the same workgroup: blocks of 64 rows, diagonal tile by
//                    four waves, greedy walk by one, later columns marked by all (round 4; until then a separate launch pair)
//   det_finalize     grid (image): max_detections_per_img limit (:154-163) = radix select of the 100-th largest score,
//                    `>=` filter (ties kept, like the reference), class-major / roi-ascending output (:165).
//
// Test-time options (dtc_postprocess_detections_ex, dtc_det_options; the reference's do_soft_nms / do_bbox_vote, :133-153):
//   Soft-NMS         det_candidates stops after the compaction and the decode and writes the candidates in dets_j order (roi
//                    ascending, :127-132) from the candidate bitmap; det_soft_nms (one wave per (class, image) segment) runs the
//                    single-segment walk of soft_nms_walk.h on an LDS copy (25 B per candidate: <= 100 KB at R = 4096) and
//                    publishes the kept rows in SELECTION order as the same (ordered decayed score, roi) keys the hard NMS
//                    writes; det_finalize's limit is unchanged and its output keeps the per-class selection order (:143, :165).
//                    One wave per segment and not the four-wave workgroup of the hard NMS: the walk is one dependent pick after
//                    another with a barrier each, which extra waves cannot shorten.
//   bbox voting      ('ID' scoring) never changes a score, and the per-image limit depends on the scores alone, so the rows that
//                    survive the limit are the same whether the vote comes before or after it: det_vote votes only the <= max_out
//                    EMITTED rows (one wave per row, box_vote.h -- the single-segment drop-in's body) against every candidate of
//                    the row's segment (the undecayed dets_j, :150), rewrites the box and det_rois_scaled; with the FPN mask
//                    mapping requested the mapping runs after the vote, on the voted boxes (det_fpn_map, one more launch).
//   Launch count is fixed per option set (graph capture): + det_soft_nms with Soft-NMS, + det_vote (+ det_fpn_map) with voting.
#include "block_sort.h"
#include "box_decode.h"
#include "box_vote.h"
#include "dtc_common.h"
#include "fpn_map.h"
#include "iou_threshold.h"
#include "radix_select.h"
#include "soft_nms_walk.h"
#include "softmax_fold.h"
#include "wave_ops.h"

namespace dtc {

constexpr int kDetThreads = 256;
constexpr int kNmsLdsCap = 512;       // candidates of a (class, image) segment whose boxes the in-workgroup NMS keeps in LDS

struct DetParams {
  const float* rois5;        // [B, R, 5]
  const int32_t* n_rois;     // [B] or NULL (all R valid)
  const float* cls_score;    // [B, R, n_cls]  probabilities, or LOGITS when sm_stats != NULL
  const double* sm_stats;    // [B, R, 2] = (row max, sum_j exp(l_j - max)) of the class logits, or NULL
  const float* bbox_pred;    // [B, R, 4*n_cls]
  const float* decoded;      // [B, R, 4*n_cls] already decoded + clipped boxes (box_results_with_nms_and_limit's input), or NULL
  const float* scale;        // [B] scaling factor per image
  const float* im_size;      // [B, 2] original (h, w)
  int R, n_cls;
  float wx, wy, ww, wh, score_thresh;
  // per (image, class) segment s = b*(n_cls-1) + (j-1), stride R
  float* sorted_boxes;       // [S, R, 4]   score order: scratch of the NMS for segments of more than kNmsLdsCap candidates
  float* q_boxes;            // [S, R, 4]   candidate order
  float* q_scores;           // [S, R]
  int32_t* q_roi;            // [S, R]
  int32_t* cand_count;       // [S]
  // per-class NMS, in this kernel: the sort keys (~ordered score << 32 | candidate index q) of the kept boxes, in score order,
  // and their number -- everything det_finalize needs about a kept box in ONE load
  uint64_t* kept_key;        // [S, R]
  int32_t* keep_count;       // [S]
  float nms_thresh;
  int np2_max;               // next_pow2(R): the sort keys occupy the first np2_max * 8 bytes of the dynamic LDS
  // options (dtc_det_options): soft -> no sort / NMS here, q_roi[seg, k] = roi of the k-th candidate in dets_j order (det_soft_nms
  // reads it); cand_bits (soft or voting, else NULL) -> the candidate bitmap of the segment, bit r of word r / 64
  int soft;
  uint64_t* cand_bits;       // [S, 64]
};

constexpr int kCandWords = 64;   // bitmap words per segment: R <= 4096

// ---- box-head epilogue fusion: class scores handed over as LOGITS -----------------------------------------
// The reference applies F.softmax to the cls_score layer's output (lib/model/detector.py:281) and hands the [R,81]
// probability map to postprocess_output.  Here the probability is formed where it is consumed: one wave per roi row
// reduces (max, sum of exp) once -- 16 bytes per roi instead of a second [R,81] map -- and det_candidates evaluates
//     prob[r,j] = float( exp(double(l[r,j]) - max_r) / sum_r )
// for the one class column it scans.  Evaluated in double and rounded once, the sum taken in a FIXED order (element j goes
// to slot j % 64 in increasing j, then a 64 -> 1 halving tree), so that oracle/oracle.py:softmax_rows gives the same bits;
// torch's float32 softmax agrees with it to rel 1e-6 (tests/test_oracle_golden.py).
__global__ __launch_bounds__(kDetThreads) void det_softmax_stats_kernel(const float* logits, int n_rows, int n_cls, double* stats) {
  const int row = blockIdx.x * (kDetThreads / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= n_rows) return;
  float m;
  double e;
  softmax_row_stats(logits + (size_t)row * n_cls, n_cls, lane, m, e);
  if (lane == 0) { stats[(size_t)row * 2] = (double)m; stats[(size_t)row * 2 + 1] = e; }
}

__global__ __launch_bounds__(kDetThreads) void det_candidates_kernel(DetParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem);
  __shared__ int running;
  __shared__ uint64_t cbits_s[kCandWords];
  const int j = blockIdx.x + 1, b = blockIdx.y;
  const int seg = b * (p.n_cls - 1) + (j - 1);
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nr = p.n_rois ? min(p.n_rois[b], p.R) : p.R;
  const float* sc = p.cls_score + (size_t)b * p.R * p.n_cls + j;
  float* qs = p.q_scores + (size_t)seg * p.R;
  if (tid == 0) running = 0;
  __syncthreads();
  // compaction of {r : scores[r, j] > thresh}  (np.where, result_utils.py:127).  Round 6: UNORDERED -- a wave claims its slots with
  // one LDS atomic, no workgroup barrier per chunk.  Nothing downstream depends on the slot order: the sort key carries the ROI INDEX r
  // ((score desc, r asc) is the order (score desc, candidate index asc) was, the candidate index being monotone in r), and the
  // per-candidate scratch (q_boxes / q_scores) is indexed by r.  The scores of FOUR chunks of 256 rois are requested before the first
  // is consumed, and before the image's roi count is known (the array is [B, R, n_cls]: every address is valid; rows past the count
  // are masked afterwards) -- one global round trip in front of the first compare instead of two dependent ones.
  int R0 = 0;
  do {
    float sv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int r = R0 + u * kDetThreads + tid;
      sv[u] = 0.f;
      if (r < p.R) {
        sv[u] = sc[(size_t)r * p.n_cls];
        if (p.sm_stats) {      // logits in: softmax column formed here (detector.py:281)
          const double* st = p.sm_stats + ((size_t)b * p.R + r) * 2;
          sv[u] = DTC_SOFTMAX_PROB(sv[u], st);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int r = R0 + u * kDetThreads + tid;
      const float s = sv[u];
      const bool ok = r < nr && s > p.score_thresh;
      const uint64_t m = __ballot(ok);
      if (p.cand_bits && lane == 0) cbits_s[((R0 + u * kDetThreads) >> 6) + wv] = m;     // rois [64 w, 64 w + 64): w < 64
      if (m == 0ull) continue;                                 // uniform per wave
      int base = 0;
      if (lane == 0) base = atomicAdd(&running, __builtin_popcountll(m));
      base = uni(base);
      if (ok) {
        qs[r] = s;
        keys[base + lanes_below(m, lane)] = make_desc_key(s, (uint32_t)r);
      }
    }
    R0 += 4 * kDetThreads;
  } while (R0 < nr);
  __syncthreads();
  const int n = running;
  if (tid == 0) {
    p.cand_count[seg] = n;
    if (n == 0) p.keep_count[seg] = 0;
  }
  const int nw = (nr + 63) >> 6;
  if (p.cand_bits)
    for (int w = tid; w < nw; w += kDetThreads) p.cand_bits[(size_t)seg * kCandWords + w] = cbits_s[w];
  if (n == 0) return;
  float4* qb = reinterpret_cast<float4*>(p.q_boxes) + (size_t)seg * p.R;
  const float sf = p.decoded ? 1.f : p.scale[b];
  const float im_h = p.decoded ? 0.f : p.im_size[b * 2 + 0], im_w = p.decoded ? 0.f : p.im_size[b * 2 + 1];
  auto box_of = [&](int r) {
    float4 v;
    if (p.decoded) {        // lib/utils/result_utils.py:128: boxes[inds, j * 4:(j + 1) * 4] taken as they are
      const float* d = p.decoded + ((size_t)b * p.R + r) * 4 * p.n_cls + 4 * j;
      v = make_float4(d[0], d[1], d[2], d[3]);
    } else {
      const float* roi = p.rois5 + ((size_t)b * p.R + r) * 5 + 1;
      const float* d = p.bbox_pred + ((size_t)b * p.R + r) * 4 * p.n_cls + 4 * j;
      const float x1 = fdiv(roi[0], sf), y1 = fdiv(roi[1], sf), x2 = fdiv(roi[2], sf), y2 = fdiv(roi[3], sf);  // result_utils.py:77
      v = decode_clip<true>(x1, y1, x2, y2, d, p.wx, p.wy, p.ww, p.wh, im_h, im_w);   // the class's box, clipped to the original image
    }
    return v;
  };
  if (p.soft) {
    // Soft-NMS input: the candidates in dets_j order (np.where is ascending, :127) -- an ordered compaction of the bitmap: wave 0
    // scans the popcounts of the <= 64 words, each lane lists its word's rois; then every thread decodes
    uint32_t* lst = reinterpret_cast<uint32_t*>(smem);        // over the (unused) sort keys: n * 4 <= np2_max * 8 bytes
    if (wv == 0) expand_bitmap(lane < nw ? cbits_s[lane] : 0ull, lane, lst);
    __syncthreads();
    for (int k = tid; k < n; k += kDetThreads) {
      const int r = (int)lst[k];
      qb[r] = box_of(r);
      p.q_roi[(size_t)seg * p.R + k] = r;
    }
    return;
  }
  const int np2 = next_pow2(n);
  for (int i = n + tid; i < np2; i += kDetThreads) keys[i] = kPadKey;
  block_bitonic_sort<kDetThreads>(keys, np2);
  // the box of rank k (decoded once): to q_boxes[r] for det_finalize, and in SCORE order for the NMS below -- in LDS when the segment
  // has at most kNmsLdsCap candidates (the usual tens to a few hundred), else in the global scratch p.sorted_boxes (LDS sized for
  // every possible segment would leave 2 workgroups per CU)
  float4* sbox_l = reinterpret_cast<float4*>(smem + (size_t)p.np2_max * sizeof(uint64_t));     // [kNmsLdsCap]
  float4* sorted_g = reinterpret_cast<float4*>(p.sorted_boxes) + (size_t)seg * p.R;
  const bool in_lds = n <= kNmsLdsCap;
  for (int k = tid; k < n; k += kDetThreads) {
    const int r = (int)desc_key_index(keys[k]);
    const float4 v = box_of(r);
    qb[r] = v;                                               // by roi index (global, det_finalize)
    if (in_lds) sbox_l[k] = v; else sorted_g[k] = v;         // score order (the NMS)
  }
  __syncthreads();
  // ---- the segment's hard NMS, here (cython_nms.pyx:37-87: greedy over the score order; the kept box of rank i suppresses every
  // later box j with inter / (area_i + area_j - inter) >= thresh, IEEE division).  The class segments of a detection batch hold tens
  // of candidates (one 64-row block); as a separate launch pair (mask tiles + reduce over 640 segments) they cost 25 us of which
  // 20 were launch latency.  Blocks of 64 rows: (1) the four waves form the block's diagonal tile (16 rows each), (2) wave 0 walks
  // the block greedily with the bits removed by earlier blocks, (3) the block's kept rows mark the later columns they suppress
  // (one 64-column word per wave and step).  n^2 / 2 pair tests by ONE workgroup: 50 candidates 3 us, 1000 ~100 us, 4096 would be
  // ~1.5 ms -- a deliberate trade for the 81-class detection heads this path serves (segments of tens of candidates); a model with a
  // handful of classes, a very low score threshold or collect_top_n >> 2000 makes a class segment the critical path of the launch
  // (timing guard: tests/test_hip_fpn_det_mask.py::test_postprocess_crowded_classes_vs_oracle, R = 1500 x 3 classes).
  {
    uint64_t* removed = reinterpret_cast<uint64_t*>(sbox_l + kNmsLdsCap);                            // [(R + 63) / 64]
    __shared__ uint32_t diag_s[kDetThreads / 64][64];
    __shared__ uint64_t keptm_s;
    __shared__ int kept_s;
    const int ncb = (n + 63) >> 6;
    for (int wd = tid; wd < ncb; wd += kDetThreads) removed[wd] = 0ull;
    if (tid == 0) kept_s = 0;
    __syncthreads();
    const float thr = p.nms_thresh;
    const bool thr_pos = thr > 0.f;
    // `inter / (area_r + area_c - inter) >= thresh` with an IEEE division -- decided from the sign of inter - thresh * u; the division
    // only when some lane of the wavefront is inside the band where that sign is not reliable (iou_threshold.h)
    auto iou_ge = [&](const float4& r, float rarea, const float4& c, float carea) {
      const float xx1 = fmaxf(r.x, c.x), yy1 = fmaxf(r.y, c.y), xx2 = fminf(r.z, c.z), yy2 = fminf(r.w, c.w);   // :76-79
      const float w = fmaxf(0.0f, xx2 - xx1 + 1.f), h = fmaxf(0.0f, yy2 - yy1 + 1.f);                         // :80-81
      const float inter = w * h;                                                                            // :82
      const float u = rarea + carea - inter;
      float d;
      const bool unsure = iou_band(inter, u, thr, d);
      if (__builtin_amdgcn_ballot_w64(unsure) == 0ull && thr_pos) return d > 0.f;
      return (unsure || !thr_pos) ? fdiv(inter, u) >= thr : d > 0.f;                                         // :83-84
    };
    uint64_t* K = p.kept_key + (size_t)seg * p.R;
    const float4 pad = make_float4(0.f, 0.f, -1.f, -1.f);
    auto run_blocks = [&](auto lds_tag) {
    const float4* sbox = decltype(lds_tag)::value ? static_cast<const float4*>(sbox_l) : static_cast<const float4*>(sorted_g);
    for (int rb = 0; rb < ncb; rb++) {
      const int i0 = rb * 64, nrow = min(64, n - i0);
      // (1) diagonal tile: which rows r < lane of this block suppress column i0 + lane; wave wv tests rows [16 wv, 16 wv + 16)
      const float4 cbx = lane < nrow ? sbox[i0 + lane] : pad;
      const float carea = box_area(cbx);
      uint32_t part = 0;
      for (int r = 16 * wv; r < min(16 * wv + 16, nrow); r++) {
        const float4 rbx = sbox[i0 + r];                       // uniform address: LDS broadcast
        const bool sup = lane > r && lane < nrow && iou_ge(rbx, box_area(rbx), cbx, carea);
        part |= sup ? (1u << (r - 16 * wv)) : 0u;
      }
      diag_s[wv][lane] = part;
      __syncthreads();
      // (2) greedy walk of the block (wave 0): a row is kept iff no earlier kept row (earlier blocks: `removed`) suppresses it
      if (wv == 0) {
        const uint64_t colword = (uint64_t)diag_s[0][lane] | ((uint64_t)diag_s[1][lane] << 16) | ((uint64_t)diag_s[2][lane] << 32) |
                                 ((uint64_t)diag_s[3][lane] << 48);
        // the greedy answer as a fixed point: row j is kept iff it is a candidate and no KEPT earlier row of the block suppresses it;
        // K <- {j : cand_j and colword_j & K == 0} from K = cand settles rows in increasing order (row 0 after one step, row j once
        // the rows before it have settled) -- a few wave-wide steps instead of one dependent step per row
        const uint64_t cand = __ballot(lane < nrow) & ~removed[rb];
        const bool mine = (cand >> lane) & 1ull;
        uint64_t keptm = cand;
        for (int it = 0; it < 64; it++) {
          const uint64_t nk = __ballot(mine && (colword & keptm) == 0ull);
          if (nk == keptm) break;
          keptm = nk;
        }
        const int base = kept_s;
        if ((keptm >> lane) & 1ull) K[base + lanes_below(keptm, lane)] = keys[i0 + lane];
        if (lane == 0) { keptm_s = keptm; kept_s = base + __builtin_popcountll(keptm); }
      }
      __syncthreads();
      // (3) the kept rows of this block against every later column: a wave takes one 64-column word per step
      const uint64_t keptm = keptm_s;
      // wave wv takes the block's rows [16 wv, 16 wv + 16) against EVERY later 64-column word (lane <-> column): a segment of ~100
      // candidates has one such word, and its ~50 kept rows are four waves' 13 instead of one wave's 50
      const uint64_t mine_rows = keptm & (0xffffull << (16 * wv));
      if (mine_rows) {
        for (int c0 = i0 + 64; c0 < n; c0 += 64) {
          const int j = c0 + lane;
          const float4 cj = j < n ? sbox[j] : pad;
          const float aj = box_area(cj);
          bool sup = false;
          for (uint64_t km = mine_rows; km; km &= km - 1ull) {   // uniform
            const float4 rbx = sbox[i0 + __builtin_ctzll(km)];
            sup = sup || iou_ge(rbx, box_area(rbx), cj, aj);
          }
          const uint64_t m = __ballot(j < n && sup);
          if (lane == 0 && m) atomicOr(reinterpret_cast<unsigned long long*>(&removed[c0 >> 6]), (unsigned long long)m);
        }
      }
      __syncthreads();
    }
    };
    if (in_lds) run_blocks(std::true_type{}); else run_blocks(std::false_type{});
    if (tid == 0) p.keep_count[seg] = kept_s;
  }
}

// ---- Soft-NMS of the (class, image) segments (cython_nms.soft_nms via box_utils.soft_nms, result_utils.py:133-140): one wavefront per
// segment walks the single-segment drop-in's algorithm (soft_nms_walk.h) on an LDS copy of the segment's dets_j, then publishes the
// survivors in selection order as (ordered decayed score, roi) keys: det_finalize reads them exactly like the hard NMS's kept keys
__global__ __launch_bounds__(64) void det_soft_nms_kernel(DetParams p, float sigma, float Nt, float threshold, int method) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int seg = blockIdx.y * (p.n_cls - 1) + blockIdx.x, lane = threadIdx.x;
  const int n = p.cand_count[seg];
  if (n == 0) { if (lane == 0) p.keep_count[seg] = 0; return; }
  const SoftNmsLds a = soft_nms_lds_arrays(smem, n);
  const float4* qb = reinterpret_cast<const float4*>(p.q_boxes) + (size_t)seg * p.R;
  const float* qs = p.q_scores + (size_t)seg * p.R;
  const int32_t* ql = p.q_roi + (size_t)seg * p.R;
  for (int k = lane; k < n; k += 64) {
    const int r = ql[k];
    const float4 v = qb[r];
    a.X1[k] = v.x; a.Y1[k] = v.y; a.X2[k] = v.z; a.Y2[k] = v.w; a.S[k] = qs[r]; a.I[k] = r; a.dead[k] = 0;
  }
  __builtin_amdgcn_wave_barrier();
  __syncthreads();
  const int N = soft_nms_walk(a.X1, a.Y1, a.X2, a.Y2, a.S, a.I, a.dead, n, sigma, Nt, threshold, method, lane);
  uint64_t* K = p.kept_key + (size_t)seg * p.R;
  for (int k = lane; k < N; k += 64) K[k] = make_desc_key(a.S[k], (uint32_t)a.I[k]);
  if (lane == 0) p.keep_count[seg] = N;
}

// ---- vote scoring of the kept rows (box_voting(nms_dets, dets_j, thresh, scoring_method), result_utils.py:145-151, scoring other than
// 'ID'): the scorings rewrite the score column and the limit (:154-163) ranks the VOTED scores, so every kept row of every segment is
// scored here, BEFORE det_finalize.  One workgroup per (class, image) segment stages the segment's candidates (dets_j: roi ascending
// from the bitmap, undecayed scores) once in LDS (20 B each: <= 80 KB at R = 4096); its waves take the kept entries in turn (Soft-NMS:
// selection order, the pre-vote box) and form the voter set as ballot words, then the score (box_vote.h: vote_score, the
// single-segment drop-in's body).  The voted score replaces the score half of the kept key (det_finalize's limit and the Soft-NMS
// emit read it) and goes to v_scores[seg, roi] (the hard-NMS emit reads it there instead of q_scores).  The boxes are voted after
// the limit by det_vote, as with 'ID' (the box vote does not depend on the scores).
constexpr int kVsThreads = 256;
struct VoteScoreParams {
  const int32_t* n_rois;      // [B] or NULL
  const uint64_t* cand_bits;  // [S, 64]
  const float* q_boxes;       // [S, R, 4]
  const float* q_scores;      // [S, R]
  const int32_t* keep_count;  // [S]
  uint64_t* kept_key;         // [S, R]
  float* v_scores;            // [S, R]
  int R, n_cls, method;
  float thresh, beta;
};

__global__ __launch_bounds__(kVsThreads) void det_vote_score_kernel(VoteScoreParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  __shared__ uint64_t cbits_s[kCandWords];
  __shared__ int wpre_s[kCandWords];
  __shared__ VoteScratch vs_s[kVsThreads / 64];
  const int seg = blockIdx.y * (p.n_cls - 1) + blockIdx.x;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nk = p.keep_count[seg];
  if (nk == 0) return;
  const int nr = p.n_rois ? min(p.n_rois[blockIdx.y], p.R) : p.R;
  const int nw = (nr + 63) >> 6;
  float4* cb = reinterpret_cast<float4*>(smem);                     // [R] candidate boxes, dets_j order
  float* cs = reinterpret_cast<float*>(cb + p.R);                    // [R] their scores
  if (wv == 0) {                                                     // the bitmap and the popcount prefix of its words
    const uint64_t w = lane < nw ? p.cand_bits[(size_t)seg * kCandWords + lane] : 0ull;
    const int pc = __builtin_popcountll(w);
    int incl = pc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) { const int o = __shfl_up(incl, off, 64); if (lane >= off) incl += o; }
    cbits_s[lane] = w;
    wpre_s[lane] = incl - pc;
  }
  __syncthreads();
  const float4* qb = reinterpret_cast<const float4*>(p.q_boxes) + (size_t)seg * p.R;
  const float* qs = p.q_scores + (size_t)seg * p.R;
  for (int r = tid; r < nr; r += kVsThreads) {
    const uint64_t w = cbits_s[r >> 6];
    if ((w >> (r & 63)) & 1ull) {
      const int k = wpre_s[r >> 6] + lanes_below(w, r & 63);
      cb[k] = qb[r];
      cs[k] = qs[r];
    }
  }
  __syncthreads();
  const int n = wpre_s[63] + __builtin_popcountll(cbits_s[63]);      // candidates of the segment
  VoteScratch& vs = vs_s[wv];
  uint64_t* K = p.kept_key + (size_t)seg * p.R;
  for (int e = wv; e < nk; e += kVsThreads / 64) {
    const uint64_t key = K[e];
    const uint32_t r = desc_key_index(key);
    const float4 B = qb[r];
    const int m = vote_words(B, n, p.thresh, [](int) { return true; }, [&](int k) { return cb[k]; }, vs, lane);
    float sc = desc_key_score(key);                                    // no voter: the score stays
    if (m > 0)
      sc = vote_score(p.method, p.beta, vs, (n + 63) >> 6, m, [&](int k) { return cs[k]; },
                      [&](int k) { return iou_bbox(B, cb[k]); }, lane);
    if (lane == 0) {
      K[e] = make_desc_key(sc, r);
      p.v_scores[(size_t)seg * p.R + r] = sc;
    }
  }
}

constexpr int kFinThreads = 1024;
constexpr int kFinMaxCls = 256;

struct FinParams {
  const uint64_t* kept_key;   // [S, R] sort keys of the kept boxes (det_candidates' NMS): ~ordered score << 32 | candidate index q
  const int32_t* keep_count;  // [S]
  const float* q_boxes;       // [S, R, 4]
  const float* q_scores;      // [S, R]  the emitted score of a hard-NMS row (the voted scores with a vote scoring: v_scores)
  const float* scale;         // [B]
  int R, n_cls, max_det, max_out;
  float* dets;                // [B, max_out, 6]
  int32_t* det_roi;           // [B, max_out]
  float* det_rois_scaled;     // [B, max_out, 4]  boxes * scaling_factor (eval_mask_FPN.ipynb:249), may be NULL
  int32_t* det_count;         // [B]
  FpnMapOut fm;               // fm.on: also emit the FPN level mapping of the detection rows (the mask branch's rois), fpn_map.h
  int soft;                   // kept_key in selection order with DECAYED scores (det_soft_nms): rows of a class in that order
};

// off[c] = sum of cnt(c') for c' < c, c = 0 .. nseg (off[nseg] = total); one wavefront, nseg <= 256.
template <typename F> __device__ __forceinline__ void fin_prefix(int* off, F cnt, int nseg, int lane) {
  int v[4], t = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) { v[k] = cnt(lane * 4 + k); t += v[k]; }
  int incl = t;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o, 64); if (lane >= o) incl += u; }
  int e = incl - t;
#pragma unroll
  for (int k = 0; k < 4; k++) { const int c = lane * 4 + k; if (c <= nseg) off[c] = e; e += v[k]; }
  if (lane == 63 && nseg >= 256) off[nseg] = e;
}

// kept entries staged in LDS (ordered score + candidate id, 8 bytes each): dynamic, sized by the launcher for the worst case the
// arguments allow up to kFinStageMax (112 KB); more -> every pass re-fetches from global
constexpr int kFinStageMax = 14336;     // 112 KB dynamic + ~37 KB static

constexpr int kFinSurvMax = 1024;    // survivors of the per-image limit the fast output path ranks by scanning (usual: ~100)

__global__ __launch_bounds__(kFinThreads) void det_finalize_kernel(FinParams p, int stage_cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fin_smem[];
  uint32_t* st_key = reinterpret_cast<uint32_t*>(fin_smem);             // [stage_cap] ordered score of kept entry f
  uint32_t* st_cq = st_key + stage_cap;                                   // [stage_cap] (class c << 12) | candidate index q of kept entry f
  // one histogram per radix pass (11 + 11 + 10 bits), cleared once under the first global round trip: a pass is its atomics, one
  // barrier and the digit selection -- not clear / barrier / atomics / barrier / select / barrier on ONE array (round 6: 15 -> 8 barriers)
  __shared__ __attribute__((aligned(16))) uint32_t h0[2048], h1[2048], h2[1024];
  __shared__ uint32_t sh[2];
  __shared__ int kcnt[kFinMaxCls];
  __shared__ int koff[kFinMaxCls + 1];
  __shared__ int ccnt[kFinMaxCls];
  __shared__ int coff[kFinMaxCls + 1];
  __shared__ uint64_t bitmap[kFinThreads / 64][64];  // per wave: up to 4096 candidates per class
  __shared__ __attribute__((aligned(16))) uint32_t surv[kFinSurvMax + 4];
  __shared__ int nsurv;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  constexpr int NWV = kFinThreads / 64, kClsPerWave = kFinMaxCls / NWV;
  const int nseg = p.n_cls - 1;
  const int seg0 = b * nseg;
  // Round 6: ONE global round trip in front of the LDS phases instead of three dependent ones (counts -> prefix -> binary search ->
  // keys: 6 us of this kernel's 20).  Wave w owns classes w, w + 16, ...: it requests the class's kept count AND, speculatively, the
  // first 64 kept keys of the class (the array is [S, R]: the addresses are valid whatever the count is; a class keeps a few dozen
  // boxes) in the same breath; entries past 64 are fetched behind the prefix, the rare case.
  int cnt_r[kClsPerWave];
  uint64_t key_r[kClsPerWave];
#pragma unroll
  for (int k = 0; k < kClsPerWave; k++) {
    const int c = wv + k * NWV;
    cnt_r[k] = 0; key_r[k] = 0;
    if (c < nseg) {
      cnt_r[k] = p.keep_count[seg0 + c];
      if (lane < p.R) key_r[k] = p.kept_key[(size_t)(seg0 + c) * p.R + lane];
    }
  }
  if (tid == 0) nsurv = 0;
  for (int i = tid; i < 2048; i += kFinThreads) { h0[i] = 0; h1[i] = 0; if (i < 1024) h2[i] = 0; }
#pragma unroll
  for (int k = 0; k < kClsPerWave; k++) { const int c = wv + k * NWV; if (c < kFinMaxCls && lane == 0) kcnt[c] = cnt_r[k]; }
  __syncthreads();
  // exclusive prefix of the per-class kept counts: wavefront 0, four classes per lane (nseg <= kFinMaxCls = 256), shuffle scan
  if (wv == 0) fin_prefix(koff, [&](int c) { return c < nseg ? kcnt[c] : 0; }, nseg, lane);
  __syncthreads();
  const int total = koff[nseg];
  const bool staged = total <= stage_cap;
  // kept entry e of class c of this image -> (ordered score, candidate index q)
  auto fetch = [&](int c, int e, uint32_t& o, int& q) {
    const uint64_t key = p.kept_key[(size_t)(seg0 + c) * p.R + e];
    q = (int)desc_key_index(key);
    o = ~(uint32_t)(key >> 32);                             // == float_to_ordered(q_scores[q]) (block_sort.h: make_desc_key)
  };
  auto class_of = [&](int f) { int lo = 0, hi = nseg; while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (koff[mid] <= f) lo = mid; else hi = mid; } return lo; };
  if (staged) {   // every later phase runs from LDS
#pragma unroll
    for (int k = 0; k < kClsPerWave; k++) {
      const int c = wv + k * NWV;
      if (c >= nseg) continue;
      const int n_c = cnt_r[k], base = koff[c];
      if (lane < n_c) {
        const uint32_t o = ~(uint32_t)(key_r[k] >> 32);
        st_key[base + lane] = o; st_cq[base + lane] = ((uint32_t)c << 12) | (p.soft ? (uint32_t)lane : desc_key_index(key_r[k]));
        atomicAdd(&h0[o >> 21], 1u);                          // the first pass of the limit's radix select, while the entry is in hand
      }
      for (int e = 64 + lane; e < n_c; e += 64) {             // a crowded class: the rest of its entries, one more round trip
        uint32_t o; int q;
        fetch(c, e, o, q);
        st_key[base + e] = o; st_cq[base + e] = ((uint32_t)c << 12) | (uint32_t)(p.soft ? e : q);
        atomicAdd(&h0[o >> 21], 1u);
      }
    }
    __syncthreads();
  }
  // ---- per-image limit (result_utils.py:154-163): threshold = max_det-th largest kept score ----
  uint32_t T = 0;  // ordered-key threshold; 0 == keep everything
  if (p.max_det > 0 && total > p.max_det) {
    uint32_t prefix = 0, krem = (uint32_t)p.max_det;
    for (int pass = 0; pass < 3; pass++) {
      uint32_t* h = pass == 0 ? h0 : pass == 1 ? h1 : h2;
      if (pass > 0 || !staged) {
        for (int f = tid; f < total; f += kFinThreads) {
          uint32_t o;
          if (staged) o = st_key[f];
          else { const int c = class_of(f); int q; fetch(c, f - koff[c], o, q); }
          if (pass == 0) atomicAdd(&h[o >> 21], 1u);
          else if (pass == 1) { if ((o >> 21) == prefix) atomicAdd(&h[(o >> 10) & 2047u], 1u); }
          else { if ((o >> 10) == prefix) atomicAdd(&h[o & 1023u], 1u); }
        }
        __syncthreads();
      }
      select_digit(h, pass == 2 ? 1024 : 2048, krem, sh);      // ends with a barrier; sh is rewritten behind the next pass's barrier
      prefix = (prefix << (pass == 2 ? 10 : 11)) | sh[0];
      krem = sh[1];
    }
    T = prefix;
  }
  __syncthreads();
  const float sf = p.scale ? p.scale[b] : 1.f;
  float4* sbox_fm = reinterpret_cast<float4*>(&bitmap[0][0]);     // fast path + fm.on: the scaled boxes by output row (max_out <= 512)
  // one detection row (:143 dets_j[keep], :165 vstack).  Soft segments: `e` is the position in the class's kept list (selection
  // order), the roi and the decayed score come from its key; otherwise q is the roi and the score the candidate's own
  auto emit = [&](int slot, int c, int q, bool to_lds, int e = -1) {
    const int seg = seg0 + c;
    float score;
    if (e >= 0) {
      const uint64_t key = p.kept_key[(size_t)seg * p.R + e];
      q = (int)desc_key_index(key);
      score = desc_key_score(key);
    } else {
      score = p.q_scores[(size_t)seg * p.R + q];
    }
    const float4 bx = reinterpret_cast<const float4*>(p.q_boxes)[(size_t)seg * p.R + q];
    if (to_lds) sbox_fm[slot] = make_float4(bx.x * sf, bx.y * sf, bx.z * sf, bx.w * sf);
    float* o = p.dets + ((size_t)b * p.max_out + slot) * 6;
    o[0] = bx.x; o[1] = bx.y; o[2] = bx.z; o[3] = bx.w;
    o[4] = score;
    o[5] = (float)(c + 1);
    p.det_roi[(size_t)b * p.max_out + slot] = q;                               // the candidate index IS the roi index (round 6)
    if (p.det_rois_scaled)
      reinterpret_cast<float4*>(p.det_rois_scaled)[(size_t)b * p.max_out + slot] = make_float4(bx.x * sf, bx.y * sf, bx.z * sf, bx.w * sf);
  };
  // ---- fast output path (round 6): the survivors of the limit are ~100 rows.  They are appended to an LDS list in any order; the
  // output row of a survivor is the number of survivors with a smaller (class, candidate) code -- class-major, candidate (= roi)
  // ascending, exactly the reference's vstack order -- found by scanning the list with broadcast 16-byte reads; then ONE round of
  // gathers.  (The per-class bitmap walk below paid five rounds of dependent loads per wave: 7 us.)
  bool fast_done = false;
  if (staged) {
    for (int f = tid; f < total; f += kFinThreads) {
      if (st_key[f] >= T) {                                                    // :161 `>=`
        const int i = atomicAdd(&nsurv, 1);
        if (i < kFinSurvMax) surv[i] = st_cq[f];
      }
    }
    __syncthreads();
    const int ns = nsurv;
    if (ns <= kFinSurvMax) {
      fast_done = true;
      if (tid < 4) surv[ns + tid] = 0xffffffffu;                              // pad to a multiple of four: never smaller
      if (tid == 0) p.det_count[b] = ns;
      __syncthreads();
      const int n4 = (ns + 3) >> 2;
      for (int i = tid; i < ns; i += kFinThreads) {
        const uint32_t me = surv[i];
        int rank = 0;
        for (int j = 0; j < n4; j++) {
          const uint4 v = reinterpret_cast<const uint4*>(surv)[j];
          rank += (v.x < me ? 1 : 0) + (v.y < me ? 1 : 0) + (v.z < me ? 1 : 0) + (v.w < me ? 1 : 0);
        }
        if (rank < p.max_out) {
          if (p.soft) emit(rank, (int)(me >> 12), 0, p.fm.on != 0, (int)(me & 4095u));
          else emit(rank, (int)(me >> 12), (int)(me & 4095u), p.fm.on != 0);
        }
      }
    }
  }
  if (fast_done) {
    if (p.fm.on) {       // the mask branch's level mapping of these rows, here instead of in a launch of its own (round 6)
      __syncthreads();
      fpn_map_rows(p.fm, b, p.max_out, min(nsurv, p.max_out), [&](int t) { return sbox_fm[t]; }, h0, h1);
    }
    return;
  }
  // ---- general path: more survivors than the list holds (max_det <= 0 on a large head, mass ties) or entries not staged ----
  // pass A: survivors per class
  for (int c = wv; c < nseg; c += kFinThreads / 64) {
    const int nk = koff[c + 1] - koff[c];
    int cnt = 0;
    for (int e0 = 0; e0 < nk; e0 += 64) {
      const int e = e0 + lane;
      bool ok = false;
      if (e < nk) {
        uint32_t o; int q;
        if (staged) o = st_key[koff[c] + e]; else fetch(c, e, o, q);
        ok = o >= T;                                                         // :161 `>=`
      }
      cnt += __builtin_popcountll(__ballot(ok));
    }
    if (lane == 0) ccnt[c] = cnt;
  }
  __syncthreads();
  if (wv == 0) {
    fin_prefix(coff, [&](int c) { return c < nseg ? ccnt[c] : 0; }, nseg, lane);
    if (lane == 0) p.det_count[b] = coff[nseg];
  }
  __syncthreads();
  // ---- pass B: class-major, candidate(roi)-ascending output (:143 dets_j[keep], :165 vstack) ----
  for (int c = wv; c < nseg; c += kFinThreads / 64) {
    const int nk = koff[c + 1] - koff[c];
    if (ccnt[c] == 0) continue;
    if (p.soft) {            // Soft-NMS: the class's kept list in selection order, filtered by `>= T` (ballot + popcount prefix)
      int slot0 = coff[c];
      for (int e0 = 0; e0 < nk; e0 += 64) {
        const int e = e0 + lane;
        bool ok = false;
        if (e < nk) {
          uint32_t o;
          if (staged) o = st_key[koff[c] + e]; else { int q; fetch(c, e, o, q); }
          ok = o >= T;                                                       // :161 `>=`
        }
        const uint64_t bal = __ballot(ok);
        const int slot = slot0 + lanes_below(bal, lane);
        if (ok && slot < p.max_out) emit(slot, c, 0, false, e);
        slot0 += __builtin_popcountll(bal);
      }
      continue;
    }
    uint64_t* bm = bitmap[wv];
    bm[lane] = 0;
    __builtin_amdgcn_wave_barrier();
    for (int e0 = 0; e0 < nk; e0 += 64) {
      const int e = e0 + lane;
      if (e < nk) {
        uint32_t o; int q;
        if (staged) { o = st_key[koff[c] + e]; q = (int)(st_cq[koff[c] + e] & 4095u); } else fetch(c, e, o, q);
        if (o >= T && q < 4096) atomicOr(reinterpret_cast<unsigned long long*>(&bm[q >> 6]), 1ull << (q & 63));
      }
    }
    __builtin_amdgcn_wave_barrier();
    uint64_t w = bm[lane];
    // exclusive prefix of popcounts across lanes
    int pc = __builtin_popcountll(w), incl = pc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    int slot = coff[c] + incl - pc;
    while (w) {
      const int bit = __builtin_ctzll(w);
      w &= w - 1;
      const int q = lane * 64 + bit;
      if (slot < p.max_out) emit(slot, c, q, false);
      slot++;
    }
    __builtin_amdgcn_wave_barrier();
  }
  if (p.fm.on) {         // general path: the rows come back from global memory (written by this workgroup: fence + barrier, uncached loads)
    __threadfence();
    __syncthreads();
    const float* ds = p.det_rois_scaled + (size_t)b * p.max_out * 4;
    auto ld = [&](const float* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
    fpn_map_rows(p.fm, b, p.max_out, min(coff[nseg], p.max_out),
                 [&](int t) { return make_float4(ld(ds + 4 * t), ld(ds + 4 * t + 1), ld(ds + 4 * t + 2), ld(ds + 4 * t + 3)); }, h0, h1);
  }
}

// ---- bbox voting of the emitted rows (box_utils.box_voting(nms_dets, dets_j, thresh, 'ID'), result_utils.py:145-151): one wavefront per
// output row; the voters are the row's segment's candidates in dets_j order (roi ascending: the bitmap), weighted by their undecayed
// scores.  Rewrites dets[:, :4] and det_rois_scaled (the emit's arithmetic); the score, class and det_roi stay.
struct VoteParams {
  const int32_t* n_rois;      // [B] or NULL
  const uint64_t* cand_bits;  // [S, 64]
  const float* q_boxes;       // [S, R, 4]
  const float* q_scores;      // [S, R]
  const float* scale;         // [B] or NULL (1)
  const int32_t* det_count;   // [B]
  float* dets;                // [B, max_out, 6]
  float* det_rois_scaled;     // [B, max_out, 4] or NULL
  int R, n_cls, max_out;
  float thresh;
};

__global__ __launch_bounds__(64) void det_vote_kernel(VoteParams p) {
  __shared__ int vl[4096];
  const int row = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  if (row >= min(p.det_count[b], p.max_out)) return;
  float* d = p.dets + ((size_t)b * p.max_out + row) * 6;
  const float4 B = make_float4(d[0], d[1], d[2], d[3]);
  const int seg = b * (p.n_cls - 1) + ((int)d[5] - 1);
  const int nr = p.n_rois ? min(p.n_rois[b], p.R) : p.R;
  const uint64_t* bits = p.cand_bits + (size_t)seg * kCandWords;
  const float4* qb = reinterpret_cast<const float4*>(p.q_boxes) + (size_t)seg * p.R;
  const float* qs = p.q_scores + (size_t)seg * p.R;
  int m = 0;
  const float v = box_vote_one(
      B, lane < 4 ? d[lane] : 0.f, nr, p.thresh, [&](int r) { return ((bits[r >> 6] >> (r & 63)) & 1ull) != 0ull; },
      [&](int r) { return qb[r]; },
      [&](int r, int c) { return reinterpret_cast<const float*>(p.q_boxes)[((size_t)seg * p.R + r) * 4 + c]; },
      [&](int r) { return qs[r]; }, vl, lane, &m);
  if (lane < 4) {
    d[lane] = v;
    if (p.det_rois_scaled) p.det_rois_scaled[((size_t)b * p.max_out + row) * 4 + lane] = v * (p.scale ? p.scale[b] : 1.f);
  }
}

// the FPN level mapping of the (voted) rows, when the vote took it out of det_finalize: what fm.on does there, from det_rois_scaled
constexpr int kMapThreads = kFpnMapMaxRows + 64;     // fpn_map_rows: blockDim >= D + 4 pads the scan
__global__ __launch_bounds__(kMapThreads) void det_fpn_map_kernel(FpnMapOut fm, const float* det_rois_scaled, const int32_t* det_count,
                                                                  int max_out) {
  __shared__ __attribute__((aligned(16))) uint32_t code_s[kFpnMapMaxRows + 4], key_s[kFpnMapMaxRows + 4];
  const int b = blockIdx.x;
  const float4* ds = reinterpret_cast<const float4*>(det_rois_scaled) + (size_t)b * max_out;
  fpn_map_rows(fm, b, max_out, min(det_count[b], max_out), [&](int t) { return ds[t]; }, code_s, key_s);
}

struct DetPlan { size_t sorted_boxes, q_boxes, q_scores, q_roi, cand_count, kept_key, keep_count, sm_stats, cand_bits, v_scores, total; };
static DetPlan det_plan(int batch, int R, int n_cls, bool with_bits, bool with_vscores) {
  DetPlan d;
  const size_t S = (size_t)batch * (n_cls - 1);
  Carve w{256};
  d.sorted_boxes = w.take(S * R * 4 * sizeof(float));
  d.q_boxes = w.take(S * R * 4 * sizeof(float));
  d.q_scores = w.take(S * R * sizeof(float));
  d.q_roi = w.take(S * R * sizeof(int32_t));           // the Soft-NMS path's dets_j order
  d.cand_count = w.take(S * sizeof(int32_t));
  d.kept_key = w.take(S * R * sizeof(uint64_t));
  d.keep_count = w.take(S * sizeof(int32_t));
  d.sm_stats = w.take((size_t)batch * R * 2 * sizeof(double));
  d.cand_bits = w.take(with_bits ? S * kCandWords * sizeof(uint64_t) : 0);
  d.v_scores = w.take(with_vscores ? S * R * sizeof(float) : 0);
  d.total = w.end;
  return d;
}

// What the options make of a call, decided once for the size entries and the launcher.
struct DetMode {
  int soft;       // Soft-NMS walk method (0 hard, 1 linear, 2 gaussian) or -1: the in-workgroup hard NMS
  bool vote;      // bbox voting of the emitted rows
  int method;     // the vote's scoring (kVoteID: the score stays)
  bool scored() const { return method != kVoteID; }
  bool bits() const { return soft >= 0 || vote; }        // the candidate bitmap is kept
};

// dtc_det_options / dtc_vote_scoring validation (host only) -> DTC_OK / DTC_EINVAL
static int det_mode(const dtc_det_options* opt, const dtc_vote_scoring* scoring, DetMode* m) {
  m->soft = -1; m->vote = false; m->method = kVoteID;
  if (opt) {
    if (opt->nms_method < 0 || opt->nms_method > 3) return DTC_EINVAL;
    if (opt->nms_method == 2 && !(opt->soft_sigma > 0.f)) return DTC_EINVAL;
    if (opt->bbox_vote != 0 && opt->bbox_vote != 1) return DTC_EINVAL;
    if (opt->bbox_vote && !(opt->bbox_vote_thresh > 0.f && opt->bbox_vote_thresh <= 1.f)) return DTC_EINVAL;
    m->soft = opt->nms_method == 0 ? -1 : opt->nms_method == 3 ? 0 : opt->nms_method;
    m->vote = opt->bbox_vote != 0;
  }
  if (scoring) {
    if (scoring->method < kVoteID || scoring->method > kVoteQuasiSum) return DTC_EINVAL;
    if (!(scoring->beta > 0.f) || !std::isfinite(scoring->beta)) return DTC_EINVAL;
    if (scoring->method != kVoteID && !(opt && opt->bbox_vote == 1)) return DTC_EINVAL;
    m->method = scoring->method;
  }
  return DTC_OK;
}

// The options checked and the workspace laid out, once per call: DTC_EINVAL for bad options, else the mode and the plan (total 0
// for a shape that has no layout).  The three *_workspace_bytes entries answer with the total, the launcher carves by the offsets.
static int det_prepare(int batch, int max_rois, int n_cls, const dtc_det_options* opt, const dtc_vote_scoring* scoring, DetMode* mode,
                       DetPlan* plan) {
  *plan = DetPlan{};
  if (det_mode(opt, scoring, mode) != DTC_OK) return DTC_EINVAL;
  if (batch >= 1 && max_rois >= 1 && n_cls >= 2) *plan = det_plan(batch, max_rois, n_cls, mode->bits(), mode->scored());
  return DTC_OK;
}
static size_t det_workspace_bytes(int batch, int max_rois, int n_cls, const dtc_det_options* opt, const dtc_vote_scoring* scoring) {
  DetMode mode;
  DetPlan pl;
  return det_prepare(batch, max_rois, n_cls, opt, scoring, &mode, &pl) == DTC_OK ? pl.total : 0;
}

// One call of the batched detection post-processing, whichever entry it came through; the entries fill it by name.
struct DetCall {
  // inputs: rois5 [B, R, 5], n_rois [B] or NULL, cls_score [B, R, n_cls] (probabilities, or logits), bbox_pred [B, R, 4 n_cls];
  // decoded_boxes [B, R, 4 n_cls] stands in for rois5 / bbox_pred / scaling_factor [B] / im_size [B, 2]
  const float *rois5 = nullptr, *cls_score = nullptr, *bbox_pred = nullptr, *decoded_boxes = nullptr, *scaling_factor = nullptr,
              *im_size = nullptr;
  const int32_t* n_rois = nullptr;
  bool scores_are_logits = false;
  int batch = 0, max_rois = 0, n_cls = 0;                                                       // shape
  float wx = 1.f, wy = 1.f, ww = 1.f, wh = 1.f, score_thresh = 0.f, nms_thresh = 0.f;           // thresholds
  int max_det = 0;
  const dtc_det_options* opt = nullptr;                                                         // options, scoring
  const dtc_vote_scoring* scoring = nullptr;
  void* workspace = nullptr;
  size_t workspace_bytes = 0;
  float *dets = nullptr, *det_rois_scaled = nullptr;                                            // outputs
  int32_t *det_roi = nullptr, *det_count = nullptr;
  int max_out = 0;
  const dtc_fpn_map_out* fpn = nullptr;
  dtc_stream_t stream = nullptr;
};

static int postprocess_detections(const DetCall& c) {
  const int batch = c.batch, max_rois = c.max_rois, n_cls = c.n_cls, max_out = c.max_out;
  const dtc_fpn_map_out* fpn = c.fpn;
  DetMode mode;
  DetPlan pl;
  if (det_prepare(batch, max_rois, n_cls, c.opt, c.scoring, &mode, &pl) != DTC_OK) return DTC_EINVAL;
  if (batch < 0 || max_rois < 1 || n_cls < 2 || n_cls - 1 > kFinMaxCls || max_out < 1) return DTC_EINVAL;
  if (fpn) {
    if (!c.det_rois_scaled || !fpn->rois5 || !fpn->roi_levels || !fpn->n_out || !fpn->rois_by_level || !fpn->level_counts ||
        !fpn->idx_restore || fpn->k_max < fpn->k_min || fpn->k_max - fpn->k_min + 1 > 8)
      return DTC_EINVAL;
    if (max_out > kFpnMapMaxRows) return DTC_EUNSUPPORTED;      // longer lists: dtc_fpn_collect_distribute on det_rois_scaled
  }
  if (batch == 0) return DTC_OK;
  if (max_rois > 4096) return DTC_EUNSUPPORTED;
  if (!c.cls_score || !c.workspace || !c.dets || !c.det_roi || !c.det_count) return DTC_EINVAL;
  if (!c.decoded_boxes && (!c.rois5 || !c.bbox_pred || !c.scaling_factor || !c.im_size)) return DTC_EINVAL;
  if (c.decoded_boxes && c.det_rois_scaled) return DTC_EINVAL;
  if (c.workspace_bytes < pl.total) return DTC_EWORKSPACE;
  const bool soft = mode.soft >= 0, vote = mode.vote, scored = mode.scored();
  unsigned char* w = reinterpret_cast<unsigned char*>(c.workspace);
  hipStream_t s = reinterpret_cast<hipStream_t>(c.stream);
  DetParams p;
  p.rois5 = c.rois5; p.n_rois = c.n_rois; p.cls_score = c.cls_score; p.bbox_pred = c.bbox_pred; p.scale = c.scaling_factor;
  p.decoded = c.decoded_boxes;
  p.sm_stats = nullptr;
  if (c.scores_are_logits) {
    double* st = reinterpret_cast<double*>(w + pl.sm_stats);
    const int rows = batch * max_rois;
    hipLaunchKernelGGL(det_softmax_stats_kernel, dim3((rows + kDetThreads / 64 - 1) / (kDetThreads / 64)), dim3(kDetThreads), 0, s,
                       c.cls_score, rows, n_cls, st);
    DTC_CHECK_LAUNCH();
    p.sm_stats = st;
  }
  p.im_size = c.im_size; p.R = max_rois; p.n_cls = n_cls; p.wx = c.wx; p.wy = c.wy; p.ww = c.ww; p.wh = c.wh;
  p.score_thresh = c.score_thresh;
  p.sorted_boxes = reinterpret_cast<float*>(w + pl.sorted_boxes);
  p.q_boxes = reinterpret_cast<float*>(w + pl.q_boxes); p.q_scores = reinterpret_cast<float*>(w + pl.q_scores);
  p.q_roi = reinterpret_cast<int32_t*>(w + pl.q_roi); p.cand_count = reinterpret_cast<int32_t*>(w + pl.cand_count);
  // dynamic LDS: sort keys [next_pow2(R)] x 8 B, then up to kNmsLdsCap boxes in score order (16 B) and one removed-bit per candidate
  const int np2 = next_pow2(max_rois);
  const size_t smem = (size_t)np2 * sizeof(uint64_t) + (size_t)kNmsLdsCap * sizeof(float4) + (size_t)((max_rois + 63) / 64) * sizeof(uint64_t);
  if (smem > 48 * 1024 && raise_lds_once<det_candidates_kernel>(152 * 1024) != DTC_OK) return DTC_ELAUNCH;
  p.kept_key = reinterpret_cast<uint64_t*>(w + pl.kept_key);
  p.keep_count = reinterpret_cast<int32_t*>(w + pl.keep_count);
  p.nms_thresh = c.nms_thresh; p.np2_max = np2;
  p.soft = soft ? 1 : 0;
  p.cand_bits = mode.bits() ? reinterpret_cast<uint64_t*>(w + pl.cand_bits) : nullptr;
  hipLaunchKernelGGL(det_candidates_kernel, dim3(n_cls - 1, batch), dim3(kDetThreads), smem, s, p);
  DTC_CHECK_LAUNCH();
  if (soft) {
    if (raise_lds_once<det_soft_nms_kernel>() != DTC_OK) return DTC_ELAUNCH;
    hipLaunchKernelGGL(det_soft_nms_kernel, dim3(n_cls - 1, batch), dim3(64), soft_nms_lds_bytes(max_rois), s, p, c.opt->soft_sigma,
                       c.nms_thresh, c.opt->soft_score_thresh, mode.soft);
    DTC_CHECK_LAUNCH();
  }
  float* v_scores = scored ? reinterpret_cast<float*>(w + pl.v_scores) : nullptr;
  if (scored) {
    VoteScoreParams vp;
    vp.n_rois = c.n_rois; vp.cand_bits = p.cand_bits; vp.q_boxes = p.q_boxes; vp.q_scores = p.q_scores; vp.keep_count = p.keep_count;
    vp.kept_key = p.kept_key; vp.v_scores = v_scores; vp.R = max_rois; vp.n_cls = n_cls; vp.method = mode.method;
    vp.thresh = c.opt->bbox_vote_thresh; vp.beta = c.scoring->beta;
    const size_t vsm = (size_t)max_rois * (sizeof(float4) + sizeof(float));
    if (vsm > 48 * 1024 && raise_lds_once<det_vote_score_kernel>(4096 * (sizeof(float4) + sizeof(float))) != DTC_OK) return DTC_ELAUNCH;
    hipLaunchKernelGGL(det_vote_score_kernel, dim3(n_cls - 1, batch), dim3(kVsThreads), vsm, s, vp);
    DTC_CHECK_LAUNCH();
  }
  FinParams f;
  f.kept_key = p.kept_key; f.keep_count = p.keep_count; f.q_boxes = p.q_boxes; f.q_scores = scored ? v_scores : p.q_scores;
  f.scale = c.scaling_factor; f.R = max_rois; f.n_cls = n_cls; f.max_det = c.max_det; f.max_out = max_out;
  f.dets = c.dets; f.det_roi = c.det_roi; f.det_rois_scaled = c.det_rois_scaled; f.det_count = c.det_count;
  f.fm.on = fpn && !vote ? 1 : 0;            // with voting the mapping follows the vote (det_fpn_map)
  f.soft = soft ? 1 : 0;
  if (fpn) {
    f.fm.rois5 = fpn->rois5; f.fm.roi_levels = fpn->roi_levels; f.fm.n_out = fpn->n_out; f.fm.rois_by_level = fpn->rois_by_level;
    f.fm.level_counts = fpn->level_counts; f.fm.idx_restore = fpn->idx_restore; f.fm.roi_order = fpn->roi_order;
    f.fm.roi_desc = fpn->roi_order ? fpn->roi_desc : nullptr; f.fm.k_min = fpn->k_min; f.fm.k_max = fpn->k_max;
    f.fm.band_log2 = kFpnBandLog2;
  }
  long long cap = (long long)max_rois * (n_cls - 1);            // every candidate of every class kept
  if (cap > kFinStageMax) cap = kFinStageMax;
  const int stage_cap = (int)((cap + 3) & ~3ll);
  const size_t fsm = (size_t)stage_cap * 8;
  if (fsm > 16 * 1024 && raise_lds_once<det_finalize_kernel>(116 * 1024) != DTC_OK) return DTC_ELAUNCH;      // + ~37 KB static: under the 160 KB of a CU
  hipLaunchKernelGGL(det_finalize_kernel, dim3(batch), dim3(kFinThreads), fsm, s, f, stage_cap);
  DTC_CHECK_LAUNCH();
  if (vote) {
    VoteParams v;
    v.n_rois = c.n_rois; v.cand_bits = p.cand_bits; v.q_boxes = p.q_boxes; v.q_scores = p.q_scores;
    v.scale = c.decoded_boxes ? nullptr : c.scaling_factor; v.det_count = c.det_count; v.dets = c.dets; v.det_rois_scaled = c.det_rois_scaled;
    v.R = max_rois; v.n_cls = n_cls; v.max_out = max_out; v.thresh = c.opt->bbox_vote_thresh;
    hipLaunchKernelGGL(det_vote_kernel, dim3(max_out, batch), dim3(64), 0, s, v);
    DTC_CHECK_LAUNCH();
    if (fpn) {
      FpnMapOut fm = f.fm;
      fm.on = 1;
      hipLaunchKernelGGL(det_fpn_map_kernel, dim3(batch), dim3(kMapThreads), 0, s, fm, c.det_rois_scaled, c.det_count, max_out);
      DTC_CHECK_LAUNCH();
    }
  }
  return DTC_OK;
}

}  // namespace dtc

DTC_API size_t dtc_postprocess_detections_workspace_bytes(int batch, int max_rois, int n_cls) {
  return dtc::det_workspace_bytes(batch, max_rois, n_cls, nullptr, nullptr);
}

DTC_API size_t dtc_postprocess_detections_ex_workspace_bytes(int batch, int max_rois, int n_cls, const dtc_det_options* opt) {
  return dtc::det_workspace_bytes(batch, max_rois, n_cls, opt, nullptr);
}

DTC_API size_t dtc_postprocess_detections_ex2_workspace_bytes(int batch, int max_rois, int n_cls, const dtc_det_options* opt,
                                                              const dtc_vote_scoring* scoring) {
  return dtc::det_workspace_bytes(batch, max_rois, n_cls, opt, scoring);
}

DTC_API int dtc_postprocess_detections(const float* rois5, const int32_t* n_rois, const float* cls_score,
                                       const float* bbox_pred, const float* scaling_factor, const float* im_size,
                                       int batch, int max_rois, int n_cls, float wx, float wy, float ww, float wh,
                                       float score_thresh, float nms_thresh, int max_det, void* workspace,
                                       size_t workspace_bytes, float* dets, int32_t* det_roi, float* det_rois_scaled,
                                       int32_t* det_count, int max_out, dtc_stream_t stream) {
  dtc::DetCall c;
  c.rois5 = rois5; c.bbox_pred = bbox_pred; c.scaling_factor = scaling_factor; c.im_size = im_size;
  c.wx = wx; c.wy = wy; c.ww = ww; c.wh = wh; c.det_rois_scaled = det_rois_scaled;
  c.n_rois = n_rois; c.batch = batch; c.max_rois = max_rois; c.n_cls = n_cls;
  c.score_thresh = score_thresh; c.nms_thresh = nms_thresh; c.max_det = max_det;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.dets = dets; c.det_roi = det_roi; c.det_count = det_count; c.max_out = max_out; c.stream = stream;
  c.cls_score = cls_score;
  return dtc::postprocess_detections(c);
}

DTC_API int dtc_postprocess_detections_logits(const float* rois5, const int32_t* n_rois, const float* cls_logits,
                                              const float* bbox_pred, const float* scaling_factor, const float* im_size,
                                              int batch, int max_rois, int n_cls, float wx, float wy, float ww, float wh,
                                              float score_thresh, float nms_thresh, int max_det, void* workspace,
                                              size_t workspace_bytes, float* dets, int32_t* det_roi, float* det_rois_scaled,
                                              int32_t* det_count, int max_out, dtc_stream_t stream) {
  dtc::DetCall c;
  c.rois5 = rois5; c.bbox_pred = bbox_pred; c.scaling_factor = scaling_factor; c.im_size = im_size;
  c.wx = wx; c.wy = wy; c.ww = ww; c.wh = wh; c.det_rois_scaled = det_rois_scaled;
  c.n_rois = n_rois; c.batch = batch; c.max_rois = max_rois; c.n_cls = n_cls;
  c.score_thresh = score_thresh; c.nms_thresh = nms_thresh; c.max_det = max_det;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.dets = dets; c.det_roi = det_roi; c.det_count = det_count; c.max_out = max_out; c.stream = stream;
  c.cls_score = cls_logits; c.scores_are_logits = true;
  return dtc::postprocess_detections(c);
}

DTC_API int dtc_postprocess_detections_fpn(const float* rois5, const int32_t* n_rois, const float* cls_score, int scores_are_logits,
                                           const float* bbox_pred, const float* scaling_factor, const float* im_size,
                                           int batch, int max_rois, int n_cls, float wx, float wy, float ww, float wh,
                                           float score_thresh, float nms_thresh, int max_det, void* workspace,
                                           size_t workspace_bytes, float* dets, int32_t* det_roi, float* det_rois_scaled,
                                           int32_t* det_count, int max_out, const dtc_fpn_map_out* fpn, dtc_stream_t stream) {
  if (!fpn) return DTC_EINVAL;
  dtc::DetCall c;
  c.rois5 = rois5; c.bbox_pred = bbox_pred; c.scaling_factor = scaling_factor; c.im_size = im_size;
  c.wx = wx; c.wy = wy; c.ww = ww; c.wh = wh; c.det_rois_scaled = det_rois_scaled;
  c.n_rois = n_rois; c.batch = batch; c.max_rois = max_rois; c.n_cls = n_cls;
  c.score_thresh = score_thresh; c.nms_thresh = nms_thresh; c.max_det = max_det;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.dets = dets; c.det_roi = det_roi; c.det_count = det_count; c.max_out = max_out; c.stream = stream;
  c.cls_score = cls_score; c.scores_are_logits = scores_are_logits != 0; c.fpn = fpn;
  return dtc::postprocess_detections(c);
}

DTC_API int dtc_box_results_nms_limit(const float* scores, const float* boxes, const int32_t* n_rois, int batch, int max_rois,
                                      int n_cls, float score_thresh, float nms_thresh, int max_det, void* workspace,
                                      size_t workspace_bytes, float* dets, int32_t* det_roi, int32_t* det_count, int max_out,
                                      dtc_stream_t stream) {
  if (!boxes) return DTC_EINVAL;
  dtc::DetCall c;                                  // no decode: the weights stay 1, there is no scale and no det_rois_scaled
  c.n_rois = n_rois; c.batch = batch; c.max_rois = max_rois; c.n_cls = n_cls;
  c.score_thresh = score_thresh; c.nms_thresh = nms_thresh; c.max_det = max_det;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.dets = dets; c.det_roi = det_roi; c.det_count = det_count; c.max_out = max_out; c.stream = stream;
  c.cls_score = scores; c.decoded_boxes = boxes;
  return dtc::postprocess_detections(c);
}

DTC_API int dtc_postprocess_detections_ex(const float* rois5, const int32_t* n_rois, const float* cls_score, int scores_are_logits,
                                          const float* bbox_pred, const float* decoded_boxes, const float* scaling_factor,
                                          const float* im_size, int batch, int max_rois, int n_cls, float wx, float wy, float ww,
                                          float wh, float score_thresh, float nms_thresh, int max_det, const dtc_det_options* opt,
                                          void* workspace, size_t workspace_bytes, float* dets, int32_t* det_roi,
                                          float* det_rois_scaled, int32_t* det_count, int max_out, const dtc_fpn_map_out* fpn,
                                          dtc_stream_t stream) {
  if (decoded_boxes && fpn) return DTC_EINVAL;           // the mapping reads det_rois_scaled, which the decoded-boxes form has not
  dtc::DetCall c;
  c.rois5 = rois5; c.bbox_pred = bbox_pred; c.scaling_factor = scaling_factor; c.im_size = im_size;
  c.wx = wx; c.wy = wy; c.ww = ww; c.wh = wh; c.det_rois_scaled = det_rois_scaled;
  c.n_rois = n_rois; c.batch = batch; c.max_rois = max_rois; c.n_cls = n_cls;
  c.score_thresh = score_thresh; c.nms_thresh = nms_thresh; c.max_det = max_det;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.dets = dets; c.det_roi = det_roi; c.det_count = det_count; c.max_out = max_out; c.stream = stream;
  c.cls_score = cls_score; c.scores_are_logits = scores_are_logits != 0; c.decoded_boxes = decoded_boxes; c.opt = opt; c.fpn = fpn;
  return dtc::postprocess_detections(c);
}

DTC_API int dtc_postprocess_detections_ex2(const float* rois5, const int32_t* n_rois, const float* cls_score, int scores_are_logits,
                                           const float* bbox_pred, const float* decoded_boxes, const float* scaling_factor,
                                           const float* im_size, int batch, int max_rois, int n_cls, float wx, float wy, float ww,
                                           float wh, float score_thresh, float nms_thresh, int max_det, const dtc_det_options* opt,
                                           const dtc_vote_scoring* scoring, void* workspace, size_t workspace_bytes, float* dets,
                                           int32_t* det_roi, float* det_rois_scaled, int32_t* det_count, int max_out,
                                           const dtc_fpn_map_out* fpn, dtc_stream_t stream) {
  if (decoded_boxes && fpn) return DTC_EINVAL;
  dtc::DetCall c;
  c.rois5 = rois5; c.bbox_pred = bbox_pred; c.scaling_factor = scaling_factor; c.im_size = im_size;
  c.wx = wx; c.wy = wy; c.ww = ww; c.wh = wh; c.det_rois_scaled = det_rois_scaled;
  c.n_rois = n_rois; c.batch = batch; c.max_rois = max_rois; c.n_cls = n_cls;
  c.score_thresh = score_thresh; c.nms_thresh = nms_thresh; c.max_det = max_det;
  c.workspace = workspace; c.workspace_bytes = workspace_bytes;
  c.dets = dets; c.det_roi = det_roi; c.det_count = det_count; c.max_out = max_out; c.stream = stream;
  c.cls_score = cls_score; c.scores_are_logits = scores_are_logits != 0; c.decoded_boxes = decoded_boxes; c.opt = opt;
  c.scoring = scoring; c.fpn = fpn;
  return dtc::postprocess_detections(c);
}
