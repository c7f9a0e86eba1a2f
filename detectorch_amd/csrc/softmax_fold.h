// The softmax the detection stage folds in (detections.hip has the why), for one row of class logits and one wave: the row's
// (max, sum_j exp(l_j - max)) once, then  prob_j = float(exp(double(l_j) - max) / sum)  where a column is consumed.  Evaluated in
// double and rounded once, the sum taken in a FIXED order (element j goes to slot j % 64 in increasing j, then a 64 -> 1 halving
// tree), so that oracle/oracle.py:softmax_rows gives the same bits.  Used by det_softmax_stats / det_candidates (detections.hip) and
// by the test-time-augmentation merge (aug/aug_merge.hip).
#pragma once
#include "dtc_common.h"

// prob_j of logit l, st = the row's (max, sum) as two doubles.  A macro and not an inline function: through a function the
// compiler scheduled det_candidates' loads differently (same arithmetic, another instruction order), and that kernel's schedule is
// kept as measured.  One text either way.
#define DTC_SOFTMAX_PROB(l, st) ((float)(exp((double)(l) - (st)[0]) / (st)[1]))

namespace dtc {

// all 64 lanes of the wave call this; every lane returns with the row's max in m and the sum in e (lane 0's are the tree's)
__device__ __forceinline__ void softmax_row_stats(const float* l, int n_cls, int lane, float& m, double& e) {
  m = -INFINITY;
  for (int j = lane; j < n_cls; j += 64) m = fmaxf(m, l[j]);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
  e = 0.0;
  for (int j = lane; j < n_cls; j += 64) e += exp((double)l[j] - (double)m);
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) e += __shfl_xor(e, off, 64);       // lane 0: ((s0+s32)+(s16+s48))+... halving tree
}

}  // namespace dtc
