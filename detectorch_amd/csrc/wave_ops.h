// Wave-wide (64-lane) idioms the kernels share: one text per idea instead of a copy per call site.  Every helper is forced inline; it
// is used only where the call compiles to what the hand-written copy compiled to (profiles/README.md lists the sites that keep their
// own text because it did not: det_finalize, det_vote_score, the general FPN kernel's rank loop, mask_paste, mask_rle).
#pragma once
#include "dtc_common.h"

namespace dtc {

// "This value is the same in every lane: keep it in SGPRs."  v_readfirstlane is free when the value already lives in SGPRs; it makes
// a value provably uniform where the compiler cannot see that it is (loop-carried, read from LDS, an atomic's result handed out by
// lane 0), so that what is formed from it is scalar arithmetic and scalar operands; and it is opaque to the optimiser, which
// otherwise turns a uniform offset inside an unrolled loop into one induction variable per address.  int and float are one
// instruction, 64-bit integers and pointers two.
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ float uni(float v) { return __int_as_float(uni(__float_as_int(v))); }
__device__ __forceinline__ uint64_t uni(uint64_t v) {
  return ((uint64_t)(uint32_t)uni((int)(uint32_t)(v >> 32)) << 32) | (uint64_t)(uint32_t)uni((int)(uint32_t)v);
}
template <typename T> __device__ __forceinline__ T* uni(T* p) { return reinterpret_cast<T*>(uni(reinterpret_cast<uint64_t>(p))); }

// Inclusive prefix sum of v over the lanes of a wavefront: six __shfl_up steps (int, uint32_t or long long).
template <typename T> __device__ __forceinline__ T wave_incl_scan(T v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) { const T o = __shfl_up(v, off, 64); if (lane >= off) v += o; }
  return v;
}

// Set bits of a ballot mask below this lane: the lane's slot in an ordered compaction of the mask's lanes.
__device__ __forceinline__ int lanes_below(uint64_t mask, int lane) { return __builtin_popcountll(mask & ((1ull << lane) - 1ull)); }

// Ordered expansion of a bitmap of <= 64 words held one word per lane of ONE wavefront (w: this lane's word, 0 past the end): the
// indices 64 * lane + bit of the set bits go to list in ascending order (np.where).
__device__ __forceinline__ void expand_bitmap(uint64_t w, int lane, uint32_t* list) {
  const int pc = __builtin_popcountll(w);
  int k = wave_incl_scan(pc, lane) - pc;
  while (w) { list[k++] = (uint32_t)(lane * 64 + __builtin_ctzll(w)); w &= w - 1ull; }
}

}  // namespace dtc
