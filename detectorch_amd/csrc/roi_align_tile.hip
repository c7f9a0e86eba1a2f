// A1  RoIAlign forward for gfx950 -- CLUSTER-STATIONARY kernel (sampling_ratio == 2: the FPN box and mask heads).
//
// Replaces roi_align_forward_kernel (lib/cppcuda/roi_align_forward_cuda.cu:82-159) and is bit-compatible with the CPU path
// roi_align_forward_loop (lib/cppcuda_cffi/src/cpp/roi_align_cpu_loop.cpp:118-219): same float32 operations, same order.
//
// Why this shape.  With NCHW features a RoI's window is a stack of short row pieces (12 pixels = 48 B on P2) cut out of
// 128-byte lines, once per channel.  A vector L1 keeps at most ~64 line fills in flight, so a CU moves 8 KB per memory
// latency whatever the kernel does with the bytes: the launch time is (line fills) x (latency) / 64 per CU, and a
// RoI-stationary workgroup (roi_align_fwd_lds in roi_align.hip) spends 16.5 fills per (RoI, channel) where 2.2 are
// compulsory -- measured 52 M fills / 0.52 ms per 8000-RoI launch, with every staging variant (round 1).
// RoIs that are neighbours in the visiting order of dtc_fpn_collect_distribute (level, row band, x) overlap about two-fold
// and sit side by side, so here a workgroup owns K consecutive RoIs of that order (K = 256 threads / bins):
//   1. their windows are merged greedily into clusters while the union window stays a compact patch -- at most merge_pct
//      (250) % of the pixels the members would stage one by one (the AREA rule, :tile kernel phase B) -- and fits the LDS
//      image and the register pipeline; a cluster's rows are 150-250 B wide instead of 48 B: every fetched line is mostly used;
//   2. the cluster's union window is staged ONCE per channel quad with 16-byte row-piece loads (4 pixels of one channel; raw
//      buffer loads, issued before the previous pass is pooled and committed after it), into an LDS image [quad][pixel][4 channels];
//   3. lane <-> (RoI, bin): sampling positions and weights are formed ONCE per lane (registers), then every channel quad
//      costs 16 ds_read_b128 + the reference's multiply-adds (packed fp32, the reference's order);
//   4. the results of a pass go to an LDS slab [RoI][channel][bin] -- contiguous per RoI exactly like the [R,C,PH,PW] output --
//      that leaves as 16-byte stores while the next pass is being committed (direct 4-byte stores from the pooling lanes cost
//      0.135 ms of a 0.61 ms launch).
// The LDS image is padded by one pixel slot every 8 pixels (phys = px + px/8): the transposing ds_write_b32 of 16
// consecutive 4-pixel groups x 2 channels then spread over all 32 banks two-way (free for ds_write_b32) instead of eight-way.
//
// Serves the FPN box head (7x7 bins) and mask head (14x14 bins), fp32 / fp16 / bf16 maps.  What was built around it and measured
// slower or equal -- a band sweep through an LDS ring, a per-launch preparation pass, LDS-DMA staging, merged-tap pooling --
// is recorded in tools/r03/README.md with the commits that hold the code.
//
// Anything the cluster path does not cover takes a correct slow path inside the same kernel: levels whose rows are not
// 16-byte aligned (P5: 42 columns) are staged with unaligned pieces or clamped scalar loads; a single RoI whose window exceeds
// the LDS image is gathered per output straight from global memory; padding rows (level < 0) are zero-filled.

#include <type_traits>

#include "roi_align_common.h"

namespace dtc {

constexpr int kTileMaxK = 32;                       // RoIs per workgroup (upper bound of the K the host picks)
constexpr int kTileRoiBytes = 48, kTileGroupBytes = 32;
constexpr int kTileHdrBytes = kTileMaxK * (kTileRoiBytes + kTileGroupBytes) + 16;
// Workgroup shape (threads, 16-byte row pieces a thread carries per pass, waves per SIMD the register budget allows):
//   256 threads x 8 pieces, 3 workgroups / CU (<= 168 VGPRs, 52 KB LDS each)   K = 5 RoIs of 7x7 bins per workgroup
// (512- and 1024-thread shapes -- K = 10 / 20 -- were built and measured in round 2: bit-exact, slower (0.42 / 0.54 ms against
// 0.37), and spilling; removed in round 3, `git show 1687f14:detectorch_amd/csrc/roi_align_tile.hip`.)
template <int NT> struct TileShape;
template <> struct TileShape<256> { static constexpr int kUnits = 8, kWaves = 3, kLdsKB = 52, kWaves16 = 4, kLds16KB = 38; };
// (16-bit maps: the LDS image is 16-bit, half the size -- 38 KB and <= 128 VGPRs put FOUR workgroups on a CU: cfg5 NCHW launch
//  0.495 -> 0.448 ms; 36 KB does not hold the slab + a 20 KB image, 44 KB is three workgroups again)

struct TileRoi {                        // 48 bytes
  int lvl, b, x0, x1, y0, y1, r, valid;   // window in feature pixels of its level, inclusive
  float sh, sw, bin_h, bin_w;             // scaled start and bin size (RoiHead): the item set-up reads them back from LDS
};
static_assert(sizeof(TileRoi) == kTileRoiBytes, "TileRoi layout");
struct TileGroup { int first, count, kind, x0, x1, y0, y1, pad; };   // kind 0: pooled cluster, 1: zero rows, 2: absent, 3: oversize
enum { kGrpPool = 0, kGrpZero = 1, kGrpAbsent = 2, kGrpGather = 3 };

// 16-byte (fp32) / 8-byte (fp16, bf16) row pieces through raw buffer loads: SGPR resource (base of this cluster's image /
// channel block) + 32-bit lane offset + SGPR pass offset -- no 64-bit address registers, and dword alignment is enough
// (rows of a level whose width is not a multiple of 4, P5's 42 columns, are read with the same instruction).
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_srd(const void* base) {
  // raw buffer, no bounds clamp (num_records = 2^32 - 1); word 3 = DATA_FORMAT 32 (the gfx9 raw-buffer encoding)
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(base), 0, 0xffffffff, 0x00020000);
}
// Piece4<T>::raw: four pixels of one channel as loaded.  16-bit maps: the four 16-bit values stay as they are (two
// dwords) -- the LDS image of a 16-bit map stays 16-bit (half the commit and tap bytes) and the taps are widened where they are
// multiplied (mul_pair16: the same float32 values).
template <typename TIn> struct Piece4;
template <> struct Piece4<float> {
  typedef float4 Raw;
  static __device__ __forceinline__ Raw raw(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0);
    return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
  }
};
template <> struct Piece4<__half> {
  typedef u32x2 Raw;
  static __device__ __forceinline__ Raw raw(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) { return __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0); }
};
template <> struct Piece4<bf16_t> {
  typedef u32x2 Raw;
  static __device__ __forceinline__ Raw raw(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) { return __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0); }
};

// element type / slot size of the LDS image: float32 maps -> float32, 16 bytes per (pixel, 4 channels); 16-bit maps -> the raw 16-bit
// values, 8 bytes per slot (tap = ds_read_b64; simulated on the bench RoIs, tools/r04/lds_taps4.py b64: 5.2 LDS cycles per tap read
// against 9.6 for ds_read_b128 on a float32 image)
template <typename TIn> struct TileLds { typedef float T; static constexpr int kSlot = 16, kShift = 4; };
template <> struct TileLds<__half> { typedef uint16_t T; static constexpr int kSlot = 8, kShift = 3; };
template <> struct TileLds<bf16_t> { typedef uint16_t T; static constexpr int kSlot = 8, kShift = 3; };

template <typename TIn, int NT> struct TileBounds { static constexpr int kWaves = TileShape<NT>::kWaves; };
template <int NT> struct TileBounds<__half, NT> { static constexpr int kWaves = TileShape<NT>::kWaves16; };
template <int NT> struct TileBounds<bf16_t, NT> { static constexpr int kWaves = TileShape<NT>::kWaves16; };   // 12-40 B of scratch per lane, still 4-6 % faster than 3

// LDS slot (one pixel x 4 channels) of window pixel px inside one quad image: one pad slot every 8 pixels
__device__ __forceinline__ int tile_phys(int px) { return px + (px >> 3); }

// Everything a lane needs to pool ITS (RoI, bin) from the LDS image, formed once per cluster.
struct TileItem {
  int a[2][2][4];           // [iy][ix][tap]: LDS byte offsets (inside a quad image) of (y.lo,x.lo) (y.lo,x.hi) (y.hi,x.lo) (y.hi,x.hi)
  float yl[2], yh[2], xl[2], xh[2];
  bool on;
};

enum { kStageScalar = 0, kStageVec = 1, kStageVecUnaligned = 2 };

struct TileGeom {            // one cluster, all uniform
  int first, count;          // RoIs troi[first .. first + count)
  int y0, x0a, ngx, npos;    // window origin (x aligned down to 4), 4-pixel pieces per row, pieces in the window
  int plane;                 // LDS slots (16 B) per quad image
  int nq_pass;               // channel quads staged + pooled per pass
  int mode;                  // kStage*
};

// One cluster: stage + pool every channel quad of this workgroup's channel block.
// Register pipeline: a thread carries up to kUnits 16-byte row pieces per pass; unit u = q * KC + i is piece-chunk i
// (16 consecutive pieces x 4 channels per wave-instruction) of channel quad q, so a pass stages nq_pass quads with
// KC * nq_pass <= kUnits.  Per pass:   commit(p) + store_slab(p-1) | barrier | issue(p+1) + pool(p) -> slab | barrier
// i.e. the loads of pass p+1 are in flight (registers) while pass p is pooled, and the pooled [RoI][channel][bin] slab of
// pass p leaves for global memory as contiguous 16-byte stores while pass p+1 is being committed.
template <typename TIn, typename TOut, int NT, bool FUSED>
__device__ __forceinline__ void tile_passes(const RoiAlignParams& p, const dtc_feat_level& L, const TIn* fbase, int c0, int nc,
                                            int bins, float* slab, typename TileLds<TIn>::T* win, const TileRoi* troi, const TileGeom& g,
                                            const TileItem& it, int rl, int bin) {
  constexpr int NW = NT / 64;
  constexpr int U = TileShape<NT>::kUnits;
  typedef typename TileLds<TIn>::T TL;
  constexpr bool L16 = sizeof(TL) == 2;
  constexpr int SB = TileLds<TIn>::kSlot;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, pl = lane & 15, cl = (lane >> 4) & 3;
  const int npos = g.npos, ngx = g.ngx, plane = g.plane, nq_pass = g.nq_pass;
  const int nchunk = (npos + 15) >> 4;
  const int KC = ceil_div(nchunk, NW);
  const float rinv = 1.0f / (float)ngx;
  const int nq_tot = ceil_div(nc, 4);
  const bool vec = g.mode != kStageScalar;
  uint32_t uoff[U];     // byte offset of the unit's piece (row, 4 pixels, channel 4q + cl) from the pass base plane; bits 30-31:
                        // how many pixels the piece was shifted left to stay inside its row (kStageVecUnaligned)
  int ulds[U];          // element index of (first pixel of the piece, channel cl) in the LDS image
  // every pass is full: nq_pass divides the number of quads (caller), so nu = KC * nq_pass units carry data; the remaining
  // register slots DUPLICATE unit 0 (same bytes to the same LDS words) -- issue / commit are branch-free straight-line code,
  // all loads of a pass leave back to back.
  const int nu = KC * nq_pass;
  if (vec) {
    const int sh32 = (int)L.stride_h, sc32 = (int)L.stride_c;
    int q = 0, i = 0;
#pragma unroll
    for (int u = 0; u < U; u++) {
      const bool dup = u >= nu;
      const int pos = min((wv + (dup ? 0 : i) * NW) * 16 + pl, npos - 1);   // lanes past the window duplicate its last piece
      const int row = (int)(((float)pos + 0.5f) * rinv);         // exact: pos < 2^13, distance to an integer >= 0.5 / ngx
      const int gx = pos - row * ngx;
      const int qq = dup ? 0 : q;
      int col = g.x0a + 4 * gx, sft = 0;
      if (g.mode == kStageVecUnaligned) { sft = max(0, col + 3 - (L.width - 1)); col -= sft; }   // last piece of a row: stay in the row
      uoff[u] = ((uint32_t)((g.y0 + row) * sh32 + col + (4 * qq + cl) * sc32) * (uint32_t)sizeof(TIn)) | ((uint32_t)sft << 30);
      ulds[u] = qq * plane * 4 + ((4 * pos + (pos >> 1)) << 2) + cl;
      if (++i == KC) { i = 0; q++; }
    }
  }
  const __amdgpu_buffer_rsrc_t srd = make_srd(fbase);
  const uint32_t pass_bytes = (uint32_t)(L.stride_c * (int64_t)sizeof(TIn));       // per channel
  typename Piece4<TIn>::Raw v[U];
  auto issue = [&](int cs) {      // vec only: every staged channel exists (nc % 4 == 0)
    const uint32_t soff = (uint32_t)cs * pass_bytes;
    if (g.mode == kStageVec) {
#pragma unroll
      for (int u = 0; u < U; u++) v[u] = Piece4<TIn>::raw(srd, uoff[u], soff);
    } else {
#pragma unroll
      for (int u = 0; u < U; u++) v[u] = Piece4<TIn>::raw(srd, uoff[u] & 0x3fffffffu, soff);
    }
  };
  // Two instances behind ONE uniform branch: left as a condition inside the unrolled loop the compiler if-converted the shifted-piece
  // selects of kStageVecUnaligned (P5's 42-column rows) into 9 v_cndmask per unit that EVERY commit executed -- 72 of the 104 vector
  // instructions of a 16-bit commit, a fifth of a pass (round 6, from the ISA).
  auto commit_as = [&](auto shifted_tag) {
    constexpr bool SHIFTED = decltype(shifted_tag)::value;
    if constexpr (SHIFTED) asm volatile("" ::: "memory");      // keeps the two instances apart (no if-conversion across it)
#pragma unroll
    for (int u = 0; u < U; u++) {
      if constexpr (L16) {
        uint32_t w0 = v[u].x & 0xffffu, w1 = v[u].x >> 16, w2 = v[u].y & 0xffffu, w3 = v[u].y >> 16;
        if constexpr (SHIFTED) {
          const uint32_t sft = uoff[u] >> 30;
          w0 = sft == 0 ? w0 : sft == 1 ? w1 : sft == 2 ? w2 : w3;
          w1 = sft == 0 ? w1 : sft == 1 ? w2 : w3;
          w2 = sft == 0 ? w2 : w3;
        }
        TL* d = win + ulds[u];
        d[0] = (TL)w0; d[4] = (TL)w1; d[8] = (TL)w2; d[12] = (TL)w3;
      } else {
        float4 w = v[u];
        if constexpr (SHIFTED) {                // shifted piece: pixel k of the piece is component k + shift of the load
          const uint32_t sft = uoff[u] >> 30;
          w.x = sft == 0 ? w.x : sft == 1 ? w.y : sft == 2 ? w.z : w.w;
          w.y = sft == 0 ? w.y : sft == 1 ? w.z : w.w;
          w.z = sft == 0 ? w.z : w.w;             // components past the row end hold a copy of its last pixel: never sampled
        }
        TL* d = win + ulds[u];
        d[0] = w.x; d[4] = w.y; d[8] = w.z; d[12] = w.w;
      }
    }
  };
  auto commit = [&]() {
    if (g.mode == kStageVecUnaligned) commit_as(std::true_type{}); else commit_as(std::false_type{});
  };
  auto lds_val = [&](const TIn& x) -> TL {          // what the LDS image holds of a map element
    if constexpr (L16) return *reinterpret_cast<const uint16_t*>(&x); else return to_f32<TIn>(x);
  };
  // Strided columns, misaligned bases or a channel tail (channels_last maps, C % 4 != 0, maps narrower than 4): no register
  // pipeline, each piece is four clamped scalar loads written straight to LDS.  Correct for any strides; not a fast path.
  auto stage_scalar = [&](int cs) {
#pragma unroll 1
    for (int q = 0; q < nq_pass; q++) {
      const int cq = cs + 4 * q;
      if (cq >= nc) break;
      const int cle = min(cl, nc - 1 - cq);                        // channel tail: clamp the plane, never stored
      const TIn* base = fbase + (int64_t)(cq + cle) * L.stride_c;
#pragma unroll 1
      for (int t = wv; t < nchunk; t += NW) {
        const int pos = min(t * 16 + pl, npos - 1);
        const int row = (int)(((float)pos + 0.5f) * rinv);
        const int gx = pos - row * ngx;
        const int rem = L.width - 1 - (g.x0a + 4 * gx);             // >= 0: a piece starts inside the map
        const TIn* s = base + (int64_t)(g.y0 + row) * L.stride_h + (int64_t)(g.x0a + 4 * gx) * L.stride_w;
        TL* d = win + q * plane * 4 + ((4 * pos + (pos >> 1)) << 2) + cl;
        d[0] = lds_val(s[0]);
        d[4] = lds_val(s[(int64_t)min(1, rem) * L.stride_w]);
        d[8] = lds_val(s[(int64_t)min(2, rem) * L.stride_w]);
        d[12] = lds_val(s[(int64_t)min(3, rem) * L.stride_w]);
      }
    }
  };
  // slab of the pass that was pooled last: [RoI of the cluster][4 * nq channels][bins] float32, contiguous per RoI exactly like
  // the [R, C, PH, PW] output -> 16-byte stores (the output offset of channel cs is a multiple of 4 elements when C % 4 == 0)
  const bool quad_ok = ((p.channels | c0) & 3) == 0;
  auto store_slab = [&](int cs, int nq) {
    const int nch = min(4 * nq, nc - cs);
    TOut* out = reinterpret_cast<TOut*>(p.out);
    if (quad_ok && nch == 4 * nq) {
      const int n4 = nq * bins, total = g.count * n4;
      const float r4 = 1.0f / (float)n4;
      // the RoI's output row for channel c0 as ONE 64-bit element offset, formed once per RoI in phase A (TileRoi::x0 / x1 in LDS):
      // the store's address is that + a uniform term + 4 e -- (r * channels + c0 + cs) * bins in 64-bit integer multiplies per 16-byte
      // store was six quarter-rate instructions, a quarter of a pass's vector time on 16-bit maps (round 6, from the ISA)
      const int cs_off = cs * bins;
      for (int idx = tid; idx < total; idx += NT) {
        const int k = (int)(((float)idx + 0.5f) * r4);            // exact for idx < 2^13
        const int e = idx - __mul24(k, n4);
        const float4 val = reinterpret_cast<const float4*>(slab)[idx];
        const uint64_t ob = *reinterpret_cast<const uint64_t*>(&troi[g.first + k].x0);
        store4<TOut>(out + (ob + (uint64_t)(uint32_t)(cs_off + 4 * e)), val);
      }
    } else {
      const int per = nch * bins, total = g.count * per;
      for (int idx = tid; idx < total; idx += NT) {
        const int k = idx / per, e = idx - k * per;
        out[((size_t)troi[g.first + k].r * p.channels + c0 + cs) * bins + e] = from_f32<TOut>(slab[k * 4 * nq * bins + e]);
      }
    }
  };

  if (vec) issue(0);
  int cs_prev = 0, nq_prev = 0;
#pragma unroll 1
  for (int qs = 0; qs < nq_tot; qs += nq_pass) {
    const int cs = 4 * qs;
    const int nq_cur = min(nq_pass, nq_tot - qs);
    if (vec) commit(); else stage_scalar(cs);
    if (nq_prev) store_slab(cs_prev, nq_prev);
    __syncthreads();
    if (vec && qs + nq_pass < nq_tot) issue(cs + 4 * nq_pass);    // next pass: in flight (registers) while this one is pooled
    if (it.on) {
      float* so = slab + rl * (4 * nq_cur * bins) + bin;
#pragma unroll 1
      for (int q = 0; q < nq_cur; q++) {
        // uniform quad offset, opaque to the optimiser: otherwise every tap address becomes its own induction variable
        const char* wq = reinterpret_cast<const char*>(win) + uni(q * plane * SB);
        // two channels per instruction (v_pk_mul_f32 / v_pk_add_f32: IEEE results, twice the fp32 rate of the scalar forms)
        f32x2 a01 = {0.f, 0.f}, a23 = {0.f, 0.f};
        // reference order: for iy { for ix { acc += w1*v1 + w2*v2 + w3*v3 + w4*v4 } }   (roi_align_cpu_loop.cpp:203-214)
#pragma unroll
        for (int iy = 0; iy < 2; iy++) {
          if constexpr (L16 && FUSED) {
            // contract mode (dtc_roi_align_set_exact(0)): every tap is one fused convert-multiply-accumulate per channel, 64
            // vector instructions per channel quad instead of 64 + 32 packed adds (see fma_pair16)
            u32x2 t[2][4];
#pragma unroll
            for (int ix = 0; ix < 2; ix++)
#pragma unroll
              for (int k = 0; k < 4; k++)
                t[ix][k] = *reinterpret_cast<const u32x2*>(__builtin_assume_aligned(wq + it.a[iy][ix][k], 8));
#pragma unroll
            for (int ix = 0; ix < 2; ix++) {
              const float w1 = it.yh[iy] * it.xh[ix], w2 = it.yh[iy] * it.xl[ix];
              const float w3 = it.yl[iy] * it.xh[ix], w4 = it.yl[iy] * it.xl[ix];
              fma_pair16<TIn>(a01, t[ix][0].x, w1); fma_pair16<TIn>(a23, t[ix][0].y, w1);
              fma_pair16<TIn>(a01, t[ix][1].x, w2); fma_pair16<TIn>(a23, t[ix][1].y, w2);
              fma_pair16<TIn>(a01, t[ix][2].x, w3); fma_pair16<TIn>(a23, t[ix][2].y, w3);
              fma_pair16<TIn>(a01, t[ix][3].x, w4); fma_pair16<TIn>(a23, t[ix][3].y, w4);
            }
          } else if constexpr (L16) {
            u32x2 t[2][4];
#pragma unroll
            for (int ix = 0; ix < 2; ix++)
#pragma unroll
              for (int k = 0; k < 4; k++)                                     // 8 ds_read_b64 in flight per sample row
                t[ix][k] = *reinterpret_cast<const u32x2*>(__builtin_assume_aligned(wq + it.a[iy][ix][k], 8));
#pragma unroll
            for (int ix = 0; ix < 2; ix++) {
              const float w1 = it.yh[iy] * it.xh[ix], w2 = it.yh[iy] * it.xl[ix];             // roi_align_cpu_loop.cpp:95
              const float w3 = it.yl[iy] * it.xh[ix], w4 = it.yl[iy] * it.xl[ix];
              f32x2 s01 = mul_pair16<TIn>(t[ix][0].x, w1) + mul_pair16<TIn>(t[ix][1].x, w2);    // :208-211, channels 0-1
              s01 = s01 + mul_pair16<TIn>(t[ix][2].x, w3);
              s01 = s01 + mul_pair16<TIn>(t[ix][3].x, w4);
              f32x2 s23 = mul_pair16<TIn>(t[ix][0].y, w1) + mul_pair16<TIn>(t[ix][1].y, w2);    // channels 2-3
              s23 = s23 + mul_pair16<TIn>(t[ix][2].y, w3);
              s23 = s23 + mul_pair16<TIn>(t[ix][3].y, w4);
              a01 = a01 + s01; a23 = a23 + s23;
            }
          } else {
            f32x4 t[2][4];
#pragma unroll
            for (int ix = 0; ix < 2; ix++)
#pragma unroll
              for (int k = 0; k < 4; k++)                                     // 8 ds_read_b128 in flight per sample row
                t[ix][k] = *reinterpret_cast<const f32x4*>(__builtin_assume_aligned(wq + it.a[iy][ix][k], 16));
#pragma unroll
            for (int ix = 0; ix < 2; ix++) {
              const float w1 = it.yh[iy] * it.xh[ix], w2 = it.yh[iy] * it.xl[ix];             // roi_align_cpu_loop.cpp:95
              const float w3 = it.yl[iy] * it.xh[ix], w4 = it.yl[iy] * it.xl[ix];
              a01 += w1 * t[ix][0].lo + w2 * t[ix][1].lo + w3 * t[ix][2].lo + w4 * t[ix][3].lo;    // :208-211
              a23 += w1 * t[ix][0].hi + w2 * t[ix][1].hi + w3 * t[ix][2].hi + w4 * t[ix][3].hi;
            }
          }
          __builtin_amdgcn_sched_barrier(0);      // keep the two sample rows apart: 32, not 64, tap registers live
        }
        // :216  output_val /= count ; count == 4 -> x * 0.25f is the same float32
        float* o = so + uni(4 * q * bins);
        const float a0 = a01.x, a1 = a01.y, a2 = a23.x, a3 = a23.y;
        o[0] = a0 * 0.25f; o[bins] = a1 * 0.25f; o[2 * bins] = a2 * 0.25f; o[3 * bins] = a3 * 0.25f;
      }
    }
    __syncthreads();
    cs_prev = cs; nq_prev = nq_cur;
  }
  if (nq_prev) store_slab(cs_prev, nq_prev);   // the next cluster writes the slab only behind its own first barrier
}

// Work item of block b: XCD x (= b % 8) owns a contiguous slice of the (cluster group, channel block) items, as in
// xcd_work_item, but walks it BACK TO FRONT: the visiting order ends with the coarsest level of an image, whose RoIs have the
// largest windows and merge least (3-4 clusters per workgroup, 2-2.5 x the average duration).  Started last they were the
// tail of the launch (no workgroup starts during its last 20 %); started first the tail is made of average workgroups.
__device__ __forceinline__ int tile_work_item(int b, int n, int reverse) {
  if (n < 2 * kXcds || (reverse & 2)) return (reverse & 1) ? n - 1 - b : b;      // bit 1: no XCD slicing (A/B knob DTC_RA_NO_XCD)
  const int x = b % kXcds, j = b / kXcds;
  const int q = n / kXcds, r = n - q * kXcds;
  const int start = x * q + min(x, r), qx = q + (x < r ? 1 : 0);
  return start + ((reverse & 1) ? qx - 1 - j : j);
}

template <typename TIn, typename TOut, int NT, bool FUSED>
__global__ __launch_bounds__(NT, (TileBounds<TIn, NT>::kWaves)) void roi_align_fwd_tile(RoiAlignParams p, int kgroup, int lds_bytes, int nq_cap, int merge_pct, int reverse) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  TileRoi* troi = reinterpret_cast<TileRoi*>(smem);
  TileGroup* tgrp = reinterpret_cast<TileGroup*>(smem + kTileMaxK * kTileRoiBytes);
  int* ngp = reinterpret_cast<int*>(smem + kTileMaxK * (kTileRoiBytes + kTileGroupBytes));
  // [header][slab: K RoIs x 4 nq_cap channels x bins float32, fixed][image: nq quads x plane slots x 16 B]
  const int slab_bytes = kgroup * p.pooled_h * p.pooled_w * 16 * nq_cap;
  float* slab = reinterpret_cast<float*>(smem + kTileHdrBytes);
  typedef typename TileLds<TIn>::T TL;
  constexpr int SB = TileLds<TIn>::kSlot;
  TL* win = reinterpret_cast<TL*>(smem + kTileHdrBytes + slab_bytes);
  const int win_bytes = lds_bytes - kTileHdrBytes - slab_bytes;
  constexpr int NW = NT / 64;
  constexpr int kMaxPos = TileShape<NT>::kUnits * NW * 16;                  // 16-byte pieces the register pipeline can carry per quad
  const int tid = threadIdx.x;
  const int nct = ceil_div(p.channels, p.ch_block);
  const int wi = tile_work_item(blockIdx.x, gridDim.x, reverse);
  int grp = wi / nct;
  int c0 = (wi - grp * nct) * p.ch_block;
  {
    // reverse bit 2: an XCD walks its groups once per CHANNEL BLOCK -- the ~100 workgroups resident on an XCD then pool the same
    // channel block of ~100 neighbouring groups, whose patches overlap 3.6-fold: measured on the bench's box-head launch (round 4,
    // profiles/r04_a_*) L2 hit rate 0.38 -> 0.51, fabric reads 1.79 -> 1.32 GB, 0.389 -> 0.379 ms.  (Needs the groups to divide
    // evenly over the XCDs; otherwise the group-major order above.)  A/B: DTC_RA_TILE_CBMAJOR=0.
    const int ngrp = (int)gridDim.x / nct;
    if ((reverse & 4) && ngrp % kXcds == 0 && ngrp >= 2 * kXcds) {
      const int x = blockIdx.x % kXcds, j = blockIdx.x / kXcds, ngx = ngrp / kXcds;
      const int cbi = j / ngx, gl = j - cbi * ngx;
      grp = x * ngx + ((reverse & 1) ? ngx - 1 - gl : gl);
      c0 = cbi * p.ch_block;
    }
  }
  const int nc = min(p.ch_block, p.channels - c0);
  const int bins = p.pooled_h * p.pooled_w;
  const int K = kgroup;

  // ---- A + B (wavefront 0). A: lane k forms the window of RoI k.  B: greedy clustering along the visiting order, by the whole
  // wave on the register copies (readlane with a uniform index: no LDS round trips, no barrier between A and B) ------------
  if (tid < 64) {
    TileRoi t;
    t.lvl = -1; t.b = 0; t.x0 = t.x1 = t.y0 = t.y1 = 0; t.r = 0; t.valid = 0; t.sh = t.sw = 0.f; t.bin_h = t.bin_w = 1.f;
    const int ri = grp * K + tid;
    if (tid < K && ri < p.n_rois) {
      const RoiHead hd = load_roi_head(p, ri);
      t.valid = 1; t.r = hd.r; t.b = hd.b; t.sh = hd.sh; t.sw = hd.sw; t.bin_h = hd.bin_h; t.bin_w = hd.bin_w;
      if (hd.lvl >= 0 && hd.lvl < p.n_levels) {
        t.lvl = hd.lvl;
        const int H = p.lv[hd.lvl].height, W = p.lv[hd.lvl].width;
        // sample positions are non-decreasing in (bin, sample): first .lo / last .hi bound the window (roi_align_cpu_loop.cpp:38-90)
        t.y0 = make_axis(hd.sh, hd.bin_h, 0, 0, 2, H).lo;
        t.y1 = make_axis(hd.sh, hd.bin_h, p.pooled_h - 1, 1, 2, H).hi;
        t.x0 = make_axis(hd.sw, hd.bin_w, 0, 0, 2, W).lo;
        t.x1 = make_axis(hd.sw, hd.bin_w, p.pooled_w - 1, 1, 2, W).hi;
      }
    }
    if (tid < K) {
      troi[tid] = t;
      // (x0 / x1 are read from the REGISTER copy below, never from LDS: their LDS words carry the RoI's output offset, see store_slab)
      *reinterpret_cast<uint64_t*>(&troi[tid].x0) = ((uint64_t)(uint32_t)t.r * (uint64_t)p.channels + (uint64_t)c0) * (uint64_t)(p.pooled_h * p.pooled_w);
    }
    auto bc = [](int v, int k) { return __builtin_amdgcn_readlane(v, k); };     // k: uniform lane index
    int ng = 0, k = 0;
    while (k < K) {
      const int ks = uni(k);
      const int a_lvl = bc(t.lvl, ks), a_b = bc(t.b, ks), a_valid = bc(t.valid, ks);
      const int a_x0 = bc(t.x0, ks), a_x1 = bc(t.x1, ks), a_y0 = bc(t.y0, ks), a_y1 = bc(t.y1, ks);
      TileGroup g;
      g.first = k; g.count = 1; g.x0 = a_x0; g.x1 = a_x1; g.y0 = a_y0; g.y1 = a_y1; g.pad = 0;
      if (!a_valid) g.kind = kGrpAbsent;
      else if (a_lvl < 0) g.kind = kGrpZero;
      else {
        const int ngx0 = (a_x1 >> 2) - (a_x0 >> 2) + 1, th0 = a_y1 - a_y0 + 1, npos0 = th0 * ngx0;
        if (npos0 > kMaxPos || (4 * npos0 + (npos0 >> 1) + 1) * SB > win_bytes || bins > NT) {
          g.kind = kGrpGather;
        } else {
          g.kind = kGrpPool;
          // merge the next RoI of the visiting order while the union window stays a compact patch: at most merge_pct % of the
          // pixels the members would stage one by one.  (Neighbours of the (level, band, x) order overlap about two-fold, so a
          // patch of K windows is hardly larger than their sum -- but its rows are K times longer, i.e. whole 128-byte lines.)
          long long sum_px = (long long)th0 * (a_x1 - a_x0 + 1);
          while (k + g.count < K && (g.count + 1) * bins <= NT) {
            const int js = uni(k + g.count);
            const int n_lvl = bc(t.lvl, js), n_b = bc(t.b, js), n_valid = bc(t.valid, js);
            if (!n_valid || n_lvl != a_lvl || n_b != a_b) break;
            const int n_x0 = bc(t.x0, js), n_x1 = bc(t.x1, js), n_y0 = bc(t.y0, js), n_y1 = bc(t.y1, js);
            const int ux0 = min(g.x0, n_x0), ux1 = max(g.x1, n_x1), uy0 = min(g.y0, n_y0), uy1 = max(g.y1, n_y1);
            const int ungx = (ux1 >> 2) - (ux0 >> 2) + 1, uth = uy1 - uy0 + 1, unpos = uth * ungx;
            if (unpos > kMaxPos || (4 * unpos + (unpos >> 1) + 1) * SB > win_bytes) break;
            const long long n_px = (long long)(n_y1 - n_y0 + 1) * (n_x1 - n_x0 + 1);
            const long long u_px = (long long)uth * (ux1 - ux0 + 1);
            if (u_px * 100 > (sum_px + n_px) * merge_pct) break;
            g.x0 = ux0; g.x1 = ux1; g.y0 = uy0; g.y1 = uy1; g.count++;
            sum_px += n_px;
          }
        }
      }
      if (tid == 0) tgrp[ng] = g;
      ng++;
      k += g.count;
    }
    if (tid == 0) *ngp = ng;
  }
  __syncthreads();

  // ---- C. clusters ----------------------------------------------------------------------------------------------------
  const int ngroups = uni(*ngp);
  for (int gi = 0; gi < ngroups; gi++) {
    const int first = uni(tgrp[gi].first), count = uni(tgrp[gi].count), kind = uni(tgrp[gi].kind);
    if (kind == kGrpAbsent) continue;
    if (kind == kGrpZero) {    // padding row of a fixed-shape batch (fpn.hip emits level -1): defined output
      TOut* oz = reinterpret_cast<TOut*>(p.out) + ((size_t)uni(troi[first].r) * p.channels + c0) * bins;
      zero_outputs<TOut, NT>(oz, nc * bins, tid);
      continue;
    }
    const int lvl = uni(troi[first].lvl), b = uni(troi[first].b);
    const dtc_feat_level L = p.lv[lvl];
    const TIn* fbase = reinterpret_cast<const TIn*>(L.data) + (int64_t)b * L.stride_n + (int64_t)c0 * L.stride_c;
    if (kind == kGrpGather) {
      // a single window larger than the LDS image: per-output gather straight from global memory, geometry on the fly
      const RoiHead hd = load_roi_head(p, grp * K + first);
      TOut* og = reinterpret_cast<TOut*>(p.out) + ((size_t)hd.r * p.channels + c0) * bins;
      for (int o = tid; o < nc * bins; o += NT) {
        const int c = o / bins, bin = o - c * bins;
        const int ph = bin / p.pooled_w, pw = bin - ph * p.pooled_w;
        const TIn* d = fbase + (int64_t)c * L.stride_c;
        float acc = 0.f;
        for (int iy = 0; iy < 2; iy++) {
          const AxisEntry y = make_axis(hd.sh, hd.bin_h, ph, iy, 2, L.height);
          const int64_t ylo = (int64_t)y.lo * L.stride_h, yhi = (int64_t)y.hi * L.stride_h;
          for (int ix = 0; ix < 2; ix++) {
            const AxisEntry x = make_axis(hd.sw, hd.bin_w, pw, ix, 2, L.width);
            const int64_t xlo = (int64_t)x.lo * L.stride_w, xhi = (int64_t)x.hi * L.stride_w;
            const float w1 = y.h * x.h, w2 = y.h * x.l, w3 = y.l * x.h, w4 = y.l * x.l;
            acc += w1 * to_f32<TIn>(d[ylo + xlo]) + w2 * to_f32<TIn>(d[ylo + xhi]) + w3 * to_f32<TIn>(d[yhi + xlo]) +
                   w4 * to_f32<TIn>(d[yhi + xhi]);
          }
        }
        og[o] = from_f32<TOut>(acc * 0.25f);
      }
      continue;
    }
    // cluster geometry (uniform)
    const int gx0 = uni(tgrp[gi].x0), gx1 = uni(tgrp[gi].x1), gy0 = uni(tgrp[gi].y0), gy1 = uni(tgrp[gi].y1);
    TileGeom g;
    g.first = first; g.count = count;
    g.y0 = gy0; g.x0a = gx0 & ~3;
    g.ngx = (gx1 >> 2) - (gx0 >> 2) + 1;
    const int tw = 4 * g.ngx, th = gy1 - gy0 + 1;
    g.npos = th * g.ngx;
    g.plane = 4 * g.npos + (g.npos >> 1) + 1;           // slots per quad image
    // staging mode: 16-byte aligned rows -> plain 16-byte pieces; 4-byte aligned rows (width % 4 != 0) -> unaligned pieces,
    // the last one of a row shifted left; anything else (strided columns, channel tails) -> scalar loads
    const int esz = (int)sizeof(TIn);
    const bool lin = L.stride_w == 1 && ((nc | c0) & 3) == 0 && L.stride_h > 0 && L.stride_c > 0 &&
                     L.stride_h * L.height + L.stride_c * 4 * TileShape<NT>::kUnits < (1ll << 26);     // lane offsets fit 30 bits
    const bool al16 = ((L.width | L.stride_h | L.stride_c | L.stride_n) & 3) == 0 &&
                      (reinterpret_cast<uintptr_t>(L.data) & (4 * sizeof(TIn) - 1)) == 0;
    const bool al4 = L.width >= 4 && (((L.width | L.stride_h | L.stride_c | L.stride_n) * esz) & 3) == 0 &&
                     (reinterpret_cast<uintptr_t>(L.data) & 3) == 0;
    g.mode = !lin ? kStageScalar : al16 ? kStageVec : al4 ? kStageVecUnaligned : kStageScalar;
    const int KC = ceil_div((g.npos + 15) >> 4, NW);
    g.nq_pass = max(1, min(min(win_bytes / (g.plane * SB), TileShape<NT>::kUnits / KC), min(ceil_div(nc, 4), nq_cap)));
    while (ceil_div(nc, 4) % g.nq_pass) g.nq_pass--;        // every pass full: no partial-pass code in the staging pipeline
    // ---- the lane's item -------------------------------------------------------------------------------------------
    const int n_it = count * bins;
    TileItem it;
    it.on = tid < n_it;
    const int itx = it.on ? tid : 0;
    const int rl = itx / bins, bin = itx - rl * bins;
    const int ph = bin / p.pooled_w, pw = bin - ph * p.pooled_w;
    const TileRoi hd = troi[first + rl];     // sh / sw / bin sizes as phase A formed them
    int ylo[2], yhi[2], xlo[2], xhi[2];      // window-relative: rows premultiplied by the window width
#pragma unroll
    for (int i = 0; i < 2; i++) {
      const AxisEntry ey = make_axis(hd.sh, hd.bin_h, ph, i, 2, L.height);
      const AxisEntry ex = make_axis(hd.sw, hd.bin_w, pw, i, 2, L.width);
      it.yl[i] = ey.l; it.yh[i] = ey.h; it.xl[i] = ex.l; it.xh[i] = ex.h;
      ylo[i] = (ey.lo - gy0) * tw; yhi[i] = (ey.hi - gy0) * tw;
      xlo[i] = ex.lo - g.x0a; xhi[i] = ex.hi - g.x0a;
    }
#pragma unroll
    for (int iy = 0; iy < 2; iy++)
#pragma unroll
      for (int ix = 0; ix < 2; ix++) {
        constexpr int SS = TileLds<TIn>::kShift;
        int t0 = tile_phys(ylo[iy] + xlo[ix]) << SS, t1 = tile_phys(ylo[iy] + xhi[ix]) << SS;
        int t2 = tile_phys(yhi[iy] + xlo[ix]) << SS, t3 = tile_phys(yhi[iy] + xhi[ix]) << SS;
        asm volatile("" : "+v"(t0), "+v"(t1), "+v"(t2), "+v"(t3));   // one finished VGPR per tap: do not re-derive in the loop
        it.a[iy][ix][0] = t0; it.a[iy][ix][1] = t1; it.a[iy][ix][2] = t2; it.a[iy][ix][3] = t3;
      }
    tile_passes<TIn, TOut, NT, FUSED>(p, L, fbase, c0, nc, bins, slab, win, troi, g, it, rl, bin);
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------
// launch shape that no knob changes (the knobs: RoiAlignKnobs::tile_*, roi_align_common.h)
constexpr int kTileThreads = 256;    // threads per workgroup
constexpr int kTileMergePct = 250;   // a cluster may stage at most this % of the pixels its members would stage separately
constexpr int kTileNqCap = 4;        // channel quads per pass, upper bound -- sizes the LDS output slab
constexpr int kTileReverse = 1;      // walk an XCD's slice of the visiting order back to front (heaviest workgroups first)

template <typename TIn, typename TOut, int NT, bool FUSED>
static int launch_tile_nt(RoiAlignParams p, hipStream_t stream) {
  const RoiAlignKnobs& cfg = roi_align_knobs();
  const int bins = p.pooled_h * p.pooled_w;
  int K = NT / bins;               // RoIs per workgroup
  K = K < 1 ? 1 : (K > kTileMaxK ? kTileMaxK : K);
  if (K * bins > NT) K = NT / bins;
  if (K < 1) return DTC_EUNSUPPORTED;
  // 16-bit maps: their LDS image is half the size
  const int lds_b = (sizeof(TIn) == 2 ? (cfg.tile_lds16_kb ? cfg.tile_lds16_kb : TileShape<NT>::kLds16KB) : TileShape<NT>::kLdsKB) * 1024;
  if (raise_lds_once<roi_align_fwd_tile<TIn, TOut, NT, FUSED>>() != DTC_OK) return DTC_ELAUNCH;
  const int nq_cap = kTileNqCap;
  if (kTileHdrBytes + K * bins * 16 * nq_cap + 20 * 1024 > lds_b) return DTC_EUNSUPPORTED;
  const int ngrp = ceil_div(p.n_rois, K);
  // channels per workgroup: the per-cluster setup (geometry, item registers) is paid once per block; keep >= ~4 workgroups per CU
  // measured on MI355X: 8000 RoIs x 256 ch (1600 groups): 32 -> 0.48, 64 -> 0.41, 128 -> 0.42 ms; 16 000 RoIs fp16 (3200 groups):
  // 64 -> 0.568, 128 -> 0.545 ms -- the larger block as soon as it still leaves ~8 workgroups per slot
  int cb = cfg.tile_ch_block ? cfg.tile_ch_block : ((long long)ngrp * ceil_div(p.channels, 128) >= 6144 ? 128 : 64);
  while (!cfg.tile_ch_block && cb > 32 && (long long)ngrp * ceil_div(p.channels, cb) < 2048) cb >>= 1;
  p.ch_block = cb;
  const int nct = ceil_div(p.channels, p.ch_block);
  hipLaunchKernelGGL((roi_align_fwd_tile<TIn, TOut, NT, FUSED>), dim3((unsigned)ngrp * nct), dim3(NT), lds_b, stream, p, K, lds_b, nq_cap, kTileMergePct, (kTileReverse ? 1 : 0) | (p.xcd_remap ? 0 : 2) | (cfg.tile_cb_major ? 4 : 0));
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}

template <typename TIn, typename TOut>
static int launch_tile_t(const RoiAlignParams& p, hipStream_t stream) {
  // 16-bit maps in contract mode (dtc_roi_align_set_exact(0), read at launch time like the C4 kernel's fast mode): fused pooling
  if constexpr (sizeof(TIn) == 2) { if (!roi_align_get_exact()) return launch_tile_nt<TIn, TOut, kTileThreads, true>(p, stream); }
  return launch_tile_nt<TIn, TOut, kTileThreads, false>(p, stream);
}

bool roi_align_tile_supported(const RoiAlignParams& p, int in_dtype, int out_dtype) {
  if (p.sampling_ratio != 2) return false;
  if (p.pooled_h * p.pooled_w > kTileThreads) return false;
  return io_pair_supported(in_dtype, out_dtype);
}

int launch_roi_align_tile(const RoiAlignParams& p, int in_dtype, int out_dtype, hipStream_t stream) {
  if (p.n_rois == 0) return DTC_OK;
  return dispatch_io_pair(in_dtype, out_dtype, [&](auto tin, auto tout) {
    return launch_tile_t<tag_type<decltype(tin)>, tag_type<decltype(tout)>>(p, stream);
  });
}

}  // namespace dtc
