// Fast R-CNN training minibatches for gfx950 -- the device form of the reference's host chain (one image at a time, NumPy, inside the
// data loader):
//   merge        lib/data/json_dataset.py:333-394   _merge_proposal_boxes_into_roidb: proposals vs ALL gt, np.argmax, max > 0
//   crowd        lib/data/json_dataset.py:397-414   _filter_crowd_proposals: pycocotools bbIou with iscrowd, > crowd_thresh -> -1
//   assign       lib/data/json_dataset.py:417-435   _add_class_assignments: max_overlaps, max_classes
//   targets      lib/data/roidb.py:176-206          _compute_targets: overlap >= bbox_thresh, argmax among the non-crowd gt
//   sample       lib/utils/fast_rcnn_sample_rois.py:41-137, expansion :139-163
// One launch, one workgroup of 1024 threads per image:
//   1  the image's gt rows go to LDS
//   2  one candidate per thread and round: overlap / class of the candidate (IoU against the gt in LDS through iou_bbox, the pinned
//      bbox_overlaps element), its sampling group, and ONE 64-bit key  group << 44 | rand_key << 12 | index  (pad: neither fg nor bg)
//   3  block_bitonic_sort of the <= 4096 keys: the fg keys in (rand_key, index) order, then the bg keys in that order
//   4  one output row per wavefront and round: the lanes share the IoU-argmax over the non-crowd gt, the deltas are uniform, and the
//      row's expanded blobs leave as 16-byte stores, the zero fill of the other classes and of the rows past n_rois fused.
// No global atomics, no inline assembly, no workspace.
#include <cmath>

#include "block_sort.h"
#include "box_vote.h"
#include "dtc_common.h"
#include "wave_ops.h"

#include "../../../include/detectorch_train_hip.h"

namespace dtc {

constexpr int kTgtThreads = 1024;
constexpr int kTgtWaves = kTgtThreads / 64;
constexpr int kTgtMaxGt = DTC_TRAIN_MAX_GT;
constexpr int kTgtMaxCand = DTC_TRAIN_MAX_GT + DTC_TRAIN_MAX_PROPOSALS;     // 2304 -> 4096 keys, four per thread
constexpr int kTgtMaxKeys = 4096;
constexpr int kTgtIdxBits = 12;                                             // candidate index < 4096
constexpr int kTgtGroupShift = 32 + kTgtIdxBits;                            // bit 44: 0 = fg, 1 = bg

struct TargetsParams {
  const float* gt_boxes; const int32_t* gt_classes; const int32_t* gt_is_crowd; const int32_t* gt_counts;
  const float* proposals; const int32_t* proposal_counts; const float* im_scale; const uint32_t* rand_keys;
  int G, P, R, n_reg, agnostic, fg_quota;
  float fg_thresh, bg_hi, bg_lo, bbox_thresh;
  double crowd_thresh;
  float wx, wy, ww, wh;
  float* rois5; int32_t* labels; float* targets5; float* targets; float* inside; float* outside;
  int32_t* keep_inds; int32_t* n_fg; int32_t* n_rois; float* max_overlaps; int32_t* max_classes;
};

// intersection over the PROPOSAL's area, as pycocotools' bbIou computes it for an iscrowd gt (common/maskApi.c): doubles, boxes as
// (x, y, w, h) whose w = x2 - x1 + 1 was formed in float32 by xyxy_to_xywh (boxes.py:121)
__device__ __forceinline__ double crowd_ioa(float4 D, float4 Gb) {
  const double dx = D.x, dy = D.y, dw = (D.z - D.x) + 1.f, dh = (D.w - D.y) + 1.f;
  const double gx = Gb.x, gy = Gb.y, gw = (Gb.z - Gb.x) + 1.f, gh = (Gb.w - Gb.y) + 1.f;
  const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
  if (w <= 0) return 0.0;
  const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
  if (h <= 0) return 0.0;
  return (w * h) / (dw * dh);
}

__global__ __launch_bounds__(kTgtThreads) void fast_rcnn_targets_kernel(TargetsParams p) {
  __shared__ uint64_t keys[kTgtMaxKeys];
  __shared__ float4 g_box[kTgtMaxGt];
  __shared__ int g_cls[kTgtMaxGt];            // the gt's class; crowd gt: -class (gt classes are > 0)
  __shared__ float c_ov[kTgtMaxCand];         // max_overlaps
  __shared__ int c_cls[kTgtMaxCand];          // max_classes
  __shared__ int n_group[2];                  // keys of group fg; of groups fg + bg
  __shared__ int any_s[2];                    // the image has a non-crowd gt; a crowd gt
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int n_g = p.G > 0 ? min(max(p.gt_counts[b], 0), p.G) : 0;
  const int n_p = p.P > 0 ? min(max(p.proposal_counts[b], 0), p.P) : 0;
  const int n_c = n_g + n_p;
  const float4* props = reinterpret_cast<const float4*>(p.proposals) + (size_t)b * p.P;

  // ---- 1: gt -> LDS
  if (tid < 2) { n_group[tid] = 0; any_s[tid] = 0; }
  __syncthreads();
  if (tid < n_g) {
    g_box[tid] = reinterpret_cast<const float4*>(p.gt_boxes)[(size_t)b * p.G + tid];
    const int cls = p.gt_classes[(size_t)b * p.G + tid];
    const bool crowd = p.gt_is_crowd[(size_t)b * p.G + tid] == 1;          // json_dataset.py:404
    g_cls[tid] = crowd ? -cls : cls;
    any_s[crowd ? 1 : 0] = 1;                                               // every writer stores the same value
  }
  __syncthreads();
  const bool crowd_filter = any_s[1] != 0 && p.crowd_thresh > 0.0;          // json_dataset.py:328, :406
  const bool has_targets = any_s[0] != 0;                                   // roidb.py:185

  // ---- 2: overlap, class and sampling key of every candidate
  const int np2 = next_pow2(n_c);
  for (int c = tid; c < np2; c += kTgtThreads) {
    uint64_t k = kPadKey;
    if (c < n_c) {
      float ov;
      int cls;
      if (c < n_g) {                           // a gt row: 1.0 at its class, -1 across a crowd row (argmax of a constant row: 0)
        const int gc = g_cls[c];
        ov = gc > 0 ? 1.f : -1.f;
        cls = gc > 0 ? gc : 0;
      } else {
        const float4 q = props[c - n_g];
        float best = 0.f;
        int arg = 0;
        bool bad = false;
        for (int j = 0; j < n_g; j++) {
          const float4 gb = g_box[j];
          const float v = iou_bbox(q, gb);                                  // bbox_overlaps(boxes = proposals, query = gt)
          if (j == 0 || v > best) { best = v; arg = j; }                    // np.argmax: the first maximum
          if (crowd_filter && g_cls[j] < 0) bad |= crowd_ioa(q, gb) > p.crowd_thresh;
        }
        ov = 0.f; cls = 0;
        if (n_g > 0 && best > 0.f) { ov = best; cls = abs(g_cls[arg]); }    // json_dataset.py:364-366
        if (bad) { ov = -1.f; cls = 0; }                                    // :413
      }
      c_ov[c] = ov;
      c_cls[c] = cls;
      const bool fg = ov >= p.fg_thresh;                                    // fast_rcnn_sample_rois.py:62
      const bool bg = ov < p.bg_hi && ov >= p.bg_lo;                        // :73-76
      if (fg || bg)
        k = ((uint64_t)(fg ? 0 : 1) << kTgtGroupShift) | ((uint64_t)p.rand_keys[(size_t)b * (p.G + p.P) + c] << kTgtIdxBits) |
            (uint64_t)c;
    }
    keys[c] = k;
  }
  if (p.max_overlaps) {
    for (int c = tid; c < p.G + p.P; c += kTgtThreads) {
      // (c_ov / c_cls of this thread's own candidates: c strides by the block size in both loops)
      p.max_overlaps[(size_t)b * (p.G + p.P) + c] = c < n_c ? c_ov[c] : 0.f;
      p.max_classes[(size_t)b * (p.G + p.P) + c] = c < n_c ? c_cls[c] : 0;
    }
  }

  // ---- 3: sort; the group boundaries are where the group bits of neighbouring keys differ
  block_bitonic_sort<kTgtThreads>(keys, np2);                               // barriers inside, before and after
  for (int i = tid; i < np2; i += kTgtThreads) {
    const uint32_t gi = (uint32_t)(keys[i] >> kTgtGroupShift);
    const uint32_t gn = i + 1 < np2 ? (uint32_t)(keys[i + 1] >> kTgtGroupShift) : 0xffffffffu;
    if (gi == 0 && gn != 0) n_group[0] = i + 1;
    if (gi <= 1 && gn > 1) n_group[1] = i + 1;
  }
  __syncthreads();
  const int n_fg_all = n_group[0], n_bg_all = n_group[1] - n_group[0];
  const int fg_take = min(p.fg_quota, n_fg_all);                            // fast_rcnn_sample_rois.py:65
  const int bg_take = min(p.R - fg_take, n_bg_all);                         // :79-80
  const int n_rois = fg_take + bg_take;
  if (tid == 0) { p.n_fg[b] = fg_take; p.n_rois[b] = n_rois; }

  // ---- 4: the output rows, one per wavefront and round
  const float s = p.im_scale[b];
  for (int r = wv; r < p.R; r += kTgtWaves) {
    const size_t row = (size_t)b * p.R + r;
    int keep = -1, label = -1, tcls = 0;
    float4 box = make_float4(0.f, 0.f, 0.f, 0.f), d = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < n_rois) {                                                       // uniform in the wavefront
      const uint64_t k = keys[r < fg_take ? r : n_fg_all + (r - fg_take)];
      keep = (int)(k & ((1u << kTgtIdxBits) - 1u));
      box = keep < n_g ? g_box[keep] : props[keep - n_g];
      const int mc = c_cls[keep];
      label = r < fg_take ? mc : 0;                                         // :90-91
      if (has_targets && c_ov[keep] >= p.bbox_thresh) {                     // roidb.py:190
        tcls = p.agnostic ? 1 : mc;                                         // :203-204
        // the first IoU maximum among the non-crowd gt: a wave-wide maximum of (IoU bits, ~index)
        uint64_t bk = 0;
        for (int j = lane; j < n_g; j += 64) {
          if (g_cls[j] < 0) continue;
          const uint64_t kk = ((uint64_t)float_to_ordered(iou_bbox(box, g_box[j])) << 32) | (uint32_t)(0xffffffffu - (uint32_t)j);
          bk = kk > bk ? kk : bk;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const uint64_t o = (uint64_t)__shfl_xor((long long)bk, off, 64);
          bk = o > bk ? o : bk;
        }
        const float4 gt = g_box[0xffffffffu - (uint32_t)bk];
        // bbox_transform_inv (boxes.py:224-238), float32, one rounding per operation
        const float ew = (box.z - box.x) + 1.f, eh = (box.w - box.y) + 1.f;
        const float ecx = box.x + 0.5f * ew, ecy = box.y + 0.5f * eh;
        const float gw = (gt.z - gt.x) + 1.f, gh = (gt.w - gt.y) + 1.f;
        const float gcx = gt.x + 0.5f * gw, gcy = gt.y + 0.5f * gh;
        d.x = fdiv(p.wx * (gcx - ecx), ew);
        d.y = fdiv(p.wy * (gcy - ecy), eh);
        d.z = p.ww * (float)log((double)fdiv(gw, ew));
        d.w = p.wh * (float)log((double)fdiv(gh, eh));
      }
    }
    if (lane < 5) {
      // lane 0: the batch index / the target class; lanes 1-4: box * im_scale (fast_rcnn_sample_rois.py:112-114) / the deltas
      const float bv = lane == 1 ? box.x : lane == 2 ? box.y : lane == 3 ? box.z : box.w;
      const float tv = lane == 1 ? d.x : lane == 2 ? d.y : lane == 3 ? d.z : d.w;
      p.rois5[row * 5 + lane] = lane == 0 ? (float)b : r < n_rois ? bv * s : 0.f;
      p.targets5[row * 5 + lane] = lane == 0 ? (float)tcls : tv;
    }
    if (lane == 0) { p.labels[row] = label; p.keep_inds[row] = keep; }
    if (p.targets) {                                                        // _expand_bbox_targets: slot k of the row is class k
      float4* t = reinterpret_cast<float4*>(p.targets) + row * p.n_reg;
      float4* wi = reinterpret_cast<float4*>(p.inside) + row * p.n_reg;
      float4* wo = reinterpret_cast<float4*>(p.outside) + row * p.n_reg;
      for (int k = lane; k < p.n_reg; k += 64) {
        const float m = tcls > 0 && k == tcls ? 1.f : 0.f;                  // :156-162 (a class >= n_reg has no slot: nothing is written)
        t[k] = make_float4(m != 0.f ? d.x : 0.f, m != 0.f ? d.y : 0.f, m != 0.f ? d.z : 0.f, m != 0.f ? d.w : 0.f);
        wi[k] = make_float4(m, m, m, m);
        wo[k] = make_float4(m, m, m, m);                                    // :107 inside > 0
      }
    }
  }
}

}  // namespace dtc

DTC_API const char* dtc_train_target_arch(void) { return "gfx950"; }

DTC_API int dtc_fast_rcnn_targets(const float* gt_boxes, const int32_t* gt_classes, const int32_t* gt_is_crowd, const int32_t* gt_counts,
                                  const float* proposals, const int32_t* proposal_counts, const float* im_scale,
                                  const uint32_t* rand_keys, int batch, int gt_stride, int proposal_stride,
                                  const dtc_train_params* params, float* rois5, int32_t* labels, float* bbox_targets5,
                                  float* bbox_targets, float* bbox_inside_weights, float* bbox_outside_weights, int32_t* keep_inds,
                                  int32_t* n_fg, int32_t* n_rois, float* max_overlaps, int32_t* max_classes, dtc_stream_t stream) {
  // shapes and parameters
  if (batch < 0 || gt_stride < 0 || proposal_stride < 0 || (int64_t)gt_stride + proposal_stride < 1 || !params) return DTC_EINVAL;
  const dtc_train_params& q = *params;
  if (q.rois_per_image < 1 || q.num_classes < 2) return DTC_EINVAL;
  if (!std::isfinite(q.fg_fraction) || q.fg_fraction < 0.0 || q.fg_fraction > 1.0 || !std::isfinite(q.crowd_thresh) ||
      !std::isfinite(q.fg_thresh) || !std::isfinite(q.bg_thresh_hi) || !std::isfinite(q.bg_thresh_lo) || !std::isfinite(q.bbox_thresh) ||
      q.bg_thresh_hi > q.fg_thresh)
    return DTC_EINVAL;
  for (int i = 0; i < 4; i++)
    if (!std::isfinite(q.reg_weights[i])) return DTC_EINVAL;
  if (batch == 0) return DTC_OK;
  // limits
  if (gt_stride > DTC_TRAIN_MAX_GT || proposal_stride > DTC_TRAIN_MAX_PROPOSALS || q.rois_per_image > DTC_TRAIN_MAX_ROIS)
    return DTC_EUNSUPPORTED;
  // pointers
  if (gt_stride > 0 && (!gt_boxes || !gt_classes || !gt_is_crowd || !gt_counts)) return DTC_EINVAL;
  if (proposal_stride > 0 && (!proposals || !proposal_counts)) return DTC_EINVAL;
  if (!im_scale || !rand_keys || !rois5 || !labels || !bbox_targets5 || !keep_inds || !n_fg || !n_rois) return DTC_EINVAL;
  const int n_exp = (bbox_targets != nullptr) + (bbox_inside_weights != nullptr) + (bbox_outside_weights != nullptr);
  if ((n_exp != 0 && n_exp != 3) || (max_overlaps != nullptr) != (max_classes != nullptr)) return DTC_EINVAL;
  const uintptr_t al = reinterpret_cast<uintptr_t>(gt_boxes) | reinterpret_cast<uintptr_t>(proposals) |
                       reinterpret_cast<uintptr_t>(bbox_targets) | reinterpret_cast<uintptr_t>(bbox_inside_weights) |
                       reinterpret_cast<uintptr_t>(bbox_outside_weights);
  if ((al & 15) != 0) return DTC_EINVAL;

  dtc::TargetsParams p;
  p.gt_boxes = gt_boxes; p.gt_classes = gt_classes; p.gt_is_crowd = gt_is_crowd; p.gt_counts = gt_counts;
  p.proposals = proposals; p.proposal_counts = proposal_counts; p.im_scale = im_scale; p.rand_keys = rand_keys;
  p.G = gt_stride; p.P = proposal_stride; p.R = q.rois_per_image;
  p.agnostic = q.cls_agnostic_bbox_reg != 0;
  p.n_reg = p.agnostic ? 2 : q.num_classes;                                 // fast_rcnn_sample_rois.py:149-151
  p.fg_quota = (int)std::nearbyint(q.fg_fraction * (double)q.rois_per_image);   // :58 np.round: half to even (the default rounding mode)
  p.fg_thresh = q.fg_thresh; p.bg_hi = q.bg_thresh_hi; p.bg_lo = q.bg_thresh_lo; p.bbox_thresh = q.bbox_thresh;
  p.crowd_thresh = q.crowd_thresh;
  p.wx = q.reg_weights[0]; p.wy = q.reg_weights[1]; p.ww = q.reg_weights[2]; p.wh = q.reg_weights[3];
  p.rois5 = rois5; p.labels = labels; p.targets5 = bbox_targets5; p.targets = bbox_targets; p.inside = bbox_inside_weights;
  p.outside = bbox_outside_weights; p.keep_inds = keep_inds; p.n_fg = n_fg; p.n_rois = n_rois; p.max_overlaps = max_overlaps;
  p.max_classes = max_classes;
  hipLaunchKernelGGL(dtc::fast_rcnn_targets_kernel, dim3(batch), dim3(dtc::kTgtThreads), 0, reinterpret_cast<hipStream_t>(stream), p);
  DTC_CHECK_LAUNCH();
  return DTC_OK;
}
