/*
 * detectorch_kps_hip.h -- C ABI of libdetectorch_kps_hip.so: keypoint inference on the batched path of the MI355X (gfx950 / CDNA4).
 * The keypoint head's K heatmaps of S x S logits per detection become K keypoints (x, y, logit, prob) per detection in image
 * coordinates.  The reference has no keypoint code: the rule is Detectron's utils/keypoints.py:heatmaps_to_keypoints with OpenCV's
 * cv2.resize(INTER_CUBIC), restated from their published sources in tests/kps_ref.py and below; parity with cv2 and with Detectron
 * themselves is unpinned (tests/README_keypoints.md).  The resized map, up to 4096 x 4096 values per keypoint, never exists in
 * memory.
 * A fourteenth shared library next to libdetectorch_hip.so and the twelve other side libraries, whose export lists are pinned and do
 * not grow; no other library exports a name that starts with dtc_kps_.  The conventions are those of detectorch_aug_hip.h:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside; the workspace is the caller's, sized by
 *     dtc_kps_workspace_bytes and 16-byte aligned,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf), checked in the order
 *     shapes and parameters, limits, pointers, workspace; a call that returns DTC_EINVAL, DTC_EUNSUPPORTED or DTC_EWORKSPACE has
 *     enqueued nothing and written nothing; DTC_ELAUNCH is the runtime refusing a launch,
 *   - the entry is THREE kernel nodes whatever the inputs hold and can be captured in a hipGraph after one eager call; a replay
 *     picks up inputs rewritten in place (person_class and min_size are baked into the captured kernel arguments),
 *   - EVERY output element is written exactly once on every call,
 *   - no count, class or coordinate read from the device is used as an address or as a loop bound before it is checked: counts are
 *     clamped to max_out, a side is at most DTC_KPS_MAX_SIDE,
 *   - no atomics; every sum is taken in a fixed order: the same bits on every run.
 */
#ifndef DETECTORCH_KPS_HIP_H_
#define DETECTORCH_KPS_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 0. Build identification of the keypoint library ("gfx950"). */
const char* dtc_kps_target_arch(void);

#define DTC_KPS_MAX_MAP 64               /* S */
#define DTC_KPS_MAX_KEYPOINTS 64         /* K */
#define DTC_KPS_MAX_OUT 4096             /* max_out */
#define DTC_KPS_MAX_BATCH 65535          /* B */
#define DTC_KPS_MAX_MAPS (1 << 20)       /* B max_out K: the grid of the two map kernels is DTC_KPS_BANDS workgroups per map */
#define DTC_KPS_MAX_SIDE 4096            /* Wr, Hr: a row with a larger resized side is refused (status -1) */
#define DTC_KPS_BANDS 8                  /* row bands per resized map, one workgroup each */
#define DTC_KPS_MIN_BAND 32              /* a band is max(ceil(Hr / 8), 32) rows: small maps use fewer bands */

/* 1. The workspace of dtc_kps_heatmaps_to_keypoints in bytes: per map and band one (maximum, position) pair and one float64 sum.
 * 0 for a shape the entry refuses. */
size_t dtc_kps_workspace_bytes(int batch, int max_out, int K);

/* 2. heatmaps_to_keypoints.  heatmaps float32 [B max_out, K, S, S] keypoint logits, row b max_out + d belongs to detection (b, d);
 * dets float32 [B, max_out, 6] = (x1, y1, x2, y2, score, class) as dtc_postprocess_detections writes them; det_count int32 [B]
 * (clamped to [0, max_out]); person_class >= 0: only rows whose class column equals it, -1: every row below the count; min_size:
 * KRCNN.INFERENCE_MIN_SIZE, 0: off.  Outputs: keyps float32 [B, max_out, 4, K] = x, y, logit, prob; kp_status int32 [B, max_out].
 *
 * Row (b, d) is, in this order,
 *   status 0, zeros   d >= min(det_count[b], max_out), or person_class >= 0 and dets[b, d, 5] != (float)person_class;
 *   status -1, zeros  one of x1, y1, x2, y2 is not finite, or a resized side (below) exceeds DTC_KPS_MAX_SIDE;
 *   status 1          otherwise.  The heatmaps of a row that is not status 1 are never read.
 * Per status-1 row, float32 unless said otherwise, one rounding per operation (-ffp-contract=off):
 *   w = max(x2 - x1, 1), h = max(y2 - y1, 1); Wr = (int)ceil(w), Hr = (int)ceil(h), each raised to min_size when min_size > 0;
 *   wc = w / (float)Wr, hc = h / (float)Hr.
 *   Each S x S map is resized to Hr x Wr (shrinking too: no anti-aliasing).  For destination index d of an axis of n_dst:
 *     f = (float)((d + 0.5) * ((double)S / n_dst) - 0.5), in double, cast once; s = floor(f); t = f - (float)s;
 *     taps s-1 .. s+2, each clamped to [0, S-1] (t is not reset at a border); with A = -0.75f and u = 1 - t
 *       c0 = ((A*(t+1) - 5A)*(t+1) + 8A)*(t+1) - 4A     c1 = ((A+2)*t - (A+3))*t*t + 1
 *       c2 = ((A+2)*u - (A+3))*u*u + 1                   c3 = 1 - c0 - c1 - c2
 *   horizontal first, H[x] = ((p0*c0 + p1*c1) + p2*c2) + p3*c3 per source row, then the same over H with the row weights.
 *   pos = the first row-major index of the maximum of the resized map, a NaN counting as the maximum and the first NaN winning
 *   (np.argmax); x_int = pos % Wr, y_int = pos / Wr;
 *   x = (float)((x_int + 0.5) * (double)wc + (double)x1), y likewise with hc and y1: in double, rounded once;
 *   logit = the resized value at pos, bit for bit;
 *   prob = (float)(1.0 / sum (double)(float)exp((double)(float)(v - logit))) over all Hr Wr resized values v: the subtraction in
 *   float32, exp evaluated in double and rounded to float32, the float32 terms added IN DOUBLE: per lane in visiting order, then a
 *   64 -> 1 halving tree, the wavefronts and then the bands in increasing order.  A term with v - logit < -104 rounds to 0 and is
 *   skipped.
 * Limits: 1 <= S <= 64, 1 <= K <= 64, 1 <= max_out <= 4096, 1 <= B <= 65535, B max_out K <= 2^20, 0 <= min_size <= 4096, person_class
 * >= -1: DTC_EUNSUPPORTED beyond the upper limits, DTC_EINVAL below the lower ones.  keyps and the workspace 16-byte aligned.
 * Three kernel nodes.  (1) and (2) run DTC_KPS_BANDS workgroups of four wavefronts per map: a workgroup stages the source rows its
 * band of resized rows reads in LDS, a lane owns a column of a 64-column strip and walks down the band's rows with the four
 * horizontal results it needs in registers; (1) leaves the band's (maximum, first position), (2) -- which needs the map's maximum
 * and recomputes the values -- the band's sum.  (3) folds the bands and writes every element of both outputs. */
int dtc_kps_heatmaps_to_keypoints(const float* heatmaps, const float* dets, const int32_t* det_count, int batch, int max_out, int K,
                                  int S, int person_class, int min_size, void* workspace, size_t workspace_bytes, float* keyps,
                                  int32_t* kp_status, dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_KPS_HIP_H_ */
