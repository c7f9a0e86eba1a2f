/*
 * detectorch_optim_hip.h -- C ABI of libdetectorch_optim_hip.so: the optimizer tail of the training step for the MI355X (gfx950 /
 * CDNA4): gradient clipping by the global norm fused with momentum SGD.
 * A fifth shared library next to libdetectorch_hip.so (include/detectorch_hip.h), libdetectorch_train_hip.so
 * (include/detectorch_train_hip.h), libdetectorch_loss_hip.so (include/detectorch_loss_hip.h) and libdetectorch_grad_hip.so
 * (include/detectorch_grad_hip.h), whose export lists are pinned and do not grow; the conventions are the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf).
 * It replaces the last lines of the reference's loop (paths relative to the detectorch tree):
 *   train_fast.py:165   clip_grad_norm(parameters, max_norm=35, norm_type=2)
 *   train_fast.py:166   optimizer.step() of torch.optim.SGD(lr, momentum=0.9, weight_decay=1e-4)   (train_fast.py:93-96)
 */
#ifndef DETECTORCH_OPTIM_HIP_H_
#define DETECTORCH_OPTIM_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the optimizer library ("gfx950"). */
const char* dtc_optim_target_arch(void);

#define DTC_SGD_MAX_TENSORS 16384           /* 1 <= n_tensors <= 2^14                                   DTC_EUNSUPPORTED */
#define DTC_SGD_MAX_ELEMENTS 1073741824     /* 1 <= n <= 2^30 elements in one tensor                    DTC_EUNSUPPORTED */
#define DTC_SGD_MAX_TOTAL 17179869184       /* at most 2^34 elements over all tensors of a call         DTC_EUNSUPPORTED */
#define DTC_SGD_MAX_GROUPS 64               /* 1 <= n_groups <= 64                                      DTC_EUNSUPPORTED */
#define DTC_SGD_CHUNK 4096                  /* the smallest chunk, in elements; a plan's chunks hold DTC_SGD_CHUNK << k */
#define DTC_SGD_BODY_CHUNKS 2048            /* k is the least one with ceil(total / chunk) <= 2048, so that
                                               n_chunks <= n_tensors + DTC_SGD_BODY_CHUNKS whatever the sizes are */
#define DTC_SGD_SKIP_NONFINITE 1            /* flags of dtc_sgd_step */

/* One parameter tensor of a step, on the HOST: dense float32 arrays of n elements on the device, each 4-byte aligned (views of a
 * flat buffer are fine, and the three may be misaligned differently).  group: the row of group_hyper with its lr and wd. */
typedef struct dtc_sgd_tensor {
  float* p;          /* the parameter, updated in place */
  const float* g;    /* its gradient, READ ONLY: never written (see below) */
  float* buf;        /* its momentum buffer, updated in place */
  int64_t n;
  int32_t group;
  int32_t _pad;
} dtc_sgd_tensor;

/* Bytes of HOST buffer dtc_sgd_plan needs for tensors of counts[0 .. n_tensors) elements: 32 per tensor and 16 per chunk, for
 * n_tensors + min(ceil(total / DTC_SGD_CHUNK), DTC_SGD_BODY_CHUNKS) chunks, which no plan of these tensors exceeds.  A bound and not
 * the table's own size, so that it is monotone in n_tensors and in every count (the chunk count itself drops where the chunk
 * doubles).  0 for arguments dtc_sgd_plan rejects (counts NULL, a count or n_tensors outside its limits). */
size_t dtc_sgd_plan_bytes(int n_tensors, const int64_t* counts);

/* Pure HOST function (no HIP call): turns records[0 .. n_tensors) into the table dtc_sgd_step reads, written to the HOST buffer
 * plan_out; the caller uploads its first 32 * n_tensors + 16 * *n_chunks bytes as they are (16-byte aligned on the device), the rest
 * of plan_out is not written.  The table is n_tensors records
 * {p, g, buf, uint32 n, int32 group} followed by *n_chunks records {uint32 tensor, offset, count, 0}: chunk c is elements
 * [offset, offset + count) of its tensor, one workgroup's share.  The chunks run through the tensors in order, never cross a
 * tensor, and cover every element exactly once; all but a tensor's last hold DTC_SGD_CHUNK << k elements (above).
 * Return codes, checked in this order; on any of them plan_out and *n_chunks are untouched:
 *   shapes     DTC_EINVAL: records or n_chunks NULL, n_tensors < 1, n_groups < 1, a record with n < 1 or group outside
 *              [0, n_groups)
 *   limits     DTC_EUNSUPPORTED: the DTC_SGD_MAX_* above
 *   pointers   DTC_EINVAL: a p, g or buf that is NULL or not 4-byte aligned; any two of the 3 * n_tensors arrays overlapping;
 *              plan_out NULL
 *   workspace  DTC_EWORKSPACE: plan_bytes < dtc_sgd_plan_bytes(n_tensors, the records' counts) */
int dtc_sgd_plan(const dtc_sgd_tensor* records, int n_tensors, int n_groups, void* plan_out, size_t plan_bytes, int* n_chunks);

/* Bytes of workspace dtc_sgd_step needs: one double per chunk, rounded up to 16.  Monotone; 0 for n_chunks outside
 * [1, DTC_SGD_MAX_TENSORS + DTC_SGD_BODY_CHUNKS]. */
size_t dtc_sgd_workspace_bytes(int n_chunks);

/* One optimizer step over every tensor of the plan.  Per element, all in float32, each operation rounded once, nothing
 * contracted (the library is built with -ffp-contract=off):
 *     gc  = g * coef
 *     d   = gc + wd * p            (wd * p rounded, then the add)
 *     buf = momentum * buf + d     (momentum * buf rounded, then the add)
 *     p   = p - lr * buf           (lr * buf rounded, then the subtract)
 * with coef = min(1, max_norm / (total_norm + 1e-6f)) in float32 (a NaN quotient stays NaN), and total_norm the float32 rounding
 * of sqrt(sum g^2) over every tensor of the call: the squares and their sum in double (a float32 square is exact in double), the
 * sum in a FIXED order that depends on the plan alone.  No float atomics, nobody waits on another workgroup: the same inputs give
 * the same bits on every run, eagerly and under graph replay.  Denormal products and sums are kept.
 * Differences from the reference's formulation that a caller can observe:
 *   - GRADIENTS ARE NOT WRITTEN: g stays unclipped, the clip factor is applied on the fly (clip_grad_norm scales .grad in place);
 *   - momentum buffers START AS ZEROS and the first step uses the general formula (torch clones d instead): the values are equal,
 *     only a -0.0 in d becomes +0.0 in buf;
 *   - the norm is accumulated in DOUBLE: denormal gradients give a non-zero norm where float32 squaring would underflow; coef is
 *     1 either way;
 *   - flags & DTC_SGD_SKIP_NONFINITE: when total_norm is NaN or inf the call leaves every p and buf untouched and reports it in
 *     stats[2].  Without the flag the formula is applied as written (what torch does): inf gives coef = 0, NaN propagates;
 *   - no dampening and no Nesterov momentum (the reference uses neither).
 * Inputs:
 *   plan_dev         the table of dtc_sgd_plan on the DEVICE, 16-byte aligned; plan_bytes, n_tensors and n_chunks as dtc_sgd_plan
 *                    gave them (plan_bytes == 32 * n_tensors + 16 * n_chunks)
 *   group_hyper_dev  float32 [n_groups][2] = (lr, wd) on the DEVICE: read by the kernels, so a captured graph sees a learning
 *                    rate that was changed in place.  n_groups is the plan's
 *   momentum         in [0, 1); max_norm > 0, +inf allowed (clipping off, the norm still reported)
 * Output: stats float32 [4] = (total_norm, coef, nonfinite (1.0 when total_norm is NaN or inf, else 0.0), 0).
 * Two kernel nodes (the norm pass: one double per chunk into the workspace; the update pass: every workgroup sums the partials
 * itself, then streams its chunk) and no memset node.  16-byte loads and stores where p, g and buf of a chunk are misaligned
 * alike, dword accesses otherwise.  No host synchronisation, no allocation.
 * Return codes, checked in this order, and on any of them nothing was launched and no byte was written:
 *   shapes     DTC_EINVAL: n_tensors < 1, n_chunks < n_tensors, n_groups < 1, plan_bytes != 32 * n_tensors + 16 * n_chunks,
 *              max_norm <= 0 or NaN, momentum outside [0, 1) or NaN, unknown flags
 *   limits     DTC_EUNSUPPORTED: n_tensors > DTC_SGD_MAX_TENSORS, n_chunks > n_tensors + DTC_SGD_BODY_CHUNKS,
 *              n_groups > DTC_SGD_MAX_GROUPS
 *   pointers   DTC_EINVAL: plan_dev, group_hyper_dev or stats NULL; plan_dev or the workspace not 16-byte aligned;
 *              group_hyper_dev or stats not 4-byte aligned
 *   workspace  DTC_EWORKSPACE: NULL, or smaller than dtc_sgd_workspace_bytes(n_chunks)
 * The workspace needs no clearing and may hold anything; workspace, stats and the plan belong to ONE call in flight at a time
 * (calls on one stream are in order). */
int dtc_sgd_step(const void* plan_dev, size_t plan_bytes, int n_tensors, int n_chunks, const float* group_hyper_dev, int n_groups,
                 float momentum, float max_norm, int flags, void* workspace, size_t workspace_bytes, float* stats,
                 dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_OPTIM_HIP_H_ */
