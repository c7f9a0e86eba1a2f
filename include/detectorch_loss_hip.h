/*
 * detectorch_loss_hip.h -- C ABI of libdetectorch_loss_hip.so: the Fast R-CNN head losses and their gradients for the MI355X
 * (gfx950 / CDNA4).  A third shared library next to libdetectorch_hip.so (include/detectorch_hip.h) and
 * libdetectorch_train_hip.so (include/detectorch_train_hip.h), whose export lists are pinned and do not grow; the conventions
 * are the same:
 *   - DEVICE pointers, caller-owned; nothing is allocated or freed inside,
 *   - kernels are enqueued on the given hipStream_t, the call returns without synchronising,
 *   - the return value is DTC_OK (0) or a negative DTC_E* code of detectorch_hip.h (no exceptions, no printf).
 * Each entry cites the reference code it replaces (paths relative to the detectorch tree).
 */
#ifndef DETECTORCH_LOSS_HIP_H_
#define DETECTORCH_LOSS_HIP_H_

#include "detectorch_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Build identification of the loss library ("gfx950"). */
const char* dtc_loss_target_arch(void);

#define DTC_LOSS_MAX_CLASSES 1024       /* 2 <= C <= 1024 */
#define DTC_LOSS_MAX_ROWS 65536         /* 1 <= N <= 65536 (dtc_fast_rcnn_loss) */
#define DTC_LOSS_MAX_ELEMS 1073741824   /* N * W <= 2^30 (dtc_smooth_l1) */

/* Bytes of workspace dtc_fast_rcnn_loss needs for N rows of C classes (a constant of some 20 KB); 0 for a shape the entry
 * rejects. */
size_t dtc_fast_rcnn_loss_workspace_bytes(int n, int c);

/* The Fast R-CNN head losses, the accuracy and both gradients over N rows: what the reference's training step computes per
 * iteration with
 *   train_fast.py:147      loss_cls  = torch.nn.functional.cross_entropy(cls_score, cls_labels)
 *   train_fast.py:148      loss_bbox = smooth_L1(bbox_pred, bbox_targets, bbox_inside_weights, bbox_outside_weights)
 *                                                                                                   lib/model/loss.py:13-20
 *   train_fast.py:151      acc       = accuracy(cls_score, cls_labels)                              lib/model/loss.py:22-26
 *   train_fast.py:158      loss.backward() as far as cls_score and bbox_pred
 * read from the COMPACT targets that dtc_fast_rcnn_targets (detectorch_train_hip.h) writes, in its padded [B, R] layout viewed
 * as N = B * R rows: the expanded [N, 4C] targets and weights (fast_rcnn_sample_rois.py:139-163) are never formed.
 * Inputs:
 *   cls_score      float32 [N, C]   (rows are only 4-byte aligned for odd C)
 *   labels         int32 [N]        any NEGATIVE value marks an ignored row (the -1 padding rows of dtc_fast_rcnn_targets)
 *   bbox_pred      float32 [N, W], 16-byte aligned; bbox_width W = 4 * C, or 8 (class-agnostic regression)
 *   bbox_targets5  float32 [N, 5] = (class k, dx, dy, dw, dh).  k selects the columns [4k, 4k + 4) of the row; with W == 8 any
 *                  k > 0 selects [4, 8).  The selection is keyed by the TARGET class, not the label, as _expand_bbox_targets keys
 *                  it (with non-default thresholds a background row can carry targets).  k == 0: no box term for the row.
 *   beta           > 0 and finite (DTC_EINVAL otherwise): the reference's default is 1.0
 *   upstream       float32 [2] on the device, or NULL for (1, 1): the factors on d loss_cls and d loss_bbox
 *   bbox_pred and bbox_targets5 may both be NULL (both or none): cross-entropy and accuracy only; loss_bbox is then 0 and
 *   grad_bbox_pred must be NULL.
 * Outputs (each group nullable, not both):
 *   losses          float32 [4] = (loss_cls, loss_bbox, accuracy, n_valid)
 *   grad_cls_score  float32 [N, C] and grad_bbox_pred float32 [N, W] (16-byte aligned): both or none (grad_bbox_pred alone is
 *                   NULL in a cross-entropy-only call).  Written on EVERY row of every call, zeros on ignored rows and
 *                   unselected columns: no memset is needed and a replay over stale buffers is clean.
 * Semantics:
 *   n_valid    the number of rows with label >= 0, counted on the device; the divisor of both means (the reference's
 *              pred.size(0), which only ever sees valid rows).
 *   loss_cls   mean over the valid rows of logsumexp(row) - row[label], computed with the row maximum subtracted (logits of
 *              1e4 do not overflow).
 *   loss_bbox  sum over the valid rows' selected columns of  x = pred - target;  |x| <= beta ? 0.5 x^2 / beta : |x| - 0.5 beta
 *              (inclusive comparison, loss.py:18), divided by n_valid: smooth_L1 with inside and outside weights 1 on the selected
 *              columns and 0 elsewhere.
 *   accuracy   mean over the valid rows of argmax(row) == label.  The argmax is taken over the LOGITS, lowest index among equal
 *              logits.  The reference takes it over softmax(row) (loss.py:24); softmax is monotonic, so the two agree whenever
 *              float32 softmax does not round two DIFFERENT logits to one probability (it can: exp of both may round to the same
 *              value; then the reference reports the lower index and this entry the larger logit).
 *   gradients  what autograd gives the reference's formulas:
 *                grad_cls_score = (softmax(row) - onehot(label)) * upstream[0] / n_valid
 *                grad_bbox_pred = (|x| <= beta ? x / beta : sign(x)) * upstream[1] / n_valid  on the selected columns.
 *   DEPARTURES from the reference, both for inputs it never sees:
 *     n_valid == 0: all four losses and every gradient element are 0 (the reference would divide by zero);
 *     a label >= C, or a target class that is not an integer in [0, C), is NEVER used as an index: the row counts as ignored for
 *     the term it would have indexed (no cross-entropy term, no gradient and no accuracy hit for such a label; no box term for
 *     such a class); a row with label >= C still counts in n_valid.
 *   Inputs on valid rows must be finite: this is not checked.  Ignored rows may hold any bits, NaN included: their cls_score,
 *   bbox_pred and bbox_targets5 are never read.
 *   ANY finite float32 is admitted, denormals included.  Logits: only differences from the row maximum are formed, so a row
 *   may span the whole float32 range as long as max - min is itself a float32 (+-1e38 in one row is); a softmax that is exactly
 *   one-hot gives an exact 0 in the label's column on a hit and exactly -upstream[0] / n_valid on a miss.  Box terms: pred - target,
 *   its square and the quotient by beta are formed in double, where none of them can overflow or vanish for float32 operands
 *   and any float32 beta > 0 (2^-149 and 3e38 included); the results are rounded to float32 once, so a loss beyond the float32
 *   range comes out as inf and a gradient element below the float32 normal range as the device rounds it.
 *   A target class is compared as the float it is: -0.0 is class 0 (no box term); a denormal, any other non-integer (0.999,
 *   C - 0.5), +-inf, NaN and any value >= C (2^24) give no box term and are never converted to an index.
 *   upstream: any two finite floats, 0 and negative ones included; they scale the gradients only (the losses of a call do not
 *   depend on them), a factor 0 gives gradients that compare equal to 0 (the sign of such a zero is not specified; the zeros of
 *   ignored rows and unselected columns are +0.0), and they are read on the device when the kernels run: a graph replay uses the
 *   values that are in the buffer at that time.
 *   Alignment: bbox_pred, grad_bbox_pred and the workspace 16 bytes, as said above; every other pointer (cls_score, labels,
 *   bbox_targets5, upstream, losses, grad_cls_score) needs the 4 bytes of its element type only.  Nothing is written outside the
 *   stated extents of the outputs and the workspace.  A call that returns DTC_EINVAL, DTC_EUNSUPPORTED or DTC_EWORKSPACE has
 *   launched nothing and written nothing.
 * The box terms and every cross-row sum are accumulated in double in a fixed order and rounded once; there are no float atomics:
 * the same inputs give the same bits on every run, eagerly and under graph replay.
 * Limits: 2 <= C <= DTC_LOSS_MAX_CLASSES, 1 <= N <= DTC_LOSS_MAX_ROWS (DTC_EUNSUPPORTED beyond; N < 1 or C < 2: DTC_EINVAL).
 * workspace: dtc_fast_rcnn_loss_workspace_bytes(n, c) bytes, 16-byte aligned (DTC_EWORKSPACE when smaller); any contents; it
 * belongs to ONE call in flight at a time.  Two kernel nodes (the count of the valid rows, which also readies the arrival counter
 * of the second; then the one pass over the rows, whose last workgroup to finish sums the workgroups' partial results in index
 * order), no memset node: capturable in a hipGraph, and a replay picks up inputs rewritten in place.  No workgroup waits for
 * another. */
int dtc_fast_rcnn_loss(const float* cls_score, const int32_t* labels, const float* bbox_pred, const float* bbox_targets5, int n,
                       int c, int bbox_width, float beta, const float* upstream, void* workspace, size_t workspace_bytes,
                       float* losses, float* grad_cls_score, float* grad_bbox_pred, dtc_stream_t stream);

/* Bytes of workspace dtc_smooth_l1 needs when it is asked for the loss (a constant of 8 KB); 0 for a shape the entry rejects. */
size_t dtc_smooth_l1_workspace_bytes(int n, int w);

/* lib/model/loss.py:13-20 smooth_L1(pred, targets, alpha_in, alpha_out, beta) on four float32 [N, W] tensors with any weights,
 * and its gradient with respect to pred (the call surface of the reference's loss module; an RPN box loss has this form too):
 *   x = (pred - targets) * alpha_in;  loss = sum((|x| <= beta ? 0.5 x^2 / beta : |x| - 0.5 beta) * alpha_out) / N
 *   grad_pred = (|x| <= beta ? x / beta : sign(x)) * alpha_in * alpha_out * upstream[0] / N
 * The divisor is N, the row count (pred.size(0)).  Each element is evaluated in double from the float32 inputs and rounded once;
 * the sum is a double sum in a fixed order: reproducible, no atomics.
 *   pred, targets, alpha_in, alpha_out, grad_pred: 16-byte aligned (DTC_EINVAL otherwise); beta > 0 and finite;
 *   loss float32 [1] and / or grad_pred float32 [N, W] (not both NULL); upstream float32 [1] on the device or NULL for 1;
 *   workspace: needed for the loss only (NULL with loss == NULL), dtc_smooth_l1_workspace_bytes(n, w) bytes, 8-byte aligned.
 * N >= 1, W >= 1 (DTC_EINVAL), N * W <= DTC_LOSS_MAX_ELEMS (DTC_EUNSUPPORTED beyond).  Inputs must be finite: not checked.
 * Any finite float32 is admitted for the four inputs and any float32 beta > 0, as for dtc_fast_rcnn_loss: weights of either sign,
 * 0 (an exact-zero gradient element) and of any magnitude; x, x^2 / beta and the products with the weights are formed in double.
 * N * W need not be a multiple of 4 and may be below 4; the row structure only sets the divisor.  loss and grad_pred are the same
 * bits whether they are asked for together or one at a time.  Nothing is written past grad_pred[N * W - 1].
 * One kernel node for the gradient alone, two with the loss (the pass, then the sum of the workgroups' partial results). */
int dtc_smooth_l1(const float* pred, const float* targets, const float* alpha_in, const float* alpha_out, int n, int w, float beta,
                  const float* upstream, void* workspace, size_t workspace_bytes, float* loss, float* grad_pred,
                  dtc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DETECTORCH_LOSS_HIP_H_ */
