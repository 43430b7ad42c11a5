/*
 * difformer_loss.h -- C ABI of libdifformer_loss.so: the two training losses of the reference's drivers on the MI355X (gfx950),
 * one pass over the logits forward and one pass backward.
 *
 *   node classification/main.py:121-129, main-batch.py:136-140, eval.py:19-29, image and text/main.py:107-109
 *       NLLLoss(log_softmax(out, dim=1)[rows], label[rows])          -> dif_nll_log_softmax_*
 *   the same lines for the multi-label datasets, physical particle/main.py:88
 *       BCEWithLogitsLoss(out[rows], target[rows].float())           -> dif_bce_with_logits_*
 *
 * both with the mean reduction.  Every logit is widened to float64 and the row is evaluated in float64:
 *   NLL   m = max_c x_c,  S' = sum_{c != label} exp(x_c - m),  d = x_label - m (<= 0),
 *         l_r = log1p(S') where d == 0, log(S' + exp(d)) - d otherwise        ( = m + log(sum exp(x - m)) - x_label, no term cancels )
 *   BCE   l   = max(x, 0) - x t + log1p(exp(-|x|)),   l_r = the sum over the row's C columns
 *   loss  = ( sum_r weight_r l_r ) / count
 * `count` is, for NLL, the sum of the weights of the rows whose label is not ignore_index, and for BCE C times the sum of the
 * weights.  The sum runs in float64 in a FIXED order: every workgroup sums a row range that depends on (n, C) only, then one
 * workgroup sums the partials in index order.  There is no floating-point atomic anywhere, so the record and the gradient of
 * two calls on equal operands are bitwise equal.
 *
 * The gradient of the loss in the logits is  weight_r * upstream / count * d l_r / d x,  every factor in float64, rounded ONCE
 * to the logits' type.  Entries that would cancel are formed without a subtraction:
 *   NLL   exp(x_c - m) / S for c != label,  -S' / S at the label column          (S = S' + exp(d))
 *   BCE   -sigmoid(-x) where t == 1,  sigmoid(x) where t == 0,  sigmoid(x) - t for any other target value
 *
 * ROW SELECTION.  `rows` with `rows_kind`:
 *   DIF_LOSS_ROWS_ALL      rows is ignored (may be NULL): every row has weight 1
 *   DIF_LOSS_ROWS_WEIGHTS  rows is int32 [n]: the multiplicity of every row (dif_loss_row_weights makes it from an index);
 *                          values below 0 count as 0
 *   DIF_LOSS_ROWS_MASK     rows is uint8 [n] (a bool tensor): non-zero = weight 1
 *
 * THE RECORD is 32 bytes on the device, 8-byte aligned:
 *   offset 0  float64 loss | offset 8  float32 loss (the float64 value rounded once) | offset 12  unused (written 0)
 *   offset 16 int64 count  | offset 24 int64 invalid
 *
 * EDGE SEMANTICS
 *   - A row of weight 0 (and an NLL row whose label is ignore_index) is not read into the sums: NaN or infinite logits there
 *     change neither the loss nor any other row's gradient, and its gradient row is +0.
 *   - A NaN logit in a selected row gives a NaN loss.  A +inf logit in a selected row gives a NaN loss; a -inf logit gives a
 *     non-finite loss under BCE, and under NLL +inf at the label column -- elsewhere in an NLL row it is a class of
 *     probability 0, as in torch, and the loss stays finite.  In all of these the gradients of the OTHER rows are what they
 *     are without it: the gradient depends on `count`, never on the value of the loss.
 *   - count == 0 (an empty index, an all-zero mask, every label ignored, n == 0) gives a NaN loss, as torch's mean over
 *     nothing, and a gradient of +0 everywhere.
 *   - An NLL label outside [0, C) that is not ignore_index, and an index outside [0, n) (counted by dif_loss_row_weights into
 *     its status word, which the forward takes as `index_status`), are counted in `invalid`, each occurrence once, and make
 *     the loss NaN.  Such a row takes no part in `count` and its gradient row is +0; the other rows get the gradient of the
 *     mean over the valid rows.  Nothing asserts or traps on the device.
 *
 * LAYOUT.  C <= 64: a row goes to a group of W = 1, 2, 4, ... 64 lanes (the smallest power of two >= C), 64 / W rows per
 * wave, reduced across lanes (no LDS).  C > 64: one wave per row, looping over the columns.  Rows need only be aligned to
 * their element (4 bytes for float32, 2 for bfloat16).
 *
 * A small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header includes for
 * them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, leading dimensions in ELEMENTS, work
 * enqueued on `stream` only (no synchronisation, capturable into a hipGraph), nothing read or written outside the operands
 * and `workspace_bytes` of the workspace, outputs and workspace unspecified on entry.  Errors of THIS library are read with
 * dif_loss_last_error().
 *
 * Limits: 1 <= C <= 65,536 (DIF_E_SHAPE), n >= 0, 0 <= m <= 2^31 - 1 (DIF_E_BADARG).
 */
#ifndef DIFFORMER_LOSS_H
#define DIFFORMER_LOSS_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_LOSS_VERSION 1

#define DIF_LOSS_ROWS_ALL 0
#define DIF_LOSS_ROWS_WEIGHTS 1
#define DIF_LOSS_ROWS_MASK 2

#define DIF_LOSS_TARGET_I64 0
#define DIF_LOSS_TARGET_F32 1
#define DIF_LOSS_TARGET_U8 2

#define DIF_LOSS_RECORD_BYTES 32

int dif_loss_version(void);
const char* dif_loss_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Host arithmetic; 0 for a rejected shape.  With W = min(64, the smallest power of two >= C), R = 256 / W rows per workgroup
 * pass and G = min(1,024, max(1, ceil(n / R))) workgroups:
 *   bytes = 24 G rounded up to a multiple of 256
 * (one float64 and two int64 partials per workgroup).  The workspace must be 16-byte aligned.  Only the forward uses one.
 * ------------------------------------------------------------------------------------- */
int64_t dif_loss_workspace_bytes(int64_t n, int C);

/* ---------------------------------------------------------------------------------------
 * index int64 [m] (any order, duplicates allowed) -> weight int32 [n]: how often every row occurs, and status int32 [1]: the
 * number of indices outside [0, n).  Integer atomics only: the result does not depend on the order of execution.  Both
 * outputs are zeroed by the call.  m == 0 or n == 0 are allowed (index / weight may then be NULL).
 * ------------------------------------------------------------------------------------- */
int dif_loss_row_weights(const int64_t* index, int64_t m, int64_t n, int32_t* weight, int32_t* status, dif_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * NLL of log_softmax.  x is [n, C] logits (ldx >= C), label int64 [n], rows / rows_kind as above, index_status NULL or the
 * status word of dif_loss_row_weights (added to `invalid`).  Writes the record.
 * The backward takes the same operands, the forward's record (only `count` is read) and a device pointer to the float32
 * upstream scalar, and writes all n x C elements of grad (ldg >= C) in the logits' type.
 * ------------------------------------------------------------------------------------- */
int dif_nll_log_softmax_fwd_f32(const float* x, int64_t ldx, const int64_t* label, int64_t ignore_index, const void* rows,
                                int rows_kind, const int32_t* index_status, int64_t n, int C, void* record, void* workspace,
                                int64_t workspace_bytes, dif_stream_t stream);
int dif_nll_log_softmax_fwd_bf16(const uint16_t* x, int64_t ldx, const int64_t* label, int64_t ignore_index, const void* rows,
                                 int rows_kind, const int32_t* index_status, int64_t n, int C, void* record, void* workspace,
                                 int64_t workspace_bytes, dif_stream_t stream);
int dif_nll_log_softmax_bwd_f32(const float* x, int64_t ldx, const int64_t* label, int64_t ignore_index, const void* rows,
                                int rows_kind, int64_t n, int C, const void* record, const float* upstream, float* grad,
                                int64_t ldg, dif_stream_t stream);
int dif_nll_log_softmax_bwd_bf16(const uint16_t* x, int64_t ldx, const int64_t* label, int64_t ignore_index, const void* rows,
                                 int rows_kind, int64_t n, int C, const void* record, const float* upstream, uint16_t* grad,
                                 int64_t ldg, dif_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * BCE with logits.  target is [n, C] (ldt >= C elements between rows) of target_type DIF_LOSS_TARGET_I64 / _F32 / _U8, read
 * in that type and widened to float64 (aligned to its element).  Everything else as for the NLL.
 * ------------------------------------------------------------------------------------- */
int dif_bce_with_logits_fwd_f32(const float* x, int64_t ldx, const void* target, int target_type, int64_t ldt, const void* rows,
                                int rows_kind, const int32_t* index_status, int64_t n, int C, void* record, void* workspace,
                                int64_t workspace_bytes, dif_stream_t stream);
int dif_bce_with_logits_fwd_bf16(const uint16_t* x, int64_t ldx, const void* target, int target_type, int64_t ldt,
                                 const void* rows, int rows_kind, const int32_t* index_status, int64_t n, int C, void* record,
                                 void* workspace, int64_t workspace_bytes, dif_stream_t stream);
int dif_bce_with_logits_bwd_f32(const float* x, int64_t ldx, const void* target, int target_type, int64_t ldt, const void* rows,
                                int rows_kind, int64_t n, int C, const void* record, const float* upstream, float* grad,
                                int64_t ldg, dif_stream_t stream);
int dif_bce_with_logits_bwd_bf16(const uint16_t* x, int64_t ldx, const void* target, int target_type, int64_t ldt,
                                 const void* rows, int rows_kind, int64_t n, int C, const void* record, const float* upstream,
                                 uint16_t* grad, int64_t ldg, dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_LOSS_H */
