/*
 * difformer_metrics.h -- C ABI of libdifformer_metrics.so: the evaluation metrics of the reference's drivers on the MI355X
 * (gfx950), as exact integers.
 *
 * `node classification/data_utils.py:238-285` (copied in `image and text/data_utils.py:180-216`) evaluates on the host:
 * eval_rocauc loops over the label columns with one sklearn roc_auc_score each, eval_acc / eval_f1 take an argmax and count.
 * This library returns the integers those results are quotients of; the host divides.  No floating-point value is
 * accumulated anywhere, so the results are bitwise reproducible.
 *
 * A small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header includes
 * for them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, leading dimensions in ELEMENTS,
 * work enqueued on `stream` only, nothing read or written outside the operands and `workspace_bytes` of the workspace,
 * outputs and workspace unspecified on entry.  Errors of THIS library are read with dif_metrics_last_error().
 */
#ifndef DIFFORMER_METRICS_H
#define DIFFORMER_METRICS_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_METRICS_VERSION 1

int dif_metrics_version(void);
const char* dif_metrics_last_error(void);

/* ---------------------------------------------------------------------------------------
 * ROC-AUC of C label columns in one pass.
 *
 * score is [n, C] float32 (lds = elements between consecutive rows, >= C; 4-byte aligned).  cls is [n, C] uint8 class
 * codes (ldc >= C): 0 = negative, 1 = positive, 2 = unlabelled, 3 (or more) = any other label value.  Scores are compared
 * as float32 values, so -0.0 == +0.0.  An element with code 0 or 1 whose score is NaN or +-inf, and every element with a
 * code above 2, is INVALID; unlabelled and invalid elements count as neither negative nor positive.
 *
 * counts is int64 [C, 5] (dense, 8-byte aligned): per column {P, N, unlabelled, invalid, U2} with P / N the valid
 * positives / negatives (P + N + unlabelled + invalid == n) and
 *   U2 = sum over positives p of ( 2 #{negatives with score < s_p} + #{negatives with score == s_p} ),
 * the Mann-Whitney statistic with mid-ranks: roc_auc_score == U2 / (2 P N) wherever P, N > 0.  U2 <= n^2 / 2.
 *
 * The columns are sorted together (a stable radix sort of n C (key, payload) pairs: four passes on the score, then
 * ceil(log2(C) / 8) on the column), tie groups are found by comparing neighbours, and three prefix sums give every group
 * its share of U2 in constant work per element, whatever the length of the group.
 *
 * Limits: 1 <= C <= 65,536 (DIF_E_SHAPE), 1 <= n (DIF_E_BADARG), n C <= 2^31 - 1 (DIF_E_RANGE: cut the columns into groups).
 *
 * dif_rocauc_workspace_bytes is host arithmetic (0 for a rejected shape).  With m = n C, r = min(64, max(8, ceil(m /
 * 262,144))), t = 256 ceil(m / (64 r)), s = max(m, t) and A(x) = x rounded up to a multiple of 256:
 *   bytes = 5 A(4 m) + A(4 t) + A(4 (ceil(s / 1,024) + 1)) + 256
 * -- 20 to 22 bytes per pair.  The workspace must be 16-byte aligned.
 * ------------------------------------------------------------------------------------- */
int64_t dif_rocauc_workspace_bytes(int64_t n, int C);
int dif_rocauc_counts_f32(const float* score, int64_t lds, const uint8_t* cls, int64_t ldc, int64_t n, int C, int64_t* counts,
                          void* workspace, int64_t workspace_bytes, dif_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * Accuracy count.  pred is [n, K] float32 (ldp >= K elements between rows; 4-byte aligned), 1 <= K <= 65,536.  The
 * prediction of a row is the FIRST index of its largest value; NaN counts as larger than every number and the first NaN
 * wins (torch.argmax, numpy.argmax).  label is int64 [n], labelled uint8 [n] (non-zero = the row takes part).
 * out is int64 [2] = {rows with labelled != 0 and label == prediction, rows with labelled != 0}.  No workspace.
 * ------------------------------------------------------------------------------------- */
int dif_argmax_correct_f32(const float* pred, int64_t ldp, const int64_t* label, const uint8_t* labelled, int64_t n, int K,
                           int64_t* out, dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_METRICS_H */
