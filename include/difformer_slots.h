/*
 * difformer_slots.h -- C ABI of libdifformer_slots.so: the slot order of the packed schedule of the feature-sliced
 * gcn_conv product (dif_sliced_* of difformer_hip.h), formed and dealt on the MI355X (gfx950).
 *
 * The sliced format stores, per (panel, tile, wave), the 8-step blocks of every round: the largest block count among
 * the 64 lock-step rows of the round's slot, padded so that the counts do not increase from round to round.  `order`
 * (dif_sliced_measure / dif_sliced_emit) decides which rows share a slot and, through the format's own slot arithmetic
 * (slot j * PW + pw on even rounds, j * PW + PW - 1 - pw on odd ones), which slots share a wave.  This call chooses an
 * order that keeps both paddings small; the format, its kernels and its results' meaning do not change.
 *
 * A small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header includes
 * for them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, work enqueued on `stream`
 * only, nothing read or written outside the operands and `workspace_bytes` of the workspace, outputs and workspace
 * unspecified on entry.  Errors of THIS library are read with dif_slots_last_error().
 */
#ifndef DIFFORMER_SLOTS_H
#define DIFFORMER_SLOTS_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_SLOTS_VERSION 1

int dif_slots_version(void);
const char* dif_slots_last_error(void);

/* ---------------------------------------------------------------------------------------
 * dif_sliced_slot_order: order int32 [n_rows], a permutation of 0 .. n_rows - 1 (indices inside the shard
 * [row_begin, row_begin + n_rows) of the CSR rowptr / blkptr over n_src source rows; blkptr may be NULL with one tile),
 * for plan = dif_sliced_plan(n_src, n_rows, F) (G, PW, R and NT are read).  No host synchronisation; two calls on the
 * same input give identical bytes: every tie below is broken by an index.
 *   a. b[row][t] = min((entries of row in tile t + 7) / 8, 4095).  Rows are sorted, stably, by the largest b descending,
 *      then by the bit set of the tiles that reach it (bit t = tile t) ascending.
 *   b. The sorted rows are cut into windows of 1,024 (the last may be shorter); inside a window, slots of 64 rows are
 *      formed one after the other until it is empty: the first row of a slot is the remaining row of the largest
 *      sum_t b (ties: lower row index); each further row is the remaining one with the least
 *      sum_t max(0, b[row][t] - m[t]), m = per-tile maximum of the slot so far (ties: larger sum_t b, then lower row
 *      index).  The rows of a slot keep this order; slots are numbered window by window.
 *   c. Slots are sorted by descending sum_t m[t] (ties: lower slot number; a last slot of fewer than 64 rows goes last)
 *      and cut into R strata of PW.  For round j = R - 1 down to 0, the pairs pw that own a slot position of the round
 *      (j * PW + (j odd ? PW - 1 - pw : pw) < G), in descending order of the sum of their envelope (ties: lower pw), each
 *      take the free slot of stratum j with the least sum_t max(0, m[t] - envelope[pw][t]) (ties: earlier in the
 *      stratum), and envelope[pw] = max(envelope[pw], m).  Envelopes start at zero.  A last slot of fewer than 64 rows
 *      is given to the pair that owns position G - 1 before round R - 1 is dealt.
 *   d. order[position * 64 + i] = i-th row of the slot dealt to that position.
 * Covers NT <= 18 tiles and PW * (32 ceil(NT / 8) + 9) <= 65,536 (DIF_E_SHAPE otherwise), n_rows < 2^28.
 * dif_sliced_slot_order_workspace_bytes: host arithmetic; 0 for arguments the call rejects.
 * ------------------------------------------------------------------------------------- */
int64_t dif_sliced_slot_order_workspace_bytes(int64_t n_rows, const int32_t* plan);
int dif_sliced_slot_order(const int32_t* rowptr, const int32_t* blkptr, int64_t n_src, int64_t row_begin, int64_t n_rows,
                          const int32_t* plan, int32_t* order, void* workspace, int64_t workspace_bytes,
                          dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_SLOTS_H */
