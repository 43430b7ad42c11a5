/*
 * difformer_maps.h -- C ABI of libdifformer_maps.so: streaming top-k attention maps for the DIFFormer layer on the
 * MI355X (gfx950).
 *
 * The reference exposes its attention maps as dense [N, L, H] tensors (`full_attention_conv(..., output_attn=True)`,
 * `DIFFormer.get_attentions`; node classification/difformer.py:42-43, :47-55, :211-226).  What a user reads off such a
 * map is, per node and head, the few keys it attends to most; this library returns exactly those without the N x L
 * tensor ever existing.
 *
 * A second, small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header
 * includes for them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, rows 16-byte
 * aligned, leading dimensions in ELEMENTS, work enqueued on `stream` only, nothing read or written outside the operands
 * and `workspace_bytes` of the workspace, outputs and workspace unspecified on entry.  Errors of THIS library are read
 * with dif_maps_last_error().
 */
#ifndef DIFFORMER_MAPS_H
#define DIFFORMER_MAPS_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_MAPS_VERSION 1

int dif_maps_version(void);
const char* dif_maps_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Top-k of every row of a score matrix that is never stored.
 *
 * q is [n_q, H, M], k is [n_k, H, M] (float32; ldq / ldk = elements between consecutive rows, multiples of 4).
 * s[n, l, h] = q[n, h, :] . k[l, h, :] on the fp32 matrix core.  Per (n, h) the `topk` largest entries over l are
 * returned in descending order under ONE total order: the larger ranking key first, among equal keys the lower l
 * first; a NaN score ranks below every number.  1 <= topk <= min(n_k, 32), M % 4 == 0, M <= 512.
 *   mode 0  ranking key and value are s itself.  (`simple`, difformer.py:20-21,32-38,43: the caller folds
 *           1 / (|q| |k| den[n, h]) into the rows of q beforehand, so s IS the attention weight.)
 *   mode 1  ranking key s, value sigma(s) / sum_l sigma(s[n, l, h])  (`sigmoid`, difformer.py:47-55; sigma is monotone,
 *           and s stays decisive where sigma saturates in float32).
 * values (float32) and indices (int32) are [n_q, H, topk], dense.  A row always holds `topk` distinct indices in
 * [0, n_k).  The result is bitwise reproducible, and the selection does not depend on dif_attn_topk_splits().
 *
 * dif_attn_topk_splits(): host arithmetic; the number S of key ranges the launch cuts the keys into (>= 1; more when the
 * query blocks alone do not fill the chip).  The workspace holds S candidate lists and S partial sums per (n, h).
 * ------------------------------------------------------------------------------------- */
int dif_attn_topk_splits(int64_t n_q, int64_t n_k, int H, int M, int topk);
int64_t dif_attn_topk_workspace_bytes(int64_t n_q, int64_t n_k, int H, int M, int topk);
int dif_attn_topk_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, int64_t n_q, int64_t n_k, int H, int M,
                      int mode, int topk, float* values, int32_t* indices, void* workspace, int64_t workspace_bytes,
                      dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_MAPS_H */
