/*
 * difformer_edges.h -- C ABI of libdifformer_edges.so: the attention of the DIFFormer layer ON THE EDGES of a graph, on the
 * MI355X (gfx950).
 *
 * The reference exposes its attention maps as dense [N, L, H] tensors (`full_attention_conv(..., output_attn=True)`,
 * `DIFFormer.get_attentions`; node classification/difformer.py:42-43, :47-55, :211-226).  For a graph model the entries of
 * such a map that are read first are those at the edges the model was given: how much attention a node puts on each of its
 * neighbours, and how much of its attention row lies on the input graph at all.  Both are sampled products -- one dot product
 * per edge, rows gathered by index -- and this library computes them without anything of size N x L:
 * E (2 H M 4 + 16 + 4 H) bytes for the per-edge values, nnz (H M 4 + 4) for the per-row sums.
 *
 * A third, small library next to libdifformer_hip.so and libdifformer_maps.so: the conventions are those of difformer_hip.h,
 * which this header includes for them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, rows
 * 16-byte aligned, leading dimensions in ELEMENTS, work enqueued on `stream` only, nothing read or written outside the
 * operands, outputs unspecified on entry.  Errors of THIS library are read with dif_edges_last_error().
 */
#ifndef DIFFORMER_EDGES_H
#define DIFFORMER_EDGES_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_EDGES_VERSION 1

int dif_edges_version(void);
const char* dif_edges_last_error(void);

/* ---------------------------------------------------------------------------------------
 * Operands of both entry points.  q is [n_q, H, M], k is [n_k, H, M] (float32; ldq / ldk = elements between consecutive
 * rows, multiples of 4); M % 4 == 0, M <= 512.  scale is [n_q, H] float32, dense, or NULL (= 1).  With
 * s = q[n, h, :] . k[l, h, :] in plain fp32 FMA the value of the pair (n, l) is
 *   mode 0  s * scale[n, h]          (`simple`, difformer.py:20-21,32-38,43: scale = 1 / (|q| |k| den[n, h]))
 *   mode 1  sigma(s) * scale[n, h]   (`sigmoid`, difformer.py:47-55: scale = 1 / sum_l sigma(s[n, l, h]))
 *
 * dif_edge_attn_f32: per-edge values in the caller's edge order.  edge_index is int64 [2, E], contiguous: row 0 the source
 * (key) id l, row 1 the target (query) id n, as gcn_conv reads it (difformer.py:65-75).  out is [E, H] float32, dense:
 * out[e, h] = value of (edge_index[1, e], edge_index[0, e]).  1 <= E < 2^31.  Duplicate edges and self-loops are ordinary
 * edges.  An edge's value does not depend on its place in the list: permuting the edges permutes `out` bit for bit.
 * An id outside [0, n_k) (source) or [0, n_q) (target) is never dereferenced: that edge's outputs are NaN, and
 * status (int32 [3], zeroed by the call on `stream`) reports it: status[0] != 0 when any id was out of range,
 * status[1] != 0 for a source id, status[2] != 0 for a target id.
 *
 * dif_edge_attn_mass_f32: per-row sums over a CSR of the target rows (rowptr int32 [n_q + 1], src int32 [nnz], as
 * dif_csr_build produces them; 0 <= nnz < 2^31): mass[n, h] = scale[n, h] * sum_j f(q[n, h, :] . k[src[j], h, :]) over
 * rowptr[n] <= j < rowptr[n + 1], f the identity (mode 0) or sigma (mode 1).  mass is [n_q, H] float32, dense.  An empty row
 * gives 0; a src outside [0, n_k) is not dereferenced and contributes NaN.  The order of the sum depends on M alone (never
 * on the launch geometry): the result is bitwise reproducible.
 * ------------------------------------------------------------------------------------- */
int dif_edge_attn_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* scale, int64_t n_q, int64_t n_k,
                      int H, int M, int mode, const int64_t* edge_index, int64_t E, float* out, int32_t* status,
                      dif_stream_t stream);
int dif_edge_attn_mass_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* scale, int64_t n_q,
                           int64_t n_k, int H, int M, int mode, const int32_t* rowptr, const int32_t* src, int64_t nnz,
                           float* mass, dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_EDGES_H */
