/*
 * difformer_nbr.h -- C ABI of libdifformer_nbr.so: neighbour graphs of a BATCH of graphs stored back to back on the MI355X
 * (gfx950) -- k nearest neighbours and all neighbours inside a radius, searched inside a row's own graph only, exact to the
 * float64 order of difformer_knn.h.
 *
 * The reference's `physical particle` datasets call torch_cluster's knn_graph (synmol.py:117, actstrack.py:178,
 * plbind.py:224) or radius_graph (tau3mu.py:95) once per sample, and spatial-temporal/main.py:96-98 rebuilds the k-NN graph
 * of every snapshot of every epoch.  This library builds the graphs of a whole batch in one launch.
 *
 * A small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header includes
 * for them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, rows 16-byte aligned, leading
 * dimensions in ELEMENTS, work enqueued on `stream` only, nothing read or written outside the operands and
 * `workspace_bytes` of the workspace, outputs and workspace unspecified on entry.  Errors of THIS library are read with
 * dif_nbr_last_error().
 */
#ifndef DIFFORMER_NBR_H
#define DIFFORMER_NBR_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_NBR_VERSION 1
#define DIF_NBR_MAX_COLUMNS 64     /* widest row (M) the kernels hold in registers */
#define DIF_NBR_MAX_K 24           /* neighbours per row of dif_nbr_knn_f32 */
#define DIF_NBR_MAX_CAP 32         /* neighbours per row of dif_nbr_radius_lists_f32 */

int dif_nbr_version(void);
const char* dif_nbr_last_error(void);

/* ---------------------------------------------------------------------------------------
 * x is [n, M] float32 (ldx = elements between consecutive rows, a multiple of 4; M % 4 == 0, M <= 64: zero-pad the
 * columns, which changes no distance).  graph_ptr is int32 [B + 1], non-decreasing, graph_ptr[0] == 0 and
 * graph_ptr[B] == n: graph b is the rows [graph_ptr[b], graph_ptr[b + 1]) and may be empty.  The candidates of row i are
 * the rows of ITS graph; every index written is a row number of x.
 *
 * Distances are computed in float64 from the float32 rows, in a fixed column order, exactly as in difformer_knn.h:
 *   metric 0  d(i, j) = sum_m (x[i, m] - x[j, m])^2
 *   metric 1  d(i, j) = 1 - (x_i . x_j) / (|x_i| |x_j|); a zero row has cosine 0 with every row (distance 1).
 * and ranked under the same total order: the smaller distance first, among equal distances the lower index first, a NaN
 * distance after every number.  loop == 0 excludes j == i by index only (duplicates of a point stay eligible).
 *
 * dif_nbr_knn_f32: row i of graph b (n_b rows) gets kk_b = min(k, n_b - (loop ? 0 : 1)) neighbours, 1 <= k <= 24.
 * edge_ptr is int64 [B + 1] with edge_ptr[b] = sum_{b' < b} n_b' kk_b' and edge_ptr[B] == E.  edge_index is int64 [2, E]:
 * edge edge_ptr[b] + (i - graph_ptr[b]) kk_b + e is the e-th nearest neighbour of row i; row `centre_row` (0 | 1) of
 * edge_index holds i, the other row the neighbour.  dist_or_null, when given, is float32 [E]: sqrt(d) for metric 0, d for
 * metric 1.  With E == 0 nothing is launched and edge_index may be NULL.
 *
 * dif_nbr_radius_lists_f32 (metric 0 only): j is a neighbour of i when d(i, j) < r * r, the product formed in double and
 * the comparison STRICT; a NaN distance is never inside, and without `loop` j == i is excluded by index.  When more than
 * `cap` rows are inside, the `cap` NEAREST under the total order are kept, 1 <= cap <= 32.  deg[i] (int32 [n]) is the
 * number of kept neighbours of row i.  The workspace of dif_nbr_workspace_bytes(n, cap) bytes receives the ranked lists:
 * uint32 indices [n][cap], then float32 sqrt(d) [n][cap]; slots at and behind deg[i] are left as they were.
 *
 * dif_nbr_radius_edges: deg_ptr is int64 [n + 1], the exclusive prefix sum of deg (deg_ptr[0] == 0, deg_ptr[n] == E); the
 * lists of the same workspace become edge_index int64 [2, E] (edge deg_ptr[i] + e: the e-th nearest kept neighbour of row
 * i, centres ascending) and, when given, dist_or_null float32 [E].  With E == 0 nothing is launched.
 *
 * dif_nbr_workspace_bytes is host arithmetic: n cap 8, or 0 for a shape the entry points reject.
 * ------------------------------------------------------------------------------------- */
int64_t dif_nbr_workspace_bytes(int64_t n, int cap);
int dif_nbr_knn_f32(const float* x, int64_t ldx, int64_t n, int M, const int32_t* graph_ptr, const int64_t* edge_ptr, int B,
                    int k, int loop, int metric, int centre_row, int64_t* edge_index, int64_t E, float* dist_or_null,
                    dif_stream_t stream);
int dif_nbr_radius_lists_f32(const float* x, int64_t ldx, int64_t n, int M, const int32_t* graph_ptr, int B, double r, int loop,
                             int cap, int32_t* deg, void* workspace, int64_t workspace_bytes, dif_stream_t stream);
int dif_nbr_radius_edges(const int64_t* deg_ptr, int64_t n, int cap, int centre_row, const void* workspace,
                         int64_t workspace_bytes, int64_t* edge_index, int64_t E, float* dist_or_null, dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_NBR_H */
