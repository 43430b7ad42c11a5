/*
 * difformer_knn.h -- C ABI of libdifformer_knn.so: k-nearest-neighbour graphs of the rows of a feature matrix on the
 * MI355X (gfx950), exact to the float64 order.
 *
 * Two of the reference's task folders build their graph from the features: `spatial-temporal/main.py:96-98` calls
 * torch_cluster's knn_graph for every snapshot of every epoch, `image and text/main.py:52-53` calls sklearn's
 * kneighbors_graph once per dataset.  This library returns that graph as an int64 edge list without an N x N tensor.
 *
 * A small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header includes
 * for them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, rows 16-byte aligned, leading
 * dimensions in ELEMENTS, work enqueued on `stream` only, nothing read or written outside the operands and
 * `workspace_bytes` of the workspace, outputs and workspace unspecified on entry.  Errors of THIS library are read with
 * dif_knn_last_error().
 */
#ifndef DIFFORMER_KNN_H
#define DIFFORMER_KNN_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_KNN_VERSION 1

int dif_knn_version(void);
const char* dif_knn_last_error(void);

/* ---------------------------------------------------------------------------------------
 * x is [n, M] float32 (ldx = elements between consecutive rows, a multiple of 4; M % 4 == 0, M <= 512: zero-pad the
 * columns, which changes no distance).  Every row i gets kk = min(k, n - (loop ? 0 : 1)) neighbours, 1 <= k <= 24.
 *
 * Distances are computed in float64 from the float32 rows, in a fixed column order:
 *   metric 0  d(i, j) = sum_m (x[i, m] - x[j, m])^2
 *   metric 1  d(i, j) = 1 - (x_i . x_j) / (|x_i| |x_j|); a zero row has cosine 0 with every row (distance 1).
 * Per row the kk smallest come first under ONE total order: the smaller distance first, among equal distances the lower
 * index first, a NaN distance after every number.  loop == 0 excludes j == i by index only (duplicates of a point stay
 * eligible); with loop != 0 self is an ordinary candidate.  The indices of a row are distinct and in [0, n).
 *
 * edge_index is int64 [2, n kk], dense: edge i kk + e is the e-th nearest neighbour of row i; row `centre_row` (0 | 1)
 * of edge_index holds i, the other row the neighbour.  dist_or_null, when given, is float32 [n kk]: sqrt(d) for metric 0,
 * d for metric 1.  With kk == 0 (one row, no self-loop) nothing is launched and edge_index may be NULL.
 *
 * Two routes compute the same list (dif_knn_route(): the one `route == -1` takes):
 *   0  direct (M <= 16 only): one lane per row, every float64 distance of the row computed and ranked as it is formed.
 *   1  sweep: float32 rank keys on the matrix core keep the best min(32, n) candidates per row; their float64 distances
 *      are then recomputed by direct difference and ranked under the order above.  The float32 key only decides
 *      membership of the candidate list: a true neighbour is lost only when more points than the 32 - kk - 1 spare
 *      slots lie within float32 rounding of the kk-th distance.  That is the one documented limit of this route.
 * The result is bitwise reproducible and does not depend on dif_knn_splits().
 *
 * dif_knn_route / dif_knn_splits / dif_knn_workspace_bytes are host arithmetic; `route` there and below is -1 (the
 * automatic choice), 0 or 1.  dif_knn_splits(): the number S of key ranges the launch cuts the rows into (>= 1; more
 * when the query rows alone do not fill the chip); 0 for a shape the entry point rejects.
 * ------------------------------------------------------------------------------------- */
int dif_knn_route(int64_t n, int M, int k);
int dif_knn_splits(int64_t n, int M, int k, int loop, int route);
int64_t dif_knn_workspace_bytes(int64_t n, int M, int k, int loop, int metric, int route);
int dif_knn_graph_f32(const float* x, int64_t ldx, int64_t n, int M, int k, int loop, int metric, int centre_row, int route,
                      int64_t* edge_index, float* dist_or_null, void* workspace, int64_t workspace_bytes,
                      dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_KNN_H */
