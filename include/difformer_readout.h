/*
 * difformer_readout.h -- C ABI of libdifformer_readout.so: the graph read-out of the reference's graph-level model on the MI355X
 * (gfx950), one pass over the node rows forward and one pass backward.
 *
 *   physical particle/models.py:16-21,30   global_add_pool / global_mean_pool / global_max_pool (h_node, batch)
 *
 * x is [n_rows, H] node rows, all graphs of the batch back to back; out is [n_graphs, H], one row per graph.
 *
 * ROWS OF A GRAPH.  Graph g is the rows [graph_ptr[g], graph_ptr[g+1]) of x.  graph_ptr is int32 [n_graphs + 1] on the device.
 * The caller guarantees a non-decreasing table with graph_ptr[0] == 0 and graph_ptr[n_graphs] == n_rows (ops.BatchLayout checks
 * that on the host; nothing here reads the table on the host).  Rows at and beyond n_rows of a larger allocation are never
 * touched: the kernels clamp what they read from the table to [0, n_rows].
 *
 * EMPTY GRAPH.  Its output row is +0 in all three modes -- torch_geometric's behaviour, with the count of `mean` clamped to 1.
 * It has no gradient rows.
 *
 * ADD AND MEAN.  Every element is widened to float64 and summed in float64 in a FIXED order that depends on (length, H) only:
 * with Wc = min(256, the smallest power of two >= H) columns in flight and P = 256 / Wc row phases, phase p sums the rows
 * p, p + P, p + 2 P, ... of the graph in ascending order, and the phases are added in the order 0, 1, ... P - 1.  `mean` divides
 * by the length in float64.  The result is rounded ONCE to the storage type.  There is no floating-point atomic anywhere: two
 * calls on equal operands are bitwise equal.
 *
 * MAX.  The numeric maximum of the column.  A NaN anywhere in the column gives NaN, as torch.amax does.  For float32 storage
 * the result is one of the input values, bitwise (for bfloat16 too: the widening is exact).  +0 and -0 compare equal; which
 * of the two a column holding both returns is unspecified.
 *
 * BACKWARD.  Every element of grad_x[0:n_rows, 0:H] is written exactly once; there is no memset and no atomic.
 *   add    the row receives grad_out[g] bitwise
 *   mean   grad_out[g] / length in float64, rounded once
 *   max    grad_out[g, c] / ties at every row with x == pooled, +0 elsewhere, where `ties` is the number of such rows of the
 *          column (torch's amax rule, which current torch_geometric inherits); in float64, rounded once.  A NaN column compares
 *          equal nowhere and gets all-zero gradients, as in torch.
 * First derivatives only.  x and pooled (the forward's output) are read for MAX only and may be NULL otherwise.
 *
 * LAYOUT.  One workgroup of 256 threads per graph, grid-strided over the graphs; lanes run over columns, looping for H > 256.
 * One graph is never split over workgroups: a batch that is a single graph of 100,000 rows runs on one CU -- correct, slow.
 * Rows need only be aligned to their element (4 bytes for float32, 2 for bfloat16); loads are one element per lane.
 *
 * A small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header includes for
 * them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, leading dimensions in ELEMENTS, work
 * enqueued on `stream` only (no workspace, no synchronisation, capturable into a hipGraph), nothing read or written outside the
 * operands, outputs unspecified on entry.  Errors of THIS library are read with dif_readout_last_error().
 *
 * Limits: 1 <= H <= 1,024 (DIF_E_SHAPE), n_graphs >= 0, 0 <= n_rows < 2^31, mode one of DIF_READOUT_* (DIF_E_BADARG).  A rejected
 * call launches nothing.  n_graphs == 0 or n_rows == 0 return DIF_OK and write whatever output there is (n_rows == 0: +0 rows).
 */
#ifndef DIFFORMER_READOUT_H
#define DIFFORMER_READOUT_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_READOUT_VERSION 1

#define DIF_READOUT_ADD 0
#define DIF_READOUT_MEAN 1
#define DIF_READOUT_MAX 2

#define DIF_READOUT_MAX_COLUMNS 1024

int dif_readout_version(void);
const char* dif_readout_last_error(void);

/* ---------------------------------------------------------------------------------------
 * x [n_rows, H] (ldx >= H), graph_ptr int32 [n_graphs + 1] -> out [n_graphs, H] (ldo >= H) in the storage type, every element
 * written.
 * ------------------------------------------------------------------------------------- */
int dif_readout_fwd_f32(const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H, int mode,
                        float* out, int64_t ldo, dif_stream_t stream);
int dif_readout_fwd_bf16(const uint16_t* x, int64_t ldx, const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H,
                         int mode, uint16_t* out, int64_t ldo, dif_stream_t stream);

/* ---------------------------------------------------------------------------------------
 * grad_out [n_graphs, H] (ldgo >= H) -> grad_x [n_rows, H] (ldgx >= H), every element of the n_rows rows written once.
 * x [n_rows, H] (ldx >= H) and pooled [n_graphs, H] (ldp >= H), the forward's operand and output, are read for DIF_READOUT_MAX
 * only; otherwise they may be NULL and their leading dimensions are ignored.
 * ------------------------------------------------------------------------------------- */
int dif_readout_bwd_f32(const float* x, int64_t ldx, const float* pooled, int64_t ldp, const float* grad_out, int64_t ldgo,
                        const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H, int mode, float* grad_x, int64_t ldgx,
                        dif_stream_t stream);
int dif_readout_bwd_bf16(const uint16_t* x, int64_t ldx, const uint16_t* pooled, int64_t ldp, const uint16_t* grad_out,
                         int64_t ldgo, const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H, int mode,
                         uint16_t* grad_x, int64_t ldgx, dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_READOUT_H */
