/*
 * difformer_snapshots.h -- C ABI of libdifformer_snapshots.so: the whole DIFFormer model on a BATCH of tiny graphs
 * ("snapshots") on the MI355X (gfx950), one workgroup per snapshot -- all snapshots of an epoch in one launch per pass.
 *
 * The reference's `spatial-temporal/` folder forwards 104 / 50 / 146 snapshots of 20 / 129 / 1,068 nodes one after another
 * (main.py:94-121, eval.py:9-22) and, for every dataset but wikimath, sums their costs before ONE backward.  Given the
 * weights the snapshots are independent and their gradients add: a cumulative epoch is one forward launch of T workgroups,
 * one backward launch and one ordered sum of T gradient slabs.
 *
 * A small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header includes
 * for them and for dif_tiny_cfg -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, work enqueued
 * on `stream` only, nothing read or written outside the operands, outputs and work buffers unspecified on entry.  Errors of
 * THIS library are read with dif_snap_last_error().  The model, its limits (one head, float32, hidden <= 8, <= 64 input
 * features, <= 8 outputs, <= 8 layers, n <= 4,096 nodes and <= 65,535 entries per snapshot) and the meaning of params /
 * grads / rnd are those of dif_tiny_forward_f32 / dif_tiny_backward_f32; the graphs are built by dif_tiny_graph_build.
 */
#ifndef DIFFORMER_SNAPSHOTS_H
#define DIFFORMER_SNAPSHOTS_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_SNAP_VERSION 1
#define DIF_SNAP_RECORD_FIELDS 12      /* int64 words per snapshot record (96 bytes) */

int dif_snap_version(void);
const char* dif_snap_last_error(void);

/* ---------------------------------------------------------------------------------------
 * The snapshots' rows are stored back to back: x [N_total, in_channels] (ldx elements between rows), y and grad_y
 * [N_total, out_channels], dx [N_total, in_channels], rnd [sum_b (num_layers + 1) n_b hidden] with snapshot b's
 * [(num_layers + 1), n_b, hidden] block at (num_layers + 1) * hidden * row0_b.
 *
 * records: DEVICE table, int64 [T][DIF_SNAP_RECORD_FIELDS], 16-byte aligned; record b =
 *   [0] n_b (1 .. max_n)   [1] row0_b (first row of the snapshot)
 *   [2] rowptr  [3] src  [4] val          destination-major CSR of dif_tiny_graph_build (addresses; 0 without use_graph)
 *   [5] rowptr_t  [6] dst_t  [7] val_t    its transpose (read by the backward only)
 *   [8] tape offset  [9] scratch offset   in floats, multiples of 4, into `tape` / `scratch`: snapshot b owns
 *                                          dif_snap_tape_floats(n_b, ..) / dif_snap_scratch_floats(n_b, ..) floats there
 *   [10], [11] reserved
 * The table is the caller's statement about device memory: the library cannot read it, and checks T, max_n and the host
 * arguments only.  cfg->n must be max_n, the largest n_b: it sizes the workgroups (as dif_tiny_* does for one snapshot);
 * cfg->nnz and cfg->launch_plan are not read (always one workgroup per snapshot).
 *
 * dif_snap_tape_floats / dif_snap_scratch_floats: host arithmetic, multiples of 4: the one-workgroup plan's share of
 *   dif_tiny_tape_floats / dif_tiny_scratch_floats, without the grid plans' partial-sum regions.
 * dif_snap_forward_f32   one launch of T workgroups: y rows of snapshot b = dif_tiny_forward_f32 of snapshot b.
 * dif_snap_backward_f32  two launches.  Workgroup b writes its parameter gradients into slab b of `slabs`
 *   [T][slab_stride] (grads: host array of pointers INTO SLAB 0 in the order of params, each the size of its parameter;
 *   slab_stride floats, a multiple of 4, covers them all) and dx (or NULL) into its own rows; then
 *   grad_out[p] = float32(sum_b slabs[b][p]) for p < slab_stride, the sum in float64 in the order b = 0 .. T - 1, rounded
 *   once: no floating-point atomics, bitwise reproducible.  Floats of a slab that belong to no parameter are zero.
 *   The tape is only read.
 * ------------------------------------------------------------------------------------- */
size_t dif_snap_tape_floats(int n, int hidden, int num_layers);
size_t dif_snap_scratch_floats(int n, int hidden, int num_layers);
int dif_snap_forward_f32(const dif_tiny_cfg* cfg, int T, const int64_t* records, const float* x, int64_t ldx,
                         const void* const* params, const float* rnd, float* tape, float* y, dif_stream_t stream);
int dif_snap_backward_f32(const dif_tiny_cfg* cfg, int T, const int64_t* records, const float* x, int64_t ldx,
                          const void* const* params, const float* rnd, float* tape, const float* grad_y, void* const* grads,
                          float* slabs, int64_t slab_stride, float* grad_out, float* dx, float* scratch,
                          dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_SNAPSHOTS_H */
