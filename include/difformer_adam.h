/*
 * difformer_adam.h -- C ABI of libdifformer_adam.so: the optimiser update of the reference's drivers on the MI355X (gfx950), one
 * launch for every parameter of a model.
 *
 *   node classification/main.py:111, image and text/main.py:95, spatial-temporal/main.py:83, physical particle/main.py:77
 *       torch.optim.Adam(model.parameters(), lr=..., weight_decay=...)  ... optimizer.step()       -> dif_adam_step_f32
 *
 * torch.optim.Adam with amsgrad=False, maximize=False; the weight decay is the L2 form (added to the gradient), not AdamW.  Per
 * element, with t = step + 1 the tensor's step count AFTER this call:
 *   g  = grad + wd p                         (grad alone where wd == 0: an infinite p does not meet 0 * inf)
 *   m' = beta1 m + (1 - beta1) g
 *   v' = beta2 v + (1 - beta2) g^2
 *   p' = p - (lr / (1 - beta1^t)) m' / ( sqrt(v') / sqrt(1 - beta2^t) + eps )
 * Every input is widened to float64 and the whole element is evaluated in float64 from the UNROUNDED m' and v'; p', m' and v'
 * are each rounded ONCE to float32 (torch rounds m and v to float32 first and divides in float32).  beta^t is the float64 pow,
 * evaluated once per thread.  An element depends on nothing but its own p, grad, m, v and the tensor's step: there is no
 * reduction and no floating-point atomic, so two calls from bitwise-equal state leave bitwise-equal state.  The gradients are
 * read and never written.
 *
 * THE TABLE is host memory: `count` rows of DIF_ADAM_TABLE_FIELDS int64,
 *   [0] p  [1] grad  [2] exp_avg m  [3] exp_avg_sq v      device addresses of float32 [numel], dense, aligned to 4 bytes only
 *   [4] step                                              device address of ONE float32: the count of steps taken so far
 *   [5] numel                                             >= 0
 * It is read during the call and travels to the kernel BY VALUE in the kernel arguments (gradient addresses change from step
 * to step, so no device copy of it could be kept), DIF_ADAM_MAX_TENSORS rows per launch: ceil(count / DIF_ADAM_MAX_TENSORS)
 * launches, one after the other on `stream`.  The tensors must not overlap one another.
 *
 * LAYOUT.  A workgroup of 256 threads owns one chunk of DIF_ADAM_CHUNK consecutive elements of one tensor; a tensor has
 * max(1, ceil(numel / DIF_ADAM_CHUNK)) chunks (an empty tensor still has its step counted).  The table carries the running
 * total of the chunk counts, and a workgroup finds its tensor by a wave-uniform search over at most DIF_ADAM_MAX_TENSORS
 * entries.  One dword per lane, coalesced.
 *
 * THE STEP COUNT lives on the device, a float32 as torch keeps it with capturable=True (exact up to 2^24 steps); the host never
 * reads it and nothing synchronises, so a call can be captured into a hipGraph as it is.  Every workgroup of a tensor reads
 * `step`, and the kernel must also write step + 1 in the same launch.  Chosen: a last-workgroup-done ticket (not a
 * one-thread-per-tensor kernel in front, which would be a second launch per step).  Thread 0 of a workgroup loads `step`,
 * hands it to the workgroup through LDS, and only THEN adds 1 to tickets[i] (an int32 atomic at device scope, acquire-release);
 * the workgroup that draws the last ticket of tensor i stores step + 1 and sets tickets[i] back to 0.  That store is ordered
 * after every other workgroup's ticket, hence after every load of `step` in the launch, so no workgroup can see the new
 * value; launches on one stream do not overlap, so the next one finds the tickets at 0.
 * `tickets` is DIF_ADAM_TICKET_BYTES of device memory, 4-byte aligned, ALL ZERO before the first call and left all zero by
 * every completed call; one buffer serves one stream at a time.
 *
 * EDGE SEMANTICS
 *   - A NaN or infinite gradient element makes that element of p, m and v non-finite and no other element.
 *   - numel == 0: only the step is counted; p, grad, m, v may be NULL.  count == 0: nothing is launched.
 *   - A tensor that is not in the table is not touched: a parameter without a gradient is left out by the caller, and its p,
 *     m, v and step stay bitwise as they were.
 *   - Denormal results are kept (no flush to zero).
 *
 * A small library next to libdifformer_hip.so: the conventions are those of difformer_hip.h, which this header includes for
 * them -- the DIF_E_* return codes, dif_stream_t, device pointers owned by the caller, work enqueued on `stream` only, nothing
 * read or written outside the operands and the tickets.  Errors of THIS library are read with dif_adam_last_error().  Every
 * row of the table is checked before the first launch: a rejected call has enqueued nothing.
 *
 * Limits: 0 <= count <= 2^20; 0 <= numel, and at most 2^31 - 1 chunks per launch (DIF_E_RANGE); lr, eps, weight_decay finite
 * and >= 0, 0 <= beta < 1 (DIF_E_BADARG, as torch's constructor).
 */
#ifndef DIFFORMER_ADAM_H
#define DIFFORMER_ADAM_H

#include "difformer_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DIF_ADAM_VERSION 1

#define DIF_ADAM_MAX_TENSORS 48
#define DIF_ADAM_CHUNK 2048
#define DIF_ADAM_TABLE_FIELDS 6
#define DIF_ADAM_TICKET_BYTES 192

int dif_adam_version(void);
const char* dif_adam_last_error(void);

/* Host arithmetic: the number of kernel launches of a call with `count` rows; -1 for a rejected count. */
int64_t dif_adam_launches(int64_t count);

/* One Adam step of every tensor of the table (above). */
int dif_adam_step_f32(const int64_t* table, int64_t count, double lr, double beta1, double beta2, double eps, double weight_decay,
                      void* tickets, dif_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DIFFORMER_ADAM_H */
