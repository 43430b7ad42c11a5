// Specific to the grid plans of the whole-model kernels (tiny_sigmoid_grid.hip, tiny_simple_grid.hip: one launch per layer stage,
// 64 nodes per workgroup): the backward's scratch layout (GridScratch, the enums), the backward stages of tiny_stages.h bound to
// that layout (tail_backward_common, input_backward; project for the forward), and grid_sums.  What a node computes is in tiny_stages.h.
#pragma once
#include "tiny_stages.h"

namespace tiny {

template <int DP>
struct GridScratch {                            // backward scratch (floats), nd = n * DP
    float *DIR, *DX0, *DPRE, *DY0, *DYX0;
    float* layer0;                              // [L][5][nd]: DQ DK DV DY DYX
    float* set0;                                // [2][5][nd]: SG Q K V DA
    float* dl0;                                 // [2][2][n]: DL as float32 hi + lo
    float* tail;                                // the key splits' partial sums [K][n][3 DP] (double)
    size_t nd;
    __device__ GridScratch(float* S, int n, int L) {
        nd = static_cast<size_t>(n) * DP;
        DIR = S; DX0 = S + nd; DPRE = S + 2 * nd; DY0 = S + 3 * nd; DYX0 = S + 4 * nd;
        layer0 = S + 5 * nd;
        set0 = layer0 + 5 * nd * L;
        dl0 = set0 + 10 * nd;
        tail = dl0 + 4 * static_cast<size_t>(n);
        tail += (-(tail - S)) & 3;              // 16-byte aligned (S is)
    }
    __device__ double* partials() const { return reinterpret_cast<double*>(tail); }
    __device__ float* per_layer(int l, int which) const { return layer0 + (static_cast<size_t>(l) * 5 + which) * nd; }
    __device__ float* in_set(int set, int which) const { return set0 + (static_cast<size_t>(set) * 5 + which) * nd; }
    __device__ float* dl(int set, int part) const { return dl0 + static_cast<size_t>(2 * set + part) * (nd / DP); }
};
enum { kDQ = 0, kDK = 1, kDV = 2, kDY = 3, kDYX = 4 };
enum { kSG = 0, kQ = 1, kK = 2, kV = 3, kDA = 4 };

// Wq / Wk / Wv of node i's layer input h -> the set's rows
template <int DP>
__device__ __forceinline__ void project(const LayerW<DP>& w, bool use_weight, const float (&h)[DP], float (&q)[DP], float (&k)[DP],
                                        float (&v)[DP]) {
    TINY_PROJECT(w, use_weight, h, q, k, v)
}

// ======================================================================================================================
// What the one-workgroup kernel's "phase 1" does for node i of layer l, from the gradient dy of the layer's OUTPUT (H[l + 1]),
// up to the attention: dropout / LayerNorm / residual backward (d LayerNorm operands kept per layer for the sums at the end),
// the direct term DIR, + x0, the aggregation's operand SG, and q, k, v recomputed into the layer's set.  -> datt, q, k, v
template <int DP>
__device__ __forceinline__ void tail_backward_common(const TinyArgs& a, const Tape<DP>& tp, const GridScratch<DP>& gs, const LayerW<DP>& w,
                                                     int l, int i, float (&dy)[DP], bool drop, float keep, float (&datt)[DP],
                                                     float (&q)[DP], float (&k)[DP], float (&v)[DP]) {
    const int n = a.n, d = a.d;
    const size_t at_i = static_cast<size_t>(i) * DP;
    const int set = l & 1;
    TINY_TAIL_BACKWARD(w.lnw, tp.Z + (static_cast<size_t>(l + 1) * n + i) * DP, gs.per_layer(l, kDY) + at_i, gs.per_layer(l, kDYX) + at_i, gs.DIR + at_i,
                       gs.DX0 + at_i, gs.in_set(set, kSG) + at_i, l, i, dy, datt)
    float h[DP];
    load_row<DP>(tp.H + (static_cast<size_t>(l) * n + i) * DP, h);
    project<DP>(w, a.use_weight, h, q, k, v);
    store_row<DP>(gs.in_set(set, kQ) + at_i, q);
    store_row<DP>(gs.in_set(set, kK) + at_i, k);
    store_row<DP>(gs.in_set(set, kV) + at_i, v);
}

// input layer backward (:188-192) for node i from dh = the gradient of H[0]: d pre-activation -> DPRE (and the LayerNorm operands)
// for the sums at the end, dx
template <int DP>
__device__ __forceinline__ void input_backward(const TinyArgs& a, const Tape<DP>& tp, const GridScratch<DP>& gs, const float* sW0,
                                               const float* sLn0w, const float* sLn0b, int i, float (&dh)[DP], bool drop, float keep) {
    const int n = a.n, d = a.d;
    (void)n;
    const size_t at_i = static_cast<size_t>(i) * DP;
    TINY_INPUT_BACKWARD(gs.DX0 + at_i, tp.Z + at_i, gs.DY0 + at_i, gs.DYX0 + at_i, gs.DPRE + at_i, i, dh)
}

// every sum over nodes of the backward (parameter gradients) from the per-layer operands: one workgroup per gradient
int grid_sums(const TinyArgs& a, hipStream_t st);

}  // namespace tiny
