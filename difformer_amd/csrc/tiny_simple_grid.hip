// The whole model on a tiny graph with the `simple` kernel, spread over the chip (the counterpart of tiny_sigmoid_grid.hip):
// spatial-temporal/run.sh:33-37 trains `simple` on wikimath's 1,068 nodes, where the one-workgroup kernel of tiny_model.hip walks
// three slots of nodes per phase and ~13 dependent edge loads per node on ONE compute unit (97 + 188 us per training snapshot).
//
// With `simple` (node classification/difformer.py:18-39) the nodes meet in five sums per layer -- K^T V, sum k, sum v, |Q|^2,
// |K|^2 -- and the backward in four -- d K^T V, d sum k, d sum v, d s.  A launch is one layer's stage for all nodes, workgroup =
// 64 nodes (a thread per node) + the threads that add the block's share of the NEXT sums (<= 82 values, float64, rows in node
// order) into memory; the next launch's workgroups each add the blocks' shares in block order (every workgroup the same
// float64 sum: bitwise reproducible, no atomics) and go on:
//     forward   L + 1 launches:  [input layer, projections 0, sums 0] , [attention l, aggregation, tail, projections l + 1, sums l + 1 | output] x L
//     backward  L + 2 launches:  [output Linear, tail L-1, attention set-up, sums] , [attention l, projections l, tail l - 1 ... | input layer] x L ,
//                                [every parameter gradient: tiny::grid_sums]
// Same tape, scratch and C calls as the one-workgroup kernel, and the same arithmetic from the same text: the per-node stages
// (the attention's closed form and its backward's set-up among them) are the TINY_* macros of tiny_stages.h, run on this plan's
// scratch layout by tail_backward_common / input_backward of tiny_grid.h.  Here: the block shares of the sums over nodes, the second
// half of the attention's backward and the launch sequences.
#include "tiny_grid.h"

using namespace tiny;

namespace {

constexpr int kThreads = 128;                   // 64 node threads + the sum threads (<= 82 sums)

template <int DP>
__host__ __device__ constexpr int fwd_sums() { return DP * DP + 2 * DP + 2; }       // K^T V | sum k | sum v | |Q|^2 | |K|^2
template <int DP>
__host__ __device__ constexpr int bwd_sums() { return DP * DP + 2 * DP + 1; }       // d K^T V | d sum k | d sum v | d s

// the blocks' shares [G][96] of one set -> sOut[0 .. NS) (float), every workgroup alike; ends with __syncthreads()
__device__ __forceinline__ void add_block_sums(const double* shares, int G, int NS, float* sOut) {
    const int t = threadIdx.x;
    if (t < NS) {
        double s = 0.0;
        int g = 0;
        for (; g + 8 <= G; g += 8) {                   // eight loads in flight, added in block order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = shares[static_cast<size_t>(g + u) * 96 + t];
#pragma unroll
            for (int u = 0; u < 8; ++u) s += v[u];
        }
        for (; g < G; ++g) s += shares[static_cast<size_t>(g) * 96 + t];
        sOut[t] = static_cast<float>(s);
    }
    __syncthreads();
}

// ======================================================================================================================
// forward
// ======================================================================================================================
template <int DP>
__global__ __launch_bounds__(kThreads) void grid_simple_forward_kernel(const TinyArgs a, const int stage) {
    __shared__ float sW0[DP * kMaxIn];
    __shared__ float sB0[DP], sLn0w[DP], sLn0b[DP];
    __shared__ LayerW<DP> sL, sNext;
    __shared__ float sWo[kMaxOut * DP], sBo[kMaxOut];
    __shared__ float sSum[96];
    __shared__ float sRows[kNodes][3 * DP];         // q | k | v of the block's nodes (zero rows beyond n)
    const int n = a.n, d = a.d, L = a.layers, T = blockDim.x, t = threadIdx.x;
    const int i = blockIdx.x * kNodes + t;
    const bool node = t < kNodes, live = node && i < n;
    const int G = gridDim.x;
    Tape<DP> tp(a.tape, n, L);
    const size_t nd = static_cast<size_t>(n) * DP;
    const bool drop = a.training && a.rnd != nullptr && a.p_drop > 0.f;
    double* shares = tp.partials();                                       // [2 sets][G][96]
    float h[DP], q[DP], k[DP], v[DP];
#pragma unroll
    for (int m = 0; m < DP; ++m) { h[m] = 0.f; q[m] = 0.f; k[m] = 0.f; v[m] = 0.f; }
    int next_set = 0;

    if (stage == 0) {
        TINY_LOAD_INPUT_CONSTS(sB0[k_] = k_ < d ? a.b0[k_] : 0.f;)
        load_layer<DP>(sNext, a.lp[0], d, a.use_weight, a.use_bn);
        __syncthreads();
        if (live) {                                                        // input layer (:188-192)
            TINY_INPUT_FORWARD(i, h)
        }
    } else {
        const int l = stage - 1;
        const bool last = l + 1 == L;
        load_layer<DP>(sL, a.lp[l], d, a.use_weight, a.use_bn);
        if (!last) load_layer<DP>(sNext, a.lp[l + 1], d, a.use_weight, a.use_bn);
        else {
            TINY_LOAD_OUTPUT_CONSTS(for (int k_ = t; k_ < kMaxOut; k_ += T) sBo[k_] = k_ < a.c ? a.bo[k_] : 0.f;)
        }
        add_block_sums(shares + static_cast<size_t>(l & 1) * G * 96, G, fwd_sums<DP>(), sSum);      // (syncs)
        if (blockIdx.x == 0 && t < fwd_sums<DP>()) tp.SUM[l * 96 + t] = sSum[t];                      // the backward reads them
        const float* set = tp.qkv(l & 1);
        const float* Vl = set + 2 * nd;
        next_set = (l + 1) & 1;
        if (live) {
            load_row<DP>(set + static_cast<size_t>(i) * DP, q);
            float att[DP];
            TINY_SIMPLE_ATTENTION_ROW(q, att)                         // :20-38  closed form of the attention from the layer's sums
            float out[DP];
            TINY_LAYER_TAIL_FORWARD(Vl, tp.H + (static_cast<size_t>(l) * n + i) * DP, sL, l, i, att, out)
#pragma unroll
            for (int m = 0; m < DP; ++m) h[m] = out[m];
            if (last) {
                TINY_OUTPUT_ROW(i, out)                                               // :208
            }
        }
        if (last) return;
    }
    // ---- projections of the next layer (:115-120) and this block's share of its sums ----
    if (live) {
        project<DP>(sNext, a.use_weight, h, q, k, v);
        float* nxt = tp.qkv(next_set);
        store_row<DP>(nxt + static_cast<size_t>(i) * DP, q);
        store_row<DP>(nxt + nd + static_cast<size_t>(i) * DP, k);
        store_row<DP>(nxt + 2 * nd + static_cast<size_t>(i) * DP, v);
    }
    if (node) {
#pragma unroll
        for (int m = 0; m < DP; ++m) {
            sRows[t][m] = live ? q[m] : 0.f;
            sRows[t][DP + m] = live ? k[m] : 0.f;
            sRows[t][2 * DP + m] = live ? v[m] : 0.f;
        }
    }
    __syncthreads();
    if (t < fwd_sums<DP>()) {
        double s = 0.0;
        if (t < DP * DP) {
            const int m = t / DP, c = t % DP;
            for (int r = 0; r < kNodes; ++r) s += static_cast<double>(sRows[r][DP + m]) * static_cast<double>(sRows[r][2 * DP + c]);
        } else if (t < DP * DP + 2 * DP) {
            const int c = DP + (t - DP * DP);                                          // k columns, then v columns
            for (int r = 0; r < kNodes; ++r) s += static_cast<double>(sRows[r][c]);
        } else {
            const int c0 = (t == DP * DP + 2 * DP) ? 0 : DP;                           // |Q|^2, |K|^2
            for (int r = 0; r < kNodes; ++r) {
#pragma unroll
                for (int m = 0; m < DP; ++m) s += static_cast<double>(sRows[r][c0 + m]) * static_cast<double>(sRows[r][c0 + m]);
            }
        }
        shares[(static_cast<size_t>(next_set) * G + blockIdx.x) * 96 + t] = s;
    }
}

// ======================================================================================================================
// backward
// ======================================================================================================================
// tail_backward_common, then the attention's set-up for node i of layer l (the one-workgroup kernel's phase 1, `simple`):
// d num, d den, the part of d q that does not wait for the sums, t_s; -> the row the block's sums are made of
template <int DP>
__device__ __forceinline__ void tail_backward(const TinyArgs& a, const Tape<DP>& tp, const GridScratch<DP>& gs, const LayerW<DP>& w,
                                              const float* sSum, int l, int i, float (&dy)[DP], bool drop, float keep,
                                              float (&row)[2 * DP + 2]) {
    const int n = a.n;
    const size_t at_i = static_cast<size_t>(i) * DP;
    float datt[DP], q[DP], k[DP], v[DP];
    tail_backward_common<DP>(a, tp, gs, w, l, i, dy, drop, keep, datt, q, k, v);
    const float q2 = sSum[DP * DP + 2 * DP], k2 = sSum[DP * DP + 2 * DP + 1];
    const float s = 1.0f / (sqrtf(q2) * sqrtf(k2));
    float dnum[DP], dden = 0.f, ts = 0.f, dq[DP];
    TINY_SIMPLE_BACKWARD_SETUP(q, datt, s, dnum, dden, ts, dq)
    store_row<DP>(gs.per_layer(l, kDQ) + at_i, dq);            // completed by the next launch (+ 2 g_q2 q)
#pragma unroll
    for (int m = 0; m < DP; ++m) { row[m] = q[m]; row[DP + m] = dnum[m]; }
    row[2 * DP] = dden;
    row[2 * DP + 1] = ts;
}

template <int DP>
__global__ __launch_bounds__(kThreads) void grid_simple_backward_kernel(const TinyArgs a, const int stage) {
    __shared__ float sW0[DP * kMaxIn];
    __shared__ float sLn0w[DP], sLn0b[DP];
    __shared__ LayerW<DP> sL, sPrev;
    __shared__ float sWo[kMaxOut * DP];
    __shared__ float sSum[96], sSumPrev[96], sG[96];
    __shared__ float sRows[kNodes][2 * DP + 2];     // q | d num | d den | t_s of the block's nodes
    const int n = a.n, d = a.d, L = a.layers, T = blockDim.x, t = threadIdx.x;
    const int i = blockIdx.x * kNodes + t;
    const bool node = t < kNodes, live = node && i < n;
    const int G = gridDim.x;
    Tape<DP> tp(a.tape, n, L);
    GridScratch<DP> gs(a.scratch, n, L);
    const size_t at_i = static_cast<size_t>(i) * DP;
    const bool drop = a.training && a.rnd != nullptr && a.p_drop > 0.f;
    const float keep = drop ? 1.0f / (1.0f - a.p_drop) : 1.0f;
    double* shares = gs.partials();                                       // [2 sets][G][96]
    float row[2 * DP + 2];
#pragma unroll
    for (int m = 0; m < 2 * DP + 2; ++m) row[m] = 0.f;
    int lp = 0;                                                            // the layer whose set-up this launch ends with

    if (stage == 0) {
        lp = L - 1;
        TINY_LOAD_OUTPUT_CONSTS()
        load_layer<DP>(sPrev, a.lp[lp], d, a.use_weight, a.use_bn);
        for (int kk = t; kk < fwd_sums<DP>(); kk += T) sSumPrev[kk] = tp.SUM[lp * 96 + kk];
        __syncthreads();
        if (live) {
            float g[DP];
#pragma unroll
            for (int m = 0; m < DP; ++m) g[m] = 0.f;
            if (a.use_source) store_row<DP>(gs.DX0 + at_i, g);
            TINY_OUTPUT_BACKWARD_ROW(i, g)
            tail_backward<DP>(a, tp, gs, sPrev, sSumPrev, lp, i, g, drop, keep, row);
        }
    } else {
        const int l = L - stage;
        lp = l - 1;
        load_layer<DP>(sL, a.lp[l], d, a.use_weight, a.use_bn);
        for (int kk = t; kk < fwd_sums<DP>(); kk += T) sSum[kk] = tp.SUM[l * 96 + kk];
        if (l > 0) {
            load_layer<DP>(sPrev, a.lp[lp], d, a.use_weight, a.use_bn);
            for (int kk = t; kk < fwd_sums<DP>(); kk += T) sSumPrev[kk] = tp.SUM[lp * 96 + kk];
        } else {
            TINY_LOAD_INPUT_CONSTS()
        }
        add_block_sums(shares + static_cast<size_t>(l & 1) * G * 96, G, bwd_sums<DP>(), sG);       // (syncs)
        const int set = l & 1;
        if (live) {
            // ---- the attention's backward in closed form (the one-workgroup kernel's phases 2-3, `simple`) ----
            const float q2 = sSum[DP * DP + 2 * DP], k2 = sSum[DP * DP + 2 * DP + 1];
            const float s = 1.0f / (sqrtf(q2) * sqrtf(k2));
            const float ds = sG[DP * DP + 2 * DP];
            const float gq2 = -0.5f * s * ds / q2, gk2 = -0.5f * s * ds / k2;                // s = q2^-1/2 k2^-1/2
            float q[DP], k[DP], v[DP], dq[DP], dk[DP], dv[DP];
            load_row<DP>(gs.in_set(set, kQ) + at_i, q);
            load_row<DP>(gs.in_set(set, kK) + at_i, k);
            load_row<DP>(gs.in_set(set, kV) + at_i, v);
            load_row<DP>(gs.per_layer(l, kDQ) + at_i, dq);
#pragma unroll
            for (int m = 0; m < DP; ++m) {
                dq[m] += 2.0f * gq2 * q[m];
                float acc = 0.f;
#pragma unroll
                for (int dd = 0; dd < DP; ++dd) acc += sG[m * DP + dd] * v[dd];
                dk[m] = acc + sG[DP * DP + m] + 2.0f * gk2 * k[m];
            }
#pragma unroll
            for (int dd = 0; dd < DP; ++dd) {
                float acc = 0.f;
#pragma unroll
                for (int m = 0; m < DP; ++m) acc += sG[m * DP + dd] * k[m];
                dv[dd] = acc + sG[DP * DP + DP + dd];
            }
            if (a.use_graph) {                              // adjoint of the aggregation: the TRANSPOSED CSR, edge order
                const float* SG = gs.in_set(set, kSG);
                TINY_GATHER_ROWS(SG, i, dv)
            }
#pragma unroll
            for (int m = 0; m < DP; ++m)
                if (m >= d) { dq[m] = 0.f; dk[m] = 0.f; dv[m] = 0.f; }
            store_row<DP>(gs.per_layer(l, kDQ) + at_i, dq);
            store_row<DP>(gs.per_layer(l, kDK) + at_i, dk);
            store_row<DP>(gs.per_layer(l, kDV) + at_i, dv);
            float dh[DP];
            TINY_BACK_PROJECT(gs.DIR + at_i, sL, dq, dk, dv, dh)
            if (l > 0) tail_backward<DP>(a, tp, gs, sPrev, sSumPrev, lp, i, dh, drop, keep, row);
            else input_backward<DP>(a, tp, gs, sW0, sLn0w, sLn0b, i, dh, drop, keep);
        }
        if (l == 0) return;
    }
    // ---- this block's share of layer lp's backward sums: d K^T V = s sum q (x) d num, d sum k = s sum d den q, d sum v, d s ----
    if (node) {
#pragma unroll
        for (int m = 0; m < 2 * DP + 2; ++m) sRows[t][m] = row[m];
    }
    __syncthreads();
    if (t < bwd_sums<DP>()) {
        const float q2 = sSumPrev[DP * DP + 2 * DP], k2 = sSumPrev[DP * DP + 2 * DP + 1];
        const double s = 1.0 / (static_cast<double>(sqrtf(q2)) * static_cast<double>(sqrtf(k2)));
        double acc = 0.0;
        if (t < DP * DP) {
            const int m = t / DP, dd = t % DP;
            for (int r = 0; r < kNodes; ++r) acc += static_cast<double>(sRows[r][m]) * static_cast<double>(sRows[r][DP + dd]);
            acc *= s;
        } else if (t < DP * DP + DP) {
            const int m = t - DP * DP;
            for (int r = 0; r < kNodes; ++r) acc += static_cast<double>(sRows[r][2 * DP]) * static_cast<double>(sRows[r][m]);
            acc *= s;
        } else if (t < DP * DP + 2 * DP) {
            const int dd = t - DP * DP - DP;
            for (int r = 0; r < kNodes; ++r) acc += static_cast<double>(sRows[r][DP + dd]);
        } else {
            for (int r = 0; r < kNodes; ++r) acc += static_cast<double>(sRows[r][2 * DP + 1]);
        }
        shares[(static_cast<size_t>(lp & 1) * G + blockIdx.x) * 96 + t] = acc;
    }
}

template <int DP>
int forward_launches(const TinyArgs& a, hipStream_t st) {
    const int G = (a.n + kNodes - 1) / kNodes;
    for (int s = 0; s <= a.layers; ++s)
        if (int rc = dif::launch("dif_tiny_forward_f32", grid_simple_forward_kernel<DP>, dim3(G), dim3(kThreads), 0, st, a, s)) return rc;
    return 0;
}

template <int DP>
int backward_launches(const TinyArgs& a, hipStream_t st) {
    const int G = (a.n + kNodes - 1) / kNodes;
    for (int s = 0; s <= a.layers; ++s)
        if (int rc = dif::launch("dif_tiny_backward_f32", grid_simple_backward_kernel<DP>, dim3(G), dim3(kThreads), 0, st, a, s)) return rc;
    return grid_sums(a, st);
}

}  // namespace

int tiny::grid_simple_forward(const TinyArgs& a, hipStream_t st) {
    return a.d <= 4 ? forward_launches<4>(a, st) : forward_launches<8>(a, st);
}

int tiny::grid_simple_backward(const TinyArgs& a, hipStream_t st) {
    return a.d <= 4 ? backward_launches<4>(a, st) : backward_launches<8>(a, st);
}
