// Whole-model kernels for TINY graphs: `spatial-temporal/` trains DIFFormer at hidden 4 on 20 / 129 / 1,068-node snapshots
// (spatial-temporal/run.sh:5-40, main.py:94-120: hundreds of forwards per epoch, each on tensors fresh from
// `snapshot.to(device)`).  At that size the layer-by-layer path is ~110 launches per training snapshot (0.33 ms of kernels,
// 1.1 ms of host time); here the whole of
//     DIFFormer.forward            node classification/difformer.py:184-209  (= spatial-temporal/difformer.py:173-198)
//       DIFFormerConv.forward      :113-145      full_attention_conv :10-61      gcn_conv :63-79
// is ONE launch of one workgroup, its backward (what autograd derives for main.py:119 `cost_tr.backward`) a second one, and
// the graph preparation (degree, normalised values, destination-major CSR and its transpose, both in stable edge order) a
// third.  One head, hidden <= 8, <= 4,096 nodes, <= 64 input features, <= 8 outputs, float32.
//
// Layout of the work: a thread owns node i (i += blockDim for more nodes than threads); everything a node needs from
// OTHER nodes goes through per-node arrays in a caller-owned scratch / tape buffer (L1 / L2 resident: 17 KB per array at
// 1,068 x 4) between __syncthreads(); sums over nodes (K^T V, weight gradients, LayerNorm gradients) are computed by
// `outer_sum`: outputs x node-chunks spread over the threads, chunk partials in LDS, added in chunk order in float64 --
// bitwise reproducible.  The sigmoid kernel's O(N^2) pair loop keeps the stationary node in registers and streams the
// others through LDS tiles (uniform addresses: broadcast reads).
//
// What ONE node computes in a stage (input layer, projections, closed-form `simple` row and its backward set-up, aggregation, layer
// tail, output row, tail / LayerNorm / input-layer backward) is the TINY_* statement macros of tiny_stages.h, defined once for this
// plan and the grid plans (tiny_sigmoid_grid.hip, tiny_simple_grid.hip); that file says why they are macros.  The one-workgroup
// plan's loops over nodes, its pair sweeps, its sums over nodes and 14 scratch slots are the BODIES of the two kernels below,
// tiny_forward_body.h / tiny_backward_body.h: text included between the kernels' braces here and in tiny_batched.hip (one workgroup
// per snapshot of a batch, libdifformer_snapshots.so), for the same reason.  Here: the two kernels around them, the graph
// preparation and the C entry points (their host-side checks shared with tiny_batched.hip: tiny_host.h).
#include "tiny_stages.h"
#include "tiny_host.h"

using namespace tiny;

namespace {

// ======================================================================================================================
// forward
// ======================================================================================================================
template <int DP>
__global__ __launch_bounds__(512) void tiny_forward_kernel(const TinyArgs a) {
#include "tiny_forward_body.h"
}

// ======================================================================================================================
// backward
// ======================================================================================================================
// scratch slots ([n][DP] each): 0 DH (gradient of the current layer input)  1 DX0  2 SG (g_s d_out)  3 DNUM / DA  4 DY
// 5 DYX  6 DIR  7 DQ  8 DK  9 DV  10 Q  11 K  12 V  13 DPRE;  then [n] arrays: DDEN / DL, TS, spare
template <int DP>
__global__ __launch_bounds__(512) void tiny_backward_kernel(const TinyArgs a) {
#include "tiny_backward_body.h"
}

// ======================================================================================================================
// graph preparation in one launch: gcn_conv's degree / values (:66-74) and the CSR of the adjacency and of its transpose,
// entries of a row in edge order (stable), by LSD radix sort on 4-bit digits of the row key, one workgroup per direction:
// a thread owns a contiguous chunk of the list; per-thread digit histograms (LDS, [16][512] uint16) scanned digit-major
// give every thread its write cursor per digit; walking its chunk in order keeps the sort stable.  ceil(log2 N / 4) passes.
// ======================================================================================================================
constexpr int kGraphThreads = 512;

// exclusive prefix sum over the block's threads (wave scans by shuffles + the wave totals in LDS); returns the exclusive
// prefix of `v`; every thread must call
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t* sWave /*[16]*/) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t up = __shfl_up(inc, off, 64);
        if (lane >= off) inc += up;
    }
    __syncthreads();                       // sWave may still be read by the previous scan
    if (lane == 63) sWave[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int w = 0; w < wave; ++w) base += sWave[w];
    return base + inc - v;
}

__device__ void radix_pass(const uint32_t* in, uint32_t* out, const int64_t* keys64, int E, int shift, uint16_t* hist /*[16][T]*/,
                           uint32_t* sWave, int N) {
    const int T = kGraphThreads, t = threadIdx.x;
    const int c = (E + T - 1) / T;
    const int e0 = min(E, t * c), e1 = min(E, e0 + c);
    for (int k = 0; k < 16; ++k) hist[k * T + t] = 0;
    auto key_of = [&](int e) -> uint32_t {
        if (keys64) {
            int64_t kv = keys64[e];
            if (kv < 0 || kv >= N) kv = 0;                  // flagged by the counting loop
            return (static_cast<uint32_t>(kv) << 16) | static_cast<uint32_t>(e);
        }
        return in[e];
    };
    for (int e = e0; e < e1; ++e) hist[(((key_of(e) >> 16) >> shift) & 15) * T + t] += 1;
    __syncthreads();
    // exclusive scan over the 16 x T counters in digit-major order: thread t owns flat entries [16 t, 16 t + 16)
    uint32_t local = 0;
    for (int k = 0; k < 16; ++k) local += hist[16 * t + k];
    uint32_t run = block_exclusive_scan(local, sWave);
    for (int k = 0; k < 16; ++k) {
        const uint32_t cnt = hist[16 * t + k];
        hist[16 * t + k] = static_cast<uint16_t>(run);
        run += cnt;
    }
    __syncthreads();
    for (int e = e0; e < e1; ++e) {
        const uint32_t kv = key_of(e);
        const uint32_t dg = ((kv >> 16) >> shift) & 15;
        const uint32_t pos = hist[dg * T + t];
        hist[dg * T + t] = static_cast<uint16_t>(pos + 1);
        out[pos] = kv;
    }
    __syncthreads();
}

// workgroup 0: the CSR over destinations; workgroup 1: its transpose.  Both count the in-degrees themselves (the values
// need deg^-1/2 of both ends), sort their own copy of the list, and share nothing.
__global__ __launch_bounds__(kGraphThreads) void tiny_graph_kernel(const int64_t* __restrict__ ei, const float* __restrict__ w, int E,
                                                                     int N, int* rowptr, int* src, float* val, int* rowptr_t,
                                                                     int* dst_t, float* val_t, int* status, uint32_t* ws /*[4 E]*/) {
    __shared__ uint16_t hist[16 * kGraphThreads];
    __shared__ uint32_t sWave[16];
    __shared__ int sCnt[kMaxNodes];             // entries per row of THIS workgroup's CSR
    __shared__ float sDinv[kMaxNodes];          // first the in-degree counts (as int bits), then deg^-1/2
    __shared__ int sBad;
    const int T = kGraphThreads, t = threadIdx.x;
    const int direction = blockIdx.x;
    uint32_t* bufA = ws + static_cast<size_t>(direction) * 2 * E;
    uint32_t* bufB = bufA + E;
    const int64_t* keys = direction == 0 ? ei + E : ei;        // forward: filed under the destination (`col`, :65)
    const int64_t* other = direction == 0 ? ei : ei + E;
    int* rp = direction == 0 ? rowptr : rowptr_t;
    int* nb = direction == 0 ? src : dst_t;
    float* vl = direction == 0 ? val : val_t;
    int* sIn = reinterpret_cast<int*>(sDinv);
    if (t == 0) sBad = 0;
    for (int k = t; k < N; k += T) { sCnt[k] = 0; sIn[k] = 0; }
    __syncthreads();
    for (int e = t; e < E; e += T) {
        const int64_t r = ei[e], c = ei[E + e];
        const bool okr = r >= 0 && r < N, okc = c >= 0 && c < N;
        if (!okr || !okc) sBad = 1;
        const int ri = okr ? static_cast<int>(r) : 0, ci = okc ? static_cast<int>(c) : 0;
        atomicAdd(&sIn[ci], 1);
        if (direction == 1) atomicAdd(&sCnt[ri], 1);
    }
    __syncthreads();
    {
        // dinv = sqrt(1 / in-degree), float32, correctly rounded (:66-68); 0 incoming entries -> inf
        int mx = 0;
        for (int k = t; k < N; k += T) {
            const int deg = sIn[k];
            if (direction == 0) sCnt[k] = deg;
            mx = max(mx, deg);
            sDinv[k] = sqrtf(1.0f / static_cast<float>(deg));
        }
        if (direction == 0) atomicMax(&status[1], mx);
    }
    __syncthreads();
    {
        // exclusive scan of the counts -> row pointers (a thread owns up to 8 consecutive rows)
        const int per = (N + T - 1) / T;
        const int r0 = min(N, t * per), r1 = min(N, r0 + per);
        uint32_t local = 0;
        for (int r = r0; r < r1; ++r) local += sCnt[r];
        uint32_t run = block_exclusive_scan(local, sWave);
        for (int r = r0; r < r1; ++r) {
            rp[r] = static_cast<int>(run);
            run += sCnt[r];
        }
        if (t == T - 1) rp[N] = E;
    }
    if (E > 0) {
        int bits = 1;
        while ((1 << bits) < N) ++bits;
        const int passes = (bits + 3) / 4;
        const uint32_t* cur = nullptr;
        uint32_t* dst = bufA;
        for (int p = 0; p < passes; ++p) {
            radix_pass(cur, dst, p == 0 ? keys : nullptr, E, 4 * p, hist, sWave, N);
            cur = dst;
            dst = (dst == bufA) ? bufB : bufA;
        }
        for (int k = t; k < E; k += T) {
            const uint32_t kv = cur[k];
            const int e = static_cast<int>(kv & 0xffffu), grp = static_cast<int>(kv >> 16);
            int64_t o = other[e];
            if (o < 0 || o >= N) o = 0;
            const int r = direction == 0 ? static_cast<int>(o) : grp;       // source      (`row`)
            const int c = direction == 0 ? grp : static_cast<int>(o);       // destination (`col`)
            float v = w ? __fmul_rn(__fmul_rn(w[e], sDinv[c]), sDinv[r]) : __fmul_rn(sDinv[c], sDinv[r]);   // :71 / :73
            if (!isfinite(v)) v = 0.f;                                       // :74
            nb[k] = static_cast<int>(o);
            vl[k] = v;
        }
    }
    __syncthreads();
    if (t == 0 && sBad) status[0] = 1;
}

// One workgroup for the whole model, or one launch per layer stage over the chip (tiny_sigmoid_grid.hip / tiny_simple_grid.hip).
// `sigmoid` (the n^2 pairs of a layer), measured on MI355X (profiles/r06_tiny_sigmoid_grid.txt): device time crosses at ~64 nodes
// (49 us against 48 per training snapshot; 72 against 225 at 129 nodes, 90 against 3,350 at 1,068); in the launch-bound training
// loop of spatial-temporal/main.py the 20-node dataset is 7 % faster on one workgroup (2 launches, not 7), the 129-node one 13 %
// faster on the grid.  `simple` has no pair loop: per training snapshot one workgroup takes 100 us at 129 nodes, 116 at 256, 300 at 1,068
// against 72 / 75 / 88 on the grid (7 launches instead of 2); the launch-bound loop at 129 nodes is 8 % FASTER on one workgroup,
// wikimath's (1,068 nodes, graph term) 24 % faster on the grid (profiles/r06_tiny_sigmoid_grid.txt section 4).
constexpr int kGridFromNodes = 64;
constexpr int kGridFromNodesSimple = 256;
bool grid_plan(const dif_tiny_cfg* cfg) {
    if (cfg->launch_plan == 1) return false;
    if (cfg->launch_plan == 2) return true;
    return cfg->n > (cfg->kernel == 1 ? kGridFromNodes : kGridFromNodesSimple);
}

}  // namespace

extern "C" size_t dif_tiny_tape_floats(int n, int hidden, int num_layers) {
    return tape_floats(n, hidden <= 4 ? 4 : 8, num_layers);
}

extern "C" size_t dif_tiny_scratch_floats(int n, int hidden, int num_layers) { return scratch_floats(n, hidden <= 4 ? 4 : 8, num_layers); }

extern "C" size_t dif_tiny_graph_workspace_bytes(int64_t E, int64_t N) {
    (void)N;
    return 4 * static_cast<size_t>(E) * 4 + 16;
}

extern "C" int dif_tiny_graph_build(const int64_t* edge_index, const float* edge_weight, int64_t E, int64_t N, int32_t* rowptr,
                                    int32_t* src, float* val, int32_t* rowptr_t, int32_t* dst_t, float* val_t, int32_t* status,
                                    void* workspace, size_t workspace_bytes, dif_stream_t stream) {
    DIF_REQUIRE(N >= 1 && N <= kMaxNodes && E >= 0 && E <= kMaxEdges, DIF_E_SHAPE,
                "dif_tiny_graph_build: N <= %d nodes and E <= %d edges (got %lld, %lld)", kMaxNodes, kMaxEdges,
                static_cast<long long>(N), static_cast<long long>(E));
    DIF_REQUIRE((E == 0 || edge_index) && rowptr && rowptr_t && status && workspace, DIF_E_BADARG, "dif_tiny_graph_build: null pointer");
    DIF_REQUIRE(E == 0 || (src && val && dst_t && val_t), DIF_E_BADARG, "dif_tiny_graph_build: null output");
    DIF_REQUIRE(workspace_bytes >= dif_tiny_graph_workspace_bytes(E, N), DIF_E_WORKSPACE, "dif_tiny_graph_build: workspace too small");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st);
    if (e != hipSuccess) return dif::fail(static_cast<int>(e), "dif_tiny_graph_build: memset: %s", hipGetErrorString(e));
    return dif::launch("dif_tiny_graph_build", tiny_graph_kernel, dim3(2), dim3(kGraphThreads), 0, st, edge_index, edge_weight,
                       static_cast<int>(E), static_cast<int>(N), rowptr, src, val, rowptr_t, dst_t, val_t, status,
                       static_cast<uint32_t*>(workspace));
}

extern "C" int dif_tiny_forward_f32(const dif_tiny_cfg* cfg, const float* x, int64_t ldx, const void* const* params,
                                    const int32_t* rowptr, const int32_t* src, const float* val, const float* rnd, float* tape,
                                    float* y, dif_stream_t stream) {
    if (int rc = check_cfg(cfg)) return rc;
    TinyArgs a{};
    if (int rc = fill(a, cfg, x, ldx, params)) return rc;
    DIF_REQUIRE(tape && y, DIF_E_BADARG, "dif_tiny_forward_f32: null tape / y");
    DIF_REQUIRE(dif::aligned16(tape), DIF_E_BADARG, "dif_tiny_forward_f32: tape must be 16-byte aligned");
    DIF_REQUIRE(!cfg->use_graph || (rowptr && (src || cfg->nnz == 0) && (val || cfg->nnz == 0)), DIF_E_BADARG,
                "dif_tiny_forward_f32: use_graph without a CSR");
    a.rowptr = rowptr; a.nbr = src; a.val = val; a.rnd = rnd; a.tape = tape; a.y = y;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (grid_plan(cfg)) return cfg->kernel == 1 ? grid_sigmoid_forward(a, st) : grid_simple_forward(a, st);
    const int T = block_threads(cfg->n);
    return dif::with_flags([&](auto NARROW) {               // hidden <= 4: rows padded to 4 columns, 8 otherwise
        return dif::launch("dif_tiny_forward_f32", tiny_forward_kernel<NARROW ? 4 : 8>, dim3(1), dim3(T), 0, st, a);
    }, cfg->hidden <= 4);
}

extern "C" int dif_tiny_backward_f32(const dif_tiny_cfg* cfg, const float* x, int64_t ldx, const void* const* params,
                                     const int32_t* rowptr_t, const int32_t* dst_t, const float* val_t, const float* rnd,
                                     float* tape, const float* grad_y, void* const* grads, float* dx, float* scratch,
                                     dif_stream_t stream) {
    if (int rc = check_cfg(cfg)) return rc;
    TinyArgs a{};
    if (int rc = fill(a, cfg, x, ldx, params)) return rc;
    DIF_REQUIRE(tape && grad_y && grads && scratch, DIF_E_BADARG, "dif_tiny_backward_f32: null tape / grad_y / grads / scratch");
    DIF_REQUIRE(dif::aligned16(tape) && dif::aligned16(scratch), DIF_E_BADARG, "dif_tiny_backward_f32: tape / scratch must be 16-byte aligned");
    DIF_REQUIRE(!cfg->use_graph || (rowptr_t && (dst_t || cfg->nnz == 0) && (val_t || cfg->nnz == 0)), DIF_E_BADARG,
                "dif_tiny_backward_f32: use_graph without the transposed CSR");
    a.rowptr = rowptr_t; a.nbr = dst_t; a.val = val_t; a.rnd = rnd; a.tape = tape; a.gy = grad_y; a.dx = dx; a.scratch = scratch;
    if (int rc = fill_grads(a, cfg, grads, "dif_tiny_backward_f32")) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (grid_plan(cfg)) return cfg->kernel == 1 ? grid_sigmoid_backward(a, st) : grid_simple_backward(a, st);
    const int T = block_threads(cfg->n);
    return dif::with_flags([&](auto NARROW) {
        return dif::launch("dif_tiny_backward_f32", tiny_backward_kernel<NARROW ? 4 : 8>, dim3(1), dim3(T), 0, st, a);
    }, cfg->hidden <= 4);
}
