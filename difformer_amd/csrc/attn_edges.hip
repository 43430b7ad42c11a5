// libdifformer_edges.so (C ABI: include/difformer_edges.h): the attention of the DIFFormer layer at the edges of a graph -- the
// entries a[col_e, row_e, h] of the reference's dense map (difformer.py:42-43 `simple`, :47-55 `sigmoid`, :211-226
// get_attentions) and their per-target sums, without the [N, L, H] tensor.  A sampled product: one dot product per edge, both
// rows gathered by index.  Gather-bound: plain fp32 FMA, no matrix core.
//
// Lane groups.  A dot product of M columns belongs to a group of G lanes, lane j of it holding columns 4 j .. 4 j + 3 (and, for
// G = 64, 256 + 4 j .. as well): one global_load_dwordx4 per lane and row, the G lanes of a row reading G 16-byte pieces in a row.
// G depends on M alone -- 4 lanes up to 16 columns, 16 up to 64, 32 up to 128, 64 beyond -- and so does every sum below: per lane
// the products in column order (fmaf), then the xor butterfly G/2 .. 1 over the group.  Neither an edge's place in its list nor
// the launch geometry enters.
//
// Edge kernel.  A workgroup of four waves holds 256 / G groups; every group takes kInFlight edges of one head, so that a wave has
// 4 (G = 64) to 64 (G = 4) pairs of rows in flight.  The groups of a wave read consecutive ids (one 8-byte word per group, the same
// address in all its lanes) and store consecutive edges.  An id out of range is replaced by row 0 for the loads -- never
// dereferenced -- and the edge's value by NaN; the status words are set with plain stores of the constant 1.
//
// Mass kernel.  One wave per target row and head, the q row in registers.  The row's entries are taken in chunks of 64: ONE
// coalesced load of 64 source ids per chunk (the next chunk's is issued before this chunk's rows), handed to the groups through
// ds_bpermute.  In step t of a chunk group g takes entry t (64 / G) + g; kInFlight steps are issued together, so 4 (G = 64) to 64
// (G = 4) key rows are in flight.  Every group adds its values in entry order; at the end the group sums are combined by the xor
// butterfly G .. 32.  A row stays on its wave however long it is.
#include <stdarg.h>
#include "dif_common.h"
#include "../../include/difformer_edges.h"

namespace {

using dif::f32x4;
using dif::sigmoid_hw;

constexpr int kMaxM = 512;
constexpr int kInFlight = 4;           // rows (edge kernel: pairs of rows) a lane group has in flight
constexpr int kBlock = 256;

// thread-local last-error text of THIS library (dif_edges_last_error)
char* edges_err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
int edges_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(edges_err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}
// post-launch check into THIS library's error text (hipGetLastError only, never synchronises)
int edges_launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return edges_fail(static_cast<int>(e), "%s: %s", what, hipGetErrorString(e));
    return 0;
}
#define EDGES_REQUIRE(cond, code, ...) \
    do { if (!(cond)) return edges_fail((code), __VA_ARGS__); } while (0)

template <int G> constexpr int pieces() { return G == 64 ? kMaxM / 256 : 1; }     // float4 pieces of a row per lane

// the lane's pieces of row `r` (a valid row), columns past M zero
template <int G>
__device__ __forceinline__ void load_row(f32x4 (&dst)[pieces<G>()], const float* __restrict__ base, int64_t ld, int64_t r, int col0,
                                         int gl, int M) {
#pragma unroll
    for (int i = 0; i < pieces<G>(); ++i) {
        const int c = 4 * gl + 4 * G * i;
        dst[i] = dif::Elem<float>::ld4g(base + r * ld + col0 + (c < M ? c : 0));
    }
}

// this lane's part of a . b, products in column order
template <int G>
__device__ __forceinline__ float dot_part(const f32x4 (&a)[pieces<G>()], const f32x4 (&b)[pieces<G>()], int gl, int M) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < pieces<G>(); ++i) {
        const bool cok = 4 * gl + 4 * G * i < M;
#pragma unroll
        for (int j = 0; j < 4; ++j) d = fmaf(cok ? a[i][j] : 0.f, cok ? b[i][j] : 0.f, d);
    }
    return d;
}

// sum over the G lanes of a group, every lane gets the total
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// grid: (ceil(E / (kBlock / G * kInFlight)), H); block kBlock
template <int G, int MODE>
__global__ __launch_bounds__(kBlock) void edge_attn_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                           int64_t ldk, const float* __restrict__ scale, int64_t n_q, int64_t n_k,
                                                           int H, int M, const int64_t* __restrict__ edge_index, int64_t E,
                                                           float* __restrict__ out, int32_t* __restrict__ status) {
    constexpr int NG = kBlock / G;
    constexpr int P = pieces<G>();
    const int gl = threadIdx.x % G;
    const int g = threadIdx.x / G;
    const int h = blockIdx.y;
    const int64_t e0 = static_cast<int64_t>(blockIdx.x) * (NG * kInFlight) + g;

    int64_t row[kInFlight], col[kInFlight];
    bool live[kInFlight], rok[kInFlight], cok[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
        const int64_t e = e0 + u * NG;
        live[u] = e < E;
        const int64_t ec = live[u] ? e : E - 1;
        row[u] = edge_index[ec];                   // source: key row
        col[u] = edge_index[E + ec];               // target: query row
        rok[u] = row[u] >= 0 && row[u] < n_k;
        cok[u] = col[u] >= 0 && col[u] < n_q;
    }
    f32x4 qv[kInFlight][P], kv[kInFlight][P];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
        load_row<G>(qv[u], q, ldq, cok[u] ? col[u] : 0, h * M, gl, M);
        load_row<G>(kv[u], k, ldk, rok[u] ? row[u] : 0, h * M, gl, M);
    }
    float sc[kInFlight];
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) sc[u] = scale != nullptr ? scale[(cok[u] ? col[u] : 0) * H + h] : 1.0f;
#pragma unroll
    for (int u = 0; u < kInFlight; ++u) {
        const float s = group_sum<G>(dot_part<G>(qv[u], kv[u], gl, M));
        const float val = (MODE == 1 ? sigmoid_hw(s) : s) * sc[u];
        if (gl == 0 && live[u]) {
            const bool ok = rok[u] && cok[u];
            out[(e0 + u * NG) * H + h] = ok ? val : __builtin_nanf("");
            if (!ok) status[0] = 1;
            if (!rok[u]) status[1] = 1;
            if (!cok[u]) status[2] = 1;
        }
    }
}

// grid: (ceil(n_q / 4), H); block kBlock = four waves, one target row each
template <int G, int MODE>
__global__ __launch_bounds__(kBlock) void edge_mass_kernel(const float* __restrict__ q, int64_t ldq, const float* __restrict__ k,
                                                           int64_t ldk, const float* __restrict__ scale, int64_t n_q, int64_t n_k,
                                                           int H, int M, const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ src, int64_t nnz, float* __restrict__ mass) {
    constexpr int NG = 64 / G;                     // groups per wave
    constexpr int P = pieces<G>();
    const int lane = threadIdx.x & 63;
    const int gl = lane % G;
    const int g = lane / G;
    const int h = blockIdx.y;
    const int64_t n = static_cast<int64_t>(blockIdx.x) * (kBlock / 64) + (threadIdx.x >> 6);
    if (n >= n_q) return;                          // the whole wave
    f32x4 qv[P];
    load_row<G>(qv, q, ldq, n, h * M, gl, M);
    int64_t beg = rowptr[n], end = rowptr[n + 1];
    beg = beg < 0 ? 0 : beg;
    end = end > nnz ? nnz : end;

    // MODE 1: the group's sum of sigma(s), the same in all its lanes.  MODE 0: this lane's part of the group's sum of s -- the
    // butterfly is linear, so it runs once at the end.
    float acc = 0.f;
    int32_t ahead = beg + lane < end ? src[beg + lane] : 0;
    for (int64_t c0 = beg; c0 < end; c0 += 64) {
        const int cnt = end - c0 < 64 ? static_cast<int>(end - c0) : 64;
        const int32_t mine = ahead;
        ahead = c0 + 64 + lane < end ? src[c0 + 64 + lane] : 0;
        for (int t = 0; t * NG < cnt; t += kInFlight) {            // (G % kInFlight == 0: t + u < G, the entry's place < 64)
            f32x4 kv[kInFlight][P];
            bool live[kInFlight], ok[kInFlight];
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                const int p = (t + u) * NG + g;
                const int32_t l = __shfl(mine, p, 64);
                live[u] = p < cnt;
                ok[u] = l >= 0 && l < n_k;
                load_row<G>(kv[u], k, ldk, ok[u] ? l : 0, h * M, gl, M);
            }
#pragma unroll
            for (int u = 0; u < kInFlight; ++u) {
                float d = dot_part<G>(qv, kv[u], gl, M);
                if (MODE == 1) d = sigmoid_hw(group_sum<G>(d));
                acc += live[u] ? (ok[u] ? d : __builtin_nanf("")) : 0.f;
            }
        }
    }
    if (MODE == 0) acc = group_sum<G>(acc);
#pragma unroll
    for (int off = G; off < 64; off <<= 1) acc += __shfl_xor(acc, off, 64);      // the groups, in a fixed order
    if (lane == 0) mass[n * H + h] = acc * (scale != nullptr ? scale[n * H + h] : 1.0f);
}

int group_lanes(int M) { return M <= 16 ? 4 : (M <= 64 ? 16 : (M <= 128 ? 32 : 64)); }

// the checks both entry points share
int check_operands(const char* who, const float* q, int64_t ldq, const float* k, int64_t ldk, const float* scale, int64_t n_q,
                   int64_t n_k, int H, int M, int mode) {
    EDGES_REQUIRE(n_q > 0 && n_k > 0 && H > 0 && M > 0, DIF_E_BADARG, "%s: n_q, n_k, H, M must be positive", who);
    EDGES_REQUIRE(q && k, DIF_E_BADARG, "%s: null pointer", who);
    EDGES_REQUIRE(dif::aligned16(q) && dif::aligned16(k), DIF_E_BADARG, "%s: q and k must be 16-byte aligned", who);
    EDGES_REQUIRE(dif::aligned<4>(scale), DIF_E_BADARG, "%s: scale must be 4-byte aligned", who);
    EDGES_REQUIRE(M % 4 == 0 && M <= kMaxM, DIF_E_SHAPE, "%s: M must be a multiple of 4 up to %d (got %d); zero-pad the columns", who,
                  kMaxM, M);
    EDGES_REQUIRE(mode == 0 || mode == 1, DIF_E_SHAPE, "%s: unknown mode %d (0: simple, 1: sigmoid)", who, mode);
    EDGES_REQUIRE(ldq >= static_cast<int64_t>(H) * M && ldk >= static_cast<int64_t>(H) * M && ldq % 4 == 0 && ldk % 4 == 0, DIF_E_BADARG,
                  "%s: leading dimensions must cover a row and be multiples of 4 elements", who);
    EDGES_REQUIRE(H <= 65535, DIF_E_RANGE, "%s: H %d exceeds the grid", who, H);
    return 0;
}

template <int G, int MODE>
int launch_edges(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* scale, int64_t n_q, int64_t n_k, int H, int M,
                 const int64_t* edge_index, int64_t E, float* out, int32_t* status, hipStream_t st) {
    constexpr int64_t per = kBlock / G * kInFlight;
    const dim3 grid(static_cast<unsigned>((E + per - 1) / per), static_cast<unsigned>(H));
    hipLaunchKernelGGL((edge_attn_kernel<G, MODE>), grid, dim3(kBlock), 0, st, q, ldq, k, ldk, scale, n_q, n_k, H, M, edge_index, E, out,
                       status);
    return edges_launch_status("edge_attn_kernel");
}

template <int G, int MODE>
int launch_mass(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* scale, int64_t n_q, int64_t n_k, int H, int M,
                const int32_t* rowptr, const int32_t* src, int64_t nnz, float* mass, hipStream_t st) {
    const dim3 grid(static_cast<unsigned>((n_q + kBlock / 64 - 1) / (kBlock / 64)), static_cast<unsigned>(H));
    hipLaunchKernelGGL((edge_mass_kernel<G, MODE>), grid, dim3(kBlock), 0, st, q, ldq, k, ldk, scale, n_q, n_k, H, M, rowptr, src, nnz,
                       mass);
    return edges_launch_status("edge_mass_kernel");
}

}  // namespace

extern "C" int dif_edges_version(void) { return DIF_EDGES_VERSION; }
extern "C" const char* dif_edges_last_error(void) { return edges_err_buf(); }

// one launcher per (lane group, mode): f(G, MODE) with both as constants, G from M alone
template <typename F>
static int with_group_and_mode(const char* who, int M, int mode, F&& f) {
    auto miss = [who](int v) { return edges_fail(DIF_E_SHAPE, "%s: no kernel variant for %d", who, v); };
    return dif::with_int<0, 1>(mode, [&](auto MODE) {
        return dif::with_int<4, 16, 32, 64>(group_lanes(M), [&](auto G) { return f(G, MODE); }, miss);
    }, miss);
}

extern "C" int dif_edge_attn_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* scale, int64_t n_q,
                                 int64_t n_k, int H, int M, int mode, const int64_t* edge_index, int64_t E, float* out,
                                 int32_t* status, dif_stream_t stream) {
    const char* who = "dif_edge_attn_f32";
    if (const int rc = check_operands(who, q, ldq, k, ldk, scale, n_q, n_k, H, M, mode)) return rc;
    EDGES_REQUIRE(edge_index && out && status, DIF_E_BADARG, "%s: null pointer", who);
    EDGES_REQUIRE(dif::aligned<8>(edge_index) && dif::aligned<4>(out) &&
                      dif::aligned<4>(status),
                  DIF_E_BADARG, "%s: edge_index must be 8-byte aligned, out and status 4-byte aligned", who);
    EDGES_REQUIRE(E >= 1 && E < (1ll << 31), DIF_E_RANGE, "%s: E must be in [1, 2^31) (got %lld)", who, static_cast<long long>(E));
    hipStream_t st = static_cast<hipStream_t>(stream);
    const hipError_t e = hipMemsetAsync(status, 0, 3 * sizeof(int32_t), st);
    if (e != hipSuccess) return edges_fail(static_cast<int>(e), "%s: hipMemsetAsync: %s", who, hipGetErrorString(e));
    return with_group_and_mode(who, M, mode, [&](auto G, auto MODE) {
        return launch_edges<G, MODE>(q, ldq, k, ldk, scale, n_q, n_k, H, M, edge_index, E, out, status, st);
    });
}

extern "C" int dif_edge_attn_mass_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* scale, int64_t n_q,
                                      int64_t n_k, int H, int M, int mode, const int32_t* rowptr, const int32_t* src, int64_t nnz,
                                      float* mass, dif_stream_t stream) {
    const char* who = "dif_edge_attn_mass_f32";
    if (const int rc = check_operands(who, q, ldq, k, ldk, scale, n_q, n_k, H, M, mode)) return rc;
    EDGES_REQUIRE(rowptr && src && mass, DIF_E_BADARG, "%s: null pointer", who);
    EDGES_REQUIRE(dif::aligned<4>(rowptr) && dif::aligned<4>(src) &&
                      dif::aligned<4>(mass),
                  DIF_E_BADARG, "%s: rowptr, src and mass must be 4-byte aligned", who);
    EDGES_REQUIRE(nnz >= 0 && nnz < (1ll << 31), DIF_E_RANGE, "%s: nnz must be in [0, 2^31) (got %lld)", who, static_cast<long long>(nnz));
    EDGES_REQUIRE((n_q + 3) / 4 < (1ll << 31), DIF_E_RANGE, "%s: grid too large", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return with_group_and_mode(who, M, mode, [&](auto G, auto MODE) {
        return launch_mass<G, MODE>(q, ldq, k, ldk, scale, n_q, n_k, H, M, rowptr, src, nnz, mass, st);
    });
}
