// Graph read-out on the device: libdifformer_readout.so, C ABI in include/difformer_readout.h.
//
// Replaces global_add_pool / global_mean_pool / global_max_pool of the reference's graph-level model (physical
// particle/models.py:16-21,30) -- a scatter with floating-point atomics forward and a gather backward, each a handful of launches --
// by one kernel each way.  The batch is stored graph after graph (ops.BatchLayout), so a graph is a row range and nothing is
// scattered: a workgroup owns a graph, sums (or maximises) its rows in a fixed order and writes the graph's row once.
//
// Arithmetic, order of summation and edge semantics: the header.
//
// Layout: Wc = min(256, the smallest power of two >= H) columns in flight, lane c of a row phase owns column cb + c (cb = 0, Wc,
// ... for H > 256); the P = 256 / Wc row phases take the rows p, p + P, ... of the graph in ascending order, so a wave reads
// min(64, Wc) consecutive elements of one row per load.  The phases meet in LDS (one value per thread) and phase 0 combines them
// in phase order.  The backward of `max` counts the ties of a column the same way before it writes.
#include <stdarg.h>
#include "dif_common.h"
#include "../../include/difformer_readout.h"

// dif::launch (csrc/dif_launch.h) reports through these; this library is linked -Bsymbolic and binds its own, so that its
// errors land in dif_readout_last_error().
namespace dif {

char* err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}
int launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(static_cast<int>(e), "%s: %s", what, hipGetErrorString(e));
    return 0;
}

}  // namespace dif

namespace {

constexpr int kBlock = 256;
constexpr int kMaxGrid = 4096;                            // workgroups; the graphs beyond are strided over
constexpr int64_t kMaxRows = (int64_t(1) << 31) - 1;      // int32 graph_ptr

// ---- operands -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double widen(const float* p) { return static_cast<double>(*p); }
__device__ __forceinline__ double widen(const dif::bf16* p) { return static_cast<double>(dif::bf16_to_f32(p->bits)); }
// one rounding from float64 (dif::f64_to_bf16 does not go through float32's)
__device__ __forceinline__ void store(float* p, double v) { *p = static_cast<float>(v); }
__device__ __forceinline__ void store(dif::bf16* p, double v) { p->bits = dif::f64_to_bf16(v); }

// what the table says, held to the rows that exist
__device__ __forceinline__ int clamp_row(int32_t r, int n_rows) { return r < 0 ? 0 : (r > n_rows ? n_rows : r); }

// the running maximum m with one more value: a NaN, once seen, stays (its own bits); otherwise the larger one, m on equality
__device__ __forceinline__ float take_max(float m, float v) { return (m != m) ? m : ((v != v || v > m) ? v : m); }

// ---- forward --------------------------------------------------------------------------------------------------------------------
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void readout_fwd_kernel(const T* __restrict__ x, int64_t ldx, const int32_t* __restrict__ graph_ptr,
                                                             int64_t n_graphs, int n_rows, int H, int Wc, T* __restrict__ out,
                                                             int64_t ldo) {
    __shared__ double sh[kBlock];
    float* shf = reinterpret_cast<float*>(sh);
    const int c = threadIdx.x & (Wc - 1), p = threadIdx.x / Wc, P = kBlock / Wc;
    for (int64_t g = blockIdx.x; g < n_graphs; g += gridDim.x) {
        const int r0 = clamp_row(graph_ptr[g], n_rows), r1 = clamp_row(graph_ptr[g + 1], n_rows);
        const int len = r1 > r0 ? r1 - r0 : 0;
        for (int cb = 0; cb < H; cb += Wc) {
            const int col = cb + c;
            const bool live = col < H;
            const T* xp = x + static_cast<int64_t>(r0 + p) * ldx + col;       // (dereferenced for r < r1 only)
            if (MODE == DIF_READOUT_MAX) {
                float m = -INFINITY;
                if (live) {
#pragma unroll 8
                    for (int r = r0 + p; r < r1; r += P, xp += P * ldx) m = take_max(m, dif::Elem<T>::ld(xp));
                }
                shf[threadIdx.x] = m;
                __syncthreads();
                if (p == 0 && live) {
                    m = shf[c];
                    for (int q = 1; q < P; ++q) m = take_max(m, shf[q * Wc + c]);
                    dif::Elem<T>::st(out + g * ldo + col, len > 0 ? m : 0.f);      // (exact: m is a value of the storage type)
                }
            } else {
                double acc = 0.0;
                if (live) {
#pragma unroll 8
                    for (int r = r0 + p; r < r1; r += P, xp += P * ldx) acc += widen(xp);
                }
                sh[threadIdx.x] = acc;
                __syncthreads();
                if (p == 0 && live) {
                    double s = sh[c];
                    for (int q = 1; q < P; ++q) s += sh[q * Wc + c];
                    if (MODE == DIF_READOUT_MEAN) s /= static_cast<double>(len > 0 ? len : 1);
                    store(out + g * ldo + col, s);
                }
            }
            __syncthreads();                                                   // the next column block / graph rewrites sh
        }
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------
template <typename T, int MODE>
__global__ __launch_bounds__(kBlock) void readout_bwd_kernel(const T* __restrict__ x, int64_t ldx, const T* __restrict__ pooled,
                                                             int64_t ldp, const T* __restrict__ grad_out, int64_t ldgo,
                                                             const int32_t* __restrict__ graph_ptr, int64_t n_graphs, int n_rows,
                                                             int H, int Wc, T* __restrict__ grad_x, int64_t ldgx) {
    __shared__ int ties_of[kBlock];
    const int c = threadIdx.x & (Wc - 1), p = threadIdx.x / Wc, P = kBlock / Wc;
    for (int64_t g = blockIdx.x; g < n_graphs; g += gridDim.x) {
        const int r0 = clamp_row(graph_ptr[g], n_rows), r1 = clamp_row(graph_ptr[g + 1], n_rows);
        if (r1 <= r0) continue;                                                // (the whole workgroup: no barrier is skipped by some)
        const int len = r1 - r0;
        for (int cb = 0; cb < H; cb += Wc) {
            const int col = cb + c;
            const bool live = col < H;
            T* gp = grad_x + static_cast<int64_t>(r0 + p) * ldgx + col;
            if (MODE == DIF_READOUT_MAX) {
                const T* xp = x + static_cast<int64_t>(r0 + p) * ldx + col;
                const float pm = live ? dif::Elem<T>::ld(pooled + g * ldp + col) : 0.f;
                int count = 0;
                if (live) {
                    const T* xq = xp;
#pragma unroll 8
                    for (int r = r0 + p; r < r1; r += P, xq += P * ldx) count += dif::Elem<T>::ld(xq) == pm ? 1 : 0;
                }
                ties_of[threadIdx.x] = count;
                __syncthreads();
                int ties = 0;
                for (int q = 0; q < P; ++q) ties += ties_of[q * Wc + c];
                __syncthreads();                                               // the next column block / graph rewrites ties_of
                if (live) {
                    T share, zero;
                    store(&zero, 0.0);
                    store(&share, ties > 0 ? widen(grad_out + g * ldgo + col) / static_cast<double>(ties) : 0.0);
                    for (int r = r0 + p; r < r1; r += P, xp += P * ldx, gp += P * ldgx) *gp = dif::Elem<T>::ld(xp) == pm ? share : zero;
                }
            } else if (live) {
                T value = grad_out[g * ldgo + col];                            // add: the bits of grad_out
                if (MODE == DIF_READOUT_MEAN) store(&value, widen(grad_out + g * ldgo + col) / static_cast<double>(len));
                for (int r = r0 + p; r < r1; r += P, gp += P * ldgx) *gp = value;
            }
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// columns in flight: the smallest power of two >= H, at most the workgroup
int columns_in_flight(int H) {
    int w = 1;
    while (w < H && w < kBlock) w *= 2;
    return w;
}

int check_shape(const char* who, int64_t n_graphs, int64_t n_rows, int H, int mode) {
    DIF_REQUIRE(H >= 1 && H <= DIF_READOUT_MAX_COLUMNS, DIF_E_SHAPE, "%s: need 1 <= H <= %d (got %d)", who, DIF_READOUT_MAX_COLUMNS, H);
    DIF_REQUIRE(n_graphs >= 0 && n_rows >= 0 && n_rows <= kMaxRows, DIF_E_BADARG,
                "%s: need n_graphs >= 0 and 0 <= n_rows < 2^31 (got n_graphs = %lld, n_rows = %lld)", who,
                static_cast<long long>(n_graphs), static_cast<long long>(n_rows));
    DIF_REQUIRE(mode == DIF_READOUT_ADD || mode == DIF_READOUT_MEAN || mode == DIF_READOUT_MAX, DIF_E_BADARG,
                "%s: mode %d is none of DIF_READOUT_*", who, mode);
    return 0;
}

template <typename T>
int readout_fwd(const char* who, const T* x, int64_t ldx, const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H, int mode,
                T* out, int64_t ldo, dif_stream_t stream) {
    if (int rc = check_shape(who, n_graphs, n_rows, H, mode)) return rc;
    if (n_graphs == 0) return 0;
    DIF_REQUIRE((x || n_rows == 0) && graph_ptr && out, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<sizeof(T)>(x) && dif::aligned<sizeof(T)>(out) && dif::aligned<4>(graph_ptr), DIF_E_BADARG,
                "%s: the rows must be aligned to their element and graph_ptr 4-byte", who);
    DIF_REQUIRE(ldx >= H && ldo >= H, DIF_E_BADARG, "%s: leading dimensions (%lld, %lld) smaller than H = %d", who,
                static_cast<long long>(ldx), static_cast<long long>(ldo), H);
    const dim3 grid = dif::grid_of(n_graphs < kMaxGrid ? n_graphs : kMaxGrid);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = static_cast<int>(n_rows), Wc = columns_in_flight(H);
    if (mode == DIF_READOUT_ADD)
        return dif::launch(who, readout_fwd_kernel<T, DIF_READOUT_ADD>, grid, dim3(kBlock), 0, st, x, ldx, graph_ptr, n_graphs, n, H, Wc, out, ldo);
    if (mode == DIF_READOUT_MEAN)
        return dif::launch(who, readout_fwd_kernel<T, DIF_READOUT_MEAN>, grid, dim3(kBlock), 0, st, x, ldx, graph_ptr, n_graphs, n, H, Wc, out, ldo);
    return dif::launch(who, readout_fwd_kernel<T, DIF_READOUT_MAX>, grid, dim3(kBlock), 0, st, x, ldx, graph_ptr, n_graphs, n, H, Wc, out, ldo);
}

template <typename T>
int readout_bwd(const char* who, const T* x, int64_t ldx, const T* pooled, int64_t ldp, const T* grad_out, int64_t ldgo,
                const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H, int mode, T* grad_x, int64_t ldgx,
                dif_stream_t stream) {
    if (int rc = check_shape(who, n_graphs, n_rows, H, mode)) return rc;
    if (n_graphs == 0 || n_rows == 0) return 0;
    const bool is_max = mode == DIF_READOUT_MAX;
    DIF_REQUIRE(grad_out && graph_ptr && grad_x && (!is_max || (x && pooled)), DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<sizeof(T)>(grad_out) && dif::aligned<sizeof(T)>(grad_x) && dif::aligned<4>(graph_ptr) &&
                (!is_max || (dif::aligned<sizeof(T)>(x) && dif::aligned<sizeof(T)>(pooled))), DIF_E_BADARG,
                "%s: the rows must be aligned to their element and graph_ptr 4-byte", who);
    DIF_REQUIRE(ldgo >= H && ldgx >= H && (!is_max || (ldx >= H && ldp >= H)), DIF_E_BADARG,
                "%s: a leading dimension is smaller than H = %d", who, H);
    const dim3 grid = dif::grid_of(n_graphs < kMaxGrid ? n_graphs : kMaxGrid);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n = static_cast<int>(n_rows), Wc = columns_in_flight(H);
    if (mode == DIF_READOUT_ADD)
        return dif::launch(who, readout_bwd_kernel<T, DIF_READOUT_ADD>, grid, dim3(kBlock), 0, st, x, ldx, pooled, ldp, grad_out, ldgo,
                           graph_ptr, n_graphs, n, H, Wc, grad_x, ldgx);
    if (mode == DIF_READOUT_MEAN)
        return dif::launch(who, readout_bwd_kernel<T, DIF_READOUT_MEAN>, grid, dim3(kBlock), 0, st, x, ldx, pooled, ldp, grad_out, ldgo,
                           graph_ptr, n_graphs, n, H, Wc, grad_x, ldgx);
    return dif::launch(who, readout_bwd_kernel<T, DIF_READOUT_MAX>, grid, dim3(kBlock), 0, st, x, ldx, pooled, ldp, grad_out, ldgo,
                       graph_ptr, n_graphs, n, H, Wc, grad_x, ldgx);
}

inline const dif::bf16* bf(const uint16_t* p) { return reinterpret_cast<const dif::bf16*>(p); }
inline dif::bf16* bf(uint16_t* p) { return reinterpret_cast<dif::bf16*>(p); }

}  // namespace

extern "C" int dif_readout_version(void) { return DIF_READOUT_VERSION; }
extern "C" const char* dif_readout_last_error(void) { return dif::err_buf(); }

extern "C" int dif_readout_fwd_f32(const float* x, int64_t ldx, const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H,
                                   int mode, float* out, int64_t ldo, dif_stream_t stream) {
    return readout_fwd("dif_readout_fwd_f32", x, ldx, graph_ptr, n_graphs, n_rows, H, mode, out, ldo, stream);
}
extern "C" int dif_readout_fwd_bf16(const uint16_t* x, int64_t ldx, const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H,
                                    int mode, uint16_t* out, int64_t ldo, dif_stream_t stream) {
    return readout_fwd("dif_readout_fwd_bf16", bf(x), ldx, graph_ptr, n_graphs, n_rows, H, mode, bf(out), ldo, stream);
}
extern "C" int dif_readout_bwd_f32(const float* x, int64_t ldx, const float* pooled, int64_t ldp, const float* grad_out, int64_t ldgo,
                                   const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H, int mode, float* grad_x,
                                   int64_t ldgx, dif_stream_t stream) {
    return readout_bwd("dif_readout_bwd_f32", x, ldx, pooled, ldp, grad_out, ldgo, graph_ptr, n_graphs, n_rows, H, mode, grad_x, ldgx,
                       stream);
}
extern "C" int dif_readout_bwd_bf16(const uint16_t* x, int64_t ldx, const uint16_t* pooled, int64_t ldp, const uint16_t* grad_out,
                                    int64_t ldgo, const int32_t* graph_ptr, int64_t n_graphs, int64_t n_rows, int H, int mode,
                                    uint16_t* grad_x, int64_t ldgx, dif_stream_t stream) {
    return readout_bwd("dif_readout_bwd_bf16", bf(x), ldx, bf(pooled), ldp, bf(grad_out), ldgo, graph_ptr, n_graphs, n_rows, H, mode,
                       bf(grad_x), ldgx, stream);
}
