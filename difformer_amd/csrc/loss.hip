// Training losses on the device: libdifformer_loss.so, C ABI in include/difformer_loss.h.
//
// Replaces, between the logits and loss.backward() of the reference's drivers (node classification/main.py:121-129,
// main-batch.py:136-140, eval.py:19-29, image and text/main.py:107-109, physical particle/main.py:88), the chain
// log_softmax -> two gathers -> nll_loss (or the label conversion -> two gathers -> binary_cross_entropy_with_logits) and its
// backward nodes by one pass over the logits each way.  The row selection arrives as a per-row weight (the multiplicity of
// the row in the index, or a boolean mask), so nothing is gathered and nothing depends on how many rows are selected.
//
// Arithmetic, order of summation and edge semantics: the header.  In short: every logit is widened to float64, the row is
// evaluated in float64 without a cancelling term, weight * loss is summed per workgroup over a row range that depends on (n, C)
// only and then by one workgroup over the partials; integers are the only thing ever added atomically (dif_loss_row_weights).
//
// Layout: W = the smallest power of two >= C, at most 64, lanes per row; a workgroup of 256 threads holds R = 256 / W rows per
// pass.  A lane owns the columns sub, sub + W, ...: for C <= 64 that is one element, reduced across the lanes of the group with
// xor shuffles below W (partners are lanes of the same row, so groups of one wave may diverge); for C > 64 the wave loops.
#include <stdarg.h>
#include "dif_common.h"
#include "../../include/difformer_loss.h"

// dif::launch (csrc/dif_launch.h) reports through these; this library is linked -Bsymbolic and binds its own, so that its
// errors land in dif_loss_last_error().
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
constexpr int kMaxColumns = 65536;
constexpr int kMaxGroups = 1024;                          // workgroups (= partials) of a forward
constexpr int64_t kMaxBwdBlocks = 1 << 16;                // the backward strides over the rows beyond that
constexpr int64_t kMaxIndex = (int64_t(1) << 31) - 1;     // int32 multiplicities
typedef long long i64;

struct Record {                                            // DIF_LOSS_RECORD_BYTES of the header
    double loss;
    float loss32;
    int32_t unused;
    i64 count;
    i64 invalid;
};
static_assert(sizeof(Record) == DIF_LOSS_RECORD_BYTES, "the record of include/difformer_loss.h");

// ---- operands -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double widen(const float* p) { return static_cast<double>(*p); }
__device__ __forceinline__ double widen(const dif::bf16* p) { return static_cast<double>(dif::bf16_to_f32(p->bits)); }

// one rounding from float64 (dif::f64_to_bf16 does not go through float32's)
__device__ __forceinline__ void store(float* p, double v) { *p = static_cast<float>(v); }
__device__ __forceinline__ void store(dif::bf16* p, double v) { p->bits = dif::f64_to_bf16(v); }

__device__ __forceinline__ int row_weight(const void* rows, int kind, int64_t r) {
    if (kind == DIF_LOSS_ROWS_WEIGHTS) {
        const int32_t w = static_cast<const int32_t*>(rows)[r];
        return w > 0 ? w : 0;
    }
    if (kind == DIF_LOSS_ROWS_MASK) return static_cast<const uint8_t*>(rows)[r] ? 1 : 0;
    return 1;
}

__device__ __forceinline__ double target_at(const void* t, int type, int64_t i) {
    if (type == DIF_LOSS_TARGET_I64) return static_cast<double>(static_cast<const i64*>(t)[i]);
    if (type == DIF_LOSS_TARGET_F32) return static_cast<double>(static_cast<const float*>(t)[i]);
    return static_cast<double>(static_cast<const uint8_t*>(t)[i]);
}

// ---- reductions -----------------------------------------------------------------------------------------------------------------
// over the W lanes of a row: every lane of the group gets the result (the same bits: a + b == b + a)
__device__ __forceinline__ double group_sum(double v, int W) {
    for (int off = W >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}
__device__ __forceinline__ double group_max(double v, int W) {
    for (int off = W >> 1; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
    return v;
}

// {loss, count, invalid} of the workgroup -> its partial; every thread of the workgroup arrives here
__device__ __forceinline__ void write_partial(double acc, i64 cnt, i64 inv, double* part_loss, i64* part_count, i64* part_invalid) {
    __shared__ double sl[kBlock / 64];
    __shared__ i64 sc[kBlock / 64], si[kBlock / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
        inv += __shfl_xor(inv, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sl[threadIdx.x >> 6] = acc;
        sc[threadIdx.x >> 6] = cnt;
        si[threadIdx.x >> 6] = inv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part_loss[blockIdx.x] = ((sl[0] + sl[1]) + sl[2]) + sl[3];
        part_count[blockIdx.x] = sc[0] + sc[1] + sc[2] + sc[3];
        part_invalid[blockIdx.x] = si[0] + si[1] + si[2] + si[3];
    }
}

// sigmoid(z) in float64 with no cancellation at either end
__device__ __forceinline__ double sigmoid64(double z) {
    if (z >= 0.0) return 1.0 / (1.0 + exp(-z));
    const double e = exp(z);
    return e / (1.0 + e);
}

// ---- the row of the NLL ---------------------------------------------------------------------------------------------------------------
// m = max, so = sum over the columns other than the label of exp(x - m), el = exp(x_label - m), d = x_label - m; in every lane
// of the row's group
template <typename T>
__device__ __forceinline__ void nll_row(const T* __restrict__ xr, int C, int W, int sub, int64_t label, double& m, double& so,
                                        double& el, double& d) {
    m = -INFINITY;
    for (int c = sub; c < C; c += W) m = fmax(m, widen(xr + c));
    m = group_max(m, W);
    double s = 0.0;
    for (int c = sub; c < C; c += W) {
        const double e = exp(widen(xr + c) - m);             // NaN (and +inf - +inf) reaches the sum; fmax alone would hide it
        if (c != label) s += e;
    }
    so = group_sum(s, W);
    d = widen(xr + label) - m;
    el = exp(d);
}

// ---- forward --------------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(kBlock) void nll_fwd_kernel(const T* __restrict__ x, int64_t ldx, const i64* __restrict__ label,
                                                         i64 ignore_index, const void* __restrict__ rows, int rows_kind, int64_t n,
                                                         int C, int W, int64_t rows_per_group, double* __restrict__ part_loss,
                                                         i64* __restrict__ part_count, i64* __restrict__ part_invalid) {
    const int sub = threadIdx.x & (W - 1), slot = threadIdx.x / W, slots = kBlock / W;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_group;
    const int64_t r1 = r0 + rows_per_group < n ? r0 + rows_per_group : n;
    double acc = 0.0;
    i64 cnt = 0, inv = 0;
    for (int64_t r = r0 + slot; r < r1; r += slots) {
        const int w = row_weight(rows, rows_kind, r);
        if (w == 0) continue;
        const i64 lab = label[r];
        if (lab == ignore_index) continue;
        if (lab < 0 || lab >= C) {
            if (sub == 0) inv += w;
            continue;
        }
        double m, so, el, d;
        nll_row(x + r * ldx, C, W, sub, lab, m, so, el, d);
        const double l = d == 0.0 ? log1p(so) : log(so + el) - d;
        if (sub == 0) {
            acc += static_cast<double>(w) * l;
            cnt += w;
        }
    }
    write_partial(acc, cnt, inv, part_loss, part_count, part_invalid);
}

template <typename T>
__global__ __launch_bounds__(kBlock) void bce_fwd_kernel(const T* __restrict__ x, int64_t ldx, const void* __restrict__ target,
                                                         int target_type, int64_t ldt, const void* __restrict__ rows, int rows_kind,
                                                         int64_t n, int C, int W, int64_t rows_per_group,
                                                         double* __restrict__ part_loss, i64* __restrict__ part_count,
                                                         i64* __restrict__ part_invalid) {
    const int sub = threadIdx.x & (W - 1), slot = threadIdx.x / W, slots = kBlock / W;
    const int64_t r0 = static_cast<int64_t>(blockIdx.x) * rows_per_group;
    const int64_t r1 = r0 + rows_per_group < n ? r0 + rows_per_group : n;
    double acc = 0.0;
    i64 cnt = 0;
    for (int64_t r = r0 + slot; r < r1; r += slots) {
        const int w = row_weight(rows, rows_kind, r);
        if (w == 0) continue;
        const T* xr = x + r * ldx;
        double s = 0.0;
        for (int c = sub; c < C; c += W) {
            const double v = widen(xr + c), t = target_at(target, target_type, r * ldt + c);
            s += (fmax(v, 0.0) - v * t) + log1p(exp(-fabs(v)));
        }
        s = group_sum(s, W);
        if (sub == 0) {
            acc += static_cast<double>(w) * s;
            cnt += static_cast<i64>(w) * C;
        }
    }
    write_partial(acc, cnt, 0, part_loss, part_count, part_invalid);
}

// one workgroup: lane t sums the partials t, t + 256, ... in index order, then the workgroup's lanes are summed in a fixed tree
__global__ __launch_bounds__(kBlock) void loss_finish_kernel(const double* __restrict__ part_loss, const i64* __restrict__ part_count,
                                                             const i64* __restrict__ part_invalid, int groups,
                                                             const int32_t* __restrict__ index_status, Record* __restrict__ rec) {
    __shared__ double sl[kBlock / 64];
    __shared__ i64 sc[kBlock / 64], si[kBlock / 64];
    double acc = 0.0;
    i64 cnt = 0, inv = 0;
    for (int g = threadIdx.x; g < groups; g += kBlock) {
        acc += part_loss[g];
        cnt += part_count[g];
        inv += part_invalid[g];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        acc += __shfl_xor(acc, off, 64);
        cnt += __shfl_xor(cnt, off, 64);
        inv += __shfl_xor(inv, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        sl[threadIdx.x >> 6] = acc;
        sc[threadIdx.x >> 6] = cnt;
        si[threadIdx.x >> 6] = inv;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double sum = ((sl[0] + sl[1]) + sl[2]) + sl[3];
        const i64 count = sc[0] + sc[1] + sc[2] + sc[3];
        i64 invalid = si[0] + si[1] + si[2] + si[3];
        if (index_status) invalid += static_cast<uint32_t>(*index_status);
        const double loss = (count > 0 && invalid == 0) ? sum / static_cast<double>(count) : static_cast<double>(NAN);
        rec->loss = loss;
        rec->loss32 = static_cast<float>(loss);
        rec->unused = 0;
        rec->count = count;
        rec->invalid = invalid;
    }
}

// ---- backward -------------------------------------------------------------------------------------------------------------------------
// upstream / count, or 0 when nothing was selected (every row then takes the +0 branch anyway)
__device__ __forceinline__ double grad_scale(const Record* rec, const float* upstream) {
    const i64 count = rec->count;
    return count > 0 ? static_cast<double>(*upstream) / static_cast<double>(count) : 0.0;
}

template <typename T>
__global__ __launch_bounds__(kBlock) void nll_bwd_kernel(const T* __restrict__ x, int64_t ldx, const i64* __restrict__ label,
                                                         i64 ignore_index, const void* __restrict__ rows, int rows_kind, int64_t n,
                                                         int C, int W, const Record* __restrict__ rec,
                                                         const float* __restrict__ upstream, T* __restrict__ grad, int64_t ldg) {
    const int sub = threadIdx.x & (W - 1), slot = threadIdx.x / W, slots = kBlock / W;
    const double scale = grad_scale(rec, upstream);
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * slots + slot; r < n; r += static_cast<int64_t>(gridDim.x) * slots) {
        const int w = row_weight(rows, rows_kind, r);
        const i64 lab = label[r];
        T* gr = grad + r * ldg;
        if (w == 0 || lab == ignore_index || lab < 0 || lab >= C) {
            for (int c = sub; c < C; c += W) store(gr + c, 0.0);
            continue;
        }
        const T* xr = x + r * ldx;
        double m, so, el, d;
        nll_row(xr, C, W, sub, lab, m, so, el, d);
        const double S = so + el, f = static_cast<double>(w) * scale;
        for (int c = sub; c < C; c += W) {
            const double g = c == lab ? -(so / S) : exp(widen(xr + c) - m) / S;
            store(gr + c, f * g);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void bce_bwd_kernel(const T* __restrict__ x, int64_t ldx, const void* __restrict__ target,
                                                         int target_type, int64_t ldt, const void* __restrict__ rows, int rows_kind,
                                                         int64_t n, int C, int W, const Record* __restrict__ rec,
                                                         const float* __restrict__ upstream, T* __restrict__ grad, int64_t ldg) {
    const int sub = threadIdx.x & (W - 1), slot = threadIdx.x / W, slots = kBlock / W;
    const double scale = grad_scale(rec, upstream);
    for (int64_t r = static_cast<int64_t>(blockIdx.x) * slots + slot; r < n; r += static_cast<int64_t>(gridDim.x) * slots) {
        const int w = row_weight(rows, rows_kind, r);
        T* gr = grad + r * ldg;
        if (w == 0) {
            for (int c = sub; c < C; c += W) store(gr + c, 0.0);
            continue;
        }
        const T* xr = x + r * ldx;
        const double f = static_cast<double>(w) * scale;
        for (int c = sub; c < C; c += W) {
            const double v = widen(xr + c), t = target_at(target, target_type, r * ldt + c);
            const double g = t == 1.0 ? -sigmoid64(-v) : (t == 0.0 ? sigmoid64(v) : sigmoid64(v) - t);
            store(gr + c, f * g);
        }
    }
}

// ---- row multiplicities -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void row_weights_kernel(const i64* __restrict__ index, int64_t m, int64_t n,
                                                             int32_t* __restrict__ weight, int32_t* __restrict__ status) {
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x; i < m; i += static_cast<int64_t>(gridDim.x) * kBlock) {
        const i64 r = index[i];
        if (r >= 0 && r < n) atomicAdd(&weight[r], 1);
        else atomicAdd(status, 1);
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
struct Geom {
    int W;                       // lanes per row
    int64_t need;                // workgroup passes that cover n rows
    int groups;                  // workgroups of the forward
    int64_t rows_per_group;
    size_t off_count, off_invalid, total;
};

int make_geom(const char* who, int64_t n, int C, Geom& g) {
    DIF_REQUIRE(n >= 0, DIF_E_BADARG, "%s: need n >= 0 (got %lld)", who, static_cast<long long>(n));
    DIF_REQUIRE(C >= 1 && C <= kMaxColumns, DIF_E_SHAPE, "%s: need 1 <= C <= %d (got %d)", who, kMaxColumns, C);
    g.W = 1;
    while (g.W < C && g.W < 64) g.W *= 2;
    const int R = kBlock / g.W;
    g.need = (n + R - 1) / R;
    if (g.need < 1) g.need = 1;
    g.groups = static_cast<int>(g.need < kMaxGroups ? g.need : kMaxGroups);
    g.rows_per_group = (g.need + g.groups - 1) / g.groups * R;
    g.off_count = static_cast<size_t>(g.groups) * 8;
    g.off_invalid = static_cast<size_t>(g.groups) * 16;
    g.total = (static_cast<size_t>(g.groups) * 24 + 255) / 256 * 256;
    return 0;
}

int check_rows(const char* who, const void* rows, int rows_kind, int64_t n) {
    DIF_REQUIRE(rows_kind == DIF_LOSS_ROWS_ALL || rows_kind == DIF_LOSS_ROWS_WEIGHTS || rows_kind == DIF_LOSS_ROWS_MASK, DIF_E_BADARG,
                "%s: rows_kind %d is none of DIF_LOSS_ROWS_*", who, rows_kind);
    DIF_REQUIRE(rows_kind == DIF_LOSS_ROWS_ALL || rows || n == 0, DIF_E_BADARG, "%s: null row selection", who);
    DIF_REQUIRE(rows_kind != DIF_LOSS_ROWS_WEIGHTS || dif::aligned<4>(rows), DIF_E_BADARG, "%s: row weights must be 4-byte aligned", who);
    return 0;
}

int check_target(const char* who, const void* target, int target_type, int64_t ldt, int64_t n, int C) {
    DIF_REQUIRE(target_type == DIF_LOSS_TARGET_I64 || target_type == DIF_LOSS_TARGET_F32 || target_type == DIF_LOSS_TARGET_U8,
                DIF_E_BADARG, "%s: target_type %d is none of DIF_LOSS_TARGET_*", who, target_type);
    DIF_REQUIRE(target || n == 0, DIF_E_BADARG, "%s: null pointer", who);
    const bool ok = target_type == DIF_LOSS_TARGET_I64 ? dif::aligned<8>(target) : target_type == DIF_LOSS_TARGET_F32 ? dif::aligned<4>(target) : true;
    DIF_REQUIRE(ok, DIF_E_BADARG, "%s: the target must be aligned to its element", who);
    DIF_REQUIRE(ldt >= C, DIF_E_BADARG, "%s: leading dimension %lld smaller than C = %d", who, static_cast<long long>(ldt), C);
    return 0;
}

// what the forward entry points share: geometry, the logits, the record and the workspace
template <typename T>
int check_fwd(const char* who, const T* x, int64_t ldx, const void* rows, int rows_kind, const int32_t* index_status, int64_t n,
              int C, void* record, void* workspace, int64_t workspace_bytes, Geom& g) {
    if (int rc = make_geom(who, n, C, g)) return rc;
    DIF_REQUIRE((x || n == 0) && record && workspace, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<sizeof(T)>(x) && dif::aligned<8>(record) && dif::aligned<16>(workspace) && dif::aligned<4>(index_status),
                DIF_E_BADARG, "%s: the logits must be aligned to their element, the record 8-byte, the workspace 16-byte and "
                "index_status 4-byte", who);
    DIF_REQUIRE(ldx >= C, DIF_E_BADARG, "%s: leading dimension %lld smaller than C = %d", who, static_cast<long long>(ldx), C);
    if (int rc = check_rows(who, rows, rows_kind, n)) return rc;
    DIF_REQUIRE(workspace_bytes >= 0 && static_cast<size_t>(workspace_bytes) >= g.total, DIF_E_WORKSPACE,
                "%s: workspace too small (%lld < %zu)", who, static_cast<long long>(workspace_bytes), g.total);
    return 0;
}

template <typename T>
int check_bwd(const char* who, const T* x, int64_t ldx, const void* rows, int rows_kind, int64_t n, int C, const void* record,
              const float* upstream, T* grad, int64_t ldg, Geom& g) {
    if (int rc = make_geom(who, n, C, g)) return rc;
    DIF_REQUIRE(((x && grad) || n == 0) && record && upstream, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<sizeof(T)>(x) && dif::aligned<sizeof(T)>(grad) && dif::aligned<8>(record) && dif::aligned<4>(upstream),
                DIF_E_BADARG, "%s: the logits and the gradient must be aligned to their element, the record 8-byte and the "
                "upstream scalar 4-byte", who);
    DIF_REQUIRE(ldx >= C && ldg >= C, DIF_E_BADARG, "%s: leading dimensions (%lld, %lld) smaller than C = %d", who,
                static_cast<long long>(ldx), static_cast<long long>(ldg), C);
    return check_rows(who, rows, rows_kind, n);
}

int finish(const char* who, const Geom& g, char* ws, const int32_t* index_status, void* record, hipStream_t st) {
    return dif::launch(who, loss_finish_kernel, dim3(1), dim3(kBlock), 0, st, reinterpret_cast<const double*>(ws),
                       reinterpret_cast<const i64*>(ws + g.off_count), reinterpret_cast<const i64*>(ws + g.off_invalid), g.groups,
                       index_status, static_cast<Record*>(record));
}

template <typename T>
int nll_fwd(const char* who, const T* x, int64_t ldx, const int64_t* label, int64_t ignore_index, const void* rows, int rows_kind,
            const int32_t* index_status, int64_t n, int C, void* record, void* workspace, int64_t workspace_bytes, dif_stream_t stream) {
    Geom g;
    if (int rc = check_fwd(who, x, ldx, rows, rows_kind, index_status, n, C, record, workspace, workspace_bytes, g)) return rc;
    DIF_REQUIRE((label || n == 0) && dif::aligned<8>(label), DIF_E_BADARG, "%s: the labels must be int64 and 8-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    if (int rc = dif::launch(who, nll_fwd_kernel<T>, dif::grid_of(g.groups), dim3(kBlock), 0, st, x, ldx,
                             reinterpret_cast<const i64*>(label), static_cast<i64>(ignore_index), rows, rows_kind, n, C, g.W,
                             g.rows_per_group, reinterpret_cast<double*>(ws), reinterpret_cast<i64*>(ws + g.off_count),
                             reinterpret_cast<i64*>(ws + g.off_invalid))) return rc;
    return finish(who, g, ws, index_status, record, st);
}

template <typename T>
int nll_bwd(const char* who, const T* x, int64_t ldx, const int64_t* label, int64_t ignore_index, const void* rows, int rows_kind,
            int64_t n, int C, const void* record, const float* upstream, T* grad, int64_t ldg, dif_stream_t stream) {
    Geom g;
    if (int rc = check_bwd(who, x, ldx, rows, rows_kind, n, C, record, upstream, grad, ldg, g)) return rc;
    DIF_REQUIRE((label || n == 0) && dif::aligned<8>(label), DIF_E_BADARG, "%s: the labels must be int64 and 8-byte aligned", who);
    if (n == 0) return 0;
    return dif::launch(who, nll_bwd_kernel<T>, dif::grid_of(g.need < kMaxBwdBlocks ? g.need : kMaxBwdBlocks), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), x, ldx, reinterpret_cast<const i64*>(label), static_cast<i64>(ignore_index),
                       rows, rows_kind, n, C, g.W, static_cast<const Record*>(record), upstream, grad, ldg);
}

template <typename T>
int bce_fwd(const char* who, const T* x, int64_t ldx, const void* target, int target_type, int64_t ldt, const void* rows,
            int rows_kind, const int32_t* index_status, int64_t n, int C, void* record, void* workspace, int64_t workspace_bytes,
            dif_stream_t stream) {
    Geom g;
    if (int rc = check_fwd(who, x, ldx, rows, rows_kind, index_status, n, C, record, workspace, workspace_bytes, g)) return rc;
    if (int rc = check_target(who, target, target_type, ldt, n, C)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    if (int rc = dif::launch(who, bce_fwd_kernel<T>, dif::grid_of(g.groups), dim3(kBlock), 0, st, x, ldx, target, target_type, ldt,
                             rows, rows_kind, n, C, g.W, g.rows_per_group, reinterpret_cast<double*>(ws),
                             reinterpret_cast<i64*>(ws + g.off_count), reinterpret_cast<i64*>(ws + g.off_invalid))) return rc;
    return finish(who, g, ws, index_status, record, st);
}

template <typename T>
int bce_bwd(const char* who, const T* x, int64_t ldx, const void* target, int target_type, int64_t ldt, const void* rows,
            int rows_kind, int64_t n, int C, const void* record, const float* upstream, T* grad, int64_t ldg, dif_stream_t stream) {
    Geom g;
    if (int rc = check_bwd(who, x, ldx, rows, rows_kind, n, C, record, upstream, grad, ldg, g)) return rc;
    if (int rc = check_target(who, target, target_type, ldt, n, C)) return rc;
    if (n == 0) return 0;
    return dif::launch(who, bce_bwd_kernel<T>, dif::grid_of(g.need < kMaxBwdBlocks ? g.need : kMaxBwdBlocks), dim3(kBlock), 0,
                       static_cast<hipStream_t>(stream), x, ldx, target, target_type, ldt, rows, rows_kind, n, C, g.W,
                       static_cast<const Record*>(record), upstream, grad, ldg);
}

inline const dif::bf16* bf(const uint16_t* p) { return reinterpret_cast<const dif::bf16*>(p); }
inline dif::bf16* bf(uint16_t* p) { return reinterpret_cast<dif::bf16*>(p); }

}  // namespace

extern "C" int dif_loss_version(void) { return DIF_LOSS_VERSION; }
extern "C" const char* dif_loss_last_error(void) { return dif::err_buf(); }

extern "C" int64_t dif_loss_workspace_bytes(int64_t n, int C) {
    Geom g;
    if (make_geom("dif_loss_workspace_bytes", n, C, g)) return 0;
    return static_cast<int64_t>(g.total);
}

extern "C" int dif_loss_row_weights(const int64_t* index, int64_t m, int64_t n, int32_t* weight, int32_t* status,
                                    dif_stream_t stream) {
    const char* who = "dif_loss_row_weights";
    DIF_REQUIRE(m >= 0 && m <= kMaxIndex && n >= 0, DIF_E_BADARG, "%s: need 0 <= m <= 2^31 - 1 and n >= 0 (got m = %lld, n = %lld)",
                who, static_cast<long long>(m), static_cast<long long>(n));
    DIF_REQUIRE((index || m == 0) && (weight || n == 0) && status, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<8>(index) && dif::aligned<4>(weight) && dif::aligned<4>(status), DIF_E_BADARG,
                "%s: index must be 8-byte, weight and status 4-byte aligned", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipError_t he = hipMemsetAsync(status, 0, 4, st);
    if (he == hipSuccess && n > 0) he = hipMemsetAsync(weight, 0, static_cast<size_t>(n) * 4, st);
    if (he != hipSuccess) return dif::fail(static_cast<int>(he), "%s: memset: %s", who, hipGetErrorString(he));
    if (m == 0) return 0;
    const int64_t blocks = (m + kBlock - 1) / kBlock;
    return dif::launch(who, row_weights_kernel, dif::grid_of(blocks < kMaxBwdBlocks ? blocks : kMaxBwdBlocks), dim3(kBlock), 0, st,
                       reinterpret_cast<const i64*>(index), m, n, weight, status);
}

extern "C" int dif_nll_log_softmax_fwd_f32(const float* x, int64_t ldx, const int64_t* label, int64_t ignore_index, const void* rows,
                                           int rows_kind, const int32_t* index_status, int64_t n, int C, void* record,
                                           void* workspace, int64_t workspace_bytes, dif_stream_t stream) {
    return nll_fwd("dif_nll_log_softmax_fwd_f32", x, ldx, label, ignore_index, rows, rows_kind, index_status, n, C, record, workspace,
                   workspace_bytes, stream);
}
extern "C" int dif_nll_log_softmax_fwd_bf16(const uint16_t* x, int64_t ldx, const int64_t* label, int64_t ignore_index,
                                            const void* rows, int rows_kind, const int32_t* index_status, int64_t n, int C,
                                            void* record, void* workspace, int64_t workspace_bytes, dif_stream_t stream) {
    return nll_fwd("dif_nll_log_softmax_fwd_bf16", bf(x), ldx, label, ignore_index, rows, rows_kind, index_status, n, C, record,
                   workspace, workspace_bytes, stream);
}
extern "C" int dif_nll_log_softmax_bwd_f32(const float* x, int64_t ldx, const int64_t* label, int64_t ignore_index, const void* rows,
                                           int rows_kind, int64_t n, int C, const void* record, const float* upstream, float* grad,
                                           int64_t ldg, dif_stream_t stream) {
    return nll_bwd("dif_nll_log_softmax_bwd_f32", x, ldx, label, ignore_index, rows, rows_kind, n, C, record, upstream, grad, ldg,
                   stream);
}
extern "C" int dif_nll_log_softmax_bwd_bf16(const uint16_t* x, int64_t ldx, const int64_t* label, int64_t ignore_index,
                                            const void* rows, int rows_kind, int64_t n, int C, const void* record,
                                            const float* upstream, uint16_t* grad, int64_t ldg, dif_stream_t stream) {
    return nll_bwd("dif_nll_log_softmax_bwd_bf16", bf(x), ldx, label, ignore_index, rows, rows_kind, n, C, record, upstream, bf(grad),
                   ldg, stream);
}

extern "C" int dif_bce_with_logits_fwd_f32(const float* x, int64_t ldx, const void* target, int target_type, int64_t ldt,
                                           const void* rows, int rows_kind, const int32_t* index_status, int64_t n, int C,
                                           void* record, void* workspace, int64_t workspace_bytes, dif_stream_t stream) {
    return bce_fwd("dif_bce_with_logits_fwd_f32", x, ldx, target, target_type, ldt, rows, rows_kind, index_status, n, C, record,
                   workspace, workspace_bytes, stream);
}
extern "C" int dif_bce_with_logits_fwd_bf16(const uint16_t* x, int64_t ldx, const void* target, int target_type, int64_t ldt,
                                            const void* rows, int rows_kind, const int32_t* index_status, int64_t n, int C,
                                            void* record, void* workspace, int64_t workspace_bytes, dif_stream_t stream) {
    return bce_fwd("dif_bce_with_logits_fwd_bf16", bf(x), ldx, target, target_type, ldt, rows, rows_kind, index_status, n, C, record,
                   workspace, workspace_bytes, stream);
}
extern "C" int dif_bce_with_logits_bwd_f32(const float* x, int64_t ldx, const void* target, int target_type, int64_t ldt,
                                           const void* rows, int rows_kind, int64_t n, int C, const void* record,
                                           const float* upstream, float* grad, int64_t ldg, dif_stream_t stream) {
    return bce_bwd("dif_bce_with_logits_bwd_f32", x, ldx, target, target_type, ldt, rows, rows_kind, n, C, record, upstream, grad, ldg,
                   stream);
}
extern "C" int dif_bce_with_logits_bwd_bf16(const uint16_t* x, int64_t ldx, const void* target, int target_type, int64_t ldt,
                                            const void* rows, int rows_kind, int64_t n, int C, const void* record,
                                            const float* upstream, uint16_t* grad, int64_t ldg, dif_stream_t stream) {
    return bce_bwd("dif_bce_with_logits_bwd_bf16", bf(x), ldx, target, target_type, ldt, rows, rows_kind, n, C, record, upstream,
                   bf(grad), ldg, stream);
}
