// libdifformer_nbr.so (C ABI: include/difformer_nbr.h): neighbour graphs of a batch of graphs stored back to back -- the k
// nearest neighbours (torch_cluster.knn_graph with `batch`) and the neighbours inside a radius (radius_graph), searched inside
// a row's own graph only and ranked under the float64 total order of csrc/knn_order.h.
//
// The kernel is the direct route of csrc/knn_graph.hip made aware of graph boundaries.  One wave owns 64 consecutive rows of
// the batch, one row per lane, the row held in registers as doubles.  A lane finds its graph b by binary search in graph_ptr
// (upper bound - 1, which skips empty graphs) and with it its candidate range [lo_i, hi_i).  The wave sweeps the UNION of its
// lanes' ranges, [lo of its first row, hi of its last valid row): at most its 64 rows plus the rest of the two boundary graphs.
// Candidate rows go through LDS in tiles of 64; every lane reads the same candidate, so the reads are broadcasts.  A lane
// masks what lies outside its own range (and j == i without loop), forms the float64 distance in the fixed column order of
// the single-graph routes -- the same arithmetic, so the lists agree with theirs bit for bit -- and keeps K entries
// (distance key, index), sorted, in registers.  Candidates arrive in ascending index order and the comparisons are strict, so
// among equal distances the lower index stays in front.  There is no work table, no workspace and no host wait.
//
// k-NN writes the first kk_b = min(k, n_b - (loop ? 0 : 1)) entries at edge_ptr[b] + (i - lo_i) kk_b.  The radius search puts
// the gate d < r^2 (strict; a NaN is never inside) in front of the list, counts what passes, and writes min(count, cap)
// entries to a [n][cap] workspace; after an exclusive scan of the counts (the host's) nbr_radius_edges_kernel compacts them.
#include <stdarg.h>
#include "dif_common.h"
#include "knn_order.h"
#include "../../include/difformer_nbr.h"

// dif::launch (csrc/dif_launch.h) reports through these; api.hip defines them for libdifformer_hip.so, this file for THIS
// library (linked -Bsymbolic: each library binds its own), so that its errors land in dif_nbr_last_error().
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

using dif::f32x4;
using dif::ld4;
using dif::kEmpty, dif::dist_key, dif::key_dist, dif::rnorm, dif::cos_dist, dif::insert2;

constexpr int kMaxM = DIF_NBR_MAX_COLUMNS;
constexpr int kMaxK = DIF_NBR_MAX_K;
constexpr int kMaxCap = DIF_NBR_MAX_CAP;

// grid: ceil(n / 64); block 64.  MQ: M rounded up to 4 | 8 | 16 | 32 | 64 (zero columns change no sum).  K >= k (k-NN) or
// >= cap (radius).  RADIUS: r2, cap, deg, ws_idx, ws_dist are used and edge_ptr, k, edge_index, dist are not; else the reverse.
template <int MQ, int K, bool COS, bool RADIUS>
__global__ __launch_bounds__(64) void nbr_kernel(const float* __restrict__ x, int64_t ldx, int64_t n, int M,
                                                 const int32_t* __restrict__ graph_ptr, int B, const int64_t* __restrict__ edge_ptr,
                                                 int k, int loop, double r2, int cap, int centre_row,
                                                 int64_t* __restrict__ edge_index, int64_t E, float* __restrict__ dist,
                                                 int32_t* __restrict__ deg, uint32_t* __restrict__ ws_idx, float* __restrict__ ws_dist) {
    constexpr int LD = MQ + 4;                       // row stride of the tile in floats: 16-byte rows off the 64-byte stride
    __shared__ __attribute__((aligned(16))) float tile[64 * LD];
    __shared__ double rn[64];
    __shared__ int64_t span[2];
    const int lane = threadIdx.x;
    const int64_t base = static_cast<int64_t>(blockIdx.x) * 64;
    const int64_t i = base + lane;
    const bool iok = i < n;
    const int64_t ic = iok ? i : n - 1;

    // the lane's graph: the last b with graph_ptr[b] <= i (upper bound - 1: empty graphs are skipped)
    int b = 0;
    {
        int lo = 0, hi = B + 1;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (static_cast<int64_t>(graph_ptr[mid]) <= ic) lo = mid + 1; else hi = mid;
        }
        b = lo - 1;
        b = b < 0 ? 0 : (b > B - 1 ? B - 1 : b);
    }
    int64_t glo = graph_ptr[b], ghi = graph_ptr[b + 1];
    glo = glo < 0 ? 0 : glo;
    ghi = ghi > n ? n : ghi;
    if (!(glo <= ic && ic < ghi)) glo = ghi = ic;    // a table that does not cover the row: no candidates, nothing out of range
    const int64_t last = (n - 1 - base) < 63 ? (n - 1 - base) : 63;
    if (lane == 0) span[0] = glo;
    if (lane == last) span[1] = ghi;
    if (!iok) glo = ghi = 0;

    double q[MQ];
#pragma unroll
    for (int c = 0; c < MQ / 4; ++c) {
        const f32x4 v = ld4<true>(x, ldx, ic, true, 0, 4 * c, M);
#pragma unroll
        for (int u = 0; u < 4; ++u) q[4 * c + u] = static_cast<double>(v[u]);
    }
    double rq = 0.0;
    if (COS) {
        double n2 = 0.0;
#pragma unroll
        for (int m = 0; m < MQ; ++m) n2 = fma(q[m], q[m], n2);
        rq = rnorm(n2);
    }

    uint64_t dk[K];
    uint32_t ix[K];
#pragma unroll
    for (int e = 0; e < K; ++e) {
        dk[e] = kEmpty;
        ix[e] = 0xFFFFFFFFu;
    }
    double thr = key_dist(kEmpty);                   // NaN: everything passes the gate until the list is full
    int inside = 0;                                  // RADIUS: candidates with d < r2, kept or not

    __syncthreads();
    const int64_t ulo = span[0], uhi = span[1];
    for (int64_t t = ulo; t < uhi; t += 64) {
        __syncthreads();                             // the previous tile has been read
        {
            const int64_t j = t + lane;
            const bool jok = j < uhi;
            const int64_t jc = jok ? j : uhi - 1;
            double n2 = 0.0;
#pragma unroll
            for (int c = 0; c < MQ / 4; ++c) {
                const f32x4 v = ld4<true>(x, ldx, jc, jok, 0, 4 * c, M);
                *reinterpret_cast<f32x4*>(&tile[lane * LD + 4 * c]) = v;
                if (COS) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) n2 = fma(static_cast<double>(v[u]), static_cast<double>(v[u]), n2);
                }
            }
            if (COS) rn[lane] = rnorm(n2);
        }
        __syncthreads();
        const int64_t left = uhi - t;
        const int cnt = left < 64 ? static_cast<int>(left) : 64;
        for (int jj = 0; jj < cnt; ++jj) {
            const float* kr = &tile[jj * LD];
            double d = 0.0;
            if (COS) {
#pragma unroll
                for (int m = 0; m < MQ; ++m) d = fma(q[m], static_cast<double>(kr[m]), d);
                d = cos_dist(d, rq, rn[jj]);
            } else {
#pragma unroll
                for (int m = 0; m < MQ; ++m) {
                    const double diff = q[m] - static_cast<double>(kr[m]);
                    d = fma(diff, diff, d);
                }
            }
            const int64_t j = t + jj;
            const bool mine = j >= glo && j < ghi && (loop || j != i);
            if (RADIUS) {
                if (mine && d < r2) {                // strict, and false for a NaN
                    ++inside;
                    if (!(d >= thr)) {
                        const uint64_t key = dist_key(d);
                        if (key < dk[K - 1]) {
                            insert2<K>(dk, ix, key, static_cast<uint32_t>(j));
                            thr = key_dist(dk[K - 1]);
                        }
                    }
                }
            } else {
                // the gate: one compare against the distance of the list's last entry, written so that a NaN on either side
                // passes (the threshold of a list that is not full is a NaN; a NaN distance still has to fill such a list)
                if (mine && !(d >= thr)) {
                    const uint64_t key = dist_key(d);
                    if (key < dk[K - 1]) {
                        insert2<K>(dk, ix, key, static_cast<uint32_t>(j));
                        thr = key_dist(dk[K - 1]);
                    }
                }
            }
        }
    }
    if (!iok) return;
    if (RADIUS) {
        const int dg = inside < cap ? inside : cap;
        deg[i] = dg;
        uint32_t* oi = ws_idx + i * cap;
        float* od = ws_dist + i * cap;
#pragma unroll
        for (int e = 0; e < K; ++e) {
            if (e < dg) {
                oi[e] = ix[e];
                od[e] = static_cast<float>(sqrt(key_dist(dk[e])));
            }
        }
    } else {
        const int64_t others = ghi - glo - (loop ? 0 : 1);
        const int kk = static_cast<int>(others < k ? others : k);
        const int64_t at = edge_ptr[b] + (i - glo) * kk;
        if (kk <= 0 || at < 0 || at + kk > E) return;            // never past the edge list, whatever the tables hold
        int64_t* centre = edge_index + static_cast<int64_t>(centre_row) * E + at;
        int64_t* other = edge_index + static_cast<int64_t>(1 - centre_row) * E + at;
#pragma unroll
        for (int e = 0; e < K; ++e) {
            if (e < kk) {
                centre[e] = i;
                other[e] = static_cast<int64_t>(ix[e]);
                if (dist) {
                    const double d = key_dist(dk[e]);
                    dist[at + e] = static_cast<float>(COS ? d : sqrt(d));
                }
            }
        }
    }
}

// one thread per (row, slot): slot e of row i, if kept, is edge deg_ptr[i] + e
__global__ __launch_bounds__(256) void nbr_radius_edges_kernel(const int64_t* __restrict__ deg_ptr, int64_t n, int cap, int centre_row,
                                                               const uint32_t* __restrict__ ws_idx, const float* __restrict__ ws_dist,
                                                               int64_t* __restrict__ edge_index, int64_t E, float* __restrict__ dist) {
    const int64_t t = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (t >= n * cap) return;
    const int64_t i = t / cap;
    const int e = static_cast<int>(t - i * cap);
    const int64_t first = deg_ptr[i];
    const int64_t at = first + e;
    if (e >= deg_ptr[i + 1] - first || at < 0 || at >= E) return;
    edge_index[static_cast<int64_t>(centre_row) * E + at] = i;
    edge_index[static_cast<int64_t>(1 - centre_row) * E + at] = static_cast<int64_t>(ws_idx[t]);
    if (dist) dist[at] = ws_dist[t];
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
int row_width(int M) { return M <= 4 ? 4 : (M <= 8 ? 8 : (M <= 16 ? 16 : (M <= 32 ? 32 : 64))); }

int common_checks(const char* who, const float* x, int64_t ldx, int64_t n, int M, const int32_t* graph_ptr, int B) {
    DIF_REQUIRE(n > 0 && M > 0 && B > 0, DIF_E_BADARG, "%s: n, M and B must be positive", who);
    DIF_REQUIRE(x && graph_ptr, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned16(x) && dif::aligned<4>(graph_ptr), DIF_E_BADARG,
                "%s: x must be 16-byte and graph_ptr 4-byte aligned", who);
    DIF_REQUIRE(M % 4 == 0 && M <= kMaxM, DIF_E_SHAPE, "%s: M must be a multiple of 4 up to %d (got %d); zero-pad the columns", who, kMaxM, M);
    DIF_REQUIRE(ldx >= M && ldx % 4 == 0, DIF_E_BADARG, "%s: the leading dimension must cover a row and be a multiple of 4 elements", who);
    DIF_REQUIRE(n < (1ll << 31), DIF_E_RANGE, "%s: n %lld exceeds the 31-bit row index", who, static_cast<long long>(n));
    return 0;
}

}  // namespace

extern "C" int dif_nbr_version(void) { return DIF_NBR_VERSION; }
extern "C" const char* dif_nbr_last_error(void) { return dif::err_buf(); }

// uint32 indices [n][cap], then float32 distances [n][cap]
extern "C" int64_t dif_nbr_workspace_bytes(int64_t n, int cap) {
    if (n <= 0 || n >= (1ll << 31) || cap < 1 || cap > kMaxCap) return 0;
    return n * cap * static_cast<int64_t>(sizeof(uint32_t) + sizeof(float));
}

extern "C" int dif_nbr_knn_f32(const float* x, int64_t ldx, int64_t n, int M, const int32_t* graph_ptr, const int64_t* edge_ptr, int B,
                               int k, int loop, int metric, int centre_row, int64_t* edge_index, int64_t E, float* dist_or_null,
                               dif_stream_t stream) {
    const char* who = "dif_nbr_knn_f32";
    if (int rc = common_checks(who, x, ldx, n, M, graph_ptr, B)) return rc;
    DIF_REQUIRE(edge_ptr, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<8>(edge_ptr) && dif::aligned<8>(edge_index) && dif::aligned<4>(dist_or_null), DIF_E_BADARG,
                "%s: edge_ptr and edge_index must be 8-byte and the distances 4-byte aligned", who);
    DIF_REQUIRE(k >= 1 && k <= kMaxK, DIF_E_SHAPE, "%s: k must be in [1, %d] (got %d)", who, kMaxK, k);
    DIF_REQUIRE(metric == 0 || metric == 1, DIF_E_SHAPE, "%s: unknown metric %d (0: Euclidean, 1: cosine)", who, metric);
    DIF_REQUIRE(centre_row == 0 || centre_row == 1, DIF_E_SHAPE, "%s: centre_row must be 0 or 1 (got %d)", who, centre_row);
    DIF_REQUIRE(E >= 0 && E <= n * k, DIF_E_SHAPE, "%s: E must be in [0, n k] (got %lld)", who, static_cast<long long>(E));
    if (E == 0) return 0;                                    // no graph has a neighbour to give: an empty edge list (which may have no address)
    DIF_REQUIRE(edge_index, DIF_E_BADARG, "%s: null pointer", who);
    hipStream_t st = static_cast<hipStream_t>(stream);
    loop = loop ? 1 : 0;
    return dif::with_flags([&](auto COS) {
        return dif::with_int<4, 8, 16, 32, 64>(row_width(M), [&](auto MQ) {
            return dif::with_int<8, 16, 24>(k <= 8 ? 8 : (k <= 16 ? 16 : 24), [&](auto K) {
                return dif::launch("nbr_kernel", nbr_kernel<MQ, K, COS, false>, dif::grid_of((n + 63) / 64), dim3(64), 0, st, x, ldx, n, M,
                                   graph_ptr, B, edge_ptr, k, loop, 0.0, 0, centre_row, edge_index, E, dist_or_null,
                                   static_cast<int32_t*>(nullptr), static_cast<uint32_t*>(nullptr), static_cast<float*>(nullptr));
            }, dif::no_variant(who));
        }, dif::no_variant(who));
    }, metric == 1);
}

extern "C" int dif_nbr_radius_lists_f32(const float* x, int64_t ldx, int64_t n, int M, const int32_t* graph_ptr, int B, double r,
                                        int loop, int cap, int32_t* deg, void* workspace, int64_t workspace_bytes,
                                        dif_stream_t stream) {
    const char* who = "dif_nbr_radius_lists_f32";
    if (int rc = common_checks(who, x, ldx, n, M, graph_ptr, B)) return rc;
    DIF_REQUIRE(deg && workspace, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<4>(deg) && dif::aligned16(workspace), DIF_E_BADARG,
                "%s: deg must be 4-byte and the workspace 16-byte aligned", who);
    DIF_REQUIRE(r >= 0.0, DIF_E_BADARG, "%s: r must be a number >= 0 (got %g)", who, r);
    DIF_REQUIRE(cap >= 1 && cap <= kMaxCap, DIF_E_SHAPE, "%s: cap must be in [1, %d] (got %d)", who, kMaxCap, cap);
    const int64_t need = dif_nbr_workspace_bytes(n, cap);
    DIF_REQUIRE(workspace_bytes >= need, DIF_E_WORKSPACE, "%s: workspace too small (%lld < %lld)", who,
                static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    hipStream_t st = static_cast<hipStream_t>(stream);
    loop = loop ? 1 : 0;
    uint32_t* ws_idx = static_cast<uint32_t*>(workspace);
    float* ws_dist = reinterpret_cast<float*>(ws_idx + n * cap);
    return dif::with_int<4, 8, 16, 32, 64>(row_width(M), [&](auto MQ) {
        return dif::with_int<8, 16, 32>(cap <= 8 ? 8 : (cap <= 16 ? 16 : 32), [&](auto K) {
            return dif::launch("nbr_kernel", nbr_kernel<MQ, K, false, true>, dif::grid_of((n + 63) / 64), dim3(64), 0, st, x, ldx, n, M,
                               graph_ptr, B, static_cast<const int64_t*>(nullptr), 0, loop, r * r, cap, 0,
                               static_cast<int64_t*>(nullptr), static_cast<int64_t>(0), static_cast<float*>(nullptr), deg, ws_idx, ws_dist);
        }, dif::no_variant(who));
    }, dif::no_variant(who));
}

extern "C" int dif_nbr_radius_edges(const int64_t* deg_ptr, int64_t n, int cap, int centre_row, const void* workspace,
                                    int64_t workspace_bytes, int64_t* edge_index, int64_t E, float* dist_or_null, dif_stream_t stream) {
    const char* who = "dif_nbr_radius_edges";
    DIF_REQUIRE(n > 0, DIF_E_BADARG, "%s: n must be positive", who);
    DIF_REQUIRE(deg_ptr && workspace, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<8>(deg_ptr) && dif::aligned16(workspace) && dif::aligned<8>(edge_index) && dif::aligned<4>(dist_or_null),
                DIF_E_BADARG, "%s: deg_ptr and edge_index must be 8-byte, the workspace 16-byte and the distances 4-byte aligned", who);
    DIF_REQUIRE(cap >= 1 && cap <= kMaxCap, DIF_E_SHAPE, "%s: cap must be in [1, %d] (got %d)", who, kMaxCap, cap);
    DIF_REQUIRE(centre_row == 0 || centre_row == 1, DIF_E_SHAPE, "%s: centre_row must be 0 or 1 (got %d)", who, centre_row);
    DIF_REQUIRE(n < (1ll << 31), DIF_E_RANGE, "%s: n %lld exceeds the 31-bit row index", who, static_cast<long long>(n));
    DIF_REQUIRE(E >= 0 && E <= n * cap, DIF_E_SHAPE, "%s: E must be in [0, n cap] (got %lld)", who, static_cast<long long>(E));
    const int64_t need = dif_nbr_workspace_bytes(n, cap);
    DIF_REQUIRE(workspace_bytes >= need, DIF_E_WORKSPACE, "%s: workspace too small (%lld < %lld)", who,
                static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    if (E == 0) return 0;                                    // no row has a neighbour inside: an empty edge list (which may have no address)
    DIF_REQUIRE(edge_index, DIF_E_BADARG, "%s: null pointer", who);
    const uint32_t* ws_idx = static_cast<const uint32_t*>(workspace);
    const float* ws_dist = reinterpret_cast<const float*>(ws_idx + n * cap);
    return dif::launch("nbr_radius_edges_kernel", nbr_radius_edges_kernel, dif::grid_of((n * cap + 255) / 256), dim3(256), 0,
                       static_cast<hipStream_t>(stream), deg_ptr, n, cap, centre_row, ws_idx, ws_dist, edge_index, E, dist_or_null);
}
