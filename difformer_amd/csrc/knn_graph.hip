// libdifformer_knn.so (C ABI: include/difformer_knn.h): the k-nearest-neighbour graph of the rows of x [N, M] as an int64 edge
// list, ranked by float64 distances under one total order (smaller distance, then lower index, NaN last) -- what
// torch_cluster.knn_graph (spatial-temporal/main.py:96-98) and sklearn's kneighbors_graph (image and text/main.py:52-53)
// hand the reference, without an N x N tensor.  Two routes behind one entry point; both rank by the SAME float64 arithmetic
// (columns ascending, explicit fma; rnorm / cos_dist below), so they agree with each other bit for bit.
//
// Direct route (M <= 16; the per-snapshot call of the spatial-temporal loop).  One lane owns one query row, held in registers
// as doubles.  Key rows are staged through LDS in tiles of 64; every lane reads the same key, so the reads are broadcasts.  The
// lane keeps K (8 | 16 | 24 >= kk) entries (distance key, index), sorted, in registers with static indices only.  A distance
// is first compared with the distance of the list's last entry; what passes is made a 64-bit key (order-preserving bits of
// the double; NaN just below the empty slot) and enters through a compare-exchange chain.  Keys arrive in ascending index
// order and the comparisons are strict, so among equal distances the lower index stays in front.  The key rows are cut into
// S ranges (grid y) so that a graph of a thousand nodes fills the chip; a merge kernel inserts the S lists of a row in range
// order under the same rule -- the result does not depend on S.  With S == 1 the sweep writes the edge list itself.
//
// Sweep route (any M <= 512).  (1) A pre-pass writes h[j] = |x_j|^2 / 2 (Euclidean) or the normalised rows and h = 0 (cosine).
// (2) The sweep of csrc/attn_topk.hip: rank keys x_i . x_j - h[j] (larger = nearer) on v_mfma_f32_16x16x4_f32, contraction in
// a fixed order (identical rows give bit-identical keys), 64-bit candidate words (csrc/topk_select.h), the best C = 32 per row
// and key range -- not kk: the spare slots are the guard band that absorbs the float32 error of the expanded form.  (3) The
// re-rank kernel, 32 lanes per row: merges the S lists (rank of every word among the other list, through LDS), recomputes the
// float64 distance of its candidate by direct difference, ranks the candidates by counting under the total order, drops self
// when asked, and writes the first kk.  The float32 key only decides membership of the candidate list; a true neighbour is
// lost only when more points than the 32 - kk - 1 spare slots lie within float32 rounding of the kk-th distance: the one
// documented limit of this route.
//
// The last kernel of either route writes edge_index [2, N kk] in the requested layout and, if asked, the distances.
#include <stdarg.h>
#include "dif_common.h"
#include "topk_select.h"
#include "knn_order.h"
#include "../../include/difformer_knn.h"

// dif::launch (csrc/dif_launch.h) reports through these; api.hip defines them for libdifformer_hip.so, this file for THIS
// library (linked -Bsymbolic: each library binds its own), so that its errors land in dif_knn_last_error().
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
using dif::candidate, dif::fold, dif::insert, dif::key_score;
using dif::kEmpty, dif::kNaNKey, dif::dist_key, dif::key_dist, dif::rnorm, dif::cos_dist, dif::insert2;

constexpr int kMaxK = 24;
constexpr int kMaxM = 512;
constexpr int kDirectM = 16;           // widest row the direct route holds in registers
constexpr int kCand = 32;              // candidates per row the sweep route keeps
constexpr int kQT = 2;                 // sweep: 16-query tiles per wave
constexpr int kQGroup = 16 * kQT;
constexpr int kMaxSplits = 32;
constexpr int kMinTilesPerSplit = 4;   // sweep: a key range holds at least this many 16-key tiles
constexpr int64_t kFillWaves = 2 * 4 * dif::kCUs;     // two waves on each of the chip's SIMDs

// ---- the float64 order: csrc/knn_order.h (shared with csrc/nbr_batched.hip) ---------------------------------------------------
// the first kk entries of row i's list -> edge_index [2][E] (row `centre_row` holds i) and dist [E]
template <int K, bool COS>
__device__ __forceinline__ void write_row(const uint64_t (&dk)[K], const uint32_t (&ix)[K], int64_t i, int kk, int centre_row,
                                          int64_t E, int64_t* __restrict__ edge_index, float* __restrict__ dist) {
    int64_t* centre = edge_index + static_cast<int64_t>(centre_row) * E + i * kk;
    int64_t* other = edge_index + static_cast<int64_t>(1 - centre_row) * E + i * kk;
#pragma unroll
    for (int e = 0; e < K; ++e) {
        if (e < kk) {
            centre[e] = i;
            other[e] = static_cast<int64_t>(ix[e]);
            if (dist) {
                const double d = key_dist(dk[e]);
                dist[i * kk + e] = static_cast<float>(COS ? d : sqrt(d));
            }
        }
    }
}

// ---- direct route --------------------------------------------------------------------------------------------------------------
// grid: (ceil(N / 64), S key ranges); block 64.  MQ: M rounded up to 4 | 8 | 16 (zero columns change no sum).  S > 1: the lists
// go to ws_key / ws_idx [S][N][K]; S == 1: the edge list is written here.
template <int MQ, int K, bool COS>
__global__ __launch_bounds__(64) void knn_direct_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int M, int kk, int loop,
                                                        uint64_t* __restrict__ ws_key, uint32_t* __restrict__ ws_idx, int centre_row,
                                                        int64_t* __restrict__ edge_index, float* __restrict__ dist) {
    constexpr int LD = MQ + 4;                       // row stride of the tile in floats: 16-byte rows off the 64-byte stride
    __shared__ __attribute__((aligned(16))) float tile[64 * LD];
    __shared__ double rn[64];
    const int lane = threadIdx.x;
    const int S = gridDim.y;
    const int split = blockIdx.y;
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 64 + lane;
    const bool iok = i < N;
    const int64_t ic = iok ? i : N - 1;

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

    const int64_t n_tiles = (N + 63) / 64;
    const int64_t per = (n_tiles + S - 1) / S;
    const int64_t t0 = split * per;
    const int64_t t1 = (t0 + per < n_tiles) ? t0 + per : n_tiles;
    for (int64_t t = t0; t < t1; ++t) {
        __syncthreads();                             // the previous tile has been read
        {
            const int64_t j = t * 64 + lane;
            const bool jok = j < N;
            const int64_t jc = jok ? j : N - 1;
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
        const int64_t left = N - t * 64;
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
            const int64_t j = t * 64 + jj;
            // the gate: one compare against the distance of the list's last entry, written so that a NaN on either side
            // passes (the threshold of a list that is not full is a NaN; a NaN distance still has to fill such a list)
            if ((loop || j != i) && !(d >= thr)) {
                const uint64_t key = dist_key(d);
                if (key < dk[K - 1]) {
                    insert2<K>(dk, ix, key, static_cast<uint32_t>(j));
                    thr = key_dist(dk[K - 1]);
                }
            }
        }
    }
    if (!iok) return;
    if (S == 1) {
        write_row<K, COS>(dk, ix, i, kk, centre_row, N * kk, edge_index, dist);
    } else {
        const int64_t base = (static_cast<int64_t>(split) * N + i) * K;
#pragma unroll
        for (int e = 0; e < K; ++e) {
            ws_key[base + e] = dk[e];
            ws_idx[base + e] = ix[e];
        }
    }
}

// one thread per row: the S lists of the row in range order -> the edge list.  A list is loaded whole, and the next one before
// this one is inserted: one memory round trip per range, not one per entry.
template <int K, bool COS>
__global__ __launch_bounds__(64) void knn_direct_merge_kernel(const uint64_t* __restrict__ ws_key, const uint32_t* __restrict__ ws_idx,
                                                              int64_t N, int S, int kk, int centre_row,
                                                              int64_t* __restrict__ edge_index, float* __restrict__ dist) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * 64 + threadIdx.x;
    if (i >= N) return;
    uint64_t dk[K], nk[K];
    uint32_t ix[K], ni[K];
#pragma unroll
    for (int e = 0; e < K; ++e) {
        dk[e] = kEmpty;
        ix[e] = 0xFFFFFFFFu;
    }
    auto load = [&](int s) {
        const int64_t base = (static_cast<int64_t>(s) * N + i) * K;
#pragma unroll
        for (int e = 0; e < K; ++e) {
            nk[e] = ws_key[base + e];
            ni[e] = ws_idx[base + e];
        }
    };
    load(0);
    for (int s = 0; s < S; ++s) {
        uint64_t ck[K];
        uint32_t ci[K];
#pragma unroll
        for (int e = 0; e < K; ++e) {
            ck[e] = nk[e];
            ci[e] = ni[e];
        }
        if (s + 1 < S) load(s + 1);
        bool open = true;                                 // sorted: once an entry stays out, what follows in this list does too
#pragma unroll
        for (int e = 0; e < K; ++e) {
            open = open && ck[e] < dk[K - 1];
            if (open) insert2<K>(dk, ix, ck[e], ci[e]);
        }
    }
    write_row<K, COS>(dk, ix, i, kk, centre_row, N * kk, edge_index, dist);
}

// ---- sweep route -----------------------------------------------------------------------------------------------------------------
// one thread per row: h[r] = |x_r|^2 / 2 (Euclidean), or xhat[r] = x_r / |x_r| and h[r] = 0 (cosine); float32, columns ascending
template <bool COS>
__global__ __launch_bounds__(256) void knn_prepass_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int M,
                                                          float* __restrict__ xhat, float* __restrict__ h) {
    const int64_t r = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (r >= N) return;
    const float* row = x + r * ldx;
    float n2 = 0.f;
    for (int c = 0; c < M; c += 4) {
        const f32x4 v = dif::Elem<float>::ld4(row + c);
#pragma unroll
        for (int u = 0; u < 4; ++u) n2 = fmaf(v[u], v[u], n2);
    }
    if (COS) {
        const float rinv = n2 == 0.f ? 0.f : 1.0f / sqrtf(n2);
        for (int c = 0; c < M; c += 4) {
            f32x4 v = dif::Elem<float>::ld4(row + c);
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] *= rinv;
            dif::Elem<float>::st4(xhat + r * M + c, v);
        }
        h[r] = 0.f;
    } else {
        h[r] = 0.5f * n2;
    }
}

// grid: (ceil(N / 32), S key ranges); block 64 = one wave: 32 query rows against one range of 16-key tiles, as
// attn_topk_sweep_kernel (S^T = K Q^T on the fp32 matrix core; the lane holds four keys of ONE query per tile).
// lists [S][N][kCand].
template <bool QREG>
__global__ __launch_bounds__(64) void knn_sweep_kernel(const float* __restrict__ r, int64_t ldr, const float* __restrict__ h, int64_t N,
                                                       int M, uint64_t* __restrict__ lists) {
    constexpr int KMAX = kCand;
    const int S = gridDim.y;
    const int split = blockIdx.y;
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15;
    const int lg = lane >> 4;
    const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kQGroup;
    const int m_chunks = (M + 63) / 64;

    int64_t qr[kQT];
    bool qok[kQT];
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
        const int64_t row = q0 + 16 * t + l15;
        qok[t] = row < N;
        qr[t] = qok[t] ? row : N - 1;
    }
    f32x4 qv[kQT][4];                  // the query fragments of the (only) m-chunk stay in registers when M <= 64
    if (QREG) {
#pragma unroll
        for (int t = 0; t < kQT; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) qv[t][c] = ld4<true>(r, ldr, qr[t], qok[t], 0, 16 * c + 4 * lg, M);
    }

    uint64_t lst[kQT][KMAX];
    float thr[kQT];
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
        thr[t] = key_score(0u);            // NaN: everything passes the gate until the list is full
#pragma unroll
        for (int i = 0; i < KMAX; ++i) lst[t][i] = 0;
    }

    const int64_t n_ktiles = (N + 15) / 16;
    const int64_t per = (n_ktiles + S - 1) / S;
    const int64_t kt0 = split * per;
    const int64_t kt1 = (kt0 + per < n_ktiles) ? kt0 + per : n_ktiles;
    for (int64_t kt = kt0; kt < kt1; ++kt) {
        const int64_t kbase = kt * 16;
        f32x4 s[kQT];
#pragma unroll
        for (int t = 0; t < kQT; ++t) s[t] = dif::zero4();
        const bool kok = kbase + l15 < N;
        const int64_t kr = kok ? kbase + l15 : N - 1;
        float hk[4];
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t key = kbase + 4 * lg + reg;
            hk[reg] = h[key < N ? key : N - 1];
        }
        for (int mc = 0; mc < m_chunks; ++mc) {
            f32x4 kx[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) kx[c] = ld4<true>(r, ldr, kr, kok, 0, mc * 64 + 16 * c + 4 * lg, M);
            if (!QREG) {
#pragma unroll
                for (int t = 0; t < kQT; ++t)
#pragma unroll
                    for (int c = 0; c < 4; ++c) qv[t][c] = ld4<true>(r, ldr, qr[t], qok[t], 0, mc * 64 + 16 * c + 4 * lg, M);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int t = 0; t < kQT; ++t)      // independent accumulator chains back to back
                        s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kx[c][u], qv[t][c][u], s[t], 0, 0, 0);
        }
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int64_t key = kbase + 4 * lg + reg;
            const bool valid = key < N;
#pragma unroll
            for (int t = 0; t < kQT; ++t) {
                const float sc = s[t][reg] - hk[reg];
                if (valid && !(sc < thr[t])) {               // a NaN on either side passes: decided by the exact order
                    const uint64_t c = candidate(sc, static_cast<uint32_t>(key));
                    if (c > lst[t][KMAX - 1]) {
                        insert<KMAX>(lst[t], c);
                        thr[t] = key_score(static_cast<uint32_t>(lst[t][KMAX - 1] >> 32));
                    }
                }
            }
        }
    }

    // the four lanes of a query: fold the lists into lane group 0, which stores them
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
        fold<KMAX>(lst[t], 16, (lg & 1) != 0, (lg & 1) == 0);
        fold<KMAX>(lst[t], 32, lg == 2, lg == 0);
        const int64_t row = q0 + 16 * t + l15;
        if (lg == 0 && row < N) {
            uint64_t* dst = lists + (static_cast<int64_t>(split) * N + row) * KMAX;
#pragma unroll
            for (int i = 0; i < KMAX; ++i) dst[i] = lst[t][i];
        }
    }
}

// grid: ceil(N / 2); block 64: 32 lanes per row, one candidate each.  x is the caller's matrix (not the normalised copy).
template <bool COS>
__global__ __launch_bounds__(64) void knn_rerank_kernel(const float* __restrict__ x, int64_t ldx, int64_t N, int M,
                                                        const uint64_t* __restrict__ lists, int S, int kk, int loop, int centre_row,
                                                        int64_t* __restrict__ edge_index, float* __restrict__ dist) {
    __shared__ uint64_t cur[2][kCand], oth[2][kCand], nxt[2][kCand];
    __shared__ uint32_t sidx[2][kCand];
    const int half = threadIdx.x >> 5;
    const int c = threadIdx.x & 31;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 2 + half;
    const bool rok = row < N;
    const int64_t rc = rok ? row : N - 1;

    // the S sorted lists of the row -> its best kCand words: a word's place in the union of two sorted lists is its own rank
    // plus the number of words of the other list above it (the real words are distinct; empty slots fall off the end)
    uint64_t mine = lists[rc * kCand + c];
    for (int s = 1; s < S; ++s) {
        const uint64_t b = lists[(static_cast<int64_t>(s) * N + rc) * kCand + c];
        cur[half][c] = mine;
        oth[half][c] = b;
        nxt[half][c] = 0;
        __syncthreads();
        int pa = c, pb = c;
#pragma unroll 8
        for (int j = 0; j < kCand; ++j) {
            pa += oth[half][j] > mine ? 1 : 0;
            pb += cur[half][j] > b ? 1 : 0;
        }
        if (mine != 0 && pa < kCand) nxt[half][pa] = mine;
        if (b != 0 && pb < kCand) nxt[half][pb] = b;
        __syncthreads();
        mine = nxt[half][c];
        __syncthreads();
    }

    // float64 distance of this lane's candidate by direct difference, columns ascending (identical rows: identical distances)
    const bool valid = mine != 0;
    const uint32_t idx = valid ? 0xFFFFFFFFu - static_cast<uint32_t>(mine) : static_cast<uint32_t>(rc);
    const float* xi = x + rc * ldx;
    const float* xj = x + static_cast<int64_t>(idx) * ldx;
    double d = 0.0, ni2 = 0.0, nj2 = 0.0;
    for (int m = 0; m < M; m += 4) {
        const f32x4 a = dif::Elem<float>::ld4(xi + m);
        const f32x4 b = dif::Elem<float>::ld4(xj + m);
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const double av = static_cast<double>(a[u]), bv = static_cast<double>(b[u]);
            if (COS) {
                d = fma(av, bv, d);
                ni2 = fma(av, av, ni2);
                nj2 = fma(bv, bv, nj2);
            } else {
                const double diff = av - bv;
                d = fma(diff, diff, d);
            }
        }
    }
    if (COS) d = cos_dist(d, rnorm(ni2), rnorm(nj2));

    // rank by counting under the total order; what is not eligible sorts behind everything
    const bool out = !valid || (!loop && static_cast<int64_t>(idx) == row);
    const uint64_t key = out ? kEmpty : dist_key(d);
    const uint32_t ridx = out ? 0xFFFFFFFFu : idx;
    cur[half][c] = key;
    sidx[half][c] = ridx;
    __syncthreads();
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < kCand; ++j) {
        const uint64_t kj = cur[half][j];
        const uint32_t ij = sidx[half][j];
        rank += (kj < key || (kj == key && ij < ridx)) ? 1 : 0;
    }
    if (rok && !out && rank < kk) {
        const int64_t E = N * kk;
        const int64_t e = row * kk + rank;
        edge_index[static_cast<int64_t>(centre_row) * E + e] = row;
        edge_index[static_cast<int64_t>(1 - centre_row) * E + e] = static_cast<int64_t>(idx);
        if (dist) dist[e] = static_cast<float>(COS ? d : sqrt(d));
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
bool shape_ok(int64_t n, int M, int k) { return n > 0 && n < (1ll << 31) && M > 0 && M % 4 == 0 && M <= kMaxM && k >= 1 && k <= kMaxK; }

int route_of(int M, int route) { return route >= 0 ? route : (M <= kDirectM ? 0 : 1); }

int neighbours(int64_t n, int k, int loop) {
    const int64_t others = n - (loop ? 0 : 1);
    return static_cast<int>(others < k ? others : k);
}

int list_len(int kk) { return kk <= 8 ? 8 : (kk <= 16 ? 16 : 24); }

// Key ranges: about kFillWaves waves in flight, at most kMaxSplits ranges, each at least `min_tiles` tiles of `tile` keys; then
// recomputed from the range length, so that no range is empty.
int key_splits(int64_t query_waves, int64_t n, int tile, int min_tiles) {
    const int64_t n_tiles = (n + tile - 1) / tile;
    int64_t s = (kFillWaves + query_waves - 1) / query_waves;
    if (s > n_tiles / min_tiles) s = n_tiles / min_tiles;
    if (s > kMaxSplits) s = kMaxSplits;
    if (s < 1) s = 1;
    const int64_t per = (n_tiles + s - 1) / s;
    return static_cast<int>((n_tiles + per - 1) / per);
}

int splits_of(int64_t n, int route) {
    return route == 0 ? key_splits((n + 63) / 64, n, 64, 1) : key_splits((n + kQGroup - 1) / kQGroup, n, 16, kMinTilesPerSplit);
}

template <int MQ, int K, bool COS>
int launch_direct(const float* x, int64_t ldx, int64_t n, int M, int kk, int loop, int S, int centre_row, int64_t* edge_index,
                  float* dist, void* workspace, hipStream_t st) {
    uint64_t* ws_key = static_cast<uint64_t*>(workspace);
    uint32_t* ws_idx = reinterpret_cast<uint32_t*>(ws_key + static_cast<int64_t>(S) * n * K);
    if (int rc = dif::launch("knn_direct_kernel", knn_direct_kernel<MQ, K, COS>, dif::grid_of((n + 63) / 64, S), dim3(64), 0, st, x, ldx,
                             n, M, kk, loop, ws_key, ws_idx, centre_row, edge_index, dist)) return rc;
    if (S == 1) return 0;
    return dif::launch("knn_direct_merge_kernel", knn_direct_merge_kernel<K, COS>, dif::grid_of((n + 63) / 64), dim3(64), 0, st,
                       ws_key, ws_idx, n, S, kk, centre_row, edge_index, dist);
}

template <bool COS>
int launch_sweep(const float* x, int64_t ldx, int64_t n, int M, int kk, int loop, int S, int centre_row, int64_t* edge_index,
                 float* dist, void* workspace, hipStream_t st) {
    uint64_t* lists = static_cast<uint64_t*>(workspace);
    float* xhat = reinterpret_cast<float*>(lists + static_cast<int64_t>(S) * n * kCand);
    float* h = xhat + (COS ? n * M : 0);
    if (int rc = dif::launch("knn_prepass_kernel", knn_prepass_kernel<COS>, dif::grid_of((n + 255) / 256), dim3(256), 0, st, x, ldx, n, M,
                             xhat, h)) return rc;
    const float* rows = COS ? xhat : x;
    const int64_t ldr = COS ? M : ldx;
    if (int rc = dif::with_flags([&](auto QREG) {
            return dif::launch("knn_sweep_kernel", knn_sweep_kernel<QREG>, dif::grid_of((n + kQGroup - 1) / kQGroup, S), dim3(64), 0, st,
                               rows, ldr, h, n, M, lists);
        }, M <= 64)) return rc;
    return dif::launch("knn_rerank_kernel", knn_rerank_kernel<COS>, dif::grid_of((n + 1) / 2), dim3(64), 0, st, x, ldx, n, M, lists, S, kk,
                       loop, centre_row, edge_index, dist);
}

}  // namespace

extern "C" int dif_knn_version(void) { return DIF_KNN_VERSION; }
extern "C" const char* dif_knn_last_error(void) { return dif::err_buf(); }

extern "C" int dif_knn_route(int64_t n, int M, int k) {
    (void)n;
    (void)k;
    return route_of(M, -1);
}

extern "C" int dif_knn_splits(int64_t n, int M, int k, int loop, int route) {
    (void)loop;
    if (!shape_ok(n, M, k) || route < -1 || route > 1) return 0;
    return splits_of(n, route_of(M, route));
}

// direct: [S][n][K] distance keys, then [S][n][K] indices (nothing when S == 1);
// sweep:  [S][n][32] candidate words, then (cosine) the normalised rows [n][M], then h [n]
extern "C" int64_t dif_knn_workspace_bytes(int64_t n, int M, int k, int loop, int metric, int route) {
    if (!shape_ok(n, M, k) || route < -1 || route > 1) return 0;
    const int rt = route_of(M, route);
    const int64_t S = splits_of(n, rt);
    if (rt == 0) return S == 1 ? 0 : S * n * list_len(neighbours(n, k, loop)) * static_cast<int64_t>(sizeof(uint64_t) + sizeof(uint32_t));
    return S * n * kCand * static_cast<int64_t>(sizeof(uint64_t)) + (metric == 1 ? n * M * static_cast<int64_t>(sizeof(float)) : 0) +
           n * static_cast<int64_t>(sizeof(float));
}

extern "C" int dif_knn_graph_f32(const float* x, int64_t ldx, int64_t n, int M, int k, int loop, int metric, int centre_row, int route,
                                 int64_t* edge_index, float* dist_or_null, void* workspace, int64_t workspace_bytes,
                                 dif_stream_t stream) {
    const char* who = "dif_knn_graph_f32";
    DIF_REQUIRE(n > 0 && M > 0, DIF_E_BADARG, "%s: n and M must be positive", who);
    DIF_REQUIRE(x && workspace, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned16(x) && dif::aligned16(workspace), DIF_E_BADARG, "%s: x and the workspace must be 16-byte aligned", who);
    DIF_REQUIRE(dif::aligned<8>(edge_index) && dif::aligned<4>(dist_or_null), DIF_E_BADARG,
                "%s: edge_index must be 8-byte and the distances 4-byte aligned", who);
    DIF_REQUIRE(M % 4 == 0 && M <= kMaxM, DIF_E_SHAPE, "%s: M must be a multiple of 4 up to %d (got %d); zero-pad the columns", who, kMaxM, M);
    DIF_REQUIRE(k >= 1 && k <= kMaxK, DIF_E_SHAPE, "%s: k must be in [1, %d] (got %d)", who, kMaxK, k);
    DIF_REQUIRE(metric == 0 || metric == 1, DIF_E_SHAPE, "%s: unknown metric %d (0: Euclidean, 1: cosine)", who, metric);
    DIF_REQUIRE(centre_row == 0 || centre_row == 1, DIF_E_SHAPE, "%s: centre_row must be 0 or 1 (got %d)", who, centre_row);
    DIF_REQUIRE(route >= -1 && route <= 1, DIF_E_SHAPE, "%s: unknown route %d (-1: automatic, 0: direct, 1: sweep)", who, route);
    DIF_REQUIRE(!(route == 0 && M > kDirectM), DIF_E_SHAPE, "%s: the direct route takes rows of up to %d columns (got %d)", who, kDirectM, M);
    DIF_REQUIRE(ldx >= M && ldx % 4 == 0, DIF_E_BADARG, "%s: the leading dimension must cover a row and be a multiple of 4 elements", who);
    DIF_REQUIRE(n < (1ll << 31), DIF_E_RANGE, "%s: n %lld exceeds the 31-bit row index", who, static_cast<long long>(n));
    const int64_t need = dif_knn_workspace_bytes(n, M, k, loop, metric, route);
    DIF_REQUIRE(workspace_bytes >= need, DIF_E_WORKSPACE, "%s: workspace too small (%lld < %lld)", who,
                static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    const int kk = neighbours(n, k, loop);
    if (kk == 0) return 0;                                   // one row, no self-loop: an empty edge list (which may have no address)
    DIF_REQUIRE(edge_index, DIF_E_BADARG, "%s: null pointer", who);
    const int rt = route_of(M, route);
    const int S = splits_of(n, rt);
    hipStream_t st = static_cast<hipStream_t>(stream);
    loop = loop ? 1 : 0;
    return dif::with_flags([&](auto COS) {
        if (rt == 1) return launch_sweep<COS>(x, ldx, n, M, kk, loop, S, centre_row, edge_index, dist_or_null, workspace, st);
        return dif::with_int<4, 8, 16>(M <= 4 ? 4 : (M <= 8 ? 8 : 16), [&](auto MQ) {
            return dif::with_int<8, 16, 24>(list_len(kk), [&](auto K) {
                return launch_direct<MQ, K, COS>(x, ldx, n, M, kk, loop, S, centre_row, edge_index, dist_or_null, workspace, st);
            }, dif::no_variant(who));
        }, dif::no_variant(who));
    }, metric == 1);
}
