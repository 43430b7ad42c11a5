// libdifformer_maps.so (C ABI: include/difformer_maps.h): the k strongest keys of every query row and head of an attention
// map that is never stored -- the visualisation output of the reference (difformer.py:42-43 `simple`, :47-55 `sigmoid`,
// :211-226 get_attentions) on graphs where the dense [N, L, H] tensor cannot exist.
//
// Sweep kernel.  One WAVE per workgroup: 32 query rows (two 16-row tiles) of one head against one range of key tiles.
// Scores are formed as in csrc/sigmoid_attn.hip, transposed on the fp32 matrix core (v_mfma_f32_16x16x4_f32):
//   S^T[key][query] = K Q^T :  A[i = lane%16 <-> key][k] = K fragment,  B[k][j = lane%16 <-> query] = Q fragment
//   the lane then holds S^T[key = 4 (lane/16) + reg][query = lane%16]: four keys of ONE query per tile,
// so the selection is private to the lane.  The contraction runs over M in chunks of 64 columns in a fixed order that does
// not depend on where a key sits in its tile: identical key rows give bit-identical scores, which the tie rule relies on.
//
// Selection (csrc/topk_select.h).  A candidate is ONE 64-bit word: the score as an order-preserving unsigned key in the upper half (NaN -> 0, the
// lowest; -0 -> +0), 0xFFFFFFFF - key index in the lower half.  Unsigned `>` on that word IS the total order of the header
// (larger score first, among equal scores the lower index first), and 0 -- below every real candidate -- is the empty slot.
// Each lane keeps KMAX words per query tile, sorted, in registers.  A score is first compared, as a float, with the score of the
// list's last entry (one VALU instruction per score); what passes is made a candidate word and compared exactly, and only when
// it beats the last entry does it enter, through a compare-exchange chain with static register indices (no dynamic indexing:
// no scratch).
// After the first tiles of a sweep few candidates enter.
// At the end the four lanes that share a query fold their lists (lane groups 1 -> 0 and 3 -> 2, then 2 -> 0): the sender hands
// over its list front first through ds_bpermute and shifts it down, the receiver inserts; the loop ends as soon as a round
// placed nothing.  Lane group 0 stores the wave's list and (mode 1) its partial sum of sigma(s) to the workspace.
//
// Merge kernel.  One thread per (query, head): inserts the S lists of its row in split order under the same order, adds the S
// partial sums in split order, decodes score and index, and (mode 1) scales sigma(s) by the reciprocal of the sum.  It
// runs for S == 1 too: 8 KMAX bytes per row and head through the workspace, against a sweep of L keys for that row.
#include <stdarg.h>
#include "dif_common.h"
#include "topk_select.h"
#include "../../include/difformer_maps.h"

namespace {

using dif::f32x4;
using dif::ld4, dif::sigmoid_hw;
using dif::candidate, dif::fold, dif::insert, dif::key_score;      // the selection: csrc/topk_select.h

constexpr int kQT = 2;                 // 16-query tiles per wave: every K fragment feeds two MFMA chains
constexpr int kQGroup = 16 * kQT;      // queries per workgroup
constexpr int kMaxTopk = 32;
constexpr int kMaxM = 512;
constexpr int kMaxSplits = 32;
constexpr int kMinTilesPerSplit = 4;   // a split sweeps at least this many 16-key tiles
constexpr int64_t kFillWaves = 2 * 4 * dif::kCUs;     // two waves on each of the chip's SIMDs

// thread-local last-error text of THIS library (dif_maps_last_error)
char* maps_err_buf() {
    static thread_local char buf[512] = {0};
    return buf;
}
int maps_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(maps_err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}
// post-launch check into THIS library's error text (hipGetLastError only, never synchronises)
int maps_launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return maps_fail(static_cast<int>(e), "%s: %s", what, hipGetErrorString(e));
    return 0;
}
#define MAPS_REQUIRE(cond, code, ...) \
    do { if (!(cond)) return maps_fail((code), __VA_ARGS__); } while (0)

// grid: (ceil(N / 32), H, S key splits); block 64.  lists [S][N * H][KMAX], psum [S][N * H] (MODE 1 only).
template <int KMAX, int MODE, bool QREG>
__global__ __launch_bounds__(64) void attn_topk_sweep_kernel(const float* __restrict__ q, int64_t ldq,
                                                             const float* __restrict__ k, int64_t ldk, int64_t N, int64_t L,
                                                             int H, int M, uint64_t* __restrict__ lists,
                                                             float* __restrict__ psum) {
    const int h = blockIdx.y;
    const int S = gridDim.z;
    const int split = blockIdx.z;
    const int lane = threadIdx.x & 63;
    const int l15 = lane & 15;
    const int lg = lane >> 4;
    const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kQGroup;
    const int m_chunks = (M + 63) / 64;

    int64_t qr[kQT];
    bool qok[kQT];
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
        const int64_t r = q0 + 16 * t + l15;
        qok[t] = r < N;
        qr[t] = qok[t] ? r : N - 1;
    }
    // Q fragments for the (only) m-chunk stay in registers when M <= 64
    f32x4 qv[kQT][4];
    if (QREG) {
#pragma unroll
        for (int t = 0; t < kQT; ++t)
#pragma unroll
            for (int c = 0; c < 4; ++c) qv[t][c] = ld4<true>(q, ldq, qr[t], qok[t], h * M, 16 * c + 4 * lg, M);
    }

    uint64_t lst[kQT][KMAX];
    float den[kQT], thr[kQT];
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
        den[t] = 0.f;
        thr[t] = key_score(0u);             // NaN: everything passes the gate until the list is full
#pragma unroll
        for (int i = 0; i < KMAX; ++i) lst[t][i] = 0;
    }

    // this workgroup's key tiles: [kt0, kt1)
    const int64_t n_ktiles = (L + 15) / 16;
    const int64_t per = (n_ktiles + S - 1) / S;
    const int64_t kt0 = split * per;
    const int64_t kt1 = (kt0 + per < n_ktiles) ? kt0 + per : n_ktiles;
    // M <= 64: the K fragments of the NEXT tile are in flight under this tile's products and selection (16 VGPRs) -- raw loads from
    // clamped (valid) addresses, masked only when used, as in csrc/sigmoid_attn.hip; the last step re-reads its own rows.  (Not
    // with KMAX = 32: its lists leave no registers for it.)
    constexpr bool PREFETCH = QREG && KMAX < 32;
    f32x4 kn[4];
    auto prefetch = [&](int64_t kt) {
        const int64_t r = kt * 16 + l15;
#pragma unroll
        for (int c = 0; c < 4; ++c) kn[c] = dif::ld4_raw<true>(k, ldk, r < L ? r : L - 1, h * M, 16 * c + 4 * lg, M);
    };
    if (PREFETCH && kt0 < kt1) prefetch(kt0);
    for (int64_t kt = kt0; kt < kt1; ++kt) {
        const int64_t kbase = kt * 16;
        f32x4 s[kQT];
#pragma unroll
        for (int t = 0; t < kQT; ++t) s[t] = dif::zero4();
        const bool kok = kbase + l15 < L;
        const int64_t kr = kok ? kbase + l15 : L - 1;
        if constexpr (PREFETCH) {
            f32x4 kx[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) kx[c] = dif::mask4<true>(kn[c], kok, 16 * c + 4 * lg, M);
            prefetch(kt + 1 < kt1 ? kt + 1 : kt);
            __builtin_amdgcn_sched_barrier(0);           // issued HERE, ahead of the products
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int t = 0; t < kQT; ++t)
                        s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(kx[c][u], qv[t][c][u], s[t], 0, 0, 0);
        } else
        for (int mc = 0; mc < m_chunks; ++mc) {
            f32x4 kx[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) kx[c] = ld4<true>(k, ldk, kr, kok, h * M, mc * 64 + 16 * c + 4 * lg, M);
            if (!QREG) {
#pragma unroll
                for (int t = 0; t < kQT; ++t)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        qv[t][c] = ld4<true>(q, ldq, qr[t], qok[t], h * M, mc * 64 + 16 * c + 4 * lg, M);
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
            const bool valid = key < L;
#pragma unroll
            for (int t = 0; t < kQT; ++t) {
                const float sc = s[t][reg];
                if (MODE == 1) den[t] += valid ? sigmoid_hw(sc) : 0.f;                 // difformer.py:50-51 row sum
                // the gate: one float compare against the score of the list's last entry.  Written so that a NaN on either
                // side passes (the threshold of a list that is not full is a NaN; a NaN score still has to fill such a list);
                // what passes -- equal scores among it -- is decided by the exact order
                if (valid && !(sc < thr[t])) {
                    const uint64_t c = candidate(sc, static_cast<uint32_t>(key));
                    if (c > lst[t][KMAX - 1]) {
                        insert<KMAX>(lst[t], c);
                        thr[t] = key_score(static_cast<uint32_t>(lst[t][KMAX - 1] >> 32));
                    }
                }
            }
        }
    }

    // the four lanes of a query: fold the lists (and the sums) into lane group 0, which stores them
#pragma unroll
    for (int t = 0; t < kQT; ++t) {
        fold<KMAX>(lst[t], 16, (lg & 1) != 0, (lg & 1) == 0);
        fold<KMAX>(lst[t], 32, lg == 2, lg == 0);
        float dsum = den[t];
        if (MODE == 1) {
            dsum += __shfl_xor(dsum, 16, 64);
            dsum += __shfl_xor(dsum, 32, 64);
        }
        const int64_t row = q0 + 16 * t + l15;
        if (lg == 0 && row < N) {
            const int64_t slot = (static_cast<int64_t>(split) * N + row) * H + h;
            uint64_t* dst = lists + slot * KMAX;
#pragma unroll
            for (int i = 0; i < KMAX; ++i) dst[i] = lst[t][i];
            if (MODE == 1) psum[slot] = dsum;
        }
    }
}

// one thread per (query, head): the S lists of the row in split order -> values / indices [N * H][topk]
template <int KMAX, int MODE>
__global__ __launch_bounds__(256) void attn_topk_merge_kernel(const uint64_t* __restrict__ lists,
                                                              const float* __restrict__ psum, int64_t rows, int S, int topk,
                                                              float* __restrict__ values, int32_t* __restrict__ indices) {
    const int64_t row = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (row >= rows) return;
    uint64_t lst[KMAX];
#pragma unroll
    for (int i = 0; i < KMAX; ++i) lst[i] = 0;
    float den = 0.f;
    for (int s = 0; s < S; ++s) {
        const uint64_t* src = lists + (static_cast<int64_t>(s) * rows + row) * KMAX;
        for (int j = 0; j < KMAX; ++j) {
            const uint64_t c = src[j];
            if (!(c > lst[KMAX - 1])) break;              // sorted: what follows in this list is lower still
            insert<KMAX>(lst, c);
        }
        if (MODE == 1) den += psum[static_cast<int64_t>(s) * rows + row];
    }
    const float rden = MODE == 1 ? 1.0f / den : 1.0f;
#pragma unroll
    for (int i = 0; i < KMAX; ++i) {
        if (i < topk) {
            const float sc = key_score(static_cast<uint32_t>(lst[i] >> 32));
            values[row * topk + i] = MODE == 1 ? sigmoid_hw(sc) * rden : sc;
            indices[row * topk + i] = static_cast<int32_t>(0xFFFFFFFFu - static_cast<uint32_t>(lst[i]));
        }
    }
}

int kmax_of(int topk) { return topk <= 8 ? 8 : (topk <= 16 ? 16 : 32); }

bool shape_ok(int64_t n_q, int64_t n_k, int H, int M, int topk) {
    return n_q > 0 && n_k > 0 && H > 0 && M > 0 && M % 4 == 0 && M <= kMaxM && topk >= 1 && topk <= kMaxTopk && topk <= n_k;
}

// Key splits: a workgroup is one wave, so the query blocks alone fill the chip from kFillWaves of them (N H >= 65,536 rows);
// below that the keys are cut so that about kFillWaves waves run, each over at least kMinTilesPerSplit tiles, at most
// kMaxSplits ranges -- then recomputed from the range length, so that no range is empty.
int key_splits(int64_t n_q, int64_t n_k, int H) {
    const int64_t groups = ((n_q + kQGroup - 1) / kQGroup) * H;
    const int64_t n_ktiles = (n_k + 15) / 16;
    int64_t s = (kFillWaves + groups - 1) / groups;
    if (s > n_ktiles / kMinTilesPerSplit) s = n_ktiles / kMinTilesPerSplit;
    if (s > kMaxSplits) s = kMaxSplits;
    if (s < 1) s = 1;
    const int64_t per = (n_ktiles + s - 1) / s;
    return static_cast<int>((n_ktiles + per - 1) / per);
}

template <int KMAX, int MODE>
int launch(const float* q, int64_t ldq, const float* k, int64_t ldk, int64_t N, int64_t L, int H, int M, int topk, int S,
           float* values, int32_t* indices, uint64_t* lists, float* psum, hipStream_t st) {
    const dim3 grid(static_cast<unsigned>((N + kQGroup - 1) / kQGroup), static_cast<unsigned>(H), static_cast<unsigned>(S));
    if (int rc = dif::with_flags([&](auto QREG) {              // heads of up to 64 columns: the query fragments stay in registers
            hipLaunchKernelGGL((attn_topk_sweep_kernel<KMAX, MODE, QREG>), grid, dim3(64), 0, st, q, ldq, k, ldk, N, L, H, M, lists, psum);
            return maps_launch_status("attn_topk_sweep_kernel");
        }, M <= 64)) return rc;
    const int64_t rows = N * H;
    hipLaunchKernelGGL((attn_topk_merge_kernel<KMAX, MODE>), dim3(static_cast<unsigned>((rows + 255) / 256)), dim3(256), 0, st,
                       lists, psum, rows, S, topk, values, indices);
    return maps_launch_status("attn_topk_merge_kernel");
}

}  // namespace

extern "C" int dif_maps_version(void) { return DIF_MAPS_VERSION; }
extern "C" const char* dif_maps_last_error(void) { return maps_err_buf(); }

extern "C" int dif_attn_topk_splits(int64_t n_q, int64_t n_k, int H, int M, int topk) {
    if (!shape_ok(n_q, n_k, H, M, topk)) return 1;
    return key_splits(n_q, n_k, H);
}

// [S][n_q * H][KMAX] candidate words, then [S][n_q * H] partial sums
extern "C" int64_t dif_attn_topk_workspace_bytes(int64_t n_q, int64_t n_k, int H, int M, int topk) {
    if (!shape_ok(n_q, n_k, H, M, topk)) return 0;
    const int64_t slots = static_cast<int64_t>(key_splits(n_q, n_k, H)) * n_q * H;
    return slots * kmax_of(topk) * static_cast<int64_t>(sizeof(uint64_t)) + slots * static_cast<int64_t>(sizeof(float));
}

extern "C" int dif_attn_topk_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, int64_t n_q, int64_t n_k, int H,
                                 int M, int mode, int topk, float* values, int32_t* indices, void* workspace,
                                 int64_t workspace_bytes, dif_stream_t stream) {
    const char* who = "dif_attn_topk_f32";
    MAPS_REQUIRE(n_q > 0 && n_k > 0 && H > 0 && M > 0, DIF_E_BADARG, "%s: n_q, n_k, H, M must be positive", who);
    MAPS_REQUIRE(q && k && values && indices && workspace, DIF_E_BADARG, "%s: null pointer", who);
    MAPS_REQUIRE(dif::aligned16(q) && dif::aligned16(k) && dif::aligned16(workspace), DIF_E_BADARG,
                 "%s: q, k and the workspace must be 16-byte aligned", who);
    MAPS_REQUIRE(dif::aligned<4>(values) && dif::aligned<4>(indices), DIF_E_BADARG,
                 "%s: values and indices must be 4-byte aligned", who);
    MAPS_REQUIRE(M % 4 == 0 && M <= kMaxM, DIF_E_SHAPE, "%s: M must be a multiple of 4 up to %d (got %d); zero-pad the columns", who,
                 kMaxM, M);
    MAPS_REQUIRE(topk >= 1 && topk <= kMaxTopk && topk <= n_k, DIF_E_SHAPE, "%s: topk must be in [1, min(n_k, %d)] (got %d, n_k %lld)",
                 who, kMaxTopk, topk, static_cast<long long>(n_k));
    MAPS_REQUIRE(mode == 0 || mode == 1, DIF_E_SHAPE, "%s: unknown mode %d (0: simple, 1: sigmoid)", who, mode);
    MAPS_REQUIRE(ldq >= static_cast<int64_t>(H) * M && ldk >= static_cast<int64_t>(H) * M && ldq % 4 == 0 && ldk % 4 == 0, DIF_E_BADARG,
                 "%s: leading dimensions must cover a row and be multiples of 4 elements", who);
    MAPS_REQUIRE(n_k < (1ll << 31), DIF_E_RANGE, "%s: n_k %lld exceeds the 31-bit key index", who, static_cast<long long>(n_k));
    const int64_t gx = (n_q + kQGroup - 1) / kQGroup;
    MAPS_REQUIRE(gx < (1ll << 31) && H <= 65535 && (n_q * H + 255) / 256 < (1ll << 31), DIF_E_RANGE, "%s: grid too large", who);
    const int64_t need = dif_attn_topk_workspace_bytes(n_q, n_k, H, M, topk);
    MAPS_REQUIRE(workspace_bytes >= need, DIF_E_WORKSPACE, "%s: workspace too small (%lld < %lld)", who,
                 static_cast<long long>(workspace_bytes), static_cast<long long>(need));
    const int S = key_splits(n_q, n_k, H);
    const int KM = kmax_of(topk);
    uint64_t* lists = static_cast<uint64_t*>(workspace);
    float* psum = reinterpret_cast<float*>(lists + static_cast<int64_t>(S) * n_q * H * KM);
    hipStream_t st = static_cast<hipStream_t>(stream);
    auto miss = [who](int v) { return maps_fail(DIF_E_SHAPE, "%s: no kernel variant for %d", who, v); };
    return dif::with_int<0, 1>(mode, [&](auto MODE) {
        return dif::with_int<8, 16, 32>(KM, [&](auto KMAX) {
            return launch<KMAX, MODE>(q, ldq, k, ldk, n_q, n_k, H, M, topk, S, values, indices, lists, psum, st);
        }, miss);
    }, miss);
}
