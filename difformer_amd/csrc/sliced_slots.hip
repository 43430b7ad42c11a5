// Slot order of the PACKED schedule of the feature-sliced product (csrc/gcn_sliced.hip), built on the device:
// libdifformer_slots.so, C ABI in include/difformer_slots.h.
//
// The sweep pays for every 8-step block a (panel, tile, wave) stores, and it stores per round the largest block count of
// the slot's 64 rows in that tile, padded to a non-increasing sequence over the wave's rounds (sliced_table_kernel).  Which
// rows share a slot, and which slots share a wave, therefore decide the padding; the entry format and the sweep do not
// care.  Four stages, all on the stream, no host read:
//   a. block vectors b[row][tile] = (entries + 7) / 8 and the profile key (largest count descending, then the set of tiles
//      that reach it: sliced.packed_slot_order's key), sorted with the stable radix sort of the graph construction;
//   b. greedy slots: the sorted rows are cut into windows of 1,024 = 16 slots; one workgroup per window seeds a slot with
//      the remaining row of the largest block total and adds, 63 times, the remaining row that raises the slot's
//      per-tile maximum vector m least, sum_t max(0, b[row][t] - m[t]); ties: the larger total, then the lower row id;
//   c. deal: slots by descending total of their maximum vector are cut into R strata of PW slots; from the last round to
//      the first, the (panel, wave) pairs in descending order of their running envelope's total (ties: lower pair index)
//      each take the free slot of their stratum that raises that envelope least (ties: the earlier slot of the stratum);
//   d. order[slot_of(j, pw) * 64 + lane] = the row: a permutation of 64-row chunks of stage b's list.
// A last slot of fewer than 64 rows keeps the last slot position (the format has no padding inside `order`): it sorts
// behind every other slot and is given to the pair that owns that position before the deal of the last round starts.
//
// Every loop is bounded by the sizes: stage b makes exactly one pick per row of its window (<= 1,024), stage c one per
// slot (G in all), on one workgroup each; no kernel waits for another workgroup.
#include <stdarg.h>
// the device sort of the graph construction (scan, radix passes, workspace layout): gcn_csr.hip is its one home and gives
// that part alone under this switch -- its kernels are compiled into this library a second time, nothing is linked across
#define DIF_GCN_CSR_SORT_ONLY
#include "gcn_csr.hip"
#include "../../include/difformer_slots.h"

// dif::launch (csrc/dif_launch.h) reports through these; api.hip defines them for libdifformer_hip.so, this file for THIS
// library (linked -Bsymbolic: each library binds its own), so that its errors land in dif_slots_last_error().
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

constexpr int kWindow = 1024;            // rows of a greedy window (16 slots)
constexpr int kWindowThreads = 256;      // ... four rows per thread
constexpr int kRowsPerThread = kWindow / kWindowThreads;
constexpr int kMaxTiles = 18;            // the profile key holds 12 bits of block count + one bit per tile
constexpr int kMaxBlocks = 4095;         // block counts are compared up to here (32,760 entries of one (row, tile) group)
constexpr uint32_t kTotalMask = 0x1ffffu;  // block total of a row or slot: <= 18 * 4095 < 2^17
constexpr int kDealThreads = 256;
constexpr int kDealLds = 65536;          // dynamic LDS of the deal: no attribute needed up to 64 KiB

// the sweep's own arithmetic (csrc/gcn_sliced.hip): slot of stratum j for pair index pw, odd strata run backwards
__host__ __device__ __forceinline__ int64_t slot_of(int j, int pw, int PW) {
    return static_cast<int64_t>(j) * PW + ((j & 1) ? PW - 1 - pw : pw);
}

// ---- block vectors in registers: two 16-bit counts per dword, V x 4 dwords (8 V tiles, the tail zero) --------------------
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t pk_excess(uint32_t a, uint32_t b) {        // per half: max(0, a - b)
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_sub_sat(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b) {
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {           // halves stay below 2^16: <= 12 x 4095 each
    return __builtin_bit_cast(uint32_t, static_cast<u16x2>(__builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t halves(uint32_t a) { return (a & 0xffffu) + (a >> 16); }

// sum_t max(0, a[t] - b[t])
template <int V>
__device__ __forceinline__ uint32_t excess(const uint32_t (&a)[4 * V], const uint32_t (&b)[4 * V]) {
    uint32_t acc = 0;
#pragma unroll
    for (int d = 0; d < 4 * V; ++d) acc = pk_add(acc, pk_excess(a[d], b[d]));
    return halves(acc);
}

// smallest value of the wave, in every lane: four row_shr steps leave each 16-lane row's minimum in its last lane
// (a lane without a source keeps its own value: min is idempotent), the four rows meet on the scalar unit
__device__ __forceinline__ uint32_t wave_min32(uint32_t v) {
    int x = static_cast<int>(v), y;
    y = __builtin_amdgcn_update_dpp(x, x, 0x111, 0xf, 0xf, false); x = static_cast<uint32_t>(y) < static_cast<uint32_t>(x) ? y : x;
    y = __builtin_amdgcn_update_dpp(x, x, 0x112, 0xf, 0xf, false); x = static_cast<uint32_t>(y) < static_cast<uint32_t>(x) ? y : x;
    y = __builtin_amdgcn_update_dpp(x, x, 0x114, 0xf, 0xf, false); x = static_cast<uint32_t>(y) < static_cast<uint32_t>(x) ? y : x;
    y = __builtin_amdgcn_update_dpp(x, x, 0x118, 0xf, 0xf, false); x = static_cast<uint32_t>(y) < static_cast<uint32_t>(x) ? y : x;
    const uint32_t a = __builtin_amdgcn_readlane(x, 15), b = __builtin_amdgcn_readlane(x, 31);
    const uint32_t c = __builtin_amdgcn_readlane(x, 47), d = __builtin_amdgcn_readlane(x, 63);
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// smallest key of a 256-thread workgroup; `red` is one of two buffers the caller alternates between (one barrier per call)
__device__ __forceinline__ uint32_t block_min32(uint32_t key, uint32_t* red) {
    key = wave_min32(key);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = key;
    __syncthreads();
    const uint32_t a = red[0], b = red[1], c = red[2], d = red[3];
    const uint32_t ab = a < b ? a : b, cd = c < d ? c : d;
    return ab < cd ? ab : cd;
}

// ---- a. block vectors and profile keys ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slot_keys_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ blkptr,
                                                        int64_t n_src, int NT, int64_t row_begin, int64_t n_rows,
                                                        uint16_t* __restrict__ bv, uint32_t* __restrict__ keys,
                                                        uint32_t* __restrict__ vals) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n_rows) return;
    const int64_t row = row_begin + i;
    int top = 0;
    for (int t = 0; t < NT; ++t) {
        int32_t e0, e1;
        if (NT == 1) { e0 = rowptr[row]; e1 = rowptr[row + 1]; }
        else { e0 = blkptr[static_cast<int64_t>(t) * n_src + row]; e1 = blkptr[static_cast<int64_t>(t + 1) * n_src + row]; }
        int b = (e1 - e0 + 7) / 8;
        b = b < 0 ? 0 : (b > kMaxBlocks ? kMaxBlocks : b);
        bv[i * NT + t] = static_cast<uint16_t>(b);
        top = b > top ? b : top;
    }
    uint32_t hot = 0;
    for (int t = 0; t < NT; ++t) hot |= (bv[i * NT + t] == top) ? (1u << t) : 0u;
    keys[i] = (static_cast<uint32_t>(kMaxBlocks - top) << NT) | hot;
    vals[i] = static_cast<uint32_t>(i);
}

// ---- b. greedy slots: one workgroup per window of kWindow sorted rows ------------------------------------------------------
// The rows of the window are first RANKED by (larger total, lower row id) and held by rank: the tie rule of a pick is then
// the rank, a pick's key is excess << 10 | rank in 32 bits, and the winner's vector is read at its rank.
template <int V>
__global__ __launch_bounds__(kWindowThreads) void slot_window_kernel(const uint32_t* __restrict__ sorted,
                                                                     const uint16_t* __restrict__ bv, int NT, int64_t n_rows,
                                                                     int32_t* __restrict__ slotrows, uint16_t* __restrict__ slotmax,
                                                                     uint32_t* __restrict__ skeys, uint32_t* __restrict__ svals) {
    __shared__ uint64_t okey[kWindow];                 // (kTotalMask - total) << 28 | row of the loaded position
    __shared__ uint32_t vec[kWindow * 4 * V];          // block vectors, by rank
    __shared__ uint32_t rowid[kWindow];                // by rank
    __shared__ uint32_t red[2][kWindowThreads / 64];
    const int tid = threadIdx.x;
    const int64_t w0 = static_cast<int64_t>(blockIdx.x) * kWindow;
    const int cnt = static_cast<int>((n_rows - w0 < kWindow) ? (n_rows - w0) : kWindow);
    uint32_t b[kRowsPerThread][4 * V];
    uint32_t myrow[kRowsPerThread];
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int q = tid + kWindowThreads * r;
        const bool live = q < cnt;
        myrow[r] = live ? sorted[w0 + q] : 0u;
        uint32_t total = 0;
#pragma unroll
        for (int d = 0; d < 4 * V; ++d) b[r][d] = 0;
#pragma unroll
        for (int t = 0; t < 8 * V; ++t) {
            const uint32_t v = (live && t < NT) ? bv[static_cast<int64_t>(myrow[r]) * NT + t] : 0u;
            b[r][t >> 1] |= v << (16 * (t & 1));
            total += v;
        }
        okey[q] = live ? (static_cast<uint64_t>(kTotalMask - total) << 28) | myrow[r] : ~0ull;
    }
    __syncthreads();
    {
        uint64_t mine[kRowsPerThread];
        int rank[kRowsPerThread];
#pragma unroll
        for (int r = 0; r < kRowsPerThread; ++r) { mine[r] = okey[tid + kWindowThreads * r]; rank[r] = 0; }
        for (int j = 0; j < cnt; ++j) {                  // the keys are distinct: the ranks of the live rows are 0 .. cnt - 1
            const uint64_t o = okey[j];
#pragma unroll
            for (int r = 0; r < kRowsPerThread; ++r) rank[r] += (o < mine[r]) ? 1 : 0;
        }
#pragma unroll
        for (int r = 0; r < kRowsPerThread; ++r) {
            if (tid + kWindowThreads * r < cnt) {
#pragma unroll
                for (int d = 0; d < 4 * V; ++d) vec[rank[r] * 4 * V + d] = b[r][d];
                rowid[rank[r]] = myrow[r];
            }
        }
    }
    __syncthreads();
    uint32_t alive = 0;                                // bit r: rank tid + 256 r is not in a slot yet
#pragma unroll
    for (int r = 0; r < kRowsPerThread; ++r) {
        const int q = tid + kWindowThreads * r;
        if (q < cnt) {
            alive |= 1u << r;
#pragma unroll
            for (int d = 0; d < 4 * V; ++d) b[r][d] = vec[q * 4 * V + d];
        }
    }
    const int64_t G = (n_rows + 63) / 64;
    uint32_t m[4 * V];
    int pick = 0;
    for (int done = 0; done < cnt; ) {
        const int k_end = (cnt - done < 64) ? cnt - done : 64;
        const int64_t g = static_cast<int64_t>(blockIdx.x) * (kWindow / 64) + done / 64;
#pragma unroll
        for (int d = 0; d < 4 * V; ++d) m[d] = 0;
        for (int k = 0; k < k_end; ++k, ++pick) {
            uint32_t key = ~0u;
#pragma unroll
            for (int r = 0; r < kRowsPerThread; ++r) {
                // the seed (k == 0, m == 0) is the best rank: every excess is taken as 0
                const uint32_t c = (k == 0) ? 0u : excess<V>(b[r], m);
                const uint32_t kk = (c << 10) | static_cast<uint32_t>(tid + kWindowThreads * r);
                key = ((alive >> r) & 1u) && kk < key ? kk : key;
            }
            const int win = static_cast<int>(block_min32(key, red[pick & 1]) & 1023u);
            if ((win & (kWindowThreads - 1)) == tid) {
                alive &= ~(1u << (win / kWindowThreads));
                slotrows[g * 64 + k] = static_cast<int32_t>(rowid[win]);
            }
#pragma unroll
            for (int d = 0; d < 4 * V; ++d) m[d] = pk_max(m[d], vec[win * 4 * V + d]);
        }
        if (tid == 0) {
            uint32_t s = 0;
#pragma unroll
            for (int t = 0; t < 8 * V; ++t) {
                const uint32_t v = (m[t >> 1] >> (16 * (t & 1))) & 0xffffu;
                if (t < NT) { slotmax[g * NT + t] = static_cast<uint16_t>(v); s += v; }
            }
            // descending total; a last slot of fewer than 64 rows behind every other
            skeys[g] = (g == G - 1 && (n_rows & 63) != 0) ? 0xffffffu : (kTotalMask - s);
            svals[g] = static_cast<uint32_t>(g);
        }
        done += k_end;
    }
}

// ---- c. the deal: one workgroup --------------------------------------------------------------------------------------------
// sslots: the slots by descending total (the partial one last).  src[g'] = the formed slot that takes slot position g'.
template <int V>
__global__ __launch_bounds__(kDealThreads) void slot_deal_kernel(const uint32_t* __restrict__ sslots,
                                                                 const uint16_t* __restrict__ slotmax, int NT, int PW, int R,
                                                                 int64_t G, int partial, int32_t* __restrict__ src) {
    extern __shared__ __align__(16) uint32_t lds[];
    constexpr int D = 4 * V;
    uint32_t* ms = lds;                                              // [PW][D] maximum vectors of the stratum
    uint32_t* env = ms + static_cast<size_t>(PW) * D;                // [PW][D] running envelope of every pair
    int32_t* envtot = reinterpret_cast<int32_t*>(env + static_cast<size_t>(PW) * D);
    int32_t* seq = envtot + PW;                                      // pairs in the order they choose
    uint8_t* free_s = reinterpret_cast<uint8_t*>(seq + PW);          // [PW] slot of the stratum not taken yet
    __shared__ uint32_t red[2][kDealThreads / 64];
    const int tid = threadIdx.x;
    for (int i = tid; i < PW * D; i += kDealThreads) env[i] = 0;
    int step_parity = 0;
    for (int j = R - 1; j >= 0; --j) {
        const int64_t s0 = static_cast<int64_t>(j) * PW;
        const int n_s = static_cast<int>((G - s0 < PW) ? (G - s0) : PW);
        __syncthreads();
        for (int i = tid; i < n_s; i += kDealThreads) {
            const int64_t g = sslots[s0 + i];
            uint32_t v[D];
#pragma unroll
            for (int d = 0; d < D; ++d) v[d] = 0;
#pragma unroll
            for (int t = 0; t < 2 * D; ++t) v[t >> 1] |= (t < NT ? static_cast<uint32_t>(slotmax[g * NT + t]) : 0u) << (16 * (t & 1));
#pragma unroll
            for (int d = 0; d < D; ++d) ms[i * D + d] = v[d];
            free_s[i] = 1;
        }
        __syncthreads();
        int pstar = -1;
        if (j == R - 1 && partial) {
            // position G - 1 belongs to this pair, and the partial slot (last of the stratum) stays there
            const int pos = static_cast<int>(G - 1 - s0);
            pstar = (j & 1) ? PW - 1 - pos : pos;
            if (tid < D) env[pstar * D + tid] = pk_max(env[pstar * D + tid], ms[(n_s - 1) * D + tid]);
            if (tid == 0) { free_s[n_s - 1] = 0; src[G - 1] = static_cast<int32_t>(sslots[s0 + n_s - 1]); }
            __syncthreads();
        }
        for (int p = tid; p < PW; p += kDealThreads) {
            uint32_t acc = 0;
#pragma unroll
            for (int d = 0; d < D; ++d) acc = pk_add(acc, env[p * D + d]);
            envtot[p] = static_cast<int32_t>(halves(acc));
        }
        __syncthreads();
        // pairs that own a slot position of this round, by descending envelope total, then pair index
        for (int p = tid; p < PW; p += kDealThreads) {
            if (slot_of(j, p, PW) >= G || p == pstar) continue;
            const int32_t mine = envtot[p];
            int rank = 0;
            for (int q = 0; q < PW; ++q) {
                if (slot_of(j, q, PW) >= G || q == pstar) continue;
                const int32_t o = envtot[q];
                rank += (o > mine || (o == mine && q < p)) ? 1 : 0;
            }
            seq[rank] = p;
        }
        __syncthreads();
        const int n_steps = n_s - (pstar >= 0 ? 1 : 0);
        for (int step = 0; step < n_steps; ++step, step_parity ^= 1) {
            const int p = seq[step];                     // one of this round's pairs: seq holds exactly n_steps of them
            uint32_t e[D];
#pragma unroll
            for (int d = 0; d < D; ++d) e[d] = env[p * D + d];
            uint32_t key = ~0u;
            for (int i = tid; i < n_s; i += kDealThreads) {
                if (!free_s[i]) continue;
                uint32_t v[D];
#pragma unroll
                for (int d = 0; d < D; ++d) v[d] = ms[i * D + d];
                const uint32_t kk = (excess<V>(v, e) << 12) | static_cast<uint32_t>(i);
                key = kk < key ? kk : key;
            }
            int win = static_cast<int>(block_min32(key, red[step_parity]) & 0xfffu);
            win = win < n_s ? win : n_s - 1;             // (a free slot always exists: as many slots as pairs)
            // the owner of the slot clears it (only the owner reads that flag); a pair chooses once per round, so the
            // envelope written here is not read again before the round's closing barrier
            if (win % kDealThreads == tid) {
                free_s[win] = 0;
                src[slot_of(j, p, PW)] = static_cast<int32_t>(sslots[s0 + win]);
            }
            if (tid < D) env[p * D + tid] = pk_max(env[p * D + tid], ms[win * D + tid]);
        }
    }
}

// ---- d. order -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void slot_emit_kernel(const int32_t* __restrict__ slotrows, const int32_t* __restrict__ src,
                                                        int64_t n_rows, int32_t* __restrict__ order) {
    const int64_t pos = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (pos >= n_rows) return;
    const int64_t G = (n_rows + 63) / 64;
    int64_t s = src[pos >> 6];
    s = (s >= 0 && s < G) ? s : (pos >> 6);              // the deal fills every position; never index outside the list
    order[pos] = slotrows[s * 64 + (pos & 63)];
}

// ---- plan: the two sorts and where the pieces sit in the workspace ------------------------------------------------------------
struct SlotPlan {
    int64_t n_rows, G;
    int NT, PW, R;
    SortGeom rows, slots;
    size_t off_bv, off_ka, off_kb, off_va, off_vb, off_ska, off_skb, off_sva, off_svb, off_table, off_bsum, off_slotrows,
        off_slotmax, off_src, total;
    size_t deal_lds;
};

size_t deal_lds_bytes(int PW, int NT) {
    return static_cast<size_t>(PW) * (32 * static_cast<size_t>((NT + 7) / 8) + 9);   // ms, env: V x 16 bytes; envtot, seq: int32; free: bytes
}

int make_slot_plan(int64_t n_rows, const int32_t* plan, SlotPlan& p) {
    DIF_REQUIRE(plan, DIF_E_BADARG, "dif_sliced_slot_order: null plan");
    DIF_REQUIRE(n_rows > 0 && n_rows < (int64_t(1) << 28), DIF_E_RANGE, "dif_sliced_slot_order: need 0 < n_rows < 2^28");
    p.n_rows = n_rows;
    p.G = (n_rows + 63) / 64;
    p.PW = plan[3]; p.R = plan[5]; p.NT = plan[7];
    DIF_REQUIRE(plan[2] == p.G && p.PW >= 1 && p.R >= 1 && static_cast<int64_t>(p.R) * p.PW >= p.G &&
                static_cast<int64_t>(p.R - 1) * p.PW < p.G, DIF_E_BADARG,
                "dif_sliced_slot_order: the plan is not dif_sliced_plan's for %lld rows", static_cast<long long>(n_rows));
    p.deal_lds = deal_lds_bytes(p.PW, p.NT < 1 ? 1 : p.NT);
    DIF_REQUIRE(p.NT >= 1 && p.NT <= kMaxTiles && p.PW <= 4096 && p.deal_lds <= static_cast<size_t>(kDealLds), DIF_E_SHAPE,
                "dif_sliced_slot_order: covers up to %d tiles and PW * (32 * ceil(NT / 8) + 9) <= %d bytes of LDS", kMaxTiles,
                kDealLds);
    p.rows = sort_geom(n_rows, (p.NT + 12 + kRadixBits - 1) / kRadixBits);
    p.slots = sort_geom(p.G, 3);
    const size_t n = static_cast<size_t>(n_rows), g = static_cast<size_t>(p.G);
    const int64_t table_len = p.rows.table_len > p.slots.table_len ? p.rows.table_len : p.slots.table_len;
    Arena a;
    p.off_bv = a.take(n * p.NT * 2);
    p.off_ka = a.take(n * 4);
    p.off_kb = a.take(n * 4);
    p.off_va = a.take(n * 4);
    p.off_vb = a.take(n * 4);
    p.off_ska = a.take(g * 4);
    p.off_skb = a.take(g * 4);
    p.off_sva = a.take(g * 4);
    p.off_svb = a.take(g * 4);
    p.off_table = a.take(static_cast<size_t>(table_len) * 4);
    p.off_bsum = a.take(scan_scratch_bytes(table_len));
    p.off_slotrows = a.take(g * 64 * 4);
    p.off_slotmax = a.take(g * p.NT * 2);
    p.off_src = a.take(g * 4);
    p.total = a.o;
    return 0;
}

}  // namespace

extern "C" int dif_slots_version(void) { return DIF_SLOTS_VERSION; }
extern "C" const char* dif_slots_last_error(void) { return dif::err_buf(); }

extern "C" int64_t dif_sliced_slot_order_workspace_bytes(int64_t n_rows, const int32_t* plan) {
    SlotPlan p;
    if (make_slot_plan(n_rows, plan, p)) return 0;
    return static_cast<int64_t>(p.total);
}

extern "C" int dif_sliced_slot_order(const int32_t* rowptr, const int32_t* blkptr, int64_t n_src, int64_t row_begin,
                                     int64_t n_rows, const int32_t* plan, int32_t* order, void* workspace,
                                     int64_t workspace_bytes, dif_stream_t stream) {
    SlotPlan p;
    if (int rc = make_slot_plan(n_rows, plan, p)) return rc;
    DIF_REQUIRE(rowptr && order && workspace && (p.NT == 1 || blkptr), DIF_E_BADARG, "dif_sliced_slot_order: null pointer");
    DIF_REQUIRE(n_src > 0 && row_begin >= 0 && row_begin + n_rows <= n_src, DIF_E_BADARG,
                "dif_sliced_slot_order: rows [row_begin, row_begin + n_rows) must lie in [0, n_src)");
    DIF_REQUIRE(workspace_bytes >= 0, DIF_E_WORKSPACE, "dif_sliced_slot_order: negative workspace size");
    if (int rc = check_workspace("dif_sliced_slot_order", workspace, static_cast<size_t>(workspace_bytes), p.total)) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const char* who = "dif_sliced_slot_order";
    uint16_t* bv = at<uint16_t>(ws, p.off_bv);
    SortBufs rb{at<uint32_t>(ws, p.off_ka), at<uint32_t>(ws, p.off_kb), at<uint32_t>(ws, p.off_va), at<uint32_t>(ws, p.off_vb),
                at<int32_t>(ws, p.off_table), at<int32_t>(ws, p.off_bsum)};
    if (int rc = dif::launch(who, slot_keys_kernel, dif::grid_of((n_rows + 255) / 256), dim3(256), 0, st, rowptr, blkptr, n_src,
                             p.NT, row_begin, n_rows, bv, rb.kin, rb.vin)) return rc;
    if (int rc = radix_sort(p.rows, rb, st)) return rc;
    SortBufs sb{at<uint32_t>(ws, p.off_ska), at<uint32_t>(ws, p.off_skb), at<uint32_t>(ws, p.off_sva), at<uint32_t>(ws, p.off_svb),
                at<int32_t>(ws, p.off_table), at<int32_t>(ws, p.off_bsum)};
    int32_t* slotrows = at<int32_t>(ws, p.off_slotrows);
    uint16_t* slotmax = at<uint16_t>(ws, p.off_slotmax);
    int32_t* src = at<int32_t>(ws, p.off_src);
    const int V = (p.NT + 7) / 8;
    const dim3 wgrid = dif::grid_of((n_rows + kWindow - 1) / kWindow);
    const int partial = (n_rows & 63) != 0 ? 1 : 0;
    auto window = [&](auto kernel) {
        return dif::launch(who, kernel, wgrid, dim3(kWindowThreads), 0, st, rb.vin, bv, p.NT, n_rows, slotrows, slotmax, sb.kin,
                           sb.vin);
    };
    if (int rc = V == 1 ? window(slot_window_kernel<1>) : (V == 2 ? window(slot_window_kernel<2>) : window(slot_window_kernel<3>)))
        return rc;
    if (int rc = radix_sort(p.slots, sb, st)) return rc;
    auto deal = [&](auto kernel) {
        return dif::launch(who, kernel, dim3(1), dim3(kDealThreads), p.deal_lds, st, sb.vin, slotmax, p.NT, p.PW, p.R, p.G, partial,
                           src);
    };
    if (int rc = V == 1 ? deal(slot_deal_kernel<1>) : (V == 2 ? deal(slot_deal_kernel<2>) : deal(slot_deal_kernel<3>))) return rc;
    return dif::launch(who, slot_emit_kernel, dif::grid_of((n_rows + 255) / 256), dim3(256), 0, st, slotrows, src, n_rows, order);
}
