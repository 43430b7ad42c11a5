// Evaluation metrics on the device: libdifformer_metrics.so, C ABI in include/difformer_metrics.h.
//
// Replaces, for node classification/data_utils.py:249-285 (copied in image and text/data_utils.py:180-216), the host loops of
// eval_rocauc (one sklearn roc_auc_score per label column) and eval_acc / eval_f1 (argmax, compare, count).
//
// ROC-AUC of one column is the Mann-Whitney statistic with mid-ranks: with P positives and N negatives among its labelled rows,
//   U2 = sum over positives p of ( 2 #{negatives with score < s_p} + #{negatives with score == s_p} ),   AUC = U2 / (2 P N).
// The device returns the INTEGERS {P, N, unlabelled, invalid, U2} per column and the host divides: nothing is accumulated in
// floating point, so the table is bitwise reproducible.  All C columns go through ONE sort:
//   a. rocauc_key_kernel    key = order-preserving uint32 image of the float32 score (-0.0 taken as +0.0), payload = the flat
//                           element index row * C + column;
//   b. radix_sort           four passes on the score key; rocauc_rekey_kernel then writes key = column from the payload and
//                           key_passes(C) more passes (stable, LSD) leave column c as the score-ordered segment [c n, (c + 1) n);
//   c. rocauc_mark_kernel   per sorted element its class (read back through the payload): negative / positive flags, the head
//                           flag of its tie group (first of the column, or a key that differs from its predecessor's: a group
//                           never crosses a column), and the per-column counts of unlabelled and invalid elements;
//   d. exclusive_scan       of the three flag arrays; rocauc_heads_kernel compacts the head positions by group id;
//   e. rocauc_groups_kernel one thread per tie group adds  pos_in_group (2 neg_before_group_in_column + neg_in_group)  to its
//                           column's U2 (64-bit integer add, summed over the workgroup first); rocauc_finish_kernel writes P, N.
// Work per element is constant whatever the length of a tie group; every loop is bounded by the sizes; no kernel waits for
// another workgroup.
//
// The accuracy count is one kernel: a lane group per row takes the argmax (first maximal index; NaN above every number, the
// first NaN wins -- torch.argmax / numpy.argmax) and the workgroup adds {correct, labelled} as integers.
#include <stdarg.h>
// the device sort of the graph construction (scan, radix passes, workspace layout): gcn_csr.hip is its one home and gives
// that part alone under this switch -- its kernels are compiled into this library too, nothing is linked across
#define DIF_GCN_CSR_SORT_ONLY
#include "gcn_csr.hip"
#include "../../include/difformer_metrics.h"

// dif::launch (csrc/dif_launch.h) reports through these; this library is linked -Bsymbolic and binds its own, so that its
// errors land in dif_metrics_last_error().
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
constexpr int kMaxColumns = 65536;                        // C of the ROC-AUC table, K of the argmax
constexpr int64_t kMaxPairs = (int64_t(1) << 31) - 1;     // uint32 payload, int32 scans
typedef unsigned long long u64;

// class codes of include/difformer_metrics.h
constexpr uint32_t kNeg = 0, kPos = 1, kUnlabelled = 2;

// float32 bits -> uint32 in the order of the values; -0.0 and +0.0 share a key
__device__ __forceinline__ uint32_t score_key(uint32_t bits) {
    if ((bits << 1) == 0u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__device__ __forceinline__ bool finite_bits(uint32_t bits) { return (bits & 0x7f800000u) != 0x7f800000u; }

// sum over the workgroup, valid in thread 0 (kBlock = 4 waves); one barrier
__device__ __forceinline__ u64 block_sum(u64 v, u64* red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return red[0] + red[1] + red[2] + red[3];
}

// ---- a. keys --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void rocauc_key_kernel(const float* __restrict__ score, int64_t lds, uint32_t m, uint32_t C,
                                                            uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t e64 = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (e64 >= m) return;
    const uint32_t e = static_cast<uint32_t>(e64);
    const uint32_t row = e / C, col = e - row * C;
    keys[e] = score_key(__float_as_uint(score[static_cast<int64_t>(row) * lds + col]));
    vals[e] = e;
}

// ---- b. the column becomes the key --------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void rocauc_rekey_kernel(const uint32_t* __restrict__ vals, uint32_t m, uint32_t C,
                                                              uint32_t* __restrict__ keys) {
    const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (i >= m) return;
    keys[i] = vals[i] % C;
}

// ---- c. flags of the sorted elements ------------------------------------------------------------------------------------------
// counts is int64 [C][5] = {P, N, unlabelled, invalid, U2}, zero on entry; this kernel adds to [2] and [3].
__global__ __launch_bounds__(kBlock) void rocauc_mark_kernel(const uint32_t* __restrict__ vals, const float* __restrict__ score,
                                                             int64_t lds, const uint8_t* __restrict__ cls, int64_t ldc, uint32_t m,
                                                             uint32_t n, uint32_t C, int32_t* __restrict__ neg,
                                                             int32_t* __restrict__ pos, int32_t* __restrict__ head,
                                                             u64* __restrict__ counts) {
    __shared__ u64 red[2][kBlock / 64];
    const int64_t j0 = static_cast<int64_t>(blockIdx.x) * kBlock;
    const int64_t j = j0 + threadIdx.x;
    const bool live = j < m;
    const int lane = threadIdx.x & 63;
    uint32_t key = 0, code = kUnlabelled;
    bool fin = true;
    if (live) {
        uint32_t e = vals[j];
        e = e < m ? e : m - 1;                              // (the sort returns a permutation; never index outside the operands)
        const uint32_t row = e / C, col = e - row * C;
        const uint32_t bits = __float_as_uint(score[static_cast<int64_t>(row) * lds + col]);
        key = score_key(bits);
        fin = finite_bits(bits);
        code = cls[static_cast<int64_t>(row) * ldc + col];
    }
    // the predecessor's key: the lane below, or for the first lane of a wave the element read again
    uint32_t prev = __shfl_up(key, 1, 64);
    if (live && lane == 0 && j > 0) {
        uint32_t e = vals[j - 1];
        e = e < m ? e : m - 1;
        const uint32_t row = e / C, col = e - row * C;
        prev = score_key(__float_as_uint(score[static_cast<int64_t>(row) * lds + col]));
    }
    const bool labelled = code == kNeg || code == kPos;
    const uint32_t unl = (live && code == kUnlabelled) ? 1u : 0u;
    const uint32_t inv = (live && (code > kUnlabelled || (labelled && !fin))) ? 1u : 0u;
    uint32_t colj = 0;
    if (live) {
        colj = static_cast<uint32_t>(j / n);
        neg[j] = (code == kNeg && fin) ? 1 : 0;
        pos[j] = (code == kPos && fin) ? 1 : 0;
        head[j] = (j % n == 0 || key != prev) ? 1 : 0;
    }
    // the workgroup's elements are consecutive: usually one column, then one add per workgroup and count
    const int64_t jl = (j0 + kBlock - 1 < m) ? j0 + kBlock - 1 : static_cast<int64_t>(m) - 1;
    if (j0 / n == jl / n) {
        const u64 su = block_sum(unl, red[0]);
        const u64 si = block_sum(inv, red[1]);
        if (threadIdx.x == 0) {
            const uint32_t c0 = static_cast<uint32_t>(j0 / n);
            if (su) atomicAdd(&counts[static_cast<int64_t>(c0) * 5 + 2], su);
            if (si) atomicAdd(&counts[static_cast<int64_t>(c0) * 5 + 3], si);
        }
    } else {
        if (unl) atomicAdd(&counts[static_cast<int64_t>(colj) * 5 + 2], u64(1));
        if (inv) atomicAdd(&counts[static_cast<int64_t>(colj) * 5 + 3], u64(1));
    }
}

// ---- d. head positions by group id ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void rocauc_heads_kernel(const int32_t* __restrict__ head, const int32_t* __restrict__ gid,
                                                              uint32_t m, int32_t* __restrict__ headpos) {
    const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (j >= m) return;
    if (head[j]) {
        const int32_t g = gid[j];
        if (g >= 0 && static_cast<uint32_t>(g) < m) headpos[g] = static_cast<int32_t>(j);
    }
}

// ---- e. one thread per tie group --------------------------------------------------------------------------------------------------
// sneg / spos: exclusive scans of the flags; tot = {negatives, positives, groups} of the whole list
__global__ __launch_bounds__(kBlock) void rocauc_groups_kernel(const int32_t* __restrict__ headpos, const int32_t* __restrict__ sneg,
                                                               const int32_t* __restrict__ spos, const int32_t* __restrict__ tot,
                                                               uint32_t m, uint32_t n, u64* __restrict__ counts) {
    __shared__ u64 red[kBlock / 64];
    int64_t G = tot[2];
    G = G < 0 ? 0 : (G > m ? m : G);
    const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kBlock;
    if (g0 >= G) return;                                     // (uniform over the workgroup)
    const int64_t g = g0 + threadIdx.x;
    const auto start_of = [&](int64_t q) -> int64_t {        // first element of group q; q == G: the end of the list
        if (q >= G) return m;
        const int64_t p = headpos[q];
        return p < 0 ? 0 : (p > m ? m : p);
    };
    u64 add = 0;
    uint32_t col = 0;
    if (g < G) {
        const int64_t a = start_of(g), b = start_of(g + 1);
        if (a < m && b > a) {
            col = static_cast<uint32_t>(a / n);
            const int64_t cs = static_cast<int64_t>(col) * n;
            const int64_t neg_a = sneg[a], pos_a = spos[a];
            const int64_t neg_b = b < m ? sneg[b] : tot[0], pos_b = b < m ? spos[b] : tot[1];
            const int64_t before = neg_a - sneg[cs], neg_in = neg_b - neg_a, pos_in = pos_b - pos_a;
            add = static_cast<u64>(pos_in) * static_cast<u64>(2 * before + neg_in);
        }
    }
    const int64_t gl = (g0 + kBlock - 1 < G) ? g0 + kBlock - 1 : G - 1;
    const int64_t first = start_of(g0), last = start_of(gl);
    if (first < m && last < m && first / n == last / n) {
        const u64 s = block_sum(add, red);
        if (threadIdx.x == 0 && s) atomicAdd(&counts[(first / n) * 5 + 4], s);
    } else if (add) {
        atomicAdd(&counts[static_cast<int64_t>(col) * 5 + 4], add);
    }
}

__global__ __launch_bounds__(kBlock) void rocauc_finish_kernel(const int32_t* __restrict__ sneg, const int32_t* __restrict__ spos,
                                                               const int32_t* __restrict__ tot, uint32_t n, uint32_t C,
                                                               int64_t* __restrict__ counts) {
    const int64_t c = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
    if (c >= C) return;
    const int64_t a = c * n, b = (c + 1) * n;
    const bool end = c + 1 == C;
    counts[c * 5 + 0] = static_cast<int64_t>(end ? tot[1] : spos[b]) - spos[a];
    counts[c * 5 + 1] = static_cast<int64_t>(end ? tot[0] : sneg[b]) - sneg[a];
}

// ---- argmax and count -----------------------------------------------------------------------------------------------------------------
// W lanes per row (a power of two up to 64).  A candidate is (value key << 32) | ~index: the largest wins, so among equal
// values the lowest index; NaN has the largest value key.
__global__ __launch_bounds__(kBlock) void argmax_correct_kernel(const float* __restrict__ pred, int64_t ldp,
                                                                const int64_t* __restrict__ label,
                                                                const uint8_t* __restrict__ labelled, int64_t n, int K, int W,
                                                                u64* __restrict__ out) {
    __shared__ u64 red[2][kBlock / 64];
    const int rows_per_block = kBlock / W;
    const int sub = threadIdx.x % W;
    const int64_t row = static_cast<int64_t>(blockIdx.x) * rows_per_block + threadIdx.x / W;
    u64 best = 0;
    if (row < n) {
        const float* p = pred + row * ldp;
        for (int k = sub; k < K; k += W) {
            const uint32_t bits = __float_as_uint(p[k]);
            const uint32_t key = ((bits & 0x7fffffffu) > 0x7f800000u) ? 0xffffffffu : score_key(bits);
            const u64 cand = (static_cast<u64>(key) << 32) | (0xffffffffu - static_cast<uint32_t>(k));
            best = cand > best ? cand : best;
        }
    }
    for (int off = W >> 1; off > 0; off >>= 1) {             // W divides 64: the partners are lanes of the same row
        const u64 o = __shfl_xor(best, off, 64);
        best = o > best ? o : best;
    }
    u64 ok = 0, lab = 0;
    if (row < n && sub == 0 && labelled[row]) {
        lab = 1;
        const int64_t arg = static_cast<int64_t>(0xffffffffu - static_cast<uint32_t>(best & 0xffffffffu));
        ok = (label[row] == arg) ? 1 : 0;
    }
    const u64 s_ok = block_sum(ok, red[0]);
    const u64 s_lab = block_sum(lab, red[1]);
    if (threadIdx.x == 0) {
        if (s_ok) atomicAdd(&out[0], s_ok);
        if (s_lab) atomicAdd(&out[1], s_lab);
    }
}

// ---- plan: the sort and where the pieces sit in the workspace --------------------------------------------------------------------------
struct RocPlan {
    int64_t m;
    SortGeom score, column;
    size_t off_ka, off_kb, off_va, off_vb, off_headpos, off_table, off_bsum, off_tot, total;
};

int make_roc_plan(const char* who, int64_t n, int C, RocPlan& p) {
    DIF_REQUIRE(n >= 1, DIF_E_BADARG, "%s: need n >= 1 (got %lld)", who, static_cast<long long>(n));
    DIF_REQUIRE(C >= 1 && C <= kMaxColumns, DIF_E_SHAPE, "%s: need 1 <= C <= %d (got %d)", who, kMaxColumns, C);
    DIF_REQUIRE(n <= kMaxPairs / C, DIF_E_RANGE, "%s: n * C = %lld * %d exceeds 2^31 - 1 pairs per call", who,
                static_cast<long long>(n), C);
    p.m = n * C;
    p.score = sort_geom(p.m, 4);
    p.column = p.score;
    p.column.passes = C > 1 ? key_passes(C) : 0;            // one column: the score order is the result
    const size_t m = static_cast<size_t>(p.m);
    const int64_t scan_n = p.m > p.score.table_len ? p.m : p.score.table_len;
    Arena a;
    p.off_ka = a.take(m * 4);
    p.off_kb = a.take(m * 4);
    p.off_va = a.take(m * 4);
    p.off_vb = a.take(m * 4);
    p.off_headpos = a.take(m * 4);
    p.off_table = a.take(static_cast<size_t>(p.score.table_len) * 4);
    p.off_bsum = a.take(scan_scratch_bytes(scan_n));
    p.off_tot = a.take(16);
    p.total = a.o;
    return 0;
}

}  // namespace

extern "C" int dif_metrics_version(void) { return DIF_METRICS_VERSION; }
extern "C" const char* dif_metrics_last_error(void) { return dif::err_buf(); }

extern "C" int64_t dif_rocauc_workspace_bytes(int64_t n, int C) {
    RocPlan p;
    if (make_roc_plan("dif_rocauc_workspace_bytes", n, C, p)) return 0;
    return static_cast<int64_t>(p.total);
}

extern "C" int dif_rocauc_counts_f32(const float* score, int64_t lds, const uint8_t* cls, int64_t ldc, int64_t n, int C,
                                     int64_t* counts, void* workspace, int64_t workspace_bytes, dif_stream_t stream) {
    const char* who = "dif_rocauc_counts_f32";
    DIF_REQUIRE(score && cls && counts && workspace, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<4>(score) && dif::aligned<8>(counts) && dif::aligned<16>(workspace), DIF_E_BADARG,
                "%s: score must be 4-byte, counts 8-byte and the workspace 16-byte aligned", who);
    RocPlan p;
    if (int rc = make_roc_plan(who, n, C, p)) return rc;
    DIF_REQUIRE(lds >= C && ldc >= C, DIF_E_BADARG, "%s: leading dimensions (%lld, %lld) smaller than C = %d", who,
                static_cast<long long>(lds), static_cast<long long>(ldc), C);
    DIF_REQUIRE(workspace_bytes >= 0 && static_cast<size_t>(workspace_bytes) >= p.total, DIF_E_WORKSPACE,
                "%s: workspace too small (%lld < %zu)", who, static_cast<long long>(workspace_bytes), p.total);
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    const uint32_t m = static_cast<uint32_t>(p.m), un = static_cast<uint32_t>(n), uC = static_cast<uint32_t>(C);
    const dim3 grid = dif::grid_of((p.m + kBlock - 1) / kBlock), block(kBlock);
    SortBufs b{at<uint32_t>(ws, p.off_ka), at<uint32_t>(ws, p.off_kb), at<uint32_t>(ws, p.off_va), at<uint32_t>(ws, p.off_vb),
               at<int32_t>(ws, p.off_table), at<int32_t>(ws, p.off_bsum)};
    int32_t* headpos = at<int32_t>(ws, p.off_headpos);
    int32_t* tot = at<int32_t>(ws, p.off_tot);
    if (int rc = zero_async(who, counts, static_cast<size_t>(C) * 5 * 8, st)) return rc;
    if (int rc = dif::launch(who, rocauc_key_kernel, grid, block, 0, st, score, lds, m, uC, b.kin, b.vin)) return rc;
    if (int rc = radix_sort(p.score, b, st)) return rc;
    if (p.column.passes > 0) {
        if (int rc = dif::launch(who, rocauc_rekey_kernel, grid, block, 0, st, b.vin, m, uC, b.kin)) return rc;
        if (int rc = radix_sort(p.column, b, st)) return rc;
    }
    // the payload stays where the sort left it; the three other arrays take the flags, the group ids go over the payload
    // once the flags are written
    int32_t* neg = reinterpret_cast<int32_t*>(b.kin);
    int32_t* pos = reinterpret_cast<int32_t*>(b.kout);
    int32_t* head = reinterpret_cast<int32_t*>(b.vout);
    int32_t* gid = reinterpret_cast<int32_t*>(b.vin);
    if (int rc = dif::launch(who, rocauc_mark_kernel, grid, block, 0, st, b.vin, score, lds, cls, ldc, m, un, uC, neg, pos, head,
                             reinterpret_cast<u64*>(counts))) return rc;
    if (int rc = exclusive_scan(neg, p.m, neg, tot + 0, b.bsum, st)) return rc;
    if (int rc = exclusive_scan(pos, p.m, pos, tot + 1, b.bsum, st)) return rc;
    if (int rc = exclusive_scan(head, p.m, gid, tot + 2, b.bsum, st)) return rc;
    if (int rc = dif::launch(who, rocauc_heads_kernel, grid, block, 0, st, head, gid, m, headpos)) return rc;
    if (int rc = dif::launch(who, rocauc_groups_kernel, grid, block, 0, st, headpos, neg, pos, tot, m, un,
                             reinterpret_cast<u64*>(counts))) return rc;
    return dif::launch(who, rocauc_finish_kernel, dif::grid_of((C + kBlock - 1) / kBlock), block, 0, st, neg, pos, tot, un, uC,
                       counts);
}

extern "C" int dif_argmax_correct_f32(const float* pred, int64_t ldp, const int64_t* label, const uint8_t* labelled, int64_t n,
                                      int K, int64_t* out, dif_stream_t stream) {
    const char* who = "dif_argmax_correct_f32";
    DIF_REQUIRE(pred && label && labelled && out, DIF_E_BADARG, "%s: null pointer", who);
    DIF_REQUIRE(dif::aligned<4>(pred) && dif::aligned<8>(label) && dif::aligned<8>(out), DIF_E_BADARG,
                "%s: pred must be 4-byte, label and out 8-byte aligned", who);
    DIF_REQUIRE(n >= 1, DIF_E_BADARG, "%s: need n >= 1 (got %lld)", who, static_cast<long long>(n));
    DIF_REQUIRE(K >= 1 && K <= kMaxColumns, DIF_E_SHAPE, "%s: need 1 <= K <= %d (got %d)", who, kMaxColumns, K);
    DIF_REQUIRE(ldp >= K, DIF_E_BADARG, "%s: leading dimension %lld smaller than K = %d", who, static_cast<long long>(ldp), K);
    int W = 1;
    while (W < K && W < 64) W *= 2;
    const int64_t blocks = (n + kBlock / W - 1) / (kBlock / W);
    DIF_REQUIRE(blocks <= kMaxPairs, DIF_E_RANGE, "%s: %lld rows of %d columns exceed the launch grid", who,
                static_cast<long long>(n), K);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (int rc = zero_async(who, out, 16, st)) return rc;
    return dif::launch(who, argmax_correct_kernel, dif::grid_of(blocks), dim3(kBlock), 0, st, pred, ldp, label, labelled, n, K, W,
                       reinterpret_cast<u64*>(out));
}
