// libdifformer_snapshots.so (C ABI: include/difformer_snapshots.h): the whole-model kernels for tiny graphs on a BATCH of
// snapshots -- `spatial-temporal/main.py:94-121` forwards 104 / 50 / 146 graphs of 20 / 129 / 1,068 nodes one after another and
// sums their costs before one backward.  Given the weights the snapshots are independent and their gradients add, so an epoch
// is ONE forward launch of T workgroups, ONE backward launch and one ordered sum of T gradient slabs.
//
// Workgroup b runs the one-workgroup model body of tiny_model.hip -- the SAME text, tiny_forward_body.h / tiny_backward_body.h
// included between the kernel's braces -- on a local view `a` of the arguments: the common TinyArgs (parameters and flags, by
// value) with n, x, the CSR, rnd, tape, y (backward: gy, dx, scratch, the gradient pointers) taken from record b of a device
// table.  The view copies scalars and pointers only; the per-layer pointer arrays stay in the kernel-argument segment (`a.lp`
// points at them; `a.lg[l]` adds the slab's offset to the common pointers on the fly), so nothing is indexed dynamically in
// private memory: the hidden <= 4 kernels use no scratch memory, the hidden 5..8 ones spill registers at 512 threads as
// tiny_forward_kernel<8> / tiny_backward_kernel<8> do (204 / 1,208 bytes per lane against 144 / 964; -Rpass-analysis=
// kernel-resource-usage, profiles/r18_snapshot_batches.md).  The body never reads blockIdx, and a workgroup touches nothing but
// its own rows, its own tape / scratch range and its own slab: a snapshot's result does not depend on its neighbours.
//
// The backward's second kernel forms grad[p] = float32(sum_b slab[b][p]), the sum in float64 in the order b = 0 .. T - 1: no
// floating-point atomics.  A workgroup zeroes its slab before it writes its gradients, so the padding between parameters is
// zero and not stale memory.
#include <stdarg.h>
#include "tiny_stages.h"
#include "tiny_host.h"
#include "../../include/difformer_snapshots.h"

// dif::launch (csrc/dif_launch.h) reports through these; api.hip defines them for libdifformer_hip.so, this file for THIS
// library (linked -Bsymbolic: each library binds its own), so that its errors land in dif_snap_last_error().
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

using namespace tiny;

namespace {

static_assert(DIF_SNAP_RECORD_FIELDS == 12, "SnapRecord is the header's record");
struct SnapRecord {
    int64_t n, row0;
    const int* rowptr; const int* src; const float* val;
    const int* rowptr_t; const int* dst_t; const float* val_t;
    int64_t tape_off, scratch_off, reserved[2];
};
static_assert(sizeof(SnapRecord) == 8 * DIF_SNAP_RECORD_FIELDS, "SnapRecord is DIF_SNAP_RECORD_FIELDS int64 words");

// every address of a record is device-global memory (the compiler cannot know that of a pointer it loaded from a table)
template <typename U>
__device__ __forceinline__ const U* global_ptr(const U* p) { return (const U*)dif::as_global(p); }

// `a.lg[l]` of the body: the common gradient pointers (into slab 0) moved to this workgroup's slab
struct SlabGrads {
    const LayerGrads* common;
    size_t off;
    __device__ __forceinline__ LayerGrads operator[](int l) const {
        const LayerGrads& g = common[l];
        return LayerGrads{g.wk + off, g.bk + off, g.wq + off, g.bq + off, g.wv + off, g.bv + off, g.lnw + off, g.lnb + off};
    }
};

// The body's `a`: TinyArgs field for field, the per-layer arrays by reference.
struct SnapArgs {
    int n, f_in, d, c, layers, sigmoid, use_bn, residual, use_weight, use_graph, use_source, training;
    float alpha, a_s, g_s, p_drop, eps;
    const float* x;
    int64_t ldx;
    const float *w0, *b0, *ln0w, *ln0b, *wo, *bo;
    const LayerPtrs* lp;
    const int* rowptr;
    const int* nbr;
    const float* val;
    const float* rnd;
    float* tape;
    float* y;
    const float* gy;
    float *gw0, *gb0, *gln0w, *gln0b, *gwo, *gbo;
    SlabGrads lg;
    float* dx;
    float* scratch;
};

// what both passes share: flags, parameters, and the snapshot's n, x, rnd, tape
__device__ __forceinline__ void snap_view(SnapArgs& a, const TinyArgs& k, const SnapRecord& r) {
    a.n = static_cast<int>(r.n); a.f_in = k.f_in; a.d = k.d; a.c = k.c; a.layers = k.layers; a.sigmoid = k.sigmoid; a.use_bn = k.use_bn;
    a.residual = k.residual; a.use_weight = k.use_weight; a.use_graph = k.use_graph; a.use_source = k.use_source; a.training = k.training;
    a.alpha = k.alpha; a.a_s = k.a_s; a.g_s = k.g_s; a.p_drop = k.p_drop; a.eps = k.eps;
    a.x = k.x + r.row0 * k.ldx; a.ldx = k.ldx;
    a.w0 = k.w0; a.b0 = k.b0; a.ln0w = k.ln0w; a.ln0b = k.ln0b; a.wo = k.wo; a.bo = k.bo;
    a.lp = k.lp;
    a.rnd = k.rnd ? k.rnd + static_cast<int64_t>(k.layers + 1) * k.d * r.row0 : nullptr;
    a.tape = k.tape + r.tape_off;
}

template <int DP>
__global__ __launch_bounds__(512) void snap_forward_kernel(const TinyArgs common, const SnapRecord* __restrict__ records) {
    const SnapRecord& rec = records[blockIdx.x];
    SnapArgs a;
    snap_view(a, common, rec);
    a.rowptr = global_ptr(rec.rowptr); a.nbr = global_ptr(rec.src); a.val = global_ptr(rec.val);
    a.y = common.y + rec.row0 * common.c;
#include "tiny_forward_body.h"
}

template <int DP>
__global__ __launch_bounds__(512) void snap_backward_kernel(const TinyArgs common, const SnapRecord* __restrict__ records,
                                                             float* __restrict__ slabs, int64_t slab_stride) {
    const SnapRecord& rec = records[blockIdx.x];
    SnapArgs a;
    snap_view(a, common, rec);
    a.rowptr = global_ptr(rec.rowptr_t); a.nbr = global_ptr(rec.dst_t); a.val = global_ptr(rec.val_t);
    a.gy = common.gy + rec.row0 * common.c;
    a.dx = common.dx ? common.dx + rec.row0 * common.f_in : nullptr;
    a.scratch = common.scratch + rec.scratch_off;
    const size_t off = static_cast<size_t>(blockIdx.x) * static_cast<size_t>(slab_stride);
    a.gw0 = common.gw0 + off; a.gb0 = common.gb0 + off; a.gln0w = common.gln0w + off; a.gln0b = common.gln0b + off;
    a.gwo = common.gwo + off; a.gbo = common.gbo + off;
    a.lg.common = common.lg; a.lg.off = off;
    // the slab's padding between parameters: zero, before any gradient lands (the body's first store into the slab comes after
    // several __syncthreads of its own; this one orders the two for the workgroup)
    for (int64_t k_ = threadIdx.x; k_ < slab_stride; k_ += blockDim.x) slabs[off + k_] = 0.f;
    __syncthreads();
#include "tiny_backward_body.h"
}

// grad[p] = float32(sum_b slab[b][p]): float64, b ascending, one rounding
__global__ __launch_bounds__(256) void snap_slab_sum_kernel(const float* __restrict__ slabs, int T, int64_t P, float* __restrict__ grad) {
    const int64_t p = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (p >= P) return;
    double s = 0.0;
    for (int b = 0; b < T; ++b) s += static_cast<double>(slabs[static_cast<size_t>(b) * P + p]);
    grad[p] = static_cast<float>(s);
}

constexpr int kMaxSnapshots = 65535;

int check_batch(const dif_tiny_cfg* cfg, int T, const int64_t* records, const char* who) {
    if (int rc = check_cfg(cfg)) return rc;
    DIF_REQUIRE(T >= 1 && T <= kMaxSnapshots, DIF_E_SHAPE, "%s: 1 <= T <= %d snapshots (got %d)", who, kMaxSnapshots, T);
    DIF_REQUIRE(records && dif::aligned16(records), DIF_E_BADARG, "%s: null or misaligned record table", who);
    return 0;
}

}  // namespace

extern "C" int dif_snap_version(void) { return DIF_SNAP_VERSION; }
extern "C" const char* dif_snap_last_error(void) { return dif::err_buf(); }

// tiny_common.h's tape without the grid plans' ATTLO rows and partial sums: H, Z [(L + 1)], ATT [L], Q, K, V rows; DEN [L][n]; SUM [L][96]
extern "C" size_t dif_snap_tape_floats(int n, int hidden, int num_layers) {
    if (n < 1 || hidden < 1 || hidden > 8 || num_layers < 1 || num_layers > kMaxLayers) return 0;
    const size_t DP = hidden <= 4 ? 4 : 8, L = static_cast<size_t>(num_layers), N = static_cast<size_t>(n);
    size_t f = N * DP * (2 * (L + 1) + L + 3) + L * N + L * 96;
    return f + ((-f) & 3);
}

// the one-workgroup backward's 14 [n][DP] slots and 3 [n] arrays
extern "C" size_t dif_snap_scratch_floats(int n, int hidden, int num_layers) {
    if (n < 1 || hidden < 1 || hidden > 8 || num_layers < 1 || num_layers > kMaxLayers) return 0;
    const size_t DP = hidden <= 4 ? 4 : 8, N = static_cast<size_t>(n);
    size_t f = N * DP * kBwdSlots + 3 * N;
    return f + ((-f) & 3);
}

extern "C" int dif_snap_forward_f32(const dif_tiny_cfg* cfg, int T, const int64_t* records, const float* x, int64_t ldx,
                                    const void* const* params, const float* rnd, float* tape, float* y, dif_stream_t stream) {
    const char* who = "dif_snap_forward_f32";
    if (int rc = check_batch(cfg, T, records, who)) return rc;
    TinyArgs a{};
    if (int rc = fill(a, cfg, x, ldx, params)) return rc;
    DIF_REQUIRE(tape && y, DIF_E_BADARG, "%s: null tape / y", who);
    DIF_REQUIRE(dif::aligned16(tape), DIF_E_BADARG, "%s: tape must be 16-byte aligned", who);
    a.rnd = rnd; a.tape = tape; a.y = y;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int threads = block_threads(cfg->n);
    return dif::with_flags([&](auto NARROW) {               // hidden <= 4: rows padded to 4 columns, 8 otherwise
        return dif::launch(who, snap_forward_kernel<NARROW ? 4 : 8>, dim3(T), dim3(threads), 0, st, a,
                           reinterpret_cast<const SnapRecord*>(records));
    }, cfg->hidden <= 4);
}

extern "C" int dif_snap_backward_f32(const dif_tiny_cfg* cfg, int T, const int64_t* records, const float* x, int64_t ldx,
                                     const void* const* params, const float* rnd, float* tape, const float* grad_y,
                                     void* const* grads, float* slabs, int64_t slab_stride, float* grad_out, float* dx,
                                     float* scratch, dif_stream_t stream) {
    const char* who = "dif_snap_backward_f32";
    if (int rc = check_batch(cfg, T, records, who)) return rc;
    TinyArgs a{};
    if (int rc = fill(a, cfg, x, ldx, params)) return rc;
    DIF_REQUIRE(tape && grad_y && grads && scratch && slabs && grad_out, DIF_E_BADARG, "%s: null tape / grad_y / grads / scratch / slabs / grad_out", who);
    DIF_REQUIRE(dif::aligned16(tape) && dif::aligned16(scratch) && dif::aligned16(slabs), DIF_E_BADARG,
                "%s: tape / scratch / slabs must be 16-byte aligned", who);
    DIF_REQUIRE(slab_stride >= 4 && slab_stride % 4 == 0, DIF_E_BADARG, "%s: slab_stride must be a positive multiple of 4 floats", who);
    if (int rc = fill_grads(a, cfg, grads, who)) return rc;
    // every gradient lies inside slab 0, whole
    const int d = cfg->hidden, L = cfg->num_layers;
    auto inside = [&](const float* g, int64_t count) { return g == nullptr || (g >= slabs && g + count <= slabs + slab_stride); };
    bool ok = inside(a.gw0, static_cast<int64_t>(d) * cfg->in_channels) && inside(a.gb0, d) && inside(a.gwo, static_cast<int64_t>(cfg->out_channels) * d) &&
              inside(a.gbo, cfg->out_channels) && (!cfg->use_bn || (inside(a.gln0w, d) && inside(a.gln0b, d)));
    for (int l = 0; l < L; ++l) {
        const LayerGrads& g = a.lg[l];
        ok = ok && inside(g.wk, d * d) && inside(g.bk, d) && inside(g.wq, d * d) && inside(g.bq, d) &&
             (!cfg->use_weight || (inside(g.wv, d * d) && inside(g.bv, d))) && (!cfg->use_bn || (inside(g.lnw, d) && inside(g.lnb, d)));
    }
    DIF_REQUIRE(ok, DIF_E_BADARG, "%s: a gradient pointer leaves slab 0 (slab_stride %lld floats)", who, static_cast<long long>(slab_stride));
    a.rnd = rnd; a.tape = tape; a.gy = grad_y; a.dx = dx; a.scratch = scratch;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int threads = block_threads(cfg->n);
    const int rc = dif::with_flags([&](auto NARROW) {
        return dif::launch(who, snap_backward_kernel<NARROW ? 4 : 8>, dim3(T), dim3(threads), 0, st, a,
                           reinterpret_cast<const SnapRecord*>(records), slabs, slab_stride);
    }, cfg->hidden <= 4);
    if (rc) return rc;
    return dif::launch(who, snap_slab_sum_kernel, dif::grid_of((slab_stride + 255) / 256), dim3(256), 0, st, slabs, T, slab_stride, grad_out);
}
