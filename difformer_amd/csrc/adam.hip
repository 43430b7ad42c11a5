// The Adam update on the device: libdifformer_adam.so, C ABI in include/difformer_adam.h.
//
// Replaces optimizer.step() of the reference's drivers (node classification/main.py:111, image and text/main.py:95,
// spatial-temporal/main.py:83, physical particle/main.py:77: torch.optim.Adam, whose foreach path is seven multi-tensor launches
// per step) by one launch over every parameter of the model.
//
// Arithmetic, rounding, the step counter's ticket and edge semantics: the header.  In short: an element is evaluated in float64
// from float32 p, grad, m, v and rounded once per output; the table of tensors is a kernel argument; a workgroup owns one chunk
// of one tensor and finds the tensor by a uniform search over the running chunk totals; the last workgroup of a tensor to
// have READ its step writes step + 1.
#include <math.h>
#include <stdarg.h>
#include "dif_common.h"
#include "../../include/difformer_adam.h"

// dif::launch (csrc/dif_launch.h) reports through these; this library is linked -Bsymbolic and binds its own, so that its
// errors land in dif_adam_last_error().
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
constexpr int kMax = DIF_ADAM_MAX_TENSORS;
constexpr int kChunk = DIF_ADAM_CHUNK;
constexpr int64_t kMaxCount = int64_t(1) << 20;
constexpr int64_t kMaxChunks = (int64_t(1) << 31) - 1;     // workgroups of one launch
typedef long long i64;

static_assert(kMax >= 32, "the issue's floor for DIF_ADAM_MAX_TENSORS");
static_assert(DIF_ADAM_TICKET_BYTES == 4 * kMax, "one int32 ticket per tensor of a launch");
static_assert(kChunk % kBlock == 0, "a chunk is a whole number of workgroup passes");

// One launch's tensors, by value in the kernel arguments (2,500 of the 4,096 bytes a kernel may take).
struct Table {
    float* p[kMax];
    const float* g[kMax];
    float* m[kMax];
    float* v[kMax];
    float* step[kMax];
    i64 numel[kMax];
    int chunk_end[kMax];          // chunks of tensors 0 .. i: workgroup b belongs to the first i with b < chunk_end[i]
    int count;
};
static_assert(sizeof(Table) + 5 * sizeof(double) + sizeof(void*) <= 4096, "the kernel arguments");

__global__ __launch_bounds__(kBlock) void adam_kernel(const Table tab, double lr, double beta1, double beta2, double eps,
                                                      double wd, unsigned* __restrict__ tickets) {
    const int b = blockIdx.x;
    int i = 0;
    while (i + 1 < tab.count && b >= tab.chunk_end[i]) ++i;             // uniform over the workgroup
    const int first = i ? tab.chunk_end[i - 1] : 0;
    const unsigned chunks = static_cast<unsigned>(tab.chunk_end[i] - first);
    float* const step = tab.step[i];

    // the step count: read by thread 0, shared, and only then is this workgroup's ticket drawn (the header's argument)
    __shared__ float s_t;
    if (threadIdx.x == 0) s_t = *step + 1.0f;
    __syncthreads();
    const float tf = s_t;
    if (threadIdx.x == 0) {
        const unsigned drawn = __hip_atomic_fetch_add(tickets + i, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (drawn + 1u == chunks) {                                      // every workgroup of this tensor has read `step`
            *step = tf;
            __hip_atomic_store(tickets + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }

    const i64 n = tab.numel[i];
    const i64 begin = static_cast<i64>(b - first) * kChunk;
    const i64 end = begin + kChunk < n ? begin + kChunk : n;
    if (begin + static_cast<i64>(threadIdx.x) >= end) return;

    const double t = static_cast<double>(tf);
    const double step_size = lr / (1.0 - pow(beta1, t));
    const double root_bc2 = sqrt(1.0 - pow(beta2, t));
    const double one_b1 = 1.0 - beta1, one_b2 = 1.0 - beta2;
    float* __restrict__ const p = tab.p[i];
    const float* __restrict__ const g = tab.g[i];
    float* __restrict__ const m = tab.m[i];
    float* __restrict__ const v = tab.v[i];
    for (i64 e = begin + threadIdx.x; e < end; e += kBlock) {
        const double pe = static_cast<double>(p[e]);
        double ge = static_cast<double>(g[e]);
        if (wd != 0.0) ge += wd * pe;
        const double me = beta1 * static_cast<double>(m[e]) + one_b1 * ge;
        const double ve = beta2 * static_cast<double>(v[e]) + one_b2 * (ge * ge);
        const double pn = pe - step_size * (me / (sqrt(ve) / root_bc2 + eps));
        p[e] = static_cast<float>(pn);
        m[e] = static_cast<float>(me);
        v[e] = static_cast<float>(ve);
    }
}

inline bool hyper_ok(double x) { return x >= 0.0 && x <= 1.79769313486231570e308; }      // finite, not NaN, not negative

}  // namespace

extern "C" int dif_adam_version(void) { return DIF_ADAM_VERSION; }
extern "C" const char* dif_adam_last_error(void) { return dif::err_buf(); }

extern "C" int64_t dif_adam_launches(int64_t count) {
    if (count < 0 || count > kMaxCount) return -1;
    return (count + kMax - 1) / kMax;
}

extern "C" int dif_adam_step_f32(const int64_t* table, int64_t count, double lr, double beta1, double beta2, double eps,
                                 double weight_decay, void* tickets, dif_stream_t stream) {
    const char* who = "dif_adam_step_f32";
    DIF_REQUIRE(count >= 0 && count <= kMaxCount, DIF_E_BADARG, "%s: need 0 <= count <= 2^20 (got %lld)", who,
                static_cast<long long>(count));
    DIF_REQUIRE(hyper_ok(lr) && hyper_ok(eps) && hyper_ok(weight_decay), DIF_E_BADARG,
                "%s: lr, eps and weight_decay must be finite and >= 0 (got %g, %g, %g)", who, lr, eps, weight_decay);
    DIF_REQUIRE(beta1 >= 0.0 && beta1 < 1.0 && beta2 >= 0.0 && beta2 < 1.0, DIF_E_BADARG, "%s: need 0 <= beta < 1 (got %g, %g)", who,
                beta1, beta2);
    DIF_REQUIRE(tickets && dif::aligned<4>(tickets), DIF_E_BADARG, "%s: the tickets must be 4-byte aligned device memory", who);
    if (count == 0) return 0;
    DIF_REQUIRE(table != nullptr, DIF_E_BADARG, "%s: null table", who);
    // every row first: a rejected call enqueues nothing
    for (int64_t first = 0; first < count; first += kMax) {
        int64_t total = 0;
        for (int64_t r = first; r < count && r < first + kMax; ++r) {
            const int64_t* row = table + r * DIF_ADAM_TABLE_FIELDS;
            const int64_t numel = row[5];
            DIF_REQUIRE(numel >= 0, DIF_E_BADARG, "%s: tensor %lld: numel %lld", who, static_cast<long long>(r),
                        static_cast<long long>(numel));
            DIF_REQUIRE(row[4] != 0 && (numel == 0 || (row[0] && row[1] && row[2] && row[3])), DIF_E_BADARG,
                        "%s: tensor %lld: null pointer", who, static_cast<long long>(r));
            DIF_REQUIRE(((row[0] | row[1] | row[2] | row[3] | row[4]) & 3) == 0, DIF_E_BADARG,
                        "%s: tensor %lld: p, grad, exp_avg, exp_avg_sq and step must be 4-byte aligned", who, static_cast<long long>(r));
            total += numel ? (numel + kChunk - 1) / kChunk : 1;
            DIF_REQUIRE(total <= kMaxChunks, DIF_E_RANGE, "%s: more than 2^31 - 1 chunks of %d elements in one launch", who, kChunk);
        }
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    for (int64_t first = 0; first < count; first += kMax) {
        Table tab = {};
        int64_t total = 0;
        const int64_t here = count - first < kMax ? count - first : kMax;
        for (int64_t k = 0; k < here; ++k) {
            const int64_t* row = table + (first + k) * DIF_ADAM_TABLE_FIELDS;
            tab.p[k] = reinterpret_cast<float*>(static_cast<uintptr_t>(row[0]));
            tab.g[k] = reinterpret_cast<const float*>(static_cast<uintptr_t>(row[1]));
            tab.m[k] = reinterpret_cast<float*>(static_cast<uintptr_t>(row[2]));
            tab.v[k] = reinterpret_cast<float*>(static_cast<uintptr_t>(row[3]));
            tab.step[k] = reinterpret_cast<float*>(static_cast<uintptr_t>(row[4]));
            tab.numel[k] = row[5];
            total += row[5] ? (row[5] + kChunk - 1) / kChunk : 1;
            tab.chunk_end[k] = static_cast<int>(total);
        }
        tab.count = static_cast<int>(here);
        if (int rc = dif::launch(who, adam_kernel, dif::grid_of(total), dim3(kBlock), 0, st, tab, lr, beta1, beta2, eps, weight_decay,
                                 static_cast<unsigned*>(tickets))) return rc;
    }
    return 0;
}
