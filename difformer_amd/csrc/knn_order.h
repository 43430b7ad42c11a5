// The float64 total order of the neighbour graphs, one definition for csrc/knn_graph.hip and csrc/nbr_batched.hip: the smaller
// distance first, among equal distances the lower index first, a NaN distance after every number.  Distances become unsigned
// 64-bit keys that compare like the doubles; a list is (key, index) sorted ascending in registers with static indices only.
#pragma once
#include <stdint.h>
#include <hip/hip_runtime.h>

namespace dif {

constexpr uint64_t kEmpty = ~0ull;           // above every key: the empty slot of a list sorted ascending
constexpr uint64_t kNaNKey = ~0ull - 1;      // a NaN distance: after every number (+inf is 0xFFF0...0), before the empty slot

// distance -> unsigned key, monotone: a < b  <=>  key(a) < key(b); -0 and +0 share one key
__device__ __forceinline__ uint64_t dist_key(double d) {
    d += 0.0;
    const uint64_t b = __builtin_bit_cast(uint64_t, d);
    const uint64_t key = b ^ (static_cast<uint64_t>(static_cast<int64_t>(b) >> 63) | 0x8000000000000000ull);
    return d != d ? kNaNKey : key;
}
__device__ __forceinline__ double key_dist(uint64_t key) {      // kNaNKey and kEmpty -> a NaN
    const uint64_t b = (key & 0x8000000000000000ull) ? key ^ 0x8000000000000000ull : ~key;
    return __builtin_bit_cast(double, b);
}

// 1 / |x| from |x|^2; a zero row has cosine 0 with every row (a NaN stays a NaN)
__device__ __forceinline__ double rnorm(double n2) { return n2 == 0.0 ? 0.0 : 1.0 / sqrt(n2); }
// 1 - (x_i . x_j) / (|x_i| |x_j|), the same three operations in every route
__device__ __forceinline__ double cos_dist(double dot, double ri, double rj) { return fma(-(dot * ri), rj, 1.0); }

// (key, index) enters a list sorted ascending by key; strict comparisons: an equal key stays behind what is there already
template <int K>
__device__ __forceinline__ void insert2(uint64_t (&dk)[K], uint32_t (&ix)[K], uint64_t key, uint32_t index) {
    dk[K - 1] = key;
    ix[K - 1] = index;
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
        const bool up = dk[i] < dk[i - 1];
        const uint64_t ka = dk[i - 1], kb = dk[i];
        const uint32_t ia = ix[i - 1], ib = ix[i];
        dk[i - 1] = up ? kb : ka;
        dk[i] = up ? ka : kb;
        ix[i - 1] = up ? ib : ia;
        ix[i] = up ? ia : ib;
    }
}

}  // namespace dif
