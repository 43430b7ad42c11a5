// Streaming selection of the largest float32 scores of a row, shared by the sweeps of csrc/attn_topk.hip and csrc/knn_graph.hip.
//
// A candidate is ONE 64-bit word: the score as an order-preserving unsigned key in the upper half (NaN -> 0, the lowest;
// -0 -> +0), 0xFFFFFFFF - index in the lower half.  Unsigned `>` on that word IS the total order (larger score first, among
// equal scores the lower index first), and 0 -- below every real candidate -- is the empty slot.  A lane keeps K words, sorted,
// in registers: every index below is static, so nothing goes to scratch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dif {

// score -> unsigned key, monotone: a < b  <=>  key(a) < key(b); NaN -> 0 (below -inf); -0 and +0 share one key
__device__ __forceinline__ uint32_t score_key(float s) {
    s += 0.f;
    const uint32_t b = __builtin_bit_cast(uint32_t, s);
    const uint32_t key = b ^ (static_cast<uint32_t>(static_cast<int32_t>(b) >> 31) | 0x80000000u);
    return s != s ? 0u : key;
}
__device__ __forceinline__ float key_score(uint32_t key) {
    const uint32_t b = (key & 0x80000000u) ? key ^ 0x80000000u : ~key;      // key 0 -> a NaN
    return __builtin_bit_cast(float, b);
}
__device__ __forceinline__ uint64_t candidate(float s, uint32_t index) {
    return (static_cast<uint64_t>(score_key(s)) << 32) | (0xFFFFFFFFu - index);
}

// `c` beats the last entry of the sorted list: it takes that slot and rises to its place
template <int K>
__device__ __forceinline__ void insert(uint64_t (&lst)[K], uint64_t c) {
    lst[K - 1] = c;
#pragma unroll
    for (int i = K - 1; i > 0; --i) {
        const uint64_t a = lst[i - 1], b = lst[i];
        lst[i - 1] = a > b ? a : b;
        lst[i] = a > b ? b : a;
    }
}

__device__ __forceinline__ uint64_t shfl_xor64(uint64_t v, int mask) {
    const uint32_t lo = __shfl_xor(static_cast<uint32_t>(v), mask, 64);
    const uint32_t hi = __shfl_xor(static_cast<uint32_t>(v >> 32), mask, 64);
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// lanes with `sender` hand their list to lane ^ mask, a `receiver`, which afterwards holds the K best of both (lanes that are
// neither only take part in the shuffle)
template <int K>
__device__ __forceinline__ void fold(uint64_t (&lst)[K], int mask, bool sender, bool receiver) {
    for (int it = 0; it < K; ++it) {
        const uint64_t c = shfl_xor64(lst[0], mask);
        bool placed = false;
        if (sender) {
#pragma unroll
            for (int i = 0; i + 1 < K; ++i) lst[i] = lst[i + 1];
            lst[K - 1] = 0;
        } else if (receiver && c > lst[K - 1]) {
            insert<K>(lst, c);
            placed = true;
        }
        if (!__any(placed)) break;           // the fronts only fall: nothing that follows can enter either
    }
}

}  // namespace dif
