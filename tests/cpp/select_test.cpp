// Stand-alone check of csrc/dif_select.h (host C++17, no HIP): built with -fsanitize=address,undefined and run by
// tests/test_select_cpp.py.  Exit status 0 and "select_test OK" on success; the first failed check is printed otherwise.
#include <cstdio>
#include <type_traits>
#include <vector>
#include "../../difformer_amd/csrc/dif_select.h"

namespace {

int g_failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failures;                                                  \
        }                                                                  \
    } while (0)

constexpr int kMiss = -2;          // what the launchers return for an unlisted value (DIF_E_SHAPE)

// leaf index from the compile-time constants: bit i = flag i
template <bool... B>
constexpr int leaf_of() {
    int idx = 0, bit = 0;
    ((idx |= (B ? 1 : 0) << bit++), ...);
    return idx;
}

// with_flags over all 2^k inputs: every leaf exactly once, the leaf reached is the one the run-time flags name, the constants
// are usable in `if constexpr`, and the return value comes back
template <int K>
void flags_case() {
    std::vector<int> hits(1 << K, 0);
    for (int in = 0; in < (1 << K); ++in) {
        auto visit = [&](auto... c) -> int {
            static_assert(sizeof...(c) == K, "one constant per flag");
            static_assert((std::is_same<decltype(c), std::bool_constant<decltype(c)::value>>::value && ...), "bool_constant values");
            constexpr int leaf = leaf_of<decltype(c)::value...>();
            ++hits[leaf];
            return 100 + leaf;
        };
        int got = -1;
        if constexpr (K == 1) got = dif::with_flags(visit, (in & 1) != 0);
        if constexpr (K == 2) got = dif::with_flags(visit, (in & 1) != 0, (in & 2) != 0);
        if constexpr (K == 3) got = dif::with_flags(visit, (in & 1) != 0, (in & 2) != 0, (in & 4) != 0);
        if constexpr (K == 4) got = dif::with_flags(visit, (in & 1) != 0, (in & 2) != 0, (in & 4) != 0, (in & 8) != 0);
        CHECK(got == 100 + in);
    }
    for (int leaf = 0; leaf < (1 << K); ++leaf) CHECK(hits[leaf] == 1);
}

// pruning as the launchers do it: excluded combinations are never instantiated (the static_assert below would fire) and
// return the error
struct OnlyBuilt {
    template <bool A, bool B>
    static int run() {
        static_assert(!(A && !B), "this combination must not be instantiated");
        return A * 2 + B;
    }
};
void pruning_case() {
    int calls = 0;
    for (int in = 0; in < 4; ++in) {
        const int got = dif::with_flags([&](auto A, auto B) -> int {
            if constexpr (A && !B) return kMiss;
            else { ++calls; return OnlyBuilt::run<A, B>(); }
        }, (in & 2) != 0, (in & 1) != 0);
        CHECK(got == (in == 2 ? kMiss : in));
    }
    CHECK(calls == 3);
}

template <int... Ns>
void ints_case(const std::vector<int>& listed) {
    for (int v = -3; v <= 70; ++v) {
        int calls = 0, seen = -1000, misses = 0, missed = -1000;
        const int got = dif::with_int<Ns...>(v, [&](auto N) -> int {
            static_assert(std::is_same<decltype(N), std::integral_constant<int, decltype(N)::value>>::value, "integral_constant");
            ++calls;
            seen = N;
            return 1000 + decltype(N)::value;
        }, [&](int u) { ++misses; missed = u; return kMiss; });
        bool is_listed = false;
        for (int n : listed) is_listed = is_listed || n == v;
        if (is_listed) {
            CHECK(calls == 1 && seen == v && got == 1000 + v && misses == 0);          // the listed value, and only that one
        } else {
            CHECK(calls == 0 && got == kMiss && misses == 1 && missed == v);           // nothing called, never a neighbour
        }
    }
}

}  // namespace

int main() {
    flags_case<1>();
    flags_case<2>();
    flags_case<3>();
    flags_case<4>();
    pruning_case();
    ints_case<1, 2, 4, 8>({1, 2, 4, 8});
    ints_case<64>({64});
    ints_case<3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16>({3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16});
    ints_case<0, 1>({0, 1});
    // nested, as a launcher with an int and flags: 3 x 4 leaves, 9 built
    int built = 0, refused = 0;
    for (int v : {1, 2, 4})
        for (int in = 0; in < 4; ++in) {
            const int got = dif::with_int<1, 2, 4>(v, [&](auto N) {
                return dif::with_flags([&](auto A, auto B) -> int {
                    if constexpr (N == 4 && A) return kMiss;
                    else if constexpr (N == 1 && A && B) return kMiss;
                    else return N * 10 + A * 2 + B;
                }, (in & 2) != 0, (in & 1) != 0);
            }, [](int) { return kMiss; });
            const bool pruned = (v == 4 && (in & 2)) || (v == 1 && in == 3);
            CHECK(got == (pruned ? kMiss : v * 10 + in));
            ++(pruned ? refused : built);
        }
    CHECK(built == 9 && refused == 3);
    if (g_failures) {
        std::printf("select_test: %d check(s) failed\n", g_failures);
        return 1;
    }
    std::printf("select_test OK\n");
    return 0;
}
