// Run-time value -> compile-time constant, written once for every launcher of the three libraries.  No HIP include: plain
// host C++17 compiles this header (tests/cpp/select_test.cpp does).
//
//     return dif::with_flags([&](auto VEC, auto SPLIT) -> int {
//         if constexpr (SPLIT && !VEC) return no_variant();           // never built: say why in a comment
//         else return dif::launch("my_kernel", my_kernel<VEC, SPLIT>, grid, block, 0, st, args...);
//     }, vec, split);
//
// The constants arrive as std::bool_constant / std::integral_constant values: usable as template arguments and inside
// `if constexpr`, which is how a launcher leaves out the combinations that are not built.
#pragma once
#include <type_traits>

namespace dif {

// f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
template <typename F>
auto with_flags(F&& f) { return f(); }
template <typename F, typename... B>
auto with_flags(F&& f, bool b0, B... rest) {
    return b0 ? with_flags([&](auto... c) { return f(std::true_type{}, c...); }, rest...)
              : with_flags([&](auto... c) { return f(std::false_type{}, c...); }, rest...);
}

// f(std::integral_constant<int, N>{}) for the listed N == v.  A value outside the list never picks a neighbour: nothing of f
// runs and miss(v) is returned (the caller's fail path).  A ladder that ended in `else` clamps v before the call.
template <int... Ns, typename F, typename Miss>
auto with_int(int v, F&& f, Miss&& miss) -> decltype(miss(v)) {
    decltype(miss(v)) r{};
    const bool hit = ((v == Ns ? (r = f(std::integral_constant<int, Ns>{}), true) : false) || ...);
    return hit ? r : miss(v);
}

}  // namespace dif
