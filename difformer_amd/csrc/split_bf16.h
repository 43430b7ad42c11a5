// Split-bfloat16: the arithmetic contract of every product that leaves the fp32 matrix core.  Defined here, once.
//
//   * Every operand is v = hi + lo: hi = bf16(v), lo = bf16(v - hi), both rounded to nearest even (the conversion the compiler
//     emits for __builtin_convertvector: v_cvt_pk_bf16_f32).
//   * A product a.b runs as three v_mfma_f32_16x16x32_bf16: al.bh + ah.bl + ah.bh.  The lo.lo term is dropped: it is 2^-16 of
//     a product, which is where the "~4e-6 of the float64 result" of every split-bf16 path comes from.
//   * Term order: the two small terms first, then hi.hi, on one fp32 accumulator.  mfma3 below is al.bh, ah.bl, ah.bh.
//
// DIFFORMER_EXACT_FP32 (dif::exact_fp32) and the 1e-4 parity budget are stated against this contract.  Every split-bf16 kernel
// follows it: simple_layer, simple_layer_wide, simple_layer_xwide, skinny_linear, sigmoid_attn, sigmoid_attn_bwd, sigmoid_wide,
// simple_attn (gram_slab_kernel, reduce_slab_kernel), simple_attn_bwd (rowgemm_wide_split_kernel) and rowgemm_split.h.  The split is
// always one of the functions below.  A site that ORDERS or ACCUMULATES the three terms differently from mfma3 writes its MFMAs
// out and says so itself: the layer kernels, the row-GEMMs and the slab kernels issue ah.bl ahead of al.bh, simple_layer_xwide
// interleaves two feature tiles, sigmoid_wide's Terms<> alternates two accumulators so that no MFMA waits for the one before it.
#pragma once
#include "dif_common.h"

namespace dif {

// the only __bf16 vector types of the library: half an MFMA operand (one f32x4 converted) and a whole one
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ void split_bf16(const f32x4& v, bf16x4& hi, bf16x4& lo) {
    hi = __builtin_convertvector(v, bf16x4);
    const f32x4 back = __builtin_convertvector(hi, f32x4);
    lo = __builtin_convertvector(v - back, bf16x4);
}
__device__ __forceinline__ bf16x8 cat8(const bf16x4& a, const bf16x4& b) {
    return bf16x8{a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
}

// two f32x4 (k-slots 0 .. 3 and 4 .. 7 of a lane) -> one operand pair; the result of split_planes<2>, kept as its own body because
// the kernels' instruction schedules follow the statement order.  Operands by value: a caller that fills them element by element
// would otherwise keep them in memory until after inlining, and compile differently.
__device__ __forceinline__ void split8(f32x4 a, f32x4 b, bf16x8& hi, bf16x8& lo) {
    const bf16x4 h0 = __builtin_convertvector(a, bf16x4), h1 = __builtin_convertvector(b, bf16x4);
    const bf16x4 l0 = __builtin_convertvector(a - __builtin_convertvector(h0, f32x4), bf16x4);
    const bf16x4 l1 = __builtin_convertvector(b - __builtin_convertvector(h1, f32x4), bf16x4);
    hi = cat8(h0, h1);
    lo = cat8(l0, l1);
}

// x -> NP bf16 planes (plane p + 1 holds what plane p left); NP = 2 gives split8's planes
template <int NP>
__device__ __forceinline__ void split_planes(f32x4 x0, f32x4 x1, bf16x8 (&pl)[NP]) {
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const bf16x4 h0 = __builtin_convertvector(x0, bf16x4), h1 = __builtin_convertvector(x1, bf16x4);
        pl[p] = cat8(h0, h1);
        if (p + 1 < NP) {
            x0 -= __builtin_convertvector(h0, f32x4);
            x1 -= __builtin_convertvector(h1, f32x4);
        }
    }
}

// acc += a.b on split operands, in the contract's order
__device__ __forceinline__ f32x4 mfma3(const bf16x8& ah, const bf16x8& al, const bf16x8& bh, const bf16x8& bl, f32x4 acc) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al, bh, acc, 0, 0, 0);          // small terms first
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bl, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah, bh, acc, 0, 0, 0);
}

}  // namespace dif
