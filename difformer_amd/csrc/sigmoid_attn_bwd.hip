// f3: backward of full_attention_conv(..., kernel='sigmoid')  -- node classification/difformer.py:45-56 under
// loss.backward() (main.py:130).  With S = Q K^T, P = sigma(S), den_n = sum_l P_nl, out_n = sum_l P_nl v_l / den_n and
// g = dL/dout:
//     delta_n = g_n . out_n                          c_n = 1 / den_n
//     dV_l    = sum_n (c_n P_nl) g_n
//     dS_nl   = c_n (g_n . v_l - delta_n) P_nl (1 - P_nl)
//     dQ_n    = sum_l dS_nl k_l                      dK_l = sum_n dS_nl q_n
// As in the forward kernel the [N,L,H] tensors never leave registers: sigma is recomputed tile by tile.  ONE sweep
// kernel serves both halves; it keeps 32 rows of the STATIONARY side in registers (as MFMA B operands) and streams the
// other side past them, 8 waves splitting the stream:
//     MODE 0 (dQ):      stationary = queries (q, g),  swept = keys    (k, v);  accumulates dQ^T += K^T dS^T
//     MODE 1 (dK, dV):  stationary = keys    (k, v),  swept = queries (q, g);  accumulates dV^T += G^T (cP), dK^T += Q^T dS
// Both score tiles are computed TRANSPOSED, T^T[swept row][stationary row] (v_mfma_f32_16x16x4_f32: swept fragment =
// A operand, stationary fragment = B operand), so that a lane's four results are four SWEPT rows -- exactly the k-index
// of the second contraction, whose B operand they become without a shuffle (the forward kernel's trick).
// Covers M, D <= 64 (one fragment set per side); wider heads re-derive the gradient with tensor ops on the host side.
// FLOPs: 14 N L H D against the forward's 4 N L H D.
#include <stdlib.h>
#include "split_bf16.h"
#include "sigmoid_wide.h"

namespace {

using dif::f32x4;
using dif::bf16x8, dif::ld4, dif::ld4_raw, dif::mask4, dif::mfma3, dif::sigmoid_hw, dif::split8;

constexpr int kWaves = 8;
constexpr int kXT = 2;                  // 16-row tiles of the stationary side per workgroup
constexpr int kXGroup = 16 * kXT;
constexpr int kCols = 64;               // M, D <= 64

// cinv[n,h] = 1 / den[n,h], delta[n,h] = g[n,h,:] . out[n,h,:]
__global__ __launch_bounds__(256) void sigmoid_bwd_prep_kernel(const float* __restrict__ g, int64_t ldg,
                                                               const float* __restrict__ out, int64_t ldo,
                                                               const float* __restrict__ den, int64_t n_rows, int H, int D,
                                                               float* __restrict__ cinv, float* __restrict__ delta) {
    const int64_t total = n_rows * H;
    const int sub = threadIdx.x & 15;           // 16 lanes per (row, head)
    for (int64_t e = (static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x) >> 4; e < ((total + 15) & ~int64_t(15));
         e += static_cast<int64_t>(gridDim.x) * 16) {
        const bool ok = e < total;
        const int64_t row = ok ? e / H : 0;
        const int h = ok ? static_cast<int>(e % H) : 0;
        float s = 0.f;
        if (ok)
            for (int d = sub; d < D; d += 16) s += g[row * ldg + h * D + d] * out[row * ldo + h * D + d];
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        if (ok && sub == 0) {
            delta[e] = s;
            cinv[e] = 1.0f / den[e];
        }
    }
}

// grid: (ceil(X / 32), H, S splits of the swept side); block 512.
// x*: stationary operands, y*: swept operands; 1 = the score pair (q / k), 2 = the value pair (g / v).
// S == 1: results written to o1 (and o2); S > 1: partials to part1 [S][X][H*M] (part2 [S][X][H*D]), summed by
// sum_parts_kernel.
// SEG (f4, physical particle/difformer-v2.py:113-135 under loss.backward()): blockIdx.z is a POSITION p inside the graphs of
// a batch, stationary and swept side are both the seg_cnt[p] nodes at position p of their graph (local row r = node
// seg_first[r] + p, graphs ranked by size as in the forward kernel); `cinv` already holds the FULL denominators (padded
// graphs add constants only: no gradient flows into them), so the arithmetic is the unbatched kernel's.  No splits.
// SPLIT (round 5): all five products on split-bfloat16 operands -- v = hi + lo, three v_mfma_f32_16x16x32_bf16 per 32-deep step
// (lo.hi + hi.lo + hi.hi) instead of eight v_mfma_f32_16x16x4_f32 at twice the cycles.  The wave sweeps TWO 16-row tiles per
// step so that the second contractions run 32 swept rows deep; their B operand is still the lane's own registers: k-slot
// 8 lg + e <-> swept row 4 lg + e of the first tile (e < 4) / 4 lg + e - 4 of the second -- the forward kernel's map.
// Gradients move by a few 1e-6 relative; DIFFORMER_EXACT_FP32=1 / dif_set_exact_fp32 keeps the fp32 chain.

template <int MODE, bool VEC, bool SEG = false, bool SPLIT = false>
__global__ __launch_bounds__(512) void sigmoid_bwd_kernel(const float* __restrict__ x1, int64_t ldx1,
                                                          const float* __restrict__ x2, int64_t ldx2,
                                                          const float* __restrict__ y1, int64_t ldy1,
                                                          const float* __restrict__ y2, int64_t ldy2,
                                                          const float* __restrict__ cinv, const float* __restrict__ delta,
                                                          int64_t X, int64_t Y, int H, int M, int D,
                                                          float* __restrict__ o1, int64_t ldo1, float* __restrict__ o2,
                                                          int64_t ldo2, float* __restrict__ part1,
                                                          float* __restrict__ part2,
                                                          const int32_t* __restrict__ seg_first = nullptr,
                                                          const int32_t* __restrict__ seg_cnt = nullptr) {
    __shared__ __attribute__((aligned(16))) float sm_o[kWaves][kXGroup * kCols];   // 64 KiB
    const int h = blockIdx.y;
    const int S = SEG ? 1 : gridDim.z, split = SEG ? 0 : blockIdx.z;
    const int pos = SEG ? blockIdx.z : 0;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int l15 = lane & 15;
    const int lg = lane >> 4;
    const int64_t x0 = static_cast<int64_t>(blockIdx.x) * kXGroup;
    if (SEG) {
        X = Y = seg_cnt[pos];
        if (x0 >= X) return;                                   // uniform: before any barrier
    }
    auto mrow = [&](int64_t r) -> int64_t { return SEG ? static_cast<int64_t>(seg_first[r]) + pos : r; };   // local -> memory row

    // stationary fragments (B operands): row = x0 + 16 t + l15, columns 16 c + 4 lg .. + 3
    f32x4 xs1[kXT][4], xs2[kXT][4];
    float cx[kXT], dx[kXT];
#pragma unroll
    for (int t = 0; t < kXT; ++t) {
        const int64_t r = x0 + 16 * t + l15;
        const bool ok = r < X;
        const int64_t rc = mrow(ok ? r : X - 1);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            xs1[t][c] = ld4<VEC>(x1, ldx1, rc, ok, h * M, 16 * c + 4 * lg, M);
            xs2[t][c] = ld4<VEC>(x2, ldx2, rc, ok, h * D, 16 * c + 4 * lg, D);
        }
        if (MODE == 0) {                         // per-query scalars ride with the stationary row
            cx[t] = ok ? cinv[rc * H + h] : 0.f;
            dx[t] = ok ? delta[rc * H + h] : 0.f;
        }
    }
    f32x4 acc1[kXT][4];                          // MODE 0: dQ^T tiles; MODE 1: dK^T tiles   (16-column tiles of M)
    f32x4 acc2[kXT][4];                          // MODE 1: dV^T tiles                        (16-column tiles of D)
#pragma unroll
    for (int t = 0; t < kXT; ++t)
#pragma unroll
        for (int i = 0; i < 4; ++i) acc1[t][i] = acc2[t][i] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int64_t n_tiles = (Y + 15) / 16;
    const int64_t per = (n_tiles + S - 1) / S;
    const int64_t t0 = split * per;
    const int64_t t1 = (t0 + per < n_tiles) ? t0 + per : n_tiles;
    if constexpr (SPLIT) {
        // The stationary fragments are the same for the 8 waves: split once, parked in LDS (16 KiB at the head of the fold
        // buffer, free until the sweep ends) as ready B operands [x1 hi, x1 lo, x2 hi, x2 lo][t][kb][lane] -- 64 VGPRs the sweep
        // needs for its own operands (the fp32 chain keeps them in registers: it has no hi/lo pairs to hold).
        bf16x8* sm_x = reinterpret_cast<bf16x8*>(&sm_o[0][0]);
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < kXT; ++t)
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    bf16x8 hi, lo;
                    split8(xs1[t][2 * kb], xs1[t][2 * kb + 1], hi, lo);
                    sm_x[((0 * kXT + t) * 2 + kb) * 64 + lane] = hi;
                    sm_x[((1 * kXT + t) * 2 + kb) * 64 + lane] = lo;
                    split8(xs2[t][2 * kb], xs2[t][2 * kb + 1], hi, lo);
                    sm_x[((2 * kXT + t) * 2 + kb) * 64 + lane] = hi;
                    sm_x[((3 * kXT + t) * 2 + kb) * 64 + lane] = lo;
                }
        }
        __syncthreads();
        const int64_t y_limit = (t1 * 16 < Y) ? t1 * 16 : Y;              // the swept rows of THIS workgroup's range end here
        for (int64_t yt = t0 + 2 * wave; yt < t1; yt += 2 * kWaves) {
            const int64_t ybase = yt * 16;
            f32x4 s[2][kXT], r[2][kXT];
#pragma unroll
            for (int tile = 0; tile < 2; ++tile) {
                asm volatile("" ::: "memory");       // the LDS operands are re-read per tile, not hoisted into registers
                const int64_t yr = ybase + 16 * tile + l15;
                const bool yok = yr < y_limit;
                const int64_t yrc = mrow(yok ? yr : Y - 1);
                f32x4 ya1[4], ya2[4];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    ya1[c] = ld4<VEC>(y1, ldy1, yrc, yok, h * M, 16 * c + 4 * lg, M);
                    ya2[c] = ld4<VEC>(y2, ldy2, yrc, yok, h * D, 16 * c + 4 * lg, D);
                }
#pragma unroll
                for (int t = 0; t < kXT; ++t) s[tile][t] = r[tile][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < 2; ++kb) {
                    bf16x8 ah, al;
                    split8(ya1[2 * kb], ya1[2 * kb + 1], ah, al);
#pragma unroll
                    for (int t = 0; t < kXT; ++t)                                              // q . k
                        s[tile][t] = mfma3(ah, al, sm_x[((0 * kXT + t) * 2 + kb) * 64 + lane], sm_x[((1 * kXT + t) * 2 + kb) * 64 + lane],
                                           s[tile][t]);
                    split8(ya2[2 * kb], ya2[2 * kb + 1], ah, al);
#pragma unroll
                    for (int t = 0; t < kXT; ++t)                                              // g . v
                        r[tile][t] = mfma3(ah, al, sm_x[((2 * kXT + t) * 2 + kb) * 64 + lane], sm_x[((3 * kXT + t) * 2 + kb) * 64 + lane],
                                           r[tile][t]);
                }
            }
            // per-swept-row scalars (MODE 1: the queries are the swept side)
            float cy[2][4], dy[2][4];
            int64_t zrow[2][4];
            bool zok[2][4];
#pragma unroll
            for (int tile = 0; tile < 2; ++tile)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const int64_t yy = ybase + 16 * tile + 4 * lg + reg;
                    zok[tile][reg] = yy < y_limit;
                    zrow[tile][reg] = mrow(zok[tile][reg] ? yy : Y - 1);
                    if (MODE == 1) {
                        cy[tile][reg] = cinv[zrow[tile][reg] * H + h] * (zok[tile][reg] ? 1.0f : 0.0f);
                        dy[tile][reg] = delta[zrow[tile][reg] * H + h] * (zok[tile][reg] ? 1.0f : 0.0f);
                    }
                }
            // weights: lane holds T^T[swept row 16 tile + 4 lg + reg][stationary row l15]
            bf16x8 dsh[kXT], dsl[kXT], pch[kXT], pcl[kXT];
#pragma unroll
            for (int t = 0; t < kXT; ++t) {
                f32x4 ds[2], pc[2];
#pragma unroll
                for (int tile = 0; tile < 2; ++tile)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        const float p = zok[tile][reg] ? sigmoid_hw(s[tile][t][reg]) : 0.f;
                        const float c = (MODE == 0) ? cx[t] : cy[tile][reg];
                        const float dl = (MODE == 0) ? dx[t] : dy[tile][reg];
                        pc[tile][reg] = p * c;
                        ds[tile][reg] = pc[tile][reg] * (r[tile][t][reg] - dl) * (1.0f - p);
                    }
                split8(ds[0], ds[1], dsh[t], dsl[t]);
                if (MODE == 1) split8(pc[0], pc[1], pch[t], pcl[t]);
            }
            asm volatile("" ::: "memory");           // the transposed reads below start after the score tiles are consumed (register budget)
            // second contraction, one 16-column tile at a time: A[i = l15 <-> column][k-slot 8 lg + 4 tile + reg] = swept row
            // ybase + 16 tile + 4 lg + reg (the rows the ld4 above just brought through the L1)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                if (MODE == 1 && ct == 2) asm volatile("" ::: "memory");      // dK/dV: two column tiles of transposed reads in flight
                const int col = 16 * ct + l15;
                f32x4 z1[2], z2[2];
#pragma unroll
                for (int tile = 0; tile < 2; ++tile)
#pragma unroll
                    for (int reg = 0; reg < 4; ++reg) {
                        // (masked by multiplication: see the fp32 sweep below)
                        const float a = y1[zrow[tile][reg] * ldy1 + h * M + (col < M ? col : 0)];
                        z1[tile][reg] = a * ((zok[tile][reg] && col < M) ? 1.0f : 0.0f);
                        if (MODE == 1) {
                            const float b = y2[zrow[tile][reg] * ldy2 + h * D + (col < D ? col : 0)];
                            z2[tile][reg] = b * ((zok[tile][reg] && col < D) ? 1.0f : 0.0f);
                        }
                    }
                bf16x8 zh, zl;
                split8(z1[0], z1[1], zh, zl);
#pragma unroll
                for (int t = 0; t < kXT; ++t) acc1[t][ct] = mfma3(zh, zl, dsh[t], dsl[t], acc1[t][ct]);
                if (MODE == 1) {
                    split8(z2[0], z2[1], zh, zl);
#pragma unroll
                    for (int t = 0; t < kXT; ++t) acc2[t][ct] = mfma3(zh, zl, pch[t], pcl[t], acc2[t][ct]);
                }
            }
        }
    } else {
        // fp32 chain, software-pipelined (round 5).  Until then a step was loads -> wait -> products, the 16-32 transposed scalar
        // reads each in its own exec-masked block (the compiler sinks a load under the select that masks it) or, pinned, each
        // waiting for itself: ~14,500 cycles per step per SIMD against 4,100 of MFMA.  Now every operand of the NEXT step is in
        // flight under this step's products: raw loads from clamped (valid) addresses, issued unconditionally (the last step
        // re-reads its own rows), masked only when used.  The registers for that come from the stationary fragments, which are
        // the same for the 8 waves: parked in LDS (16 KiB at the head of the fold buffer, free until the sweep ends) as B operands
        // [x1 | x2][t][c][lane], re-read per step behind a compiler barrier.
        f32x4* sm_x = reinterpret_cast<f32x4*>(&sm_o[0][0]);
        if (wave == 0) {
#pragma unroll
            for (int t = 0; t < kXT; ++t)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    sm_x[((0 * kXT + t) * 4 + c) * 64 + lane] = xs1[t][c];
                    sm_x[((1 * kXT + t) * 4 + c) * 64 + lane] = xs2[t][c];
                }
        }
        __syncthreads();
        // Two half-step prefetches into the registers their predecessors just left (no second register set): the row fragments
        // of the next step are issued after this step's score products, the transposed scalars after its second contraction.
        f32x4 ya1n[4], ya2n[4];
        float z1n[4][4], z2n[4][4], cyn[4], dyn[4];
        auto prefetch_rows = [&](int64_t ybase) {
            const int64_t yr = ybase + l15;
            const int64_t yrc = mrow(yr < Y ? yr : Y - 1);
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                ya1n[c] = ld4_raw<VEC>(y1, ldy1, yrc, h * M, 16 * c + 4 * lg, M);
                ya2n[c] = ld4_raw<VEC>(y2, ldy2, yrc, h * D, 16 * c + 4 * lg, D);
            }
        };
        auto prefetch_cols = [&](int64_t ybase) {
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const int64_t yy = ybase + 4 * lg + reg;
                const int64_t yc = mrow(yy < Y ? yy : Y - 1);
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int col = 16 * ct + l15;
                    z1n[ct][reg] = y1[yc * ldy1 + h * M + (col < M ? col : 0)];
                    if (MODE == 1) z2n[ct][reg] = y2[yc * ldy2 + h * D + (col < D ? col : 0)];
                }
                if (MODE == 1) {
                    cyn[reg] = cinv[yc * H + h];
                    dyn[reg] = delta[yc * H + h];
                }
            }
        };
        if (t0 + wave < t1) {
            prefetch_rows((t0 + wave) * 16);
            prefetch_cols((t0 + wave) * 16);
        }
        for (int64_t yt = t0 + wave; yt < t1; yt += kWaves) {
            const int64_t ybase = yt * 16;
            const int64_t ynext = ((yt + kWaves < t1) ? yt + kWaves : yt) * 16;
            asm volatile("" ::: "memory");           // the LDS operands are re-read per step, not hoisted into registers
            f32x4 s[kXT], r[kXT];
#pragma unroll
            for (int t = 0; t < kXT; ++t) s[t] = r[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f32x4 ya1 = mask4<VEC>(ya1n[c], ybase + l15 < Y, 16 * c + 4 * lg, M);
                const f32x4 ya2 = mask4<VEC>(ya2n[c], ybase + l15 < Y, 16 * c + 4 * lg, D);
                f32x4 b1[kXT], b2[kXT];
#pragma unroll
                for (int t = 0; t < kXT; ++t) {
                    b1[t] = sm_x[((0 * kXT + t) * 4 + c) * 64 + lane];
                    b2[t] = sm_x[((1 * kXT + t) * 4 + c) * 64 + lane];
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int t = 0; t < kXT; ++t) {
                        s[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ya1[u], b1[t][u], s[t], 0, 0, 0);      // q . k
                        r[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(ya2[u], b2[t][u], r[t], 0, 0, 0);      // g . v
                    }
            }
            __builtin_amdgcn_sched_barrier(0);
            prefetch_rows(ynext);                    // into the registers the score products just left
            __builtin_amdgcn_sched_barrier(0);
            // ---- weights: lane holds T^T[swept row 4 lg + reg][stationary row l15] ----
            f32x4 ds[kXT], pc[kXT];
#pragma unroll
            for (int t = 0; t < kXT; ++t)
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) {
                    const bool ok = ybase + 4 * lg + reg < Y;
                    const float p = ok ? sigmoid_hw(s[t][reg]) : 0.f;
                    const float c = (MODE == 0) ? cx[t] : (ok ? cyn[reg] : 0.f);      // per-query scalars ride with the swept row
                    const float dl = (MODE == 0) ? dx[t] : (ok ? dyn[reg] : 0.f);
                    pc[t][reg] = p * c;
                    ds[t][reg] = pc[t][reg] * (r[t][reg] - dl) * (1.0f - p);
                }
            // ---- second contraction: A[i = l15 <-> column][k = swept row 4 lg + reg], masked out of the prefetch registers ----
#pragma unroll
            for (int reg = 0; reg < 4; ++reg) {
                const bool ok = ybase + 4 * lg + reg < Y;
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    const int col = 16 * ct + l15;
                    const float zf1 = (ok && col < M) ? z1n[ct][reg] : 0.f;       // dQ^T += K^T dS (MODE 0: y1 = k) | dK^T += Q^T dS (MODE 1: y1 = q)
                    const float zf2 = (MODE == 1 && ok && col < D) ? z2n[ct][reg] : 0.f;      // dV^T += G^T (c P)   (y2 = g)
#pragma unroll
                    for (int t = 0; t < kXT; ++t) {
                        acc1[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(zf1, ds[t][reg], acc1[t][ct], 0, 0, 0);
                        if (MODE == 1) acc2[t][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(zf2, pc[t][reg], acc2[t][ct], 0, 0, 0);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            prefetch_cols(ynext);                    // into the registers the second contraction just left
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // fold the 8 waves through LDS; lane holds O^T[col = 16 ct + 4 lg + reg][row = 16 t + l15] -> stored as [row][col]
    auto fold_store = [&](f32x4 (&acc)[kXT][4], int width, float* __restrict__ dst, int64_t ldd, float* __restrict__ part) {
#pragma unroll
        for (int t = 0; t < kXT; ++t)
#pragma unroll
            for (int ct = 0; ct < 4; ++ct)
                *reinterpret_cast<f32x4*>(&sm_o[wave][(16 * t + l15) * kCols + 16 * ct + 4 * lg]) = acc[t][ct];
        __syncthreads();
        for (int e = threadIdx.x; e < kXGroup * kCols; e += 512) {
            const int ri = e / kCols, col = e % kCols;
            float o = 0.f;
#pragma unroll
            for (int w = 0; w < kWaves; ++w) o += sm_o[w][e];
            const int64_t row = x0 + ri;
            if (row < X && col < width) {
                if (S == 1) dst[mrow(row) * ldd + h * width + col] = o;
                else part[(static_cast<int64_t>(split) * X + row) * (static_cast<int64_t>(H) * width) + h * width + col] = o;
            }
        }
        __syncthreads();
    };
    __syncthreads();                               // every wave is done with the operands parked in the fold buffer
    fold_store(acc1, M, o1, ldo1, part1);
    if (MODE == 1) fold_store(acc2, D, o2, ldo2, part2);
}

// out[row, :width] = sum_s part[s][row][:width]   (fixed order: deterministic)
__global__ __launch_bounds__(256) void sum_parts_kernel(const float* __restrict__ part, int S, int64_t rows, int width,
                                                        float* __restrict__ out, int64_t ldo) {
    const int64_t total = rows * width;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; e < total;
         e += static_cast<int64_t>(gridDim.x) * 256) {
        float o = 0.f;
        for (int s = 0; s < S; ++s) o += part[static_cast<int64_t>(s) * total + e];
        out[(e / width) * ldo + e % width] = o;
    }
}

// splits of the swept side: fill the chip when the stationary side has few 32-row groups (Cora: 85)
int sweep_splits(int64_t X, int64_t Y, int H) {
    const int64_t groups = ((X + kXGroup - 1) / kXGroup) * H;
    const int64_t n_tiles = (Y + 15) / 16;
    int64_t smax = (n_tiles + kWaves - 1) / kWaves;
    if (smax > 16) smax = 16;
    int best = 1;
    double best_cost = -1.0;
    for (int64_t s = 1; s <= smax; ++s) {
        const int64_t rounds = (groups * s + dif::kCUs - 1) / dif::kCUs;            // one workgroup per CU (64 KiB of LDS, ~200 VGPRs)
        const double cost = static_cast<double>(rounds) * (static_cast<double>(n_tiles) / (kWaves * s) + 4.0);
        if (best_cost < 0 || cost < best_cost * 0.98) { best_cost = cost; best = static_cast<int>(s); }
    }
    return best;
}

size_t align16(size_t b) { return (b + 15) & ~size_t(15); }

}  // namespace

extern "C" size_t dif_sigmoid_bwd_workspace_bytes(int64_t N, int64_t L, int H, int M, int D) {
    if (N <= 0 || L <= 0 || H <= 0 || M <= 0 || D <= 0) return 0;
    if (dif::sigw_covers(M, D)) return dif::sigw_bwd_workspace_bytes(N, L, H, M, D);
    const size_t S0 = sweep_splits(N, L, H), S1 = sweep_splits(L, N, H);
    size_t b = 2 * align16(static_cast<size_t>(N) * H * sizeof(float));                        // cinv, delta
    if (S0 > 1) b += align16(S0 * N * H * M * sizeof(float));
    if (S1 > 1) b += align16(S1 * L * H * M * sizeof(float)) + align16(S1 * L * H * D * sizeof(float));
    return b;
}

extern "C" int dif_sigmoid_attn_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                        int64_t ldv, const float* out, int64_t ldo, const float* den, const float* g,
                                        int64_t ldg, int64_t N, int64_t L, int H, int M, int D, float* dq, int64_t lddq,
                                        float* dk, int64_t lddk, float* dv, int64_t lddv, void* workspace,
                                        size_t workspace_bytes, dif_stream_t stream) {
    DIF_REQUIRE(N > 0 && L > 0 && H > 0 && M > 0 && D > 0, DIF_E_BADARG, "dif_sigmoid_attn_bwd_f32: sizes must be positive");
    const bool wide = dif::sigw_covers(M, D);
    DIF_REQUIRE((M <= kCols && D <= kCols) || wide, DIF_E_SHAPE, "dif_sigmoid_attn_bwd_f32: covers M, D <= 512 (got %d, %d)", M, D);
    DIF_REQUIRE(!(wide && dif::exact_fp32()), DIF_E_SHAPE,
                "dif_sigmoid_attn_bwd_f32: heads wider than 64 columns run on split-bfloat16 planes; under dif_set_exact_fp32(1) the "
                "fp32 chain covers M, D <= 64 (got %d, %d)", M, D);
    DIF_REQUIRE(q && k && v && out && den && g && dq && dk && dv && workspace, DIF_E_BADARG,
                "dif_sigmoid_attn_bwd_f32: null pointer");
    DIF_REQUIRE(ldq >= H * M && ldk >= H * M && ldv >= H * D && ldo >= H * D && ldg >= H * D && lddq >= H * M &&
                    lddk >= H * M && lddv >= H * D, DIF_E_BADARG, "dif_sigmoid_attn_bwd_f32: leading dimension smaller than a row");
    if (wide)
        return dif::sigw_bwd(q, ldq, k, ldk, v, ldv, out, ldo, den, g, ldg, N, L, H, M, D, dq, lddq, dk, lddk, dv, lddv, workspace,
                             workspace_bytes, static_cast<hipStream_t>(stream));
    DIF_REQUIRE(H <= 65535, DIF_E_RANGE, "dif_sigmoid_attn_bwd_f32: too many heads");
    DIF_REQUIRE(workspace_bytes >= dif_sigmoid_bwd_workspace_bytes(N, L, H, M, D) && dif::aligned16(workspace), DIF_E_WORKSPACE,
                "dif_sigmoid_attn_bwd_f32: workspace too small or not 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int S0 = sweep_splits(N, L, H), S1 = sweep_splits(L, N, H);
    char* w = static_cast<char*>(workspace);
    float* cinv = reinterpret_cast<float*>(w);
    w += align16(static_cast<size_t>(N) * H * sizeof(float));
    float* delta = reinterpret_cast<float*>(w);
    w += align16(static_cast<size_t>(N) * H * sizeof(float));
    float* pq = nullptr, *pk = nullptr, *pv = nullptr;
    if (S0 > 1) { pq = reinterpret_cast<float*>(w); w += align16(static_cast<size_t>(S0) * N * H * M * sizeof(float)); }
    if (S1 > 1) {
        pk = reinterpret_cast<float*>(w); w += align16(static_cast<size_t>(S1) * L * H * M * sizeof(float));
        pv = reinterpret_cast<float*>(w);
    }
    int64_t pg = (N * H * 16 + 255) / 256;
    if (pg > 8 * dif::kCUs) pg = 8 * dif::kCUs;
    if (int rc = dif::launch("sigmoid_bwd_prep_kernel", sigmoid_bwd_prep_kernel, dif::grid_of(pg), dim3(256), 0, st, g, ldg, out,
                             ldo, den, N, H, D, cinv, delta)) return rc;
    auto al = [](const void* p, int64_t ld) { return ld % 4 == 0 && dif::aligned16(p); };
    const bool vec = (M % 4 == 0) && (D % 4 == 0) && al(q, ldq) && al(k, ldk) && al(v, ldv) && al(g, ldg);
    // split-bfloat16 operands on the bf16 matrix core (sigmoid_bwd_kernel<..., SPLIT>): OPT-IN (DIFFORMER_SIGMOID_BWD_SPLIT=1).
    // 1.24x faster, every gradient within 8e-6 of the fp32 chain relative to its own tensor -- but bias gradients that are sums
    // of cancelling rows (Wk.bias: sum_l dK_l, 3e-4 of the step's largest gradient) then sit at 1.0e-4 of THEMSELVES against the
    // reference's float64 gradient (the fp32 chain: 5e-6; tests/golden model/a_nobn_src), on the parity bar instead of inside it.
    static const bool split_opt_in = [] { const char* e = getenv("DIFFORMER_SIGMOID_BWD_SPLIT"); return e && e[0] == '1'; }();
    const bool split = split_opt_in && !dif::exact_fp32();
    // dQ: stationary queries (q, g), swept keys (k, v)
    {
        dim3 grid(static_cast<unsigned>((N + kXGroup - 1) / kXGroup), H, S0), block(512);
        if (int rc = dif::with_flags([&](auto VEC, auto SPLIT) {
                return dif::launch("sigmoid_bwd_kernel<dQ>", sigmoid_bwd_kernel<0, VEC, false, SPLIT>, grid, block, 0, st, q, ldq, g, ldg,
                                   k, ldk, v, ldv, cinv, delta, N, L, H, M, D, dq, lddq, nullptr, int64_t{0}, pq, nullptr, nullptr,
                                   nullptr);
            }, vec, split)) return rc;
    }
    // dK, dV: stationary keys (k, v), swept queries (q, g)
    {
        dim3 grid(static_cast<unsigned>((L + kXGroup - 1) / kXGroup), H, S1), block(512);
        if (int rc = dif::with_flags([&](auto VEC, auto SPLIT) {
                return dif::launch("sigmoid_bwd_kernel<dK,dV>", sigmoid_bwd_kernel<1, VEC, false, SPLIT>, grid, block, 0, st, k, ldk, v,
                                   ldv, q, ldq, g, ldg, cinv, delta, L, N, H, M, D, dk, lddk, dv, lddv, pk, pv, nullptr, nullptr);
            }, vec, split)) return rc;
    }
    auto combine = [&](const float* part, int S, int64_t rows, int width, float* o, int64_t ldo_) -> int {
        int64_t gsz = (rows * width + 255) / 256;
        if (gsz > 8 * dif::kCUs) gsz = 8 * dif::kCUs;
        return dif::launch("sum_parts_kernel", sum_parts_kernel, dif::grid_of(gsz), dim3(256), 0, st, part, S, rows, width, o,
                           ldo_);
    };
    if (S0 > 1) if (int rc = combine(pq, S0, N, H * M, dq, lddq)) return rc;
    if (S1 > 1) {
        if (int rc = combine(pk, S1, L, H * M, dk, lddk)) return rc;
        if (int rc = combine(pv, S1, L, H * D, dv, lddv)) return rc;
    }
    return 0;
}

// f4: backward of TransConv.full_attention(kernel='sigmoid') over a batch of graphs (physical particle/difformer-v2.py:113-135
// under loss.backward(), main.py:89-93).  `den` = the full denominators dif_batched_sigmoid_attn_fwd_f32 left.  Every node is
// query and key of exactly one position group, so every row of dq / dk / dv is written once.  workspace: 2 x N x H floats.
extern "C" size_t dif_batched_sigmoid_bwd_workspace_bytes(int64_t N, int H) {
    if (N <= 0 || H <= 0) return 0;
    return 2 * align16(static_cast<size_t>(N) * H * sizeof(float));
}

extern "C" int dif_batched_sigmoid_attn_bwd_f32(const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v,
                                                int64_t ldv, const float* out, int64_t ldo, const float* den, const float* g,
                                                int64_t ldg, const int32_t* ranked_first, const int32_t* pos_count,
                                                int n_graphs, int max_nodes, int64_t N, int H, int M, int D, float* dq,
                                                int64_t lddq, float* dk, int64_t lddk, float* dv, int64_t lddv,
                                                void* workspace, size_t workspace_bytes, dif_stream_t stream) {
    DIF_REQUIRE(N > 0 && n_graphs > 0 && max_nodes > 0 && H > 0 && M > 0 && D > 0, DIF_E_BADARG,
                "dif_batched_sigmoid_attn_bwd_f32: sizes must be positive");
    DIF_REQUIRE(M <= kCols && D <= kCols, DIF_E_SHAPE, "dif_batched_sigmoid_attn_bwd_f32: covers M, D <= 64 (got %d, %d)", M, D);
    DIF_REQUIRE(q && k && v && out && den && g && dq && dk && dv && workspace && ranked_first && pos_count, DIF_E_BADARG,
                "dif_batched_sigmoid_attn_bwd_f32: null pointer");
    DIF_REQUIRE(ldq >= H * M && ldk >= H * M && ldv >= H * D && ldo >= H * D && ldg >= H * D && lddq >= H * M &&
                    lddk >= H * M && lddv >= H * D, DIF_E_BADARG, "dif_batched_sigmoid_attn_bwd_f32: leading dimension smaller than a row");
    DIF_REQUIRE(H <= 65535 && max_nodes <= 65535, DIF_E_RANGE, "dif_batched_sigmoid_attn_bwd_f32: too many heads / positions");
    DIF_REQUIRE(workspace_bytes >= dif_batched_sigmoid_bwd_workspace_bytes(N, H) && dif::aligned16(workspace), DIF_E_WORKSPACE,
                "dif_batched_sigmoid_attn_bwd_f32: workspace too small or not 16-byte aligned");
    hipStream_t st = static_cast<hipStream_t>(stream);
    char* w = static_cast<char*>(workspace);
    float* cinv = reinterpret_cast<float*>(w);
    float* delta = reinterpret_cast<float*>(w + align16(static_cast<size_t>(N) * H * sizeof(float)));
    int64_t pg = (N * H * 16 + 255) / 256;
    if (pg > 8 * dif::kCUs) pg = 8 * dif::kCUs;
    if (int rc = dif::launch("sigmoid_bwd_prep_kernel", sigmoid_bwd_prep_kernel, dif::grid_of(pg), dim3(256), 0, st, g, ldg, out,
                             ldo, den, N, H, D, cinv, delta)) return rc;
    auto al = [](const void* p, int64_t ld) { return ld % 4 == 0 && dif::aligned16(p); };
    const bool vec = (M % 4 == 0) && (D % 4 == 0) && al(q, ldq) && al(k, ldk) && al(v, ldv) && al(g, ldg);
    dim3 grid(static_cast<unsigned>((n_graphs + kXGroup - 1) / kXGroup), H, static_cast<unsigned>(max_nodes)), block(512);
    return dif::with_flags([&](auto VEC) -> int {
        if (int rc = dif::launch("sigmoid_bwd_kernel<dQ, batched>", sigmoid_bwd_kernel<0, VEC, true>, grid, block, 0, st, q, ldq, g,
                                 ldg, k, ldk, v, ldv, cinv, delta, int64_t{0}, int64_t{0}, H, M, D, dq, lddq, nullptr, int64_t{0},
                                 nullptr, nullptr, ranked_first, pos_count)) return rc;
        return dif::launch("sigmoid_bwd_kernel<dK dV, batched>", sigmoid_bwd_kernel<1, VEC, true>, grid, block, 0, st, k, ldk, v, ldv,
                           q, ldq, g, ldg, cinv, delta, int64_t{0}, int64_t{0}, H, M, D, dk, lddk, dv, lddv, nullptr, nullptr,
                           ranked_first, pos_count);
    }, vec);
}
