// The per-node stages of the whole-model kernels for tiny graphs, ONE definition each, for the one-workgroup plan (tiny_model.hip)
// and the grid plans (tiny_sigmoid_grid.hip, tiny_simple_grid.hip; their backward's scratch layout is in tiny_grid.h).
//
// They are statement MACROS, not functions, on purpose.  These files are built with -ffp-contract=fast, and which multiply-add
// pairs of a kernel end up fused is decided by the SLP vectoriser over the whole inlined kernel: wrapping a stage into a
// __forceinline__ function -- same statements, same order -- already moves last-place bits of the hidden 5..8 kernels and of the grid
// backward kernels (profiles/tiny_stages_bitwise.txt).  A macro puts the same tokens where the kernels had them, so the device code
// of every kernel is the one it had with the stages written out (scripts/device_asm_diff.py --per-kernel says `identical`), and a fix
// to a stage is still made in one place.  scripts/exp_tiny_bitwise.py compares two builds of the library bit for bit.
//
// Conventions: a macro is one braced statement; it reads `a` (TinyArgs), `tp` (Tape<DP>), `n`, `d`, `DP`, and where said `drop`, `keep`
// from the scope it is used in; row arguments are float[DP] register rows; pointer arguments are the node's row (already offset by
// i * DP) unless called a base.  Keep the statements and their order: float32 sums in m / edge order, no re-association, no fmaf.
#pragma once
#include "tiny_common.h"

#define TINY_UNROLL _Pragma("unroll")

// ---- constants into LDS, zero-padded (every thread of the workgroup; the caller syncs).  T, t: blockDim.x, threadIdx.x -----------
// input layer: W0 [DP][kMaxIn], LayerNorm weight / bias; B0_STMT: `sB0[k_] = k_ < d ? a.b0[k_] : 0.f;` in the forward, empty otherwise
#define TINY_LOAD_INPUT_CONSTS(B0_STMT)                                                            \
    {                                                                                              \
        for (int k_ = t; k_ < DP * kMaxIn; k_ += T) {                                              \
            const int m_ = k_ / kMaxIn, f_ = k_ % kMaxIn;                                          \
            sW0[k_] = (m_ < d && f_ < a.f_in) ? a.w0[m_ * a.f_in + f_] : 0.f;                      \
        }                                                                                          \
        for (int k_ = t; k_ < DP; k_ += T) {                                                       \
            B0_STMT                                                                                \
            sLn0w[k_] = (k_ < d && a.use_bn) ? a.ln0w[k_] : 0.f;                                   \
            sLn0b[k_] = (k_ < d && a.use_bn) ? a.ln0b[k_] : 0.f;                                   \
        }                                                                                          \
    }
// output layer: Wo [kMaxOut][DP]; BO_STMT: `for (int k_ = t; k_ < kMaxOut; k_ += T) sBo[k_] = k_ < a.c ? a.bo[k_] : 0.f;` or empty
#define TINY_LOAD_OUTPUT_CONSTS(BO_STMT)                                                           \
    {                                                                                              \
        for (int k_ = t; k_ < kMaxOut * DP; k_ += T) {                                             \
            const int c_ = k_ / DP, m_ = k_ % DP;                                                  \
            sWo[k_] = (c_ < a.c && m_ < d) ? a.wo[c_ * d + m_] : 0.f;                              \
        }                                                                                          \
        BO_STMT                                                                                    \
    }

// ======================================================================================================================
// forward
// ======================================================================================================================
// input layer of node i: Linear -> Z[0] -> LayerNorm -> ReLU -> dropout -> H[0] (:188-192); h = the node's H[0] row.  Reads `drop`.
#define TINY_INPUT_FORWARD(i, h)                                                                   \
    {                                                                                              \
        TINY_UNROLL                                                                                \
        for (int m = 0; m < DP; ++m) h[m] = sB0[m];                                                \
        const float* xr = a.x + i * a.ldx;                                                         \
        for (int f = 0; f < a.f_in; ++f) {                                                         \
            const float xv = xr[f];                                                                \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) h[m] += sW0[m * kMaxIn + f] * xv;                         \
        }                                                                                          \
        store_row<DP>(tp.Z + static_cast<size_t>(i) * DP, h);                                      \
        if (a.use_bn) {                                                                            \
            float mean, rstd;                                                                      \
            ln_stats<DP>(h, d, a.eps, mean, rstd);                                                 \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) h[m] = (m < d) ? (h[m] - mean) * rstd * sLn0w[m] + sLn0b[m] : 0.f; \
        }                                                                                          \
        TINY_UNROLL                                                                                \
        for (int m = 0; m < DP; ++m) h[m] = fmaxf(h[m], 0.f);                                      \
        if (drop) dropout_row<DP>(h, a.rnd, static_cast<int64_t>(i) * d, d, a.p_drop);             \
        store_row<DP>(tp.H + static_cast<size_t>(i) * DP, h);                                      \
    }

// Wq / Wk / Wv (LayerW W) of a node's layer input h (:115-120)
#define TINY_PROJECT(W, USE_WV, h, q, k, v)                                                        \
    {                                                                                              \
        matvec<DP>(W.wq, W.bq, h, q);                                                              \
        matvec<DP>(W.wk, W.bk, h, k);                                                              \
        if (USE_WV) matvec<DP>(W.wv, W.bv, h, v);                                                  \
        else {                                                                                     \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) v[m] = h[m];                                              \
        }                                                                                          \
    }

// `simple` (:20-38): a node's attention row att from its q in closed form, from the layer's sums over nodes in sSum:
// K^T V [DP * DP] | sum k | sum v | |Q|^2 | |K|^2
#define TINY_SIMPLE_ATTENTION_ROW(q, att)                                                          \
    {                                                                                              \
        const float q2 = sSum[DP * DP + 2 * DP], k2 = sSum[DP * DP + 2 * DP + 1];                  \
        const float s = 1.0f / (sqrtf(q2) * sqrtf(k2));                      /* :20-21 global Frobenius norms */ \
        float den = 0.f;                                                                           \
        TINY_UNROLL                                                                                \
        for (int m = 0; m < DP; ++m) den += q[m] * sSum[DP * DP + m];                              \
        den = s * den + static_cast<float>(n);                               /* :31-38  (+N from qs.shape[0]) */ \
        TINY_UNROLL                                                                                \
        for (int dd = 0; dd < DP; ++dd) {                                                          \
            float num = 0.f;                                                                       \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) num += q[m] * sSum[m * DP + dd];                          \
            att[dd] = (s * num + sSum[DP * DP + DP + dd]) / den;             /* :25-29 */          \
        }                                                                                          \
    }

// acc += sum over the entries e of CSR row i, in edge order, of val[e] * SRC[nbr[e]] (SRC: base of [n][DP] rows): gcn_conv's row
// (:75-78) with SRC = V in the forward; in the backward `a` holds the transposed CSR and SRC = SG gives the aggregation's adjoint
#define TINY_GATHER_ROWS(SRC, i, acc)                                                              \
    {                                                                                              \
        const int e1 = a.rowptr[i + 1];                                                            \
        for (int e = a.rowptr[i]; e < e1; ++e) {                                                   \
            const float wgt = a.val[e];                                                            \
            float vr[DP];                                                                          \
            load_row<DP>(SRC + static_cast<size_t>(a.nbr[e]) * DP, vr);                            \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) acc[m] += wgt * vr[m];                                    \
        }                                                                                          \
    }

// layer l's tail of node i from its attention row: ATT[l], a_s att + g_s (gcn_conv row of V, V: base), + x0, residual -> Z[l + 1],
// LayerNorm (LayerW W), dropout -> H[l + 1]; HROW: the node's H[l] row; out = the node's H[l + 1] row.  Reads `drop`.
#define TINY_LAYER_TAIL_FORWARD(V, HROW, W, l, i, att, out)                                        \
    {                                                                                              \
        store_row<DP>(tp.ATT + (static_cast<size_t>(l) * n + i) * DP, att);                        \
        if (a.use_graph) {                                                                         \
            float g[DP];                                                                           \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) g[m] = 0.f;                                               \
            TINY_GATHER_ROWS(V, i, g)                                                              \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) out[m] = a.a_s * att[m] + a.g_s * g[m];   /* :130-134 */  \
        } else {                                                                                   \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) out[m] = att[m];                                          \
        }                                                                                          \
        float hl[DP];                                                                              \
        load_row<DP>(HROW, hl);                                                                    \
        if (a.use_source) {                                                        /* :139-140 */  \
            float x0[DP];                                                                          \
            load_row<DP>(tp.H + static_cast<size_t>(i) * DP, x0);                                  \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) out[m] += x0[m];                                          \
        }                                                                                          \
        if (a.residual) {                                                          /* :200-201 */  \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) out[m] = a.alpha * out[m] + (1.0f - a.alpha) * hl[m];     \
        }                                                                                          \
        store_row<DP>(tp.Z + (static_cast<size_t>(l + 1) * n + i) * DP, out);                      \
        if (a.use_bn) {                                                            /* :202-203 */  \
            float mean, rstd;                                                                      \
            ln_stats<DP>(out, d, a.eps, mean, rstd);                                               \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) out[m] = (m < d) ? (out[m] - mean) * rstd * W.lnw[m] + W.lnb[m] : 0.f; \
        }                                                                                          \
        if (drop) dropout_row<DP>(out, a.rnd, (static_cast<int64_t>(l + 1) * n + i) * d, d, a.p_drop);   /* :204 */ \
        store_row<DP>(tp.H + (static_cast<size_t>(l + 1) * n + i) * DP, out);                      \
    }

// output Linear (:208) of node i from its H[L] row h
#define TINY_OUTPUT_ROW(i, h)                                                                      \
    {                                                                                              \
        for (int c = 0; c < a.c; ++c) {                                                            \
            float acc = sBo[c];                                                                    \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) acc += sWo[c * DP + m] * h[m];                            \
            a.y[static_cast<size_t>(i) * a.c + c] = acc;                                           \
        }                                                                                          \
    }

// ======================================================================================================================
// backward
// ======================================================================================================================
// output Linear: g += the node's row of d H[L] = gy Wo
#define TINY_OUTPUT_BACKWARD_ROW(i, g)                                                             \
    {                                                                                              \
        for (int c = 0; c < a.c; ++c) {                                                            \
            const float gv = a.gy[static_cast<size_t>(i) * a.c + c];                               \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) g[m] += gv * sWo[c * DP + m];                             \
        }                                                                                          \
    }

// the forward's dropout mask and scale on a gradient row; AT: index of the row's first uniform.  Reads `keep`.
#define TINY_DROPOUT_BACKWARD(dy, AT)                                                              \
    {                                                                                              \
        const int64_t at = AT;                                                                     \
        TINY_UNROLL                                                                                \
        for (int m = 0; m < DP; ++m)                                                               \
            if (m < d) dy[m] = (a.rnd[at + m] >= a.p_drop) ? dy[m] * keep : 0.f;                   \
    }

// Layer l's tail of node i, from the gradient dy of the layer's OUTPUT (H[l + 1]) up to the attention: dropout / LayerNorm (weight
// LNW, pre-LayerNorm row at ZROW) / residual backward, dy and dy * xh -> DYROW, DYXROW (the operands of the LayerNorm gradients'
// sums over nodes), the direct term -> DIRROW, + x0 into DX0ROW, the aggregation's operand -> SGROW.  -> datt.  Reads `drop`, `keep`.
#define TINY_TAIL_BACKWARD(LNW, ZROW, DYROW, DYXROW, DIRROW, DX0ROW, SGROW, l, i, dy, datt)        \
    {                                                                                              \
        float z[DP], dz[DP];                                                                       \
        if (drop) TINY_DROPOUT_BACKWARD(dy, (static_cast<int64_t>(l + 1) * n + i) * d)             \
        if (a.use_bn) {                                                                            \
            load_row<DP>(ZROW, z);                                                                 \
            float mean, rstd;                                                                      \
            ln_stats<DP>(z, d, a.eps, mean, rstd);                                                 \
            float xh[DP], m1 = 0.f, m2 = 0.f;                                                      \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) {                                                         \
                xh[m] = (m < d) ? (z[m] - mean) * rstd : 0.f;                                      \
                const float gw = LNW[m] * dy[m];                                                   \
                m1 += gw;                                                                          \
                m2 += gw * xh[m];                                                                  \
            }                                                                                      \
            m1 /= static_cast<float>(d);                                                           \
            m2 /= static_cast<float>(d);                                                           \
            float dyx[DP];                                                                         \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) {                                                         \
                dyx[m] = dy[m] * xh[m];                                                            \
                dz[m] = (m < d) ? rstd * (LNW[m] * dy[m] - m1 - xh[m] * m2) : 0.f;                 \
            }                                                                                      \
            store_row<DP>(DYROW, dy);                                                              \
            store_row<DP>(DYXROW, dyx);                                                            \
        } else {                                                                                   \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) dz[m] = dy[m];                                            \
        }                                                                                          \
        float dout[DP], dir[DP];                                                                   \
        TINY_UNROLL                                                                                \
        for (int m = 0; m < DP; ++m) {                                                             \
            dout[m] = a.residual ? a.alpha * dz[m] : dz[m];                                        \
            dir[m] = a.residual ? (1.0f - a.alpha) * dz[m] : 0.f;                                  \
        }                                                                                          \
        store_row<DP>(DIRROW, dir);                                                                \
        if (a.use_source) {                                                                        \
            float acc[DP];                                                                         \
            load_row<DP>(DX0ROW, acc);                                                             \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) acc[m] += dout[m];                                        \
            store_row<DP>(DX0ROW, acc);                                                            \
        }                                                                                          \
        if (a.use_graph) {                                                                         \
            float sg[DP];                                                                          \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) { sg[m] = a.g_s * dout[m]; datt[m] = a.a_s * dout[m]; }   \
            store_row<DP>(SGROW, sg);                                                              \
        } else {                                                                                   \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) datt[m] = dout[m];                                        \
        }                                                                                          \
    }

// `simple`: the attention's set-up of one node from datt, its q and the layer's scale s (sums in sSum): d num, d den, t_s (the node's
// term of d s) and the part of d q that does not wait for the backward's sums over nodes
#define TINY_SIMPLE_BACKWARD_SETUP(q, datt, s, dnum, dden, ts, dq)                                 \
    {                                                                                              \
        float A[DP], b = 0.f;                                                                      \
        TINY_UNROLL                                                                                \
        for (int dd = 0; dd < DP; ++dd) {                                                          \
            float acc = 0.f;                                                                       \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) acc += q[m] * sSum[m * DP + dd];                          \
            A[dd] = acc;                                                                           \
        }                                                                                          \
        TINY_UNROLL                                                                                \
        for (int m = 0; m < DP; ++m) b += q[m] * sSum[DP * DP + m];                                \
        const float den = s * b + static_cast<float>(n);                                           \
        TINY_UNROLL                                                                                \
        for (int dd = 0; dd < DP; ++dd) {                                                          \
            const float att = (s * A[dd] + sSum[DP * DP + DP + dd]) / den;                         \
            dnum[dd] = datt[dd] / den;                                                             \
            dden -= dnum[dd] * att;                                                                \
            ts += dnum[dd] * A[dd];                                                                \
        }                                                                                          \
        ts += dden * b;                                                                            \
        TINY_UNROLL                                                                                \
        for (int m = 0; m < DP; ++m) {                                                             \
            float acc = 0.f;                                                                       \
            TINY_UNROLL                                                                            \
            for (int dd = 0; dd < DP; ++dd) acc += sSum[m * DP + dd] * dnum[dd];                   \
            dq[m] = s * (acc + dden * sSum[DP * DP + m]);                                          \
        }                                                                                          \
    }

// dq, dk, dv -> the gradient of the node's layer input: dh = DIR + dq Wq + dk Wk + dv Wv (LayerW W)
#define TINY_BACK_PROJECT(DIRROW, W, dq, dk, dv, dh)                                               \
    {                                                                                              \
        load_row<DP>(DIRROW, dh);                                                                  \
        matvec_t_add<DP>(W.wq, dq, dh);                                                            \
        matvec_t_add<DP>(W.wk, dk, dh);                                                            \
        if (a.use_weight) matvec_t_add<DP>(W.wv, dv, dh);                                          \
        else {                                                                                     \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) dh[m] += dv[m];                                           \
        }                                                                                          \
    }

// input layer backward (:188-192) of node i from dh = the gradient of H[0]: + DX0, dropout, ReLU and LayerNorm backward -> DPREROW
// (d pre-activation; dh and dh * xh -> DYROW, DYXROW) for the sums over nodes, and dx.  Reads `drop`, `keep`.
#define TINY_INPUT_BACKWARD(DX0ROW, ZROW, DYROW, DYXROW, DPREROW, i, dh)                           \
    {                                                                                              \
        float z[DP];                                                                               \
        if (a.use_source) {                                                                        \
            float acc[DP];                                                                         \
            load_row<DP>(DX0ROW, acc);                                                             \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) dh[m] += acc[m];                                          \
        }                                                                                          \
        if (drop) TINY_DROPOUT_BACKWARD(dh, static_cast<int64_t>(i) * d)                           \
        load_row<DP>(ZROW, z);                                                                     \
        float dpre[DP];                                                                            \
        if (a.use_bn) {                                                                            \
            float mean, rstd;                                                                      \
            ln_stats<DP>(z, d, a.eps, mean, rstd);                                                 \
            float xh[DP], m1 = 0.f, m2 = 0.f, dyx[DP];                                             \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) {                                                         \
                xh[m] = (m < d) ? (z[m] - mean) * rstd : 0.f;                                      \
                const float yv = xh[m] * sLn0w[m] + sLn0b[m];                                      \
                if (!(yv > 0.f)) dh[m] = 0.f;                                            /* ReLU */ \
                const float gw = sLn0w[m] * dh[m];                                                 \
                m1 += gw;                                                                          \
                m2 += gw * xh[m];                                                                  \
                dyx[m] = dh[m] * xh[m];                                                            \
            }                                                                                      \
            m1 /= static_cast<float>(d);                                                           \
            m2 /= static_cast<float>(d);                                                           \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) dpre[m] = (m < d) ? rstd * (sLn0w[m] * dh[m] - m1 - xh[m] * m2) : 0.f; \
            store_row<DP>(DYROW, dh);                                                              \
            store_row<DP>(DYXROW, dyx);                                                            \
        } else {                                                                                   \
            TINY_UNROLL                                                                            \
            for (int m = 0; m < DP; ++m) dpre[m] = (m < d && z[m] > 0.f) ? dh[m] : 0.f;            \
        }                                                                                          \
        store_row<DP>(DPREROW, dpre);                                                              \
        if (a.dx) {                                                                                \
            for (int f = 0; f < a.f_in; ++f) {                                                     \
                float acc = 0.f;                                                                   \
                TINY_UNROLL                                                                        \
                for (int m = 0; m < DP; ++m) acc += dpre[m] * sW0[m * kMaxIn + f];                 \
                a.dx[static_cast<size_t>(i) * a.f_in + f] = acc;                                   \
            }                                                                                      \
        }                                                                                          \
    }
