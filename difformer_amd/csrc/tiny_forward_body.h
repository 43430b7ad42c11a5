// The body of the one-workgroup FORWARD kernel for tiny graphs, ONE definition, included textually between the braces of
//     tiny_forward_kernel<DP>           tiny_model.hip     one workgroup, one snapshot; `a` is the kernel's TinyArgs parameter
//     snap_forward_kernel<DP>           tiny_batched.hip   one workgroup per snapshot of a batch; `a` is a local view of the common
//                                                          arguments with the snapshot's record patched in
// It is an include, not a __device__ function template, for the reason tiny_stages.h gives for its macros: under
// -ffp-contract=fast which multiply-add pairs fuse is decided over the whole inlined kernel, and the device code of
// tiny_forward_kernel<4|8> must stay what it was (scripts/device_asm_diff.py --per-kernel).  No include guard: it is a body, not
// a declaration.  It reads `a` (fields of TinyArgs; `a.lp[l]` a LayerPtrs) and the template parameter DP, and uses
// threadIdx / blockDim only: never blockIdx.
    constexpr int TK = 4096 / DP;                 // keys per LDS tile of the sigmoid sweep (K and V rows: 32 KiB)
    __shared__ float sW0[DP * kMaxIn];
    __shared__ float sB0[DP], sLn0w[DP], sLn0b[DP];
    __shared__ LayerW<DP> sL;
    __shared__ float sWo[kMaxOut * DP], sBo[kMaxOut];
    __shared__ float sSum[96];
    __shared__ double sPart[1024];
    __shared__ float sKV[TK * 2 * DP];
    const int n = a.n, d = a.d, L = a.layers, T = blockDim.x, t = threadIdx.x;
    Tape<DP> tp(a.tape, n, L);
    const bool drop = a.training && a.rnd != nullptr && a.p_drop > 0.f;

    TINY_LOAD_INPUT_CONSTS(sB0[k_] = k_ < d ? a.b0[k_] : 0.f;)
    TINY_LOAD_OUTPUT_CONSTS(for (int k_ = t; k_ < kMaxOut; k_ += T) sBo[k_] = k_ < a.c ? a.bo[k_] : 0.f;)
    __syncthreads();

    // ---- input layer: Linear -> LayerNorm -> ReLU -> dropout (:188-192) ----
    for (int i = t; i < n; i += T) {
        float h[DP];
        TINY_INPUT_FORWARD(i, h)
    }

    for (int l = 0; l < L; ++l) {
        __syncthreads();
        load_layer<DP>(sL, a.lp[l], d, a.use_weight, a.use_bn);
        __syncthreads();
        const float* Hl = tp.H + static_cast<size_t>(l) * n * DP;
        // ---- projections (:115-120) ----
        for (int i = t; i < n; i += T) {
            float h[DP], q[DP], k[DP], v[DP];
            load_row<DP>(Hl + static_cast<size_t>(i) * DP, h);
            TINY_PROJECT(sL, a.use_weight, h, q, k, v)
            store_row<DP>(tp.Q + static_cast<size_t>(i) * DP, q);
            store_row<DP>(tp.K + static_cast<size_t>(i) * DP, k);
            store_row<DP>(tp.V + static_cast<size_t>(i) * DP, v);
        }
        __syncthreads();
        if (!a.sigmoid) {
            // K^T V, ksum, vsum, |Q|^2, |K|^2 (:20-34): sums over nodes
            outer_sum(tp.K, DP, DP, tp.V, DP, DP, n, 1.f, sSum, sPart);
            outer_sum(tp.K, DP, DP, nullptr, 0, 1, n, 1.f, sSum + DP * DP, sPart);
            outer_sum(tp.V, DP, DP, nullptr, 0, 1, n, 1.f, sSum + DP * DP + DP, sPart);
            // sum of squares: diagonal of Q^T Q / K^T K summed -- one output per column, then over the columns
            __shared__ float sSq[2 * DP];
            for (int which = 0; which < 2; ++which) {
                const float* P = which ? tp.K : tp.Q;
                // outer_sum of P with itself restricted to the diagonal: A = B = P, but only m == c wanted -> use M = DP, C = 1
                // on the element-wise squares: done by a dedicated chunked loop below
                const int Ob = DP;
                int chunks = T / Ob;
                if (chunks > 64) chunks = 64;
                const int len = (n + chunks - 1) / chunks;
                const int o = t % Ob, ch = t / Ob;
                if (ch < chunks) {
                    double acc = 0.0;
                    const int i1 = min(n, (ch + 1) * len);
                    for (int i = ch * len; i < i1; ++i) {
                        const double vq = P[static_cast<size_t>(i) * DP + o];
                        acc += vq * vq;
                    }
                    sPart[ch * Ob + o] = acc;
                }
                __syncthreads();
                if (t < Ob) {
                    double s = 0.0;
                    for (int k = 0; k < chunks; ++k) s += sPart[k * Ob + t];
                    sSq[which * DP + t] = static_cast<float>(s);
                }
                __syncthreads();
            }
            if (t == 0) {
                double q2 = 0.0, k2 = 0.0;
                for (int m = 0; m < DP; ++m) { q2 += sSq[m]; k2 += sSq[DP + m]; }
                sSum[DP * DP + 2 * DP] = static_cast<float>(q2);
                sSum[DP * DP + 2 * DP + 1] = static_cast<float>(k2);
            }
            __syncthreads();
            for (int k = t; k < DP * DP + 2 * DP + 2; k += T) tp.SUM[l * 96 + k] = sSum[k];
        }
        // ---- attention + aggregation + tail per node ----
        const int slots = (n + T - 1) / T;
        for (int slot = 0; slot < slots; ++slot) {
            const int i = slot * T + t;
            const bool live = i < n;
            float q[DP], att[DP];
#pragma unroll
            for (int m = 0; m < DP; ++m) { q[m] = 0.f; att[m] = 0.f; }
            if (live) load_row<DP>(tp.Q + static_cast<size_t>(i) * DP, q);
            if (a.sigmoid) {
                // :47-56  sigma(q k^T) / row sum, applied to v; the keys stream through LDS tiles; a tile's sums in float32,
                // the tiles added in float64
                double den = 0.0, accd[DP];
#pragma unroll
                for (int m = 0; m < DP; ++m) accd[m] = 0.0;
                for (int j0 = 0; j0 < n; j0 += TK) {
                    const int cnt = min(TK, n - j0);
                    __syncthreads();
                    for (int k = t; k < cnt * DP; k += T) {
                        sKV[k] = tp.K[static_cast<size_t>(j0) * DP + k];
                        sKV[TK * DP + k] = tp.V[static_cast<size_t>(j0) * DP + k];
                    }
                    __syncthreads();
                    if (live) {
                        for (int j0b = 0; j0b < cnt; j0b += 64) {
                            float denf = 0.f, accf[DP];
#pragma unroll
                            for (int m = 0; m < DP; ++m) accf[m] = 0.f;
                            const int j1 = min(cnt, j0b + 64);
                            for (int j = j0b; j < j1; ++j) {
                                float dot = 0.f;
#pragma unroll
                                for (int m = 0; m < DP; ++m) dot += q[m] * sKV[j * DP + m];
                                const float p = sigmoidf(dot);
                                denf += p;
#pragma unroll
                                for (int m = 0; m < DP; ++m) accf[m] += p * sKV[TK * DP + j * DP + m];
                            }
                            den += static_cast<double>(denf);
#pragma unroll
                            for (int m = 0; m < DP; ++m) accd[m] += static_cast<double>(accf[m]);
                        }
                    }
                }
                if (live) {
#pragma unroll
                    for (int m = 0; m < DP; ++m) att[m] = static_cast<float>(accd[m] / den);
                    tp.DEN[static_cast<size_t>(l) * n + i] = static_cast<float>(den);
                }
            } else if (live) {
                TINY_SIMPLE_ATTENTION_ROW(q, att)
            }
            if (live) {
                float out[DP];
                TINY_LAYER_TAIL_FORWARD(tp.V, Hl + static_cast<size_t>(i) * DP, sL, l, i, att, out)
            }
        }
    }
    // ---- output Linear (:208): a node's own row, no exchange needed ----
    for (int i = t; i < n; i += T) {
        float h[DP];
        load_row<DP>(tp.H + (static_cast<size_t>(L) * n + i) * DP, h);
        TINY_OUTPUT_ROW(i, h)
    }
