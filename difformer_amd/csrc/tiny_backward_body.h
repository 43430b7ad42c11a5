// The body of the one-workgroup BACKWARD kernel for tiny graphs, ONE definition, included textually between the braces of
// tiny_backward_kernel<DP> (tiny_model.hip) and snap_backward_kernel<DP> (tiny_batched.hip); see tiny_forward_body.h.  It reads `a`
// (fields of TinyArgs; `a.lp[l]` a LayerPtrs, `a.lg[l]` a LayerGrads) and the template parameter DP; never blockIdx.
    constexpr int TK = 2048 / DP;                 // nodes per LDS tile of the sigmoid backward sweep (4 rows + 1 scalar each)
    __shared__ float sW0[DP * kMaxIn];
    __shared__ float sLn0w[DP], sLn0b[DP];
    __shared__ LayerW<DP> sL;
    __shared__ float sWo[kMaxOut * DP];
    __shared__ float sSum[96];                    // forward sums of the layer (simple)
    __shared__ float sG[96];                      // their gradients: dKtV [DP*DP], dksum [DP], dvsum [DP], ds
    __shared__ float sVec[4 * DP];
    __shared__ double sPart[1024];
    __shared__ float sTile[TK * (4 * DP + 1)];
    const int n = a.n, d = a.d, L = a.layers, T = blockDim.x, t = threadIdx.x;
    Tape<DP> tp(a.tape, n, L);
    const size_t nd = static_cast<size_t>(n) * DP;
    float* S = a.scratch;
    float *DH = S, *DX0 = S + nd, *SG = S + 2 * nd, *DNUM = S + 3 * nd, *DY = S + 4 * nd, *DYX = S + 5 * nd, *DIR = S + 6 * nd,
          *DQ = S + 7 * nd, *DK = S + 8 * nd, *DV = S + 9 * nd, *Q = S + 10 * nd, *K = S + 11 * nd, *V = S + 12 * nd,
          *DPRE = S + 13 * nd;
    float* DDEN = S + kBwdSlots * nd;
    float* TS = DDEN + n;
    const bool drop = a.training && a.rnd != nullptr && a.p_drop > 0.f;
    const float keep = drop ? 1.0f / (1.0f - a.p_drop) : 1.0f;

    TINY_LOAD_INPUT_CONSTS()
    TINY_LOAD_OUTPUT_CONSTS()
    __syncthreads();

    // ---- output Linear: d H[L] = gy Wo; d Wo = gy^T H[L]; d bo = sum gy ----
    for (int i = t; i < n; i += T) {
        float g[DP];
#pragma unroll
        for (int m = 0; m < DP; ++m) g[m] = 0.f;
        TINY_OUTPUT_BACKWARD_ROW(i, g)
        store_row<DP>(DH + static_cast<size_t>(i) * DP, g);
        if (a.use_source) {
#pragma unroll
            for (int m = 0; m < DP; ++m) g[m] = 0.f;
            store_row<DP>(DX0 + static_cast<size_t>(i) * DP, g);
        }
    }
    {
        const float* HL = tp.H + static_cast<size_t>(L) * nd;
        // d Wo [c][m] = sum_i gy[i][c] H[L][i][m]  (true width d in the output)
        for (int c = 0; c < a.c; ++c) {
            outer_sum(a.gy + c, a.c, 1, HL, DP, DP, n, 1.f, sVec, sPart);
            if (t < d) a.gwo[c * d + t] = sVec[t];
            __syncthreads();
        }
        outer_sum(a.gy, a.c, a.c, nullptr, 0, 1, n, 1.f, sVec, sPart);
        if (t < a.c) a.gbo[t] = sVec[t];
        __syncthreads();
    }

    for (int l = L - 1; l >= 0; --l) {
        load_layer<DP>(sL, a.lp[l], d, a.use_weight, a.use_bn);
        if (!a.sigmoid)
            for (int k = t; k < DP * DP + 2 * DP + 2; k += T) sSum[k] = tp.SUM[l * 96 + k];
        __syncthreads();
        const float* Hl = tp.H + static_cast<size_t>(l) * nd;
        const float q2 = sSum[DP * DP + 2 * DP], k2 = sSum[DP * DP + 2 * DP + 1];
        const float s = a.sigmoid ? 0.f : 1.0f / (sqrtf(q2) * sqrtf(k2));
        // ---- phase 1: tail backward, attention set-up, per node ----
        for (int i = t; i < n; i += T) {
            float dy[DP], datt[DP];
            load_row<DP>(DH + static_cast<size_t>(i) * DP, dy);
            TINY_TAIL_BACKWARD(sL.lnw, tp.Z + (static_cast<size_t>(l + 1) * n + i) * DP, DY + static_cast<size_t>(i) * DP, DYX + static_cast<size_t>(i) * DP,
                               DIR + static_cast<size_t>(i) * DP, DX0 + static_cast<size_t>(i) * DP, SG + static_cast<size_t>(i) * DP, l, i, dy, datt)
            float h[DP], q[DP], k[DP], v[DP];
            load_row<DP>(Hl + static_cast<size_t>(i) * DP, h);
            TINY_PROJECT(sL, a.use_weight, h, q, k, v)
            store_row<DP>(Q + static_cast<size_t>(i) * DP, q);
            store_row<DP>(K + static_cast<size_t>(i) * DP, k);
            store_row<DP>(V + static_cast<size_t>(i) * DP, v);
            if (a.sigmoid) {
                float att[DP], da[DP];
                load_row<DP>(tp.ATT + (static_cast<size_t>(l) * n + i) * DP, att);
                const float rden = 1.0f / tp.DEN[static_cast<size_t>(l) * n + i];
                float dl = 0.f;
#pragma unroll
                for (int m = 0; m < DP; ++m) { da[m] = datt[m] * rden; dl += datt[m] * att[m]; }
                store_row<DP>(DNUM + static_cast<size_t>(i) * DP, da);          // DA_i = d att_i / den_i
                DDEN[i] = dl * rden;                                             // DL_i = (d att_i . att_i) / den_i
            } else {
                float dnum[DP], dden = 0.f, ts = 0.f, dq[DP];
                TINY_SIMPLE_BACKWARD_SETUP(q, datt, s, dnum, dden, ts, dq)
                store_row<DP>(DNUM + static_cast<size_t>(i) * DP, dnum);
                store_row<DP>(DQ + static_cast<size_t>(i) * DP, dq);
                DDEN[i] = dden;
                TS[i] = ts;
            }
        }
        __syncthreads();
        // ---- phase 2: sums over nodes ----
        if (a.use_bn) {
            outer_sum(DYX, DP, DP, nullptr, 0, 1, n, 1.f, sVec, sPart);
            if (t < d) a.lg[l].lnw[t] = sVec[t];
            __syncthreads();
            outer_sum(DY, DP, DP, nullptr, 0, 1, n, 1.f, sVec, sPart);
            if (t < d) a.lg[l].lnb[t] = sVec[t];
            __syncthreads();
        }
        float gq2 = 0.f, gk2 = 0.f;
        if (!a.sigmoid) {
            outer_sum(Q, DP, DP, DNUM, DP, DP, n, s, sG, sPart);                       // d KtV [m][dd] = s sum q[m] dnum[dd]
            outer_sum(Q, DP, DP, DDEN, 1, 1, n, s, sG + DP * DP, sPart);               // d ksum [m]    = s sum dden q[m]
            outer_sum(DNUM, DP, DP, nullptr, 0, 1, n, 1.f, sG + DP * DP + DP, sPart);  // d vsum [dd]   = sum dnum[dd]
            outer_sum(TS, 1, 1, nullptr, 0, 1, n, 1.f, sG + DP * DP + 2 * DP, sPart);  // d s
            const float ds = sG[DP * DP + 2 * DP];
            gq2 = -0.5f * s * ds / q2;                                                // s = q2^-1/2 k2^-1/2
            gk2 = -0.5f * s * ds / k2;
        }
        // ---- phase 3: attention + aggregation + projection backward per node ----
        const int slots = (n + T - 1) / T;
        for (int slot = 0; slot < slots; ++slot) {
            const int i = slot * T + t;
            const bool live = i < n;
            float q[DP], k[DP], v[DP], dq[DP], dk[DP], dv[DP];
#pragma unroll
            for (int m = 0; m < DP; ++m) { q[m] = k[m] = v[m] = dq[m] = dk[m] = dv[m] = 0.f; }
            if (live) {
                load_row<DP>(Q + static_cast<size_t>(i) * DP, q);
                load_row<DP>(K + static_cast<size_t>(i) * DP, k);
                load_row<DP>(V + static_cast<size_t>(i) * DP, v);
            }
            if (a.sigmoid) {
                float da[DP], dl = 0.f;
                double dqd[DP], dkd[DP], dvd[DP];
#pragma unroll
                for (int m = 0; m < DP; ++m) { da[m] = 0.f; dqd[m] = 0.0; dkd[m] = 0.0; dvd[m] = 0.0; }
                if (live) {
                    load_row<DP>(DNUM + static_cast<size_t>(i) * DP, da);
                    dl = DDEN[i];
                }
                for (int o0 = 0; o0 < n; o0 += TK) {
                    const int cnt = min(TK, n - o0);
                    __syncthreads();
                    for (int kk = t; kk < cnt * DP; kk += T) {
                        sTile[kk] = Q[static_cast<size_t>(o0) * DP + kk];
                        sTile[TK * DP + kk] = K[static_cast<size_t>(o0) * DP + kk];
                        sTile[2 * TK * DP + kk] = V[static_cast<size_t>(o0) * DP + kk];
                        sTile[3 * TK * DP + kk] = DNUM[static_cast<size_t>(o0) * DP + kk];
                    }
                    for (int kk = t; kk < cnt; kk += T) sTile[4 * TK * DP + kk] = DDEN[o0 + kk];
                    __syncthreads();
                    if (live) {
                      for (int ob = 0; ob < cnt; ob += 64) {
                        float dqf[DP], dkf[DP], dvf[DP];
#pragma unroll
                        for (int m = 0; m < DP; ++m) { dqf[m] = 0.f; dkf[m] = 0.f; dvf[m] = 0.f; }
                        const int o1 = min(cnt, ob + 64);
                        for (int o = ob; o < o1; ++o) {
                            const float* qo = sTile + o * DP;
                            const float* ko = sTile + TK * DP + o * DP;
                            const float* vo = sTile + 2 * TK * DP + o * DP;
                            const float* dao = sTile + 3 * TK * DP + o * DP;
                            const float dlo = sTile[4 * TK * DP + o];
                            // this node as the QUERY against key o:   dq_i += dS k_o
                            float dot = 0.f, dp = -dl;
#pragma unroll
                            for (int m = 0; m < DP; ++m) { dot += q[m] * ko[m]; dp += da[m] * vo[m]; }
                            float p = sigmoidf(dot);
                            float dsv = dp * p * (1.0f - p);
#pragma unroll
                            for (int m = 0; m < DP; ++m) dqf[m] += dsv * ko[m];
                            // this node as the KEY against query o:   dv_j += P DA_o;  dk_j += dS' q_o
                            dot = 0.f;
                            dp = -dlo;
#pragma unroll
                            for (int m = 0; m < DP; ++m) { dot += qo[m] * k[m]; dp += dao[m] * v[m]; }
                            p = sigmoidf(dot);
                            dsv = dp * p * (1.0f - p);
#pragma unroll
                            for (int m = 0; m < DP; ++m) { dvf[m] += p * dao[m]; dkf[m] += dsv * qo[m]; }
                        }
                        // 64 pairs in float32, the blocks of 64 added in float64 (the sums cancel: their terms are larger than they)
#pragma unroll
                        for (int m = 0; m < DP; ++m) {
                            dqd[m] += static_cast<double>(dqf[m]);
                            dkd[m] += static_cast<double>(dkf[m]);
                            dvd[m] += static_cast<double>(dvf[m]);
                        }
                      }
                    }
                }
#pragma unroll
                for (int m = 0; m < DP; ++m) {
                    dq[m] = static_cast<float>(dqd[m]);
                    dk[m] = static_cast<float>(dkd[m]);
                    dv[m] = static_cast<float>(dvd[m]);
                }
            } else if (live) {
                load_row<DP>(DQ + static_cast<size_t>(i) * DP, dq);
#pragma unroll
                for (int m = 0; m < DP; ++m) {
                    dq[m] += 2.0f * gq2 * q[m];
                    float acc = 0.f;
#pragma unroll
                    for (int dd = 0; dd < DP; ++dd) acc += sG[m * DP + dd] * v[dd];
                    dk[m] = acc + sG[DP * DP + m] + 2.0f * gk2 * k[m];
                }
#pragma unroll
                for (int dd = 0; dd < DP; ++dd) {
                    float acc = 0.f;
#pragma unroll
                    for (int m = 0; m < DP; ++m) acc += sG[m * DP + dd] * k[m];
                    dv[dd] = acc + sG[DP * DP + DP + dd];
                }
            }
            if (live) {
                if (a.use_graph) TINY_GATHER_ROWS(SG, i, dv)      // adjoint of the aggregation: the TRANSPOSED CSR, edge order
                // padded columns carry nothing
#pragma unroll
                for (int m = 0; m < DP; ++m)
                    if (m >= d) { dq[m] = 0.f; dk[m] = 0.f; dv[m] = 0.f; }
                store_row<DP>(DQ + static_cast<size_t>(i) * DP, dq);
                store_row<DP>(DK + static_cast<size_t>(i) * DP, dk);
                store_row<DP>(DV + static_cast<size_t>(i) * DP, dv);
                float dh[DP];
                TINY_BACK_PROJECT(DIR + static_cast<size_t>(i) * DP, sL, dq, dk, dv, dh)
                store_row<DP>(DH + static_cast<size_t>(i) * DP, dh);
            }
        }
        __syncthreads();
        // ---- phase 4: weight gradients ----
        for (int which = 0; which < (a.use_weight ? 3 : 2); ++which) {
            const float* G = which == 0 ? DQ : (which == 1 ? DK : DV);
            float* gw = which == 0 ? a.lg[l].wq : (which == 1 ? a.lg[l].wk : a.lg[l].wv);
            float* gb = which == 0 ? a.lg[l].bq : (which == 1 ? a.lg[l].bk : a.lg[l].bv);
            outer_sum(G, DP, DP, Hl, DP, DP, n, 1.f, sG, sPart);
            for (int kk = t; kk < d * d; kk += T) gw[kk] = sG[(kk / d) * DP + kk % d];
            __syncthreads();
            outer_sum(G, DP, DP, nullptr, 0, 1, n, 1.f, sVec, sPart);
            if (t < d) gb[t] = sVec[t];
            __syncthreads();
        }
    }

    // ---- input layer backward (:188-192) ----
    for (int i = t; i < n; i += T) {
        float dy[DP];
        load_row<DP>(DH + static_cast<size_t>(i) * DP, dy);
        TINY_INPUT_BACKWARD(DX0 + static_cast<size_t>(i) * DP, tp.Z + static_cast<size_t>(i) * DP, DY + static_cast<size_t>(i) * DP, DYX + static_cast<size_t>(i) * DP,
                            DPRE + static_cast<size_t>(i) * DP, i, dy)
    }
    __syncthreads();
    if (a.use_bn) {
        outer_sum(DYX, DP, DP, nullptr, 0, 1, n, 1.f, sVec, sPart);
        if (t < d) a.gln0w[t] = sVec[t];
        __syncthreads();
        outer_sum(DY, DP, DP, nullptr, 0, 1, n, 1.f, sVec, sPart);
        if (t < d) a.gln0b[t] = sVec[t];
        __syncthreads();
    }
    for (int m = 0; m < d; ++m) {                  // d W0 [m][f] = sum_i dpre[i][m] x[i][f]
        outer_sum(DPRE + m, DP, 1, a.x, a.ldx, a.f_in, n, 1.f, sW0, sPart);
        for (int f = t; f < a.f_in; f += T) a.gw0[m * a.f_in + f] = sW0[f];
        __syncthreads();
    }
    outer_sum(DPRE, DP, DP, nullptr, 0, 1, n, 1.f, sVec, sPart);
    if (t < d) a.gb0[t] = sVec[t];
