// Host side shared by the entry points of the whole-model kernels for tiny graphs (tiny_model.hip in libdifformer_hip.so,
// tiny_batched.hip in libdifformer_snapshots.so): the configuration check, the argument block from the C ABI's pointer arrays and
// the workgroup size.  Inline: each library reports through its own dif::fail.
#pragma once
#include "tiny_common.h"

namespace tiny {

inline int check_cfg(const dif_tiny_cfg* cfg) {
    DIF_REQUIRE(cfg != nullptr, DIF_E_BADARG, "dif_tiny: null configuration");
    DIF_REQUIRE(cfg->n >= 1 && cfg->n <= kMaxNodes, DIF_E_SHAPE, "dif_tiny: 1 <= n <= %d nodes (got %d)", kMaxNodes, cfg->n);
    DIF_REQUIRE(cfg->hidden >= 1 && cfg->hidden <= 8, DIF_E_SHAPE, "dif_tiny: hidden width 1..8 (got %d)", cfg->hidden);
    DIF_REQUIRE(cfg->in_channels >= 1 && cfg->in_channels <= kMaxIn, DIF_E_SHAPE, "dif_tiny: 1..%d input features (got %d)", kMaxIn,
                cfg->in_channels);
    DIF_REQUIRE(cfg->out_channels >= 1 && cfg->out_channels <= kMaxOut, DIF_E_SHAPE, "dif_tiny: 1..%d outputs (got %d)", kMaxOut,
                cfg->out_channels);
    DIF_REQUIRE(cfg->num_layers >= 1 && cfg->num_layers <= kMaxLayers, DIF_E_SHAPE, "dif_tiny: 1..%d layers (got %d)", kMaxLayers,
                cfg->num_layers);
    DIF_REQUIRE(cfg->kernel == 0 || cfg->kernel == 1, DIF_E_BADARG, "dif_tiny: kernel 0 (simple) or 1 (sigmoid)");
    DIF_REQUIRE(cfg->dropout >= 0.f && cfg->dropout < 1.f, DIF_E_BADARG, "dif_tiny: dropout in [0, 1)");
    DIF_REQUIRE(cfg->launch_plan >= 0 && cfg->launch_plan <= 2, DIF_E_BADARG, "dif_tiny: launch_plan 0 (by size), 1 (one workgroup) or 2 (grid)");
    return 0;
}

// params / grads: 6 + 8 * layers pointers in the order
//   fcs.0.weight, fcs.0.bias, bns.0.weight, bns.0.bias, fcs.1.weight, fcs.1.bias,
//   then per layer: Wk.weight, Wk.bias, Wq.weight, Wq.bias, Wv.weight, Wv.bias, bns.{l+1}.weight, bns.{l+1}.bias
inline int fill(TinyArgs& a, const dif_tiny_cfg* cfg, const float* x, int64_t ldx, const void* const* params) {
    a.n = cfg->n; a.f_in = cfg->in_channels; a.d = cfg->hidden; a.c = cfg->out_channels; a.layers = cfg->num_layers;
    a.sigmoid = cfg->kernel; a.use_bn = cfg->use_bn; a.residual = cfg->use_residual; a.use_weight = cfg->use_weight;
    a.use_graph = cfg->use_graph; a.use_source = cfg->use_source; a.training = cfg->training;
    a.alpha = cfg->alpha; a.a_s = cfg->attn_scale; a.g_s = cfg->gcn_scale; a.p_drop = cfg->dropout; a.eps = cfg->eps;
    a.x = x; a.ldx = ldx;
    DIF_REQUIRE(x != nullptr && params != nullptr && ldx >= cfg->in_channels, DIF_E_BADARG, "dif_tiny: null x / params or ldx < in_channels");
    auto P = [&](int k) { return static_cast<const float*>(params[k]); };
    a.w0 = P(0); a.b0 = P(1); a.ln0w = P(2); a.ln0b = P(3); a.wo = P(4); a.bo = P(5);
    DIF_REQUIRE(a.w0 && a.b0 && a.wo && a.bo, DIF_E_BADARG, "dif_tiny: null Linear parameter");
    DIF_REQUIRE(!cfg->use_bn || (a.ln0w && a.ln0b), DIF_E_BADARG, "dif_tiny: use_bn without LayerNorm parameters");
    for (int l = 0; l < cfg->num_layers; ++l) {
        LayerPtrs& p = a.lp[l];
        p.wk = P(6 + 8 * l); p.bk = P(7 + 8 * l); p.wq = P(8 + 8 * l); p.bq = P(9 + 8 * l);
        p.wv = P(10 + 8 * l); p.bv = P(11 + 8 * l); p.lnw = P(12 + 8 * l); p.lnb = P(13 + 8 * l);
        DIF_REQUIRE(p.wk && p.bk && p.wq && p.bq, DIF_E_BADARG, "dif_tiny: null Wq / Wk of layer %d", l);
        DIF_REQUIRE(!cfg->use_weight || (p.wv && p.bv), DIF_E_BADARG, "dif_tiny: use_weight without Wv of layer %d", l);
        DIF_REQUIRE(!cfg->use_bn || (p.lnw && p.lnb), DIF_E_BADARG, "dif_tiny: use_bn without LayerNorm of layer %d", l);
    }
    return 0;
}

inline int block_threads(int n) {
    int t = (n + 63) / 64 * 64;
    return t < 64 ? 64 : (t > 512 ? 512 : t);     // 512: two waves per SIMD, 256 VGPRs each (no spills at hidden 8)
}

// the backward's gradient pointers, in the order of params (each the size of its parameter)
inline int fill_grads(TinyArgs& a, const dif_tiny_cfg* cfg, void* const* grads, const char* who) {
    auto G = [&](int k) { return static_cast<float*>(grads[k]); };
    a.gw0 = G(0); a.gb0 = G(1); a.gln0w = G(2); a.gln0b = G(3); a.gwo = G(4); a.gbo = G(5);
    DIF_REQUIRE(a.gw0 && a.gb0 && a.gwo && a.gbo && (!cfg->use_bn || (a.gln0w && a.gln0b)), DIF_E_BADARG, "%s: null gradient buffer", who);
    for (int l = 0; l < cfg->num_layers; ++l) {
        LayerGrads& g = a.lg[l];
        g.wk = G(6 + 8 * l); g.bk = G(7 + 8 * l); g.wq = G(8 + 8 * l); g.bq = G(9 + 8 * l);
        g.wv = G(10 + 8 * l); g.bv = G(11 + 8 * l); g.lnw = G(12 + 8 * l); g.lnb = G(13 + 8 * l);
        DIF_REQUIRE(g.wk && g.bk && g.wq && g.bq && (!cfg->use_weight || (g.wv && g.bv)) && (!cfg->use_bn || (g.lnw && g.lnb)),
                    DIF_E_BADARG, "%s: null gradient buffer of layer %d", who, l);
    }
    return 0;
}

}  // namespace tiny
