"""DIFFORMER_EXACT_FP32 (ops.set_exact_fp32 / dif_set_exact_fp32) against every split-bfloat16 path of the library.

In the default float32 mode about a dozen products run on split-bfloat16 operands; exact mode promises that no product of the
forward does (ops.EXACT_FP32).  What a split costs on N(0, 1) operands (~1e-6 of sum |a b|, random signs) hides below what a
norm-wise test resolves, so each test here feeds its path the operands of tests/precision.py -- positive `lo_heavy` values whose
split drops ~1e-5 of every product, all of it with one sign -- and measures the path in both modes against float64:
  (a) the default mode within the 1e-4 contract;
  (b) exact mode within B, about 3x the exact-mode error measured on the MI355X;
  (c) the default mode at 3 B or more: the shape does take the split product by default, so (b) catches a split product
      leaking into exact mode (the one exception, the wide sigmoid backward, says why in its docstring).
Docstrings give the errors measured on the MI355X as "default / exact".  The gates are `grep -n "exact_fp32()"
difformer_amd/csrc/*.hip` and `grep -n EXACT_FP32 difformer_amd/*.py`; only the bfloat16-storage gate of
csrc/skinny_linear.hip has no test here (its bf16 x bf16 products are exact in either mode)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import grad_err, rel_err
from oracle import difformer_oracle as orc
from precision import exact_bf16, lo_heavy, mixed

pytestmark = pytest.mark.gpu

TOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def both_modes(fn):
    """-> {False: fn() in the default mode, True: fn() under ops.set_exact_fp32(True)}; the previous setting comes back."""
    from difformer_amd import ops
    out = {}
    was = ops.set_exact_fp32(False)
    try:
        for exact in (False, True):
            ops.set_exact_fp32(exact)
            out[exact] = fn()
            torch.cuda.synchronize()
    finally:
        ops.set_exact_fp32(was)
    return out


def check(errs, bound, what, sens=3.0):
    d, e = errs[False], errs[True]
    print(f"\n[exact_fp32] {what}: default {d:.3e}  exact {e:.3e}  (B = {bound:.1e})")
    assert d < TOL, (what, errs)                                  # (a)
    assert e <= bound, (what, errs)                               # (b)
    assert d >= sens * bound, (what, errs)                        # (c)


# ================================================================== 1: dense 64 x 64 layer kernel (csrc/simple_layer.hip:1500-1505)
@pytest.mark.parametrize("graph_w", [False, True])
def test_dense_64x64_layer_kernel(graph_w, dev):
    """simple_layer_kernel<EXACT, GRAPH_W, float, ..., SPLIT> through backend.simple_layer (dif_simple_layer_f32): C = D = 64,
    16-byte aligned coef / Wv, no gather.  Synthetic coefficients coef = [MnT | cn | u | cd] make the attention product
    x MnT^T lo-heavy on both sides (in a model the +N of the simple kernel hides it); graph_w adds the graph product ax Wv^T.
    Measured: graph_w=False 1.15e-5 / 5.1e-7; graph_w=True 1.12e-5 / 6.5e-7."""
    from difformer_amd import ops
    be = ops.get_backend()
    n, C = 5000, 64
    x, MnT, u = lo_heavy((n, C), 1), lo_heavy((C, C), 2), exact_bf16((C,), 3)
    coef = np.concatenate([MnT.reshape(-1), np.zeros(C, np.float32), u, [np.float32(1.0)]]).astype(np.float32)
    x64 = x.astype(np.float64)
    ref = (x64 @ MnT.astype(np.float64).T) / (x64 @ u.astype(np.float64) + 1.0)[:, None]
    ax = Wv = bv = None
    if graph_w:
        ax, Wv = lo_heavy((n, C), 4), lo_heavy((C, C), 5, 2.0 ** -6)
        bv = np.zeros(C, np.float32)
        ref = ref + ax.astype(np.float64) @ Wv.astype(np.float64).T
    xd, cd_, axd, Wvd, bvd = (None if a is None else t(a, dev) for a in (x, coef, ax, Wv, bv))
    outs = both_modes(lambda: be.simple_layer(xd, cd_, C, axd, Wvd, bvd, None, 1.0).cpu().numpy())
    check({m: rel_err(o, ref) for m, o in outs.items()}, 2.0e-6 if graph_w else 1.5e-6, f"dense layer graph_w={graph_w}")


# ================================================================== 2: output Linear folded into the last layer (difformer.py:574)
def test_output_linear_folded_into_the_last_layer(dev):
    """Eval model, last layer, no grad: the default mode runs the output Linear inside the last layer kernel on split operands
    (the HEAD product of csrc/simple_layer.hip is split in every instantiation); exact mode keeps it out (Python gate).  The
    output Linear's weight is lo-heavy and the last LayerNorm's bias lifts every row above zero, so all terms of the head
    product carry the same sign.  Measured: 5.7e-6 / 4.7e-7."""
    from difformer_amd import DIFFormer
    torch.manual_seed(3)
    n, f_in, hidden, classes = 6000, 32, 64, 16
    model = DIFFormer(f_in, hidden, classes, num_layers=1, kernel="simple", use_graph=False).to(dev).eval()
    model.auto_graph = False
    with torch.no_grad():
        model.fcs[1].weight.copy_(t(lo_heavy((classes, hidden), 11, 2.0 ** -3), dev))
        model.fcs[1].bias.zero_()
        model.bns[1].bias.fill_(8.0)
    x = np.random.default_rng(12).standard_normal((n, f_in)).astype(np.float32)
    cfg = dict(hidden_channels=hidden, num_layers=1, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
               use_weight=True, use_graph=False, graph_weight=-1, use_source=False)
    p = {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()}
    ref = orc.difformer_forward(p, x.astype(np.float64), None, None, cfg)
    xd = t(x, dev)

    def run():
        with torch.no_grad():
            return model(xd, None).cpu().numpy()
    outs = both_modes(run)
    check({m: rel_err(o, ref) for m, o in outs.items()}, 1.4e-6, "head folded into the last layer")


# ================================================================== 3: long-row input Linear (csrc/skinny_linear.hip:917-948, HipBackend.linear)
@pytest.mark.parametrize("n,c_in,path,bound", [(32768, 300, "resident", 3.0e-6), (20000, 300, "chunked", 3.2e-6),
                                               (3000, 300, "packed", 1.0e-6), (20000, 301, "packed-unaligned", 1.1e-6)])
def test_long_row_input_linear(n, c_in, path, bound, dev):
    """long_linear_resident_kernel (>= 32,768 aligned rows), long_linear_split_kernel (fewer), the packed-weight K-split
    (dif_linear_packed_f32: < 16,384 rows or unaligned rows; Python gate) -- exact mode: long_linear_kernel /
    long_linear_ksplit_exact_kernel on the fp32 MFMA.  Measured: resident 1.12e-5 / 9.9e-7, chunked 1.11e-5 / 1.06e-6,
    packed 1.10e-5 / 3.5e-7, packed-unaligned 1.12e-5 / 3.7e-7."""
    from difformer_amd import ops
    be = ops.get_backend()
    c_out = 48
    x, W = lo_heavy((n, c_in), n + c_in), lo_heavy((c_out, c_in), 7, 2.0 ** -8)
    b = np.zeros(c_out, np.float32)
    ref = x.astype(np.float64) @ W.astype(np.float64).T
    xd, Wd, bd = t(x, dev), t(W, dev), t(b, dev)
    outs = both_modes(lambda: be.linear(xd, Wd, bd).cpu().numpy())
    check({m: rel_err(o, ref) for m, o in outs.items()}, bound, f"long-row linear {path}")


# ================================================================== 4: wide-output Linear (ops.py:1160-1170)
@pytest.mark.parametrize("c_in,c_out,bound", [(200, 96, 3.1e-6), (512, 300, 3.8e-6)])
def test_wide_output_linear(c_in, c_out, bound, dev):
    """dif_linear_xwide_f32 (split operands; 512 inputs as two accumulating halves) from 16,384 rows, 65..416 outputs, more
    than 128 inputs -- ops.linear_xwide_covers is the gate (Python); exact mode: the vendor GEMM.  Measured: 200 -> 96 1.10e-5 / 1.03e-6; 512 -> 300 1.15e-5 / 1.54e-6
    (B there is 2.5x the exact error: 3x would put 3 B above the default error)."""
    from difformer_amd import autograd_ops as ag
    n = 16384
    x, W = lo_heavy((n, c_in), c_in), lo_heavy((c_out, c_in), c_out, 2.0 ** -8)
    b = np.zeros(c_out, np.float32)
    ref = x.astype(np.float64) @ W.astype(np.float64).T
    xd, Wd, bd = t(x, dev), t(W, dev), t(b, dev)

    def run():
        with torch.no_grad():
            return ag.linear(xd, Wd, bd).cpu().numpy()
    outs = both_modes(run)
    check({m: rel_err(o, ref) for m, o in outs.items()}, bound, f"wide-output linear {c_in}->{c_out}")


# ================================================================== 5: wide closed-form layer kernels (ops.py:1028, :1037)
@pytest.mark.parametrize("c", [128, 300])
def test_wide_closed_form_layer_kernels(c, dev):
    """simple_layer_wide (max(C, D) <= 128) / simple_layer_xwide (129..416) through DIFFormerConv._layer (inference,
    3,000 rows: the Gram record stays on the fp32 kernels in both modes).  Their attention product is 1 / N of the output
    (the +N and sum v of the simple kernel), so the test reads their second product: a graph of self loops makes the
    aggregated rows x itself, and x and Wv are lo-heavy.  Exact mode (Python gate): the operator path at 128 columns
    (ops.CLOSED_FORM_WIDE_MIN), the vendor GEMMs + tail pass at 300.  Measured: C = 128 5.9e-6 / 3.9e-7; C = 300 6.2e-6 / 5.6e-7."""
    from difformer_amd import DIFFormerConv
    n = 3000
    torch.manual_seed(c)
    conv = DIFFormerConv(c, c, 1, kernel="simple", use_graph=True, use_weight=True).to(dev).eval()
    with torch.no_grad():
        conv.Wv.weight.copy_(t(lo_heavy((c, c), c + 1, 2.0 ** -8), dev))
        conv.Wv.bias.zero_()
    x = lo_heavy((n, c), c + 2)
    ei = np.stack([np.arange(n), np.arange(n)])
    p = {"c." + k: v.detach().cpu().double().numpy() for k, v in conv.state_dict().items()}
    cfg = dict(num_heads=1, kernel="simple", use_graph=True, use_weight=True, graph_weight=-1, use_source=False, hidden_channels=c)
    x64 = x.astype(np.float64)
    ref = orc.difformer_conv(p, "c.", x64, x64, ei, None, None, cfg)
    xd, eid = t(x, dev), torch.from_numpy(ei).to(dev)

    def run():
        conv.invalidate_caches()
        with torch.no_grad():
            return conv._layer(xd, xd, eid, None)[0].cpu().numpy()
    outs = both_modes(run)
    check({m: rel_err(o, ref) for m, o in outs.items()}, 1.2e-6 if c <= 128 else 1.7e-6, f"wide closed-form layer C={c}")


# ================================================================== 6: Gram record (csrc/simple_attn.hip:911, HipBackend.gram_sym)
@pytest.mark.parametrize("c", [128, 200])
def test_gram_record(c, dev):
    """gram_slab_kernel (C > 64, >= 4,096 rows) through backend.gram_sym; at 65..128 columns the host picks dif_gram128_f32
    instead under exact mode (Python gate), beyond the library does (simple_reduce_kernel<sym>).  X^T X of lo-heavy rows:
    every entry a positive sum.  Measured: C = 128 1.09e-5 / 1.8e-7; C = 200 1.10e-5 / 2.1e-7."""
    from difformer_amd import ops
    be = ops.get_backend()
    n = 4096
    x = lo_heavy((n, c), c)
    x64 = x.astype(np.float64)
    ref = x64.T @ x64
    blk = np.arange(c) // 64
    upper = blk[:, None] <= blk[None, :]                          # the 64-blocks on and above the diagonal are written
    xd = t(x, dev)
    outs = both_modes(lambda: be.gram_sym(xd)[: c * c].cpu().numpy().reshape(c, c))
    check({m: rel_err(np.where(upper, o, 0.0), np.where(upper, ref, 0.0)) for m, o in outs.items()}, 6e-7,
          f"Gram record C={c}")


# ================================================================== 7: simple attention reduce (csrc/simple_attn.hip:533)
@pytest.mark.parametrize("m,d", [(128, 128), (68, 100)])
def test_simple_attention_reduce(m, d, dev):
    """reduce_slab_kernel: one head of 65..128 columns from 4,096 rows, K^T V on split operands (backend.simple_reduce).
    Measured: 128 x 128 1.12e-5 / 2.3e-7; 68 x 100 1.13e-5 / 2.3e-7."""
    from difformer_amd import ops
    be = ops.get_backend()
    n = 4096
    q, k, v = lo_heavy((n, 1, m), 1), lo_heavy((n, 1, m), 2), lo_heavy((n, 1, d), 3)
    ktv = np.einsum("lhm,lhd->hmd", k.astype(np.float64), v.astype(np.float64)).reshape(-1)
    qd, kd, vd = t(q, dev), t(k, dev), t(v, dev)
    outs = both_modes(lambda: be.simple_reduce(qd, kd, vd)[: m * d].cpu().numpy())
    check({mode: rel_err(o, ktv) for mode, o in outs.items()}, 7e-7, f"simple reduce {m}x{d}")


# ================================================================== 8: simple attention apply (csrc/simple_attn.hip:568)
@pytest.mark.parametrize("m,d", [(128, 128), (96, 72)])
def test_simple_attention_apply(m, d, dev):
    """rowgemm_split in its apply mode (backend.simple_apply): one head, M, D <= 128 (not a single 64-tile), 4,096 rows.  The
    kernel scales K^T V by 1 / (|Q| |K|) before the split: the record's squared norms are 2^-20 each, so that scale is 2^20
    and K^T V stays lo-heavy; it also makes the attention term dominate the +N.  Measured: 128 x 128 1.16e-5 / 7.1e-7; 96 x 72 1.17e-5 / 6.8e-7."""
    from difformer_amd import ops
    be = ops.get_backend()
    n = 4096
    q = lo_heavy((n, 1, m), 5)
    ktv, ksum = lo_heavy((m, d), 6), exact_bf16((m,), 7)
    rec = np.concatenate([ktv.reshape(-1), ksum, np.zeros(d, np.float32), np.float32([2.0 ** -20, 2.0 ** -20])]).astype(np.float32)
    s = 2.0 ** 20
    q64 = q[:, 0, :].astype(np.float64)
    ref = (s * (q64 @ ktv.astype(np.float64))) / (s * (q64 @ ksum.astype(np.float64)) + n)[:, None]
    qd, rd = t(q, dev), t(rec, dev)
    outs = both_modes(lambda: be.simple_apply(qd, rd, n, d).cpu().numpy()[:, 0, :])
    check({mode: rel_err(o, ref) for mode, o in outs.items()}, 2.1e-6, f"simple apply {m}x{d}")


# ================================================================== 9: backward row GEMMs (csrc/simple_attn_bwd.hip:553, :557)
@pytest.mark.parametrize("n,k,c,kernel,bound", [(4096, 128, 96, "rowgemm_split", 2.0e-6), (2048, 200, 160, "rowgemm_wide_split", 2.8e-6)])
def test_backward_row_gemm(n, k, c, kernel, bound, dev):
    """dif_rowgemm_f32 through backend.row_gemm (the simple kernel's backward and autograd_ops' row GEMMs call it): K or C > 64;
    both <= 128 at >= 4,096 rows (rowgemm_split_kernel), wider from 1,024 rows (rowgemm_wide_split_kernel).  Measured: rowgemm_split 1.11e-5 / 6.8e-7; wide 1.12e-5 / 9.2e-7."""
    from difformer_amd import ops
    be = ops.get_backend()
    A, mat = lo_heavy((n, k), k), lo_heavy((k, c), c, 2.0 ** -7)
    ref = A.astype(np.float64) @ mat.astype(np.float64)
    Ad, md = t(A, dev), t(mat, dev)
    outs = both_modes(lambda: be.row_gemm(Ad, md).cpu().numpy())
    check({m: rel_err(o, ref) for m, o in outs.items()}, bound, f"row GEMM {kernel}")


# ================================================================== 10-12: sigmoid attention
def _paired_keys(n, pairs, width, seed):
    """Queries and 2 * pairs keys / values: key 2i = y_i, key 2i+1 = -y_i, value 2i = x_i, value 2i+1 = -x_i (q, x, y
    lo-heavy).  Every score is +-(q . y_i), beyond +-16: sigma is exactly 1 on the even keys and 0 on the odd ones, the
    normaliser is exactly `pairs`, and the column means that the plane kernels subtract (V - mean V) are zero -- the value
    product takes the lo-heavy values as they are.  (With sigma exactly 1 the split drops only the values' own remainder,
    ~5e-6 of the output.)"""
    q = lo_heavy((n, 1, width), seed)
    y, x = lo_heavy((pairs, 1, width), seed + 1), lo_heavy((pairs, 1, width), seed + 2)
    k = np.stack([y, -y], axis=1).reshape(2 * pairs, 1, width)
    v = np.stack([x, -x], axis=1).reshape(2 * pairs, 1, width)
    return q, k, v


@pytest.mark.parametrize("n,pairs,width,path,bound", [(2000, 512, 64, "split sweep <= 64", 4e-7), (2000, 512, 128, "planes 65..512", 5.5e-7),
                                                      (6000, 3000, 64, "planes 33..64 from 2^25 pairs", 5.5e-7)])
def test_sigmoid_inference(n, pairs, width, path, bound, dev):
    """Inference forward (backend.sigmoid_attention, no row sums): sigmoid_attn_kernel<..., SPLIT> up to 64 columns
    (csrc/sigmoid_attn.hip:466), the split-bfloat16 planes of csrc/sigmoid_wide.hip at 65..512 columns and at 33..64 columns
    from 2^25 (query, key) pairs (:461).  Measured: split sweep 4.1e-6 / 1.2e-7; planes 65..512 4.2e-6 / 1.8e-7;
    planes 33..64 4.4e-6 / 1.8e-7."""
    from difformer_amd import ops
    be = ops.get_backend()
    q, k, v = _paired_keys(n, pairs, width, width + n)
    ref = orc.sigmoid_attention_blocked(*(a.astype(np.float64) for a in (q, k, v)))
    qd, kd, vd = t(q, dev), t(k, dev), t(v, dev)

    def run():
        with torch.no_grad():
            return be.sigmoid_attention(qd, kd, vd).cpu().numpy()
    outs = both_modes(run)
    check({m: rel_err(o, ref) for m, o in outs.items()}, bound, f"sigmoid inference {path}")


def _sigmoid_grads(q, k, v, go, dev):
    from difformer_amd import autograd_ops as ag
    leaves = [t(a, dev).requires_grad_(True) for a in (q, k, v)]
    ag.sigmoid_attention(*leaves).backward(t(go, dev))
    return [l.grad.cpu().numpy() for l in leaves]


def _grad_errors(grads, refs):
    gmax = max(float(np.abs(r).max()) for r in refs)
    return max(grad_err(g, r, gmax) for g, r in zip(grads, refs))


def test_sigmoid_backward_wide_planes(dev):
    """Training at 65..512 columns: the backward on the split-bfloat16 planes of csrc/sigmoid_wide.hip in the default mode;
    exact mode keeps the tensor-op gradient (autograd_ops.py:147, Python gate).  512 pairs: the normaliser is 512 exactly,
    so the planes' G / den keeps the lo-heavy cotangent lo-heavy; dv carries the split.  Measured: 4.2e-6 / 1.17e-6.
    This row cannot meet (c) at 3x: the exact mode's gradient is the tensor-op recompute, whose own float32 error (1.2e-6) is
    already a third of what the split costs here.  B = 2.5e-6 still fails a leaked split (4.2e-6) at (b); (c) is held at
    1.5 B."""
    q, k, v = _paired_keys(1024, 512, 128, 77)
    go = lo_heavy((1024, 1, 128), 78)
    refs = orc.sigmoid_attention_grad_blocked(*(a.astype(np.float64) for a in (q, k, v, go)))
    outs = both_modes(lambda: _sigmoid_grads(q, k, v, go, dev))
    check({m: _grad_errors(g, refs) for m, g in outs.items()}, 2.5e-6, "sigmoid backward planes", sens=1.5)


_BWD_SPLIT_CHILD = r'''
import json, sys, numpy as np, torch
sys.path.insert(0, "tests")
from conftest import grad_err
from precision import lo_heavy
from difformer_amd import autograd_ops as ag, ops
from oracle import difformer_oracle as orc
dev = torch.device("cuda:0")
pairs, w = 512, 64
q = lo_heavy((1024, 1, w), 81)
y, x = lo_heavy((pairs, 1, w), 82), lo_heavy((pairs, 1, w), 83)
k = np.stack([y, -y], axis=1).reshape(2 * pairs, 1, w)
v = np.stack([x, -x], axis=1).reshape(2 * pairs, 1, w)
go = lo_heavy((1024, 1, w), 84)
refs = orc.sigmoid_attention_grad_blocked(*(a.astype(np.float64) for a in (q, k, v, go)))
gmax = max(float(np.abs(r).max()) for r in refs)
errs = {}
for exact in (False, True):
    ops.set_exact_fp32(exact)
    leaves = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (q, k, v)]
    ag.sigmoid_attention(*leaves).backward(torch.from_numpy(go).to(dev))
    errs[str(exact)] = max(grad_err(l.grad.cpu().numpy(), r, gmax) for l, r in zip(leaves, refs))
ops.set_exact_fp32(False)
print(json.dumps(errs))
'''


def test_sigmoid_backward_opt_in_split_sweep():
    """sigmoid_bwd_kernel<..., SPLIT> (csrc/sigmoid_attn_bwd.hip:535): the opt-in split backward up to 64 columns
    (DIFFORMER_SIGMOID_BWD_SPLIT=1 is read once per process: a child runs both modes).  Measured: 4.2e-6 / 2.0e-7."""
    r = subprocess.run([sys.executable, "-c", _BWD_SPLIT_CHILD], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, DIFFORMER_SIGMOID_BWD_SPLIT="1"))
    assert r.returncode == 0, r.stderr[-2000:]
    errs = json.loads(r.stdout.strip().splitlines()[-1])
    check({False: errs["False"], True: errs["True"]}, 6e-7, "sigmoid backward opt-in split sweep")


# ================================================================== the switch itself
def test_captured_forward_follows_the_switch(dev):
    """A forward captured by the auto-graph in the default mode must not be replayed after ops.set_exact_fp32(True) (no
    invalidate_caches() in between): the graph key holds the setting.  The first layer's input Linear (300 -> 64, the packed
    split kernel by default) gets lo-heavy rows and, in every other output feature, a lo-heavy weight row, so the two modes
    differ clearly through its LayerNorm."""
    from difformer_amd import DIFFormer, ops
    torch.manual_seed(21)
    n, f_in, hidden = 2000, 300, 64
    model = DIFFormer(f_in, hidden, 8, num_layers=1, kernel="simple", use_graph=False).to(dev).eval()
    with torch.no_grad():
        model.fcs[0].weight.copy_(t(mixed((hidden, f_in), 31, np.arange(0, hidden, 2), axis=0, scale=2.0 ** -6), dev))
    x = t(lo_heavy((n, f_in), 32), dev)
    was = ops.set_exact_fp32(False)
    try:
        with torch.no_grad():
            model.auto_graph = False
            y_def = model(x, None).clone()
            ops.set_exact_fp32(True)
            y_exact = model(x, None).clone()
            ops.set_exact_fp32(False)
            model.auto_graph = True
            for _ in range(4):
                model(x, None)
            assert model._ag_state is not None and model._ag_state[2] is not None, "the forward should have been captured"
            ops.set_exact_fp32(True)
            y = model(x, None).clone()
            ops.set_exact_fp32(False)
            y_back = model(x, None).clone()
    finally:
        ops.set_exact_fp32(was)
    gap = rel_err(y_def.cpu().numpy(), y_exact.cpu().numpy())
    print(f"\n[exact_fp32] captured forward: modes differ by {gap:.3e}")
    assert gap > 1e-7
    assert rel_err(y.cpu().numpy(), y_exact.cpu().numpy()) < 0.1 * gap
    assert rel_err(y_back.cpu().numpy(), y_def.cpu().numpy()) < 0.1 * gap


@pytest.mark.parametrize("width", [64, 300])
@pytest.mark.parametrize("first", [False, True])
def test_sigmoid_backward_after_a_switch(first, width, dev):
    """ops.set_exact_fp32 flipped between a sigmoid forward and its backward: a forward on the plane kernels (65..512 columns,
    default mode) whose backward runs in exact mode takes the tensor-op gradient instead of the refused plane backward; the
    other direction and the 64-column head keep what the forward recorded."""
    from difformer_amd import autograd_ops as ag, ops
    g_ = torch.Generator().manual_seed(width + int(first))
    q, k, v, go = (torch.randn(200, 1, width, generator=g_) * 0.2 for _ in range(4))
    was = ops.set_exact_fp32(first)
    try:
        leaves = [a.to(dev).requires_grad_(True) for a in (q, k, v)]
        out = ag.sigmoid_attention(*leaves)
        ops.set_exact_fp32(not first)
        out.backward(go.to(dev))
    finally:
        ops.set_exact_fp32(was)
    refs = orc.sigmoid_attention_grad_blocked(*(a.double().numpy() for a in (q, k, v, go)))
    gmax = max(float(np.abs(r).max()) for r in refs)
    errs = [grad_err(l.grad.cpu().numpy(), r, gmax) for l, r in zip(leaves, refs)]
    assert max(errs) <= 1e-5, errs
