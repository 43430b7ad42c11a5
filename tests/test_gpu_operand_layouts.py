"""Operand layouts: every HipBackend method that takes row operands, with offset, odd-stride and padded views (part 1),
and the public API on column slices, permuted storage and non-dense gradients (part 2).

The other GPU files hand the library dense operands or views whose rows start on a 16-byte boundary with a leading
dimension that is a multiple of 4.  The layer that deals with everything else -- `_row_major` / `_rows(align=True)` in
difformer_amd/backend_hip.py and the `vec` decisions of the launchers -- runs here.

Part 1, table ROWS: one row per method that calls `_row_major` or `_rows` (tests/test_operand_layouts_host.py holds the
table to that list) = (method, variant, build(dt) -> (CPU operands, run, check), row operands in order, which of them the
Python layer replaces by a dense copy, whether the method declines misplaced rows).  References and tolerances are those of
tests/test_gpu_guarded_inputs.py for the same method (1e-4 float32, 1e-2 bfloat16 storage, norm-wise; gradients against the
step's largest gradient entry).  Shapes: T + 1 rows for the T rows of the method's workgroup, widths 64 (2 heads x 32),
plus the shape at which the launcher's `vec` flag selects another kernel family (and 8,192 nodes x 48 entries per row for
the two methods of the feature-sliced product, which does not exist below that).

Placements of ONE row operand at a time, then of all of them, in tests/guarded.py blocks (pad columns and surroundings NaN):
    off1   payload one element past a 512-byte boundary, ld = width rounded up to a multiple of 4
    ld1    ld = width + 1, first row aligned: the rows cycle through all four alignments
    ld4    ld = width + 4, aligned: the control, stays on the vector path
The dense aligned call runs first; a `copies` operand must give its bits again (same kernel, same values).  A method that
is documented to decline rows it cannot read four at a time returns exactly None for off1 and ld1.

Part 2 (below the sweep): full_attention_conv, gcn_conv, attention_topk, ops.linear, TransConv.full_attention, DIFFormer and
DIFFormerConv on column slices `wide[:, 1:1 + W]` (element offset, odd ld), permuted [H, n, M] storage, `pairs.t()` and
`w2[::2]`, with gradients that arrive as a stride-0 expand, permuted or as a column slice -- against the float64 oracle and
against the same call on .contiguous() clones."""
import numpy as np
import pytest
import torch

import test_gpu_guarded_inputs as gi
from conftest import grad_err, rel_err
from guarded import GuardedArena, guarded_inputs, poisoned_allocations  # noqa: F401
from oracle import difformer_oracle as orc

pytestmark = pytest.mark.gpu

TOL, BF16_TOL = gi.TOL, gi.BF16_TOL
F32, BF16 = torch.float32, torch.bfloat16
FAKE = gi.FAKE
_g, _rn, _d, _tol = gi._g, gi._rn, gi._d, gi._tol
PLACEMENTS = ("off1", "ld1", "ld4")

# Methods with row operands that no row of the table calls, and why.
LEFT_OUT = {}

ROWS = []


def row(method, variant, operands, copies=(), contiguous=(), declines=False, dtypes=(F32,)):
    """copies: operands that go through _rows(align=True) (a dense copy unless aligned with ld % 4 == 0); contiguous: operands
    the method makes .contiguous() (a copy when ld != width); declines: the method returns None for misplaced rows."""
    def add(build):
        for dt in dtypes:
            ROWS.append(dict(id=f"{method}-{variant}-{'f32' if dt == F32 else 'bf16'}",
                             method=method, build=build, dt=dt, operands=tuple(operands), copies=frozenset(copies),
                             contiguous=frozenset(contiguous), declines=declines))
        return build
    return add


# ================================================================== a1
def _simple_qkv(dt, n, h, m):
    g = _g(n + m)
    return _rn(g, n, h, m, dt=dt), _rn(g, n, h, m, dt=dt), _rn(g, n, h, m, dt=dt, shift=0.2)


def _reduce(n, h, m):
    def build(dt):
        q, k, v = _simple_qkv(dt, n, h, m)
        ref = gi._simple_record(_d(q), _d(k), _d(v))
        return (dict(q=q, k=k, v=v), lambda be, d: [be.simple_reduce(d["q"], d["k"], d["v"])],
                lambda o: [("record", o[0][: ref.size], ref, _tol(dt))])
    return build


row("simple_reduce", "65x2x32", "qkv", dtypes=(F32, BF16))(_reduce(65, 2, 32))
row("simple_reduce", "4096x1x128", "qkv", dtypes=(F32, BF16))(_reduce(4096, 1, 128))          # reduce_slab_kernel's threshold


def _apply(n, h, m):
    def build(dt):
        q, k, v = _simple_qkv(dt, n, h, m)
        rec = torch.from_numpy(gi._simple_record(_d(q), _d(k), _d(v)).astype(np.float32))
        ref = _d(FAKE.simple_apply(q.float(), rec, n + 5, m))
        return (dict(q=q, rec=rec), lambda be, d: [be.simple_apply(d["q"], d["rec"], n + 5, m)],
                lambda o: [("out", o[0], ref, _tol(dt))])
    return build


row("simple_apply", "65x2x32", "q", dtypes=(F32, BF16))(_apply(65, 2, 32))
row("simple_apply", "4096x1x128", "q", dtypes=(F32, BF16))(_apply(4096, 1, 128))             # rowgemm_split in apply mode


@row("project_reduce", "65x64->2x32", ("x",), dtypes=(F32, BF16))
def _(dt):
    n, c, h, d = 65, 64, 2, 32
    g = _g(c + d + n)
    x = _rn(g, n, c, dt=dt)
    W = [_rn(g, h * d, c, dt=dt, scale=c ** -0.5) for _ in range(3)]
    b = [_rn(g, h * d, dt=dt, scale=0.3) for _ in range(3)]
    q64, k64, v64 = ((_d(x) @ _d(W[i]).T + _d(b[i])).reshape(n, h, d) for i in range(3))
    ktv = np.einsum("lhm,lhd->hmd", k64, v64)
    names = ("Wq", "bq", "Wk", "bk", "Wv", "bv")
    ops = dict(x=x, Wq=W[0], bq=b[0], Wk=W[1], bk=b[1], Wv=W[2], bv=b[2])
    return (ops, lambda be, d_: list(be.project_reduce(d_["x"], *[d_[k] for k in names], h, d)),
            lambda o: [("q", o[0], q64, _tol(dt)), ("v", o[1], v64, _tol(dt)), ("KtV", o[2][: ktv.size], ktv.ravel(), _tol(dt))])


def _grad_rows(names, got, leaves):
    gmax = max(float(t.grad.abs().max()) for t in leaves)
    return [(f"d{nm}", _d(a) / gmax, _d(b.grad) / gmax, -TOL) for nm, a, b in zip(names, got, leaves)]


@row("simple_backward", "129x2x32", ("q", "k", "v", "out", "g"), contiguous=("out", "g"))
def _(dt):
    n, h, m = 129, 2, 32
    q, k, v = _simple_qkv(dt, n, h, m)
    go = _rn(_g(5), n, h, m)
    l64 = [t.double().requires_grad_(True) for t in (q, k, v)]
    out64 = gi._simple_expr64(*l64)
    out64.backward(go.double())

    def run(be, d):
        rec = be.simple_reduce(d["q"], d["k"], d["v"])
        return list(be.simple_backward(d["q"], d["k"], d["v"], rec, d["out"], d["g"]))
    return dict(q=q, k=k, v=v, out=out64.detach().float().contiguous(), g=go), run, lambda o: _grad_rows("qkv", o, l64)


# ================================================================== a2
def _sigmoid_qkv(dt, n, l, h, m):
    g = _g(n + l + m)
    return _rn(g, n, h, m, dt=dt, scale=3.0 / m ** 0.5), _rn(g, l, h, m, dt=dt, scale=0.5), _rn(g, l, h, m, dt=dt)


def _sigmoid(n, l, h, m, den):
    def build(dt):
        q, k, v = _sigmoid_qkv(dt, n, l, h, m)
        ref = orc.sigmoid_attention(_d(q), _d(k), _d(v))

        def run(be, d):
            if den and dt == F32:
                return list(be.sigmoid_attention(d["q"], d["k"], d["v"], want_den=True))
            return [be.sigmoid_attention(d["q"], d["k"], d["v"])]
        return dict(q=q, k=k, v=v), run, lambda o: [("out", o[0], ref, _tol(dt))]
    return build


row("sigmoid_attention", "129x129x2x32-den", "qkv", dtypes=(F32, BF16))(_sigmoid(129, 129, 2, 32, True))
row("sigmoid_attention", "129x129x1x64", "qkv", dtypes=(F32, BF16))(_sigmoid(129, 129, 1, 64, False))   # split-bf16 kernel: M <= 64, no den


@row("attn_topk", "129x129x2x32", ("q", "k"), copies=("q", "k"))
def _(dt):
    import topk_ref
    n, h, m, top = 129, 2, 32, 8
    q, k, _v = _sigmoid_qkv(dt, n, n, h, m)
    attn = topk_ref.dense_attention(_d(q), _d(k), "sigmoid")
    ref_values, _ = topk_ref.topk_rows(attn, top)

    def check(o):
        values, indices = _d(o[0]), o[1].cpu().numpy().astype(np.int64)
        e1, e2, valid = topk_ref.figures(values, indices, attn, ref_values)
        at = np.take_along_axis(np.transpose(attn, (0, 2, 1)), np.clip(indices, 0, n - 1), axis=2)
        return [("values", values, ref_values, topk_ref.TOL), ("values at indices", values, at, topk_ref.TOL),
                ("indices valid", np.array([float(valid)]), np.ones(1), 0)]
    return dict(q=q, k=k), lambda be, d: list(be.attn_topk(d["q"], d["k"], 1, top)), check


@row("sigmoid_backward", "129x129x2x32", ("q", "k", "v", "g", "out"), contiguous=("out",))
def _(dt):
    n, h, m = 129, 2, 32
    g_ = _g(n + m)
    q, k, v, go = _rn(g_, n, h, m, scale=0.4), _rn(g_, n, h, m, scale=0.4), _rn(g_, n, h, m), _rn(g_, n, h, m)
    refs = orc.sigmoid_attention_grad_blocked(_d(q), _d(k), _d(v), _d(go))
    out64, den64 = orc.sigmoid_attention_blocked(_d(q), _d(k), _d(v), return_den=True)
    gmax = max(np.abs(r).max() for r in refs)
    ops = dict(q=q, k=k, v=v, g=go, out=torch.from_numpy(out64.astype(np.float32)), den=torch.from_numpy(den64.astype(np.float32)))
    return (ops, lambda be, d: list(be.sigmoid_backward(d["q"], d["k"], d["v"], d["out"], d["den"], d["g"])),
            lambda o: [(f"d{nm}", _d(a) / gmax, b / gmax, -TOL) for nm, a, b in zip("qkv", o, refs)])


# ================================================================== f4: batches of graphs
N_NODES = [20, 1, 45, 63]                                                # 129 rows


def _layout_ops():
    from difformer_amd import ops
    lay = ops.BatchLayout(torch.tensor(N_NODES), "cpu")
    return dict(graph_ptr=lay.graph_ptr, ranked_first=lay.ranked_first, pos_count=lay.pos_count)


@row("batched_simple_attention", "129x1x64", "qkv")
def _(dt):
    from oracle import difformer_oracle_grad as og
    q, k, v = _simple_qkv(dt, 129, 1, 64)
    ref = _d(og.v2_simple_attention(q.double(), k.double(), v.double(), torch.tensor(N_NODES)))
    return (dict(q=q, k=k, v=v, **_layout_ops()), lambda be, d: [be.batched_simple_attention(d["q"], d["k"], d["v"], d["graph_ptr"])],
            lambda o: [("out", o[0], ref, TOL)])


def _batched_sigmoid_leaves():
    from oracle import difformer_oracle_grad as og
    g_ = _g(64)
    q, k, v, go = _rn(g_, 129, 1, 64, scale=0.4), _rn(g_, 129, 1, 64, scale=0.4), _rn(g_, 129, 1, 64), _rn(g_, 129, 1, 64)
    l64 = [t.double().requires_grad_(True) for t in (q, k, v)]
    ref = og.v2_sigmoid_attention(*l64, torch.tensor(N_NODES))
    ref.backward(go.double())
    return q, k, v, go, l64, ref.detach()


@row("batched_sigmoid_attention", "129x1x64", "qkv")
def _(dt):
    q, k, v, _go, _l, ref = _batched_sigmoid_leaves()
    return (dict(q=q, k=k, v=v, **_layout_ops()),
            lambda be, d: [be.batched_sigmoid_attention(d["q"], d["k"], d["v"], d["ranked_first"], d["pos_count"])],
            lambda o: [("out", o[0], _d(ref), TOL)])


@row("batched_sigmoid_backward", "129x1x64", ("q", "k", "v", "out", "g"), contiguous=("out", "g"))
def _(dt):
    q, k, v, go, l64, ref = _batched_sigmoid_leaves()

    def run(be, d):
        _out, den = be.batched_sigmoid_attention(d["q"], d["k"], d["v"], d["ranked_first"], d["pos_count"], want_den=True)
        return list(be.batched_sigmoid_backward(d["q"], d["k"], d["v"], d["out"], den, d["g"], d["ranked_first"], d["pos_count"]))
    # per tensor, as tests/test_gpu_guarded_inputs.py holds this entry point for a batch of several graphs
    return (dict(q=q, k=k, v=v, out=ref.float(), g=go, **_layout_ops()), run,
            lambda o: [(f"d{nm}", _d(a) / float(b.grad.abs().max()), _d(b.grad) / float(b.grad.abs().max()), -TOL)
                       for nm, a, b in zip("qkv", o, l64)])


# ================================================================== a3
@row("edge_weight_grad", "129x64", ("g", "x"))
def _(dt):
    n, F = 129, 64
    ei = gi._graph(n, 5, n + F)
    g_ = _g(n)
    w = torch.rand(ei.shape[1], generator=g_) + 0.5
    gr, x = _rn(g_, n, F), _rn(g_, n, F)
    rp = gi._csr(ei, w, n)[0]
    ref = _d(FAKE.edge_weight_grad(ei, w, rp, n, gr, x, 1.5))
    return (dict(edge_index=ei, edge_weight=w, rowptr=rp, g=gr, x=x),
            lambda be, d: [be.edge_weight_grad(d["edge_index"], d["edge_weight"], d["rowptr"], n, d["g"], d["x"], 1.5)],
            lambda o: [("dw", o[0], ref, TOL)])


def _spmm(tail):
    def build(dt):
        n, F, nb = 257, 64, 3 if tail else 1
        ei = gi._graph(n, 6, F + nb, hubs=4 if tail else 0)
        g_ = _g(F)
        x, a = _rn(g_, n, F, dt=dt), _rn(g_, n, F, dt=dt)
        rp, blk, src, val, nnz = gi._csr(ei, None, n, nb)
        ops = dict(rowptr=rp, blkptr=blk, src=src, val=val, x=x, attn=a)
        t = None
        if tail:
            t = dict(x0=_rn(g_, n, F, dt=dt), prev=_rn(g_, n, F, dt=dt), alpha=0.4, ln_weight=(torch.rand(F, generator=g_) + 0.5).to(dt),
                     ln_bias=_rn(g_, F, dt=dt), eps=1e-5, relu=True)
            ops.update(x0=t["x0"], prev=t["prev"], ln_weight=t["ln_weight"], ln_bias=t["ln_bias"])
        ref = gi._spmm_ref(x, ei, a, t)

        def run(be, d):
            td = dict(t, x0=d["x0"], prev=d["prev"], ln_weight=d["ln_weight"], ln_bias=d["ln_bias"]) if tail else None
            return [be.spmm(d["rowptr"], d["blkptr"], nb, d["src"], d["val"], n, nnz, d["x"], 0, n, d["attn"], 0.5, 2.0, td, None)]
        return ops, run, lambda o: [("out", o[0], ref, (2 if tail else 1) * _tol(dt))]
    return build


row("spmm", "257x64", ("x", "attn"), dtypes=(F32, BF16))(_spmm(False))
row("spmm", "257x64-blocked-tail", ("x", "attn", "x0", "prev"), dtypes=(F32, BF16))(_spmm(True))


def _sliced(which):
    """The smallest graph that takes the feature-sliced product (8,192 nodes x 48 entries per row, every degree 48), as
    tests/test_gpu_guarded_inputs.py::_sliced: x of sliced_prescale and attn of sliced_spmm."""
    def build(dt):
        n, F = 8192, 64
        g_ = _g(1)
        ei = torch.stack([torch.cat([torch.randint(0, n, (n * 47,), generator=g_), torch.arange(n)]),
                          torch.cat([torch.arange(n).repeat_interleave(47), torch.arange(n)])])
        x, a = _rn(g_, n, F), _rn(g_, n, F)
        ys_ref = (_d(x) * 48.0 ** -0.5).reshape(n, F // 4, 4).transpose(1, 0, 2)            # slice-major, rows scaled by deg^-1/2
        ref = gi._spmm_ref(x, ei, a)

        def run(be, d):
            from difformer_amd import ops
            csr = ops.csr_cache.get(d["edge_index"], None, n, F * 4)
            sl = csr.sliced(0, n, F)
            assert sl is not None
            ys = be.sliced_prescale(d["x"], csr.rowptr, n, sl.plan)
            out = None if which == "prescale" else be.sliced_spmm(sl, ys, csr.rowptr, n, 0, n, F, d["attn"], 0.5, 2.0)
            ops.csr_cache.drop(d["edge_index"])
            return [ys[:, :n, :]] if which == "prescale" else [out]
        return (dict(edge_index=ei, x=x, attn=a), run,
                lambda o: [("ys", o[0], ys_ref, TOL)] if which == "prescale" else [("out", o[0], ref, TOL)])
    return build


row("sliced_prescale", "8192x64", ("x",), copies=("x",))(_sliced("prescale"))
row("sliced_spmm", "8192x64", ("attn",), copies=("attn",))(_sliced("spmm"))


# ================================================================== the closed form: records, coefficients, layers
@row("gram", "65x64", ("x",), copies=("x",), dtypes=(F32, BF16))
def _(dt):
    x = _rn(_g(65), 65, 64, dt=dt, shift=0.3)
    ref = gi._record_ref(_d(x))
    return dict(x=x), lambda be, d: [be.gram(d["x"])[0]], lambda o: [("record", o[0][: ref.size], ref, _tol(dt))]


@row("input_gram", "65x64->64", ("x",))
def _(dt):
    n, c, d_ = 65, 64, 64
    g_ = _g(n + c)
    x, W, b = _rn(g_, n, c), _rn(g_, d_, c, scale=c ** -0.5), _rn(g_, d_)
    lw, lb = torch.rand(d_, generator=g_) + 0.5, _rn(g_, d_)
    h64 = np.maximum(orc.layer_norm(_d(x) @ _d(W).T + _d(b), _d(lw), _d(lb)), 0.0)
    ref = gi._record_ref(h64)
    return (dict(x=x, weight=W, bias=b, ln_weight=lw, ln_bias=lb),
            lambda be, d: list(be.input_gram(d["x"], d["weight"], d["bias"], d["ln_weight"], d["ln_bias"], 1e-5, True)[:2]),
            lambda o: [("h", o[0], h64, TOL), ("record", o[1][: ref.size], ref, TOL)])


_WB = ("Wq", "bq", "Wk", "bk", "Wv", "bv")


def _coef_case(n=65, c=64, d_=64):
    g_ = _g(n + c)
    x = _rn(g_, n, c, shift=0.2)
    wb = gi._coef_params(g_, c, d_)
    rec = torch.from_numpy(np.concatenate([gi._record_ref(_d(x)), [0.0, 0.0]]).astype(np.float32))
    coef = FAKE.simple_coeffs(rec, n, c, d_, *wb, 0.7)
    return x, wb, rec, coef


def _coef_rows(how, got, want, c, d_):
    return [(f"{how} {nm}", a, b, TOL) for (nm, a), (_, b) in zip(gi._coef_parts(got, c, d_), gi._coef_parts(want, c, d_))]


@row("gram_coeffs", "65x64", ("x",), copies=("x",))
def _(dt):
    x, wb, rec, coef = _coef_case()
    ref = gi._record_ref(_d(x))
    return (dict(x=x, **dict(zip(_WB, wb))), lambda be, d: list(be.gram_coeffs(d["x"], 65, 64, 64, *[d[k] for k in _WB], 0.7)),
            lambda o: [("record", o[0][: ref.size], ref, TOL)] + _coef_rows("coef", o[1], _d(coef), 64, 64))


@row("coeffs_bg", "65x64", ("x",), copies=("x",))
def _(dt):
    from difformer_amd import ops as pkg_ops
    x, wb, rec, coef = _coef_case()

    def run(be, d):
        return [be.coeffs_bg(d["x"], None, 65, pkg_ops.NarrowFactors(*[d[k] for k in _WB]), 64, 64, 0.7)]
    return dict(x=x, **dict(zip(_WB, wb))), run, lambda o: _coef_rows("coef", o[0], _d(coef), 64, 64)


def _row_gemm(n, K, C):
    def build(dt):
        g_ = _g(n + K)
        A, mat, bias, acc = _rn(g_, n, K), _rn(g_, K, C, scale=K ** -0.5), _rn(g_, C), _rn(g_, n, C)
        ref = _d(A) @ _d(mat)
        return (dict(A=A, mat=mat, bias=bias, accumulate=acc),
                lambda be, d: [be.row_gemm(d["A"], d["mat"], d["bias"], d["accumulate"]), be.row_gemm(d["A"], d["mat"])],
                lambda o: [("full", o[0], ref + _d(bias) + _d(acc), TOL), ("plain", o[1], ref, TOL)])
    return build


row("row_gemm", "129x64x64", ("A", "accumulate"))(_row_gemm(129, 64, 64))
row("row_gemm", "4096x128x128", ("A", "accumulate"))(_row_gemm(4096, 128, 128))              # rowgemm_split's threshold
row("row_gemm", "1024x132x196", ("A", "accumulate"))(_row_gemm(1024, 132, 196))


@row("closed_form_attn_backward", "65x64", ("x", "d", "dx_in"), declines=True)
def _(dt):
    n, c, d_ = 65, 64, 64
    g_ = _g(n + c)
    x, dd, dx_in, rs = _rn(g_, n, c), _rn(g_, n, d_), _rn(g_, n, c), torch.rand(n, generator=g_)
    coef = _rn(g_, d_ * c + d_ + c + 4, scale=0.2)
    coef[d_ * c + d_ + c] = 25.0
    cf, x64, d64 = _d(coef), _d(x), _d(dd)
    MnT, cn, u, cdn = cf[: d_ * c].reshape(d_, c), cf[d_ * c: d_ * c + d_], cf[d_ * c + d_: d_ * c + d_ + c], cf[d_ * c + d_ + c]
    den = x64 @ u + cdn
    att = (x64 @ MnT.T + cn) / den[:, None]
    d_num = d64 / den[:, None]
    d_den = -(d64 * att).sum(1) / den
    dx = _d(dx_in) + d_num @ MnT + d_den[:, None] * u[None, :]
    refs = (d_num, d_den, dx, x64.T @ d_den, np.array([d_den.sum()]), _d(rs) @ d64)
    names = ("d_num", "d_den", "dx", "d_u", "d_cd", "rs_d")

    def run(be, d):
        got = be.closed_form_attn_backward(d["x"], d["coef"], d_, d["d"], d["dx_in"], d["row_sums"])
        return None if got is None else list(got)
    return (dict(x=x, coef=coef, d=dd, dx_in=dx_in, row_sums=rs), run,
            lambda o: [(nm, a.reshape(b.shape), b, TOL) for nm, a, b in zip(names, o, refs)])


@row("simple_layer", "65x64", ("x", "ax", "x0"), copies=("x", "ax", "x0"), dtypes=(F32, BF16))
def _(dt):
    n, c = 65, 64
    x, wb, rec, coef = _coef_case()
    g_ = _g(3)
    ax, x0, Wv, bv, rs = _rn(g_, n, c), _rn(g_, n, c), _rn(g_, c, c, scale=c ** -0.5), _rn(g_, c, scale=0.3), torch.rand(n, generator=g_)
    lw, lb = torch.rand(c, generator=g_) + 0.5, _rn(g_, c)
    x, ax, x0 = x.to(dt), ax.to(dt), x0.to(dt)
    kw = dict(gcn_scale=1.3, residual=True, alpha=0.4, eps=1e-5, relu=True)
    ref = _d(FAKE.simple_layer(x.float(), coef, c, ax=ax.float(), Wv=Wv, bv=bv, row_sums=rs, x0=x0.float(), ln_weight=lw, ln_bias=lb, **kw))

    def run(be, d):
        return [be.simple_layer(d["x"], d["coef"], c, ax=d["ax"], Wv=d["Wv"], bv=d["bv"], row_sums=d["rs"], x0=d["x0"],
                                ln_weight=d["lw"], ln_bias=d["lb"], **kw)]
    return dict(x=x, coef=coef, ax=ax, Wv=Wv, bv=bv, rs=rs, x0=x0, lw=lw, lb=lb), run, lambda o: [("out", o[0], ref, _tol(dt))]


@row("gram_sym", "65x128", ("x",))
def _(dt):
    n, c = 65, 128
    x = _rn(_g(n + c), n, c, shift=0.3)
    x64 = _d(x)
    blk = np.arange(c) // 64

    def check(o):
        got = _d(o[0][: c * c]).reshape(c, c)
        got = np.where(blk[:, None] <= blk[None, :], got, got.T)              # blocks on and above the diagonal are valid
        return [("X^T X", got, x64.T @ x64, TOL), ("sums", o[0][c * c: c * c + c], x64.sum(0), TOL)]
    return dict(x=x), lambda be, d: [be.gram_sym(d["x"])], check


def _mix_ref(num, den, conv_scale, add, add_scale, rs, bv, x0, prev, alpha, lw, lb, relu):
    z = conv_scale * num / den[:, None] + add_scale * (_d(add) + _d(rs)[:, None] * _d(bv)[None, :])
    z = alpha * (z + _d(x0)) + (1.0 - alpha) * _d(prev)
    z = orc.layer_norm(z, _d(lw), _d(lb))
    return np.maximum(z, 0.0) if relu else z


@row("layer_tail_mix", "257x64", ("add", "x0", "prev"), copies=("add", "x0", "prev"))
def _(dt):
    n, D = 257, 64
    g_ = _g(D + n)
    Z = _rn(g_, n, D + 4)
    Z[:, D] = torch.rand(n, generator=g_) + 1.0
    add, rs, bv, x0, prev = _rn(g_, n, D), torch.rand(n, generator=g_), _rn(g_, D), _rn(g_, n, D), _rn(g_, n, D)
    lw, lb = torch.rand(D, generator=g_) + 0.5, _rn(g_, D)
    ref = _mix_ref(_d(Z[:, :D]), _d(Z[:, D]), 0.7, add, 1.3, rs, bv, x0, prev, 0.4, lw, lb, False)

    def run(be, d):
        return [be.layer_tail_mix(d["Z"], D, D, 0.7, d["add"], 1.3, d["rs"], d["bv"], d["x0"], d["prev"], 0.4, d["lw"], d["lb"], 1e-5)]
    return dict(Z=Z, add=add, rs=rs, bv=bv, x0=x0, prev=prev, lw=lw, lb=lb), run, lambda o: [("out", o[0], ref, TOL)]


def _wide(method, n, C):
    def build(dt):
        D = C
        g_ = _g(n + C)
        x, ax, x0 = _rn(g_, n, C), _rn(g_, n, C), _rn(g_, n, C)
        B, bias = _rn(g_, C, D + 4, scale=0.2 * C ** -0.5), _rn(g_, D + 4, scale=0.2)
        bias[D] = 25.0
        Wv, bv, rs = _rn(g_, D, C, scale=C ** -0.5), _rn(g_, D, scale=0.3), torch.rand(n, generator=g_)
        lw, lb = torch.rand(D, generator=g_) + 0.5, _rn(g_, D)
        Z = _d(x) @ _d(B) + _d(bias)
        ref = _mix_ref(Z[:, :D], Z[:, D], 0.7, torch.from_numpy(_d(ax) @ _d(Wv).T), 1.3, rs, bv, x0, x, 0.4, lw, lb, False)

        def run(be, d):
            return [getattr(be, method)(d["x"], d["B"], d["bias"], D, 0.7, d["ax"], d["Wv"], d["bv"], d["rs"], 1.3, d["x0"], True, 0.4,
                                        d["lw"], d["lb"], 1e-5)]
        return dict(x=x, B=B, bias=bias, ax=ax, Wv=Wv, bv=bv, rs=rs, x0=x0, lw=lw, lb=lb), run, lambda o: [("out", o[0], ref, TOL)]
    return build


row("_simple_layer_wide", "wide-257x128", ("x", "ax", "x0"), copies=("x", "ax", "x0"))(_wide("simple_layer_wide", 257, 128))
row("_simple_layer_wide", "xwide-129x132", ("x", "ax", "x0"), copies=("x", "ax", "x0"))(_wide("simple_layer_xwide", 129, 132))


# ================================================================== Linear layers and tails
def _linear(n, ci, co):
    def build(dt):
        g_ = _g(n + ci)
        x, w, b = _rn(g_, n, ci, dt=dt), _rn(g_, co, ci, dt=dt, scale=ci ** -0.5), _rn(g_, co, dt=dt)
        lw, lb = (torch.rand(co, generator=g_) + 0.5).to(dt), _rn(g_, co, dt=dt)

        def run(be, d):
            return [be.linear(d["x"], d["w"], d["b"]), be.linear(d["x"], d["w"], d["b"], d["lw"], d["lb"], 1e-5, True)]
        return (dict(x=x, w=w, b=b, lw=lw, lb=lb), run,
                lambda o: [("plain", o[0], gi._linear_ref(x, w, b, None, None, False), _tol(dt)),
                           ("LN ReLU", o[1], gi._linear_ref(x, w, b, lw, lb, True), _tol(dt))])
    return build


row("linear", "129x64->64", ("x",), dtypes=(F32, BF16))(_linear(129, 64, 64))
row("linear", "16384x132->64", ("x",), copies=("x",))(_linear(16384, 132, 64))               # aligned long-row Linear's threshold (C > 128: copied)


def _tail_ops(dt, n, H, D):
    g_ = _g(D * 10 + H)
    conv, x0, prev = _rn(g_, n, H, D, dt=dt), _rn(g_, n, D, dt=dt), _rn(g_, n, D, dt=dt)
    return conv, x0, prev, (torch.rand(D, generator=g_) + 0.5).to(dt), _rn(g_, D, dt=dt), _rn(g_, n, D)


@row("layer_tail", "65x2x32", ("conv", "x0", "prev"), dtypes=(F32, BF16))
def _(dt):
    conv, x0, prev, lw, lb, _go = _tail_ops(dt, 65, 2, 32)
    ref = gi._tail_ref(conv, x0, prev, 0.4, lw, lb, True)
    return (dict(conv=conv, x0=x0, prev=prev, lw=lw, lb=lb),
            lambda be, d: [be.layer_tail(d["conv"], d["x0"], d["prev"], 0.4, d["lw"], d["lb"], 1e-5, True)],
            lambda o: [("out", o[0], ref, _tol(dt))])


@row("layer_tail_bwd", "65x2x32", ("conv", "grad_out", "x0", "prev"), declines=True)
def _(dt):
    conv, x0, prev, lw, lb, go = _tail_ops(dt, 65, 2, 32)
    leaves = [t.double().requires_grad_(True) for t in (conv, x0, prev, lw, lb)]
    z = 0.4 * (leaves[0].mean(dim=1) + leaves[1]) + 0.6 * leaves[2]
    torch.nn.functional.layer_norm(z, (32,), leaves[3], leaves[4], 1e-5).backward(go.double())
    names = ("d_conv", "d_x0", "d_prev", "d_ln_weight", "d_ln_bias")

    def run(be, d):
        got = be.layer_tail_bwd(d["conv"], d["x0"], d["prev"], 0.4, d["lw"], d["lb"], 1e-5, False, d["grad_out"], (True, True, True, True))
        return None if got is None else list(got)
    return (dict(conv=conv, x0=x0, prev=prev, lw=lw, lb=lb, grad_out=go), run,
            lambda o: [(nm, a, _d(b.grad), TOL) for nm, a, b in zip(names, o, leaves)])


# ================================================================== part 1: the sweep
def _place(arena, dev, t, placement):
    """CPU tensor [rows, ...] -> its copy on `dev` in a guarded block at `placement`."""
    width, item = t.numel() // t.shape[0], t.element_size()
    ld = {"off1": -(-width // 4) * 4, "ld1": width + 1, "ld4": width + 4}[placement]
    d = arena.alloc(t.shape, t.dtype, dev, ld=ld, offset_bytes=item if placement == "off1" else 0, site=f"placed({placement})")
    d.copy_(t)
    assert d.stride(0) == ld and (d.data_ptr() % 512 == (item if placement == "off1" else 0))
    return d


def _device_operands(arena, dev, cpu_ops, placed, placement):
    out = {}
    for name, t in cpu_ops.items():
        if t is None:
            out[name] = None
        elif name in placed:
            out[name] = _place(arena, dev, t, placement)
        else:
            out[name], = guarded_inputs(arena, dev, **{name: t})
    return out


def _judge(tag, results):
    """The criterion of tests/test_gpu_guarded_inputs.py: tol > 0 norm-wise, tol < 0 pre-scaled absolute, 0 exact; finite."""
    failures = []
    for label, got, ref, tol in results:
        got = _d(got) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
        ref = np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (tag, label, got.shape, ref.shape)
        finite = bool(np.isfinite(got).all())
        if tol == 0:
            ok = np.array_equal(got, ref)
            err = float(not ok)
        elif tol < 0:
            err = float(np.max(np.abs(got - ref))) if ref.size else 0.0
            ok = err < -tol
        else:
            err = rel_err(got, ref)
            ok = err < tol
        print(f"{tag} {label}: err {err:.3e} (tol {abs(tol):.0e}) finite={finite}")
        if not (ok and finite):
            failures.append((tag, label, err, finite))
    return failures


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _launch(tag, run, be, operands):
    """run(be, operands); a fault of the device ends the whole session here -- nothing more is started on a GPU that faulted."""
    try:
        outs = run(be, operands)
        torch.cuda.synchronize()
        return outs
    except RuntimeError as e:
        # a launcher that rejects its arguments (DifformerHipError with a negative DIF_E_* code) is an ordinary failure of
        # the case; a positive code is a hipError_t
        if getattr(e, "code", 0) > 0 or (getattr(e, "code", 0) == 0 and ("HIP error" in str(e) or "illegal memory access" in str(e))):
            pytest.exit(f"{tag}: the device faulted ({e}); find the cause in the launcher before running again", returncode=3)
        raise


def _same_bits(a, b):
    """torch.equal on the bytes: entries a kernel leaves unwritten (the two spare floats of a Gram record) hold the poison,
    a NaN that no value comparison calls equal to itself."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


DENSE = {}                                                                  # row id -> the dense call's outputs (CPU copies)
BUILT = {}                                                                  # row id -> build(dt): operands and reference, made once


def _built(r):
    if r["id"] not in BUILT:
        BUILT[r["id"]] = r["build"](r["dt"])
    return BUILT[r["id"]]


def _dense(r, be, dev):
    if r["id"] not in DENSE:
        cpu_ops, run, check = _built(r)
        inputs = GuardedArena()
        outs = _launch(f"{r['id']}[dense]", run, be, _device_operands(inputs, dev, cpu_ops, (), None))
        inputs.check()
        assert outs is not None, f"{r['id']}: the dense call declined"
        failures = _judge(f"{r['id']}[dense]", check(outs))
        assert not failures, failures
        DENSE[r["id"]] = [o.detach().cpu().clone() for o in outs]
    return DENSE[r["id"]]


@pytest.mark.parametrize("r", ROWS, ids=[r["id"] for r in ROWS])
def test_dense_control(r, dev, poisoned_allocations):
    """The dense aligned call of every row, first in the file: the value the placements are compared with."""
    from difformer_amd import ops
    DENSE.pop(r["id"], None)
    _dense(r, ops.get_backend(), dev)


@pytest.mark.parametrize("placement", PLACEMENTS)
@pytest.mark.parametrize("r", ROWS, ids=[r["id"] for r in ROWS])
def test_row_operand_placements(r, placement, dev, poisoned_allocations):
    from difformer_amd import ops
    be = ops.get_backend()
    dense = _dense(r, be, dev)
    cpu_ops, run, check = _built(r)
    failures = []
    for placed in [(name,) for name in r["operands"]] + [tuple(r["operands"])]:
        tag = f"{r['id']}[{placement}:{'+'.join(placed)}]"
        inputs = GuardedArena()
        outs = _launch(tag, run, be, _device_operands(inputs, dev, cpu_ops, placed, placement))   # a raise fails the test: every view is legal
        inputs.check()
        if r["declines"] and placement != "ld4":
            assert outs is None, f"{tag}: documented to decline rows that are not 16-byte aligned with ld % 4 == 0"
            print(f"{tag}: declined")
            continue
        assert outs is not None, f"{tag}: declined an aligned view"
        failures += _judge(tag, check(outs))
        # the Python layer hands the kernel a dense copy (or, at ld4, the same rows at another stride): the same bits
        same = all(name in r["copies"] or (name in r["contiguous"] and placement != "off1") for name in placed)
        if same:
            for i, (a, b) in enumerate(zip(outs, dense)):
                if not _same_bits(a.detach().cpu(), b):
                    failures.append((tag, f"output {i} differs from the dense call's bits"))
    assert not failures, failures


# ================================================================== part 2: the public API on views
# n = 129 rows, hidden 64 (2 heads x 32); graphs of 129 nodes x 6 entries per row plus self loops.  Every call is held to the
# float64 oracle (1e-4 norm-wise; gradients: conftest.grad_err with the step's largest entry) AND to the same call on
# .contiguous() clones (the same 1e-4: a view may take another kernel family, so the bits may differ).
N2, H2, M2 = 129, 2, 32
W2 = H2 * M2
NAN = float("nan")


def _column_view(t, dev, requires_grad=False, left=1, right=2):
    """layout (a): t [n, ...] as columns [left, left + W) of a NaN-filled [n, left + W + right] leaf: an element offset and an
    odd leading dimension -> (wide leaf, view shaped like t)."""
    n, width = t.shape[0], t.numel() // t.shape[0]
    wide = torch.full((n, left + width + right), NAN, dtype=t.dtype)
    wide[:, left: left + width] = t.reshape(n, width)
    wide = wide.to(dev).requires_grad_(requires_grad)
    return wide, wide[:, left: left + width].view(t.shape)


def _permuted_view(t, dev, requires_grad=False):
    """layout (b): t [n, H, M] stored as [H, n, M] -> (storage leaf, its .permute(1, 0, 2))."""
    store = t.permute(1, 0, 2).contiguous().to(dev).requires_grad_(requires_grad)
    return store, store.permute(1, 0, 2)


def _graph_views(n, dev, seed, weighted=True):
    """layout (c): edge_index = pairs.t() of an [E, 2] tensor, edge_weight = w2[::2] -> (ei CPU, w CPU, pairs.t(), w2 leaf, view)."""
    ei = gi._graph(n, 6, seed)
    w = torch.rand(ei.shape[1], generator=_g(seed)) + 0.5
    pairs = ei.t().contiguous().to(dev)
    w2 = torch.full((2 * ei.shape[1],), NAN)
    w2[::2] = w
    w2 = w2.to(dev).requires_grad_(weighted)
    assert not pairs.t().is_contiguous() and not w2[::2].is_contiguous()
    return ei, w, pairs.t(), w2, w2[::2]


def _gradient_views(kind, G, dev):
    """A gradient for `out.backward(...)` that is not dense: permuted storage, or a column slice of a wider buffer."""
    if kind == "permuted":
        dims = list(range(G.dim()))
        dims[0], dims[-1] = dims[-1], dims[0]
        g = G.permute(*dims).contiguous().to(dev).permute(*dims)
    else:
        g = _column_view(G, dev)[1]
    assert not g.is_contiguous() and g.shape == G.shape
    return g


def _backward(out, kind, G, dev):
    """kind 'sum': out.sum().backward(), whose gradient is a stride-0 expand (G must be ones); else backward(view of G)."""
    if kind == "sum":
        out.sum().backward()
    elif kind == "dense":
        out.backward(G.to(dev))
    else:
        out.backward(_gradient_views(kind, G, dev))


def _G(kind, shape, seed=11):
    return torch.ones(shape) if kind == "sum" else _rn(_g(seed), *shape)


def _hold(tag, got, ref, tol=TOL):
    err = rel_err(_d(got), np.asarray(ref, dtype=np.float64))
    print(f"{tag}: err {err:.3e} (tol {tol:.0e})")
    assert np.isfinite(_d(got)).all() and err < tol, (tag, err)


def _hold_grads(tag, named):
    """named: [(name, got, float64 reference)] of ONE backward pass: grad_err against the step's largest entry."""
    gmax = max(float(np.abs(_d(ref)).max()) for _, _, ref in named)
    bad = []
    for name, got, ref in named:
        err = grad_err(_d(got), _d(ref), gmax)
        print(f"{tag} d{name}: err {err:.3e} (tol {TOL:.0e})")
        if not (np.isfinite(_d(got)).all() and err < TOL):
            bad.append((tag, name, err))
    assert not bad, bad


def _slice_grad(wide, left, width, shape):
    """gradient of a layout-(a) leaf -> its slice, after asserting it is exactly zero outside the slice"""
    g = wide.grad
    assert g is not None and g.shape == wide.shape
    outside = torch.cat([g[:, :left], g[:, left + width:]], dim=1)
    assert bool((outside == 0).all()), "gradient outside the slice of the wide leaf"
    return g[:, left: left + width].reshape(shape)


def _attn_operands(kernel):
    return _simple_qkv(F32, N2, H2, M2) if kernel == "simple" else _sigmoid_qkv(F32, N2, N2, H2, M2)


def _attn_reference(kernel, q, k, v, G):
    from oracle import difformer_oracle_grad as og
    l64 = [t.double().requires_grad_(True) for t in (q, k, v)]
    ref = og.full_attention_conv(*l64, kernel)
    ref.backward(G.double())
    return ref.detach(), [t.grad for t in l64]


@pytest.mark.parametrize("layout,grad", [("slices", "dense"), ("one_buffer_kqv", "dense"), ("permuted", "dense"), ("slices", "sum"),
                                         ("slices", "permuted"), ("slices", "slice")])
@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_full_attention_conv_on_views(kernel, layout, grad, dev, poisoned_allocations, monkeypatch):
    """Forward and backward with q, k, v as (a) column slices of three wide leaves, as three slices k | q | v of ONE leaf
    with gaps between them, and (b) as permuted [H, n, M] storage; the gradient arrives dense, as a stride-0 expand, permuted
    or as a column slice.  Gradients reach the leaves: the oracle's inside the slices, exactly zero outside."""
    from difformer_amd import autograd_ops as ag, full_attention_conv
    q, k, v = _attn_operands(kernel)
    G = _G(grad, (N2, H2, M2))
    ref, ref_grads = _attn_reference(kernel, q, k, v, G)
    fired = []
    real = ag._adjacent_columns
    monkeypatch.setattr(ag, "_adjacent_columns", lambda *a: fired.append(real(*a)) or fired[-1])
    if layout == "slices":
        leaves, views = zip(*[_column_view(t, dev, True) for t in (q, k, v)])
        grads_of = lambda: [_slice_grad(w, 1, W2, (N2, H2, M2)) for w in leaves]
    elif layout == "one_buffer_kqv":
        # [gap 1 | k | gap 3 | q | gap 2 | v | gap 1] through split_columns, the package's own slicing of a fused projection
        wide = torch.full((N2, 3 * W2 + 7), NAN)
        offs = {"k": 1, "q": 1 + W2 + 3, "v": 1 + 2 * W2 + 5}
        for name, t in (("q", q), ("k", k), ("v", v)):
            wide[:, offs[name]: offs[name] + W2] = t.reshape(N2, W2)
        wide = wide.to(dev).requires_grad_(True)
        cols = ag.split_columns(wide, 1, W2, 3, W2, 2, W2, 1)
        views = [cols[3].view(N2, H2, M2), cols[1].view(N2, H2, M2), cols[5].view(N2, H2, M2)]

        def grads_of():
            g = wide.grad
            keep = torch.zeros(wide.shape[1], dtype=torch.bool)
            for o in offs.values():
                keep[o: o + W2] = True
            assert bool((g[:, ~keep.to(dev)] == 0).all()), "gradient in a gap of the wide leaf"
            return [g[:, offs[nm]: offs[nm] + W2].reshape(N2, H2, M2) for nm in "qkv"]
    else:
        leaves, views = zip(*[_permuted_view(t, dev, True) for t in (q, k, v)])
        grads_of = lambda: [s.grad.permute(1, 0, 2) for s in leaves]
    out = full_attention_conv(*views, kernel)
    _hold(f"{kernel} {layout} out", out, ref)
    with torch.no_grad():
        dense = full_attention_conv(*[t.detach().contiguous() for t in views], kernel)
    _hold(f"{kernel} {layout} out vs contiguous clones", out, _d(dense))
    _backward(out, grad, G, dev)
    _hold_grads(f"{kernel} {layout} grad={grad}", list(zip("qkv", grads_of(), ref_grads)))
    assert all(f is None for f in fired), "the fused-gradient shortcut fired for slices that are not adjacent"


@pytest.mark.parametrize("grad", ["dense", "sum", "permuted", "slice"])
def test_gcn_conv_on_views(grad, dev, poisoned_allocations):
    """x as a column slice, edge_index = pairs.t(), edge_weight = w2[::2]: forward, dx into the wide leaf, dw into w2."""
    from difformer_amd import gcn_conv, ops
    from oracle import difformer_oracle_grad as og
    x = _rn(_g(4), N2, H2, M2)
    ei, w, ei_view, w2, w_view = _graph_views(N2, dev, 21)
    G = _G(grad, (N2, H2, M2))
    x64, w64 = x.double().requires_grad_(True), w.double().requires_grad_(True)
    ref = og.gcn_conv(x64, ei, w64)
    ref.backward(G.double())
    wide, xv = _column_view(x, dev, True)
    out = gcn_conv(xv, ei_view, w_view)
    _hold("gcn_conv out", out, _d(ref))
    with torch.no_grad():
        dense = gcn_conv(xv.detach().contiguous(), ei_view.contiguous(), w_view.detach().contiguous())
    _hold("gcn_conv out vs contiguous clones", out, _d(dense))
    _backward(out, grad, G, dev)
    assert bool((w2.grad[1::2] == 0).all()), "gradient between the entries of the strided edge_weight"
    _hold_grads(f"gcn_conv grad={grad}", [("x", _slice_grad(wide, 1, W2, (N2, H2, M2)), x64.grad), ("w", w2.grad[::2], w64.grad)])
    ops.csr_cache.clear()


@pytest.mark.parametrize("layout", ["slices", "permuted"])
@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_attention_topk_on_views(kernel, layout, dev, poisoned_allocations):
    import topk_ref
    from difformer_amd.attention_maps import attention_topk
    q, k, _v = _attn_operands(kernel)
    make = _column_view if layout == "slices" else _permuted_view
    qv, kv = make(q, dev)[1], make(k, dev)[1]
    attn = topk_ref.dense_attention(_d(q), _d(k), kernel)
    values, indices = attention_topk(qv, kv, kernel, 8)
    topk_ref.check_topk(values.cpu().numpy(), indices.cpu().numpy(), attn, 8, f"{kernel} {layout}")
    dv, di = attention_topk(qv.contiguous(), kv.contiguous(), kernel, 8)
    _hold(f"topk {kernel} {layout} values vs contiguous clones", values, _d(dv))


@pytest.mark.parametrize("ci", [64, 132])
def test_ops_linear_on_views(ci, dev, poisoned_allocations):
    """ops.linear with x as a column slice: the skinny kernel (C_in <= 128: rows as they are) and the long-row path
    (C_in > 128: rows copied to a 4-element boundary)."""
    from difformer_amd import ops
    g_ = _g(ci)
    x, w, b = _rn(g_, N2, ci), _rn(g_, 64, ci, scale=ci ** -0.5), _rn(g_, 64)
    lw, lb = torch.rand(64, generator=g_) + 0.5, _rn(g_, 64)
    xv = _column_view(x, dev)[1]
    wd, bd, lwd, lbd = (t.to(dev) for t in (w, b, lw, lb))
    for tag, args, ref in (("plain", (), gi._linear_ref(x, w, b, None, None, False)),
                           ("LN ReLU", (lwd, lbd, 1e-5, True), gi._linear_ref(x, w, b, lw, lb, True))):
        out = ops.linear(xv, wd, bd, *args)
        _hold(f"linear {ci}->64 {tag}", out, ref)
        _hold(f"linear {ci}->64 {tag} vs contiguous clone", out, _d(ops.linear(xv.contiguous(), wd, bd, *args)))


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_v2_full_attention_on_views(kernel, dev, poisoned_allocations):
    """difformer_v2.TransConv.full_attention over a batch of four graphs with q, k, v as column slices, forward and backward."""
    from difformer_amd.difformer_v2 import TransConv
    from oracle import difformer_oracle_grad as og
    g_ = _g(64)
    q, k, v, G = (_rn(g_, N2, 1, 64, scale=0.4), _rn(g_, N2, 1, 64, scale=0.4), _rn(g_, N2, 1, 64), _rn(g_, N2, 1, 64))
    n_nodes = torch.tensor(N_NODES)
    l64 = [t.double().requires_grad_(True) for t in (q, k, v)]
    ref = (og.v2_simple_attention if kernel == "simple" else og.v2_sigmoid_attention)(*l64, n_nodes)
    ref.backward(G.double())
    conv = TransConv(64, 64, kernel=kernel).to(dev)
    leaves, views = zip(*[_column_view(t, dev, True) for t in (q, k, v)])
    out = conv.full_attention(*views, kernel, n_nodes.to(dev))
    _hold(f"v2 {kernel} out", out, _d(ref))
    with torch.no_grad():
        dense = conv.full_attention(*[t.detach().contiguous() for t in views], kernel, n_nodes.to(dev))
    _hold(f"v2 {kernel} out vs contiguous clones", out, _d(dense))
    out.backward(_gradient_views("slice", G, dev))
    # as tests/test_gpu_guarded_inputs.py holds the batched kernels: simple against the step's largest entry, sigmoid (a
    # batch of several graphs) per tensor
    gmax = max(float(t.grad.abs().max()) for t in l64)
    for nm, w, t in zip("qkv", leaves, l64):
        got, want = _d(_slice_grad(w, 1, 64, (N2, 1, 64))), _d(t.grad)
        err = float(np.abs(got - want).max() / (gmax if kernel == "simple" else np.abs(want).max()))
        print(f"v2 {kernel} d{nm}: err {err:.3e}")
        assert np.isfinite(got).all() and err < TOL, (kernel, nm, err)


def _model_cfg(hidden, kernel, **kw):
    cfg = dict(hidden_channels=hidden, num_layers=2, num_heads=1, kernel=kernel, alpha=0.5, use_bn=True, use_residual=True,
               use_weight=True, use_graph=True, graph_weight=-1, use_source=False)
    cfg.update(kw)
    return cfg


@pytest.mark.parametrize("grad", [None, "sum", "permuted", "slice"])
@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_model_on_views(kernel, grad, dev, poisoned_allocations):
    """DIFFormer.forward with x as a column slice and the graph as pairs.t(): eval() against the oracle; train() with the
    gradient of the logits arriving as a stride-0 expand, permuted and as a column slice, every parameter gradient and dx
    into the wide leaf against float64 autograd."""
    from difformer_amd import DIFFormer, ops
    from oracle import difformer_oracle_grad as og
    f_in, hidden, classes = 24, 64, 10
    torch.manual_seed(5)
    model = DIFFormer(f_in, hidden, classes, num_layers=2, num_heads=1, kernel=kernel, dropout=0.0)
    cfg = _model_cfg(hidden, kernel)
    sd = {k_: v_.clone() for k_, v_ in model.state_dict().items()}
    model = model.to(dev)
    x = _rn(_g(7), N2, f_in)
    ei, _w, ei_view, _w2, _wv = _graph_views(N2, dev, 22, weighted=False)
    wide, xv = _column_view(x, dev, grad is not None)
    if grad is None:
        model.eval()
        with torch.no_grad():
            out = model(xv, ei_view)
            dense = model(xv.contiguous(), ei_view.contiguous())
        ref = orc.difformer_forward({k_: _d(v_) for k_, v_ in sd.items()}, _d(x), ei.numpy(), None, cfg)
        _hold(f"model {kernel} logits", out, ref)
        _hold(f"model {kernel} logits vs contiguous clones", out, _d(dense))
    else:
        model.train()
        G = _G(grad, (N2, classes))
        pl = og.leaves({k_: v_.numpy() for k_, v_ in sd.items()})
        x64 = x.double().requires_grad_(True)
        og.difformer_forward(pl, x64, ei, None, cfg).backward(G.double())
        out = model(xv, ei_view)
        _backward(out, grad, G, dev)
        named = [(k_, p.grad, pl[k_].grad) for k_, p in model.named_parameters()]
        _hold_grads(f"model {kernel} grad={grad}", named + [("x", _slice_grad(wide, 1, f_in, (N2, f_in)), x64.grad)])
    ops.csr_cache.clear()


@pytest.mark.parametrize("route,hidden,n,train", [("closed_narrow", 64, N2, False), ("closed_train", 64, N2, True),
                                                   ("closed_wide", 128, 513, False)])
def test_conv_closed_form_routes_on_views(route, hidden, n, train, dev, poisoned_allocations, monkeypatch):
    """DIFFormerConv.forward with query_input = source_input and x_0 as column slices (element offset, odd leading
    dimension) on each closed-form route that hidden 64 and hidden 128 reach (tests/golden/layer_routes.txt; the wide route
    starts at n = 4 C rows): the operands reach simple_layer / layer_tail_mix / coeffs_bg as the caller passed them."""
    from difformer_amd import DIFFormerConv, ops
    from oracle import difformer_oracle_grad as og
    torch.manual_seed(hidden)
    conv = DIFFormerConv(hidden, hidden, 1, kernel="simple", use_source=True)
    cfg = _model_cfg(hidden, "simple", use_source=True)
    sd = {k_: v_.clone() for k_, v_ in conv.state_dict().items()}
    conv = conv.to(dev)
    conv.train(train)
    for p in conv.parameters():
        p.requires_grad_(train)
    x, x0 = _rn(_g(1), n, hidden), _rn(_g(2), n, hidden)
    ei, _w, ei_view, _w2, _wv = _graph_views(n, dev, 23, weighted=False)
    wide, xv = _column_view(x, dev, train)
    wide0, x0v = _column_view(x0, dev, train)
    routes = []
    real = DIFFormerConv._route
    monkeypatch.setattr(DIFFormerConv, "_route", lambda self, *a: routes.append(real(self, *a)) or routes[-1])
    pl = og.leaves({k_: v_.numpy() for k_, v_ in sd.items()})
    x64, x064 = x.double().requires_grad_(True), x0.double().requires_grad_(True)
    ref = og.difformer_conv(pl, "", x64, x64, ei, None, x064, cfg)
    out = conv(xv, xv, ei_view, None, x0v)
    assert routes == [route], routes
    _hold(f"{route} out", out, _d(ref))
    with torch.no_grad():
        xc = xv.detach().contiguous()
        dense = conv(xc, xc, ei_view.contiguous(), None, x0v.detach().contiguous())
    _hold(f"{route} out vs contiguous clones", out, _d(dense))
    if train:
        G = _rn(_g(3), n, hidden)
        ref.backward(G.double())
        out.backward(_gradient_views("slice", G, dev))
        named = [(k_, p.grad, pl[k_].grad) for k_, p in conv.named_parameters()]
        named += [("x", _slice_grad(wide, 1, hidden, (n, hidden)), x64.grad), ("x0", _slice_grad(wide0, 1, hidden, (n, hidden)), x064.grad)]
        _hold_grads(f"{route} grad", named)
    ops.csr_cache.clear()


@pytest.mark.parametrize("grad", ["sum", "permuted", "slice"])
def test_layer_tail_with_gradients_that_arrive_non_dense(grad, dev, poisoned_allocations):
    """The layer-tail path (autograd_ops.layer_tail -> dif_layer_tail_bwd_f32, which declines rows it cannot read four at
    a time and leaves the gradient to tensor ops): conv, x0, prev as column slices."""
    from difformer_amd import autograd_ops as ag
    conv, x0, prev, lw, lb, _go = _tail_ops(F32, N2, H2, M2)
    G = _G(grad, (N2, M2))
    leaves64 = [t.double().requires_grad_(True) for t in (conv, x0, prev, lw, lb)]
    z = 0.4 * (leaves64[0].mean(dim=1) + leaves64[1]) + 0.6 * leaves64[2]
    ref = torch.nn.functional.layer_norm(z, (M2,), leaves64[3], leaves64[4], 1e-5)
    ref.backward(G.double())
    (wc, cv), (w0, x0v), (wp, pv) = (_column_view(t, dev, True) for t in (conv, x0, prev))
    lwd, lbd = lw.to(dev).requires_grad_(True), lb.to(dev).requires_grad_(True)
    out = ag.layer_tail(cv, x0v, pv, 0.4, lwd, lbd, 1e-5)
    _hold("layer_tail out", out, _d(ref))
    _backward(out, grad, G, dev)
    named = [("conv", _slice_grad(wc, 1, W2, (N2, H2, M2)), leaves64[0].grad), ("x0", _slice_grad(w0, 1, M2, (N2, M2)), leaves64[1].grad),
             ("prev", _slice_grad(wp, 1, M2, (N2, M2)), leaves64[2].grad), ("ln_weight", lwd.grad, leaves64[3].grad),
             ("ln_bias", lbd.grad, leaves64[4].grad)]
    # each tensor against itself, as tests/test_gpu_guarded_inputs.py holds dif_layer_tail_bwd_f32
    for nm, got, want in named:
        _hold(f"layer_tail grad={grad} d{nm}", got, _d(want))
