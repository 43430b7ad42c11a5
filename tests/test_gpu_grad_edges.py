"""Gradient parity of every HIP backward path at the row counts where its launch arithmetic changes state: one row, one
short of / exactly / one past a tile, a workgroup's rows or a split of the swept side (tests/grad_edges.py holds the tables
and says which state each shape reaches).

Every op-level case runs with a dense upstream gradient and with two spotlight ones (only the last row; only the first row
of the last 16-row tile), so that a dropped, doubled or misplaced boundary row is a 100 % error in every gradient that sums
over rows.  Yardstick, metric and bar are the project's: float64 autograd of the oracle, conftest.grad_err against the
largest gradient entry of the case, TOL = 1e-4; the 1e-2 floor goes only to the gradients that vanish identically
(tests/test_grad_edges_host.py holds that, and that the float32 run of the oracle itself meets TOL / 4 on every case).
Each test asserts that the HIP entry point under test ran, and prints one `edge | case | pattern | tensor | hip | f32-oracle`
line per gradient before it asserts (profiles/r09_backward_edges.txt is that output).
"""
import numpy as np
import pytest
import torch

import grad_edges as ge
from grad_edges import TOL

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def be():
    from difformer_amd import ops
    return ops.get_backend()


def _np(t):
    return t.detach().cpu().numpy()


def _leaves(problem, dev):
    return {k: v.to(dev).requires_grad_(True) for k, v in problem.leaves.items()}


def _grads(t):
    return {k: (np.zeros(tuple(v.shape)) if v.grad is None else _np(v.grad)) for k, v in t.items()}


# ---- the HIP side of each family: (problem, cotangent on the device) -> (out, {leaf: gradient}) ------------------------
def _run_attention(p, cot, dev):
    from difformer_amd import full_attention_conv
    t = _leaves(p, dev)
    out = full_attention_conv(t["q"], t["k"], t["v"], p.consts["kernel"])
    out.backward(cot)
    return _np(out), _grads(t)


def _run_tail(p, cot, dev):
    from difformer_amd import autograd_ops as ag
    t = _leaves(p, dev)
    out = ag.layer_tail(t["conv"], t.get("x0"), t.get("prev"), ge.TAIL_ALPHA, t.get("w"), t.get("b"), 1e-5, p.consts["relu"])
    out.backward(cot)
    return _np(out), _grads(t)


def _run_linear_reduce(p, cot, dev):
    """_Linear itself: d_W = g^T x and d_b = colsum(g) from stage 1 of the simple kernel (ag.linear takes it from 1,024 rows)."""
    from difformer_amd import autograd_ops as ag
    t = _leaves(p, dev)
    out = ag._Linear.apply(t["x"], t["w"], t["b"])
    out.backward(cot)
    return _np(out), _grads(t)


def _run_linear(p, cot, dev):
    from difformer_amd import autograd_ops as ag
    t = _leaves(p, dev)
    out = ag.linear(t["x"], t["w"], t["b"])
    out.backward(cot)
    return _np(out), _grads(t)


def _run_gcn(p, cot, dev):
    from difformer_amd import gcn_conv
    t = _leaves(p, dev)
    out = gcn_conv(t["x"], p.consts["edge_index"].to(dev), t.get("w"))
    out.backward(cot)
    return _np(out), _grads(t)


def _run_batched(p, cot, dev):
    from difformer_amd.difformer_v2 import TransConv
    t = _leaves(p, dev)
    H, D = p.leaves["q"].shape[1:]
    conv = TransConv(D, D, num_heads=H, kernel=p.consts["kernel"]).to(dev)
    out = conv.full_attention(t["q"], t["k"], t["v"], p.consts["kernel"], torch.tensor(p.consts["n_nodes"]))
    out.backward(cot)
    return _np(out), _grads(t)


def _sweep(problem, run, required, be, dev, forbidden=(), tag=""):
    """The three cotangent patterns of one case: figures printed, then the bar, the route and the forward asserted."""
    failures = []
    for pattern in ge.PATTERNS:
        cot = problem.cotangent(pattern)
        out64, ref64 = problem.reference(cot)
        _, ref32 = problem.reference(cot, torch.float32)
        with ge.entry_points(be) as ran:
            out, got = run(problem, cot.to(dev), dev)
            torch.cuda.synchronize()
        errs = ge.errors(got, ref64, problem.floored)
        ge.report(problem, pattern + tag, errs, ge.errors(ref32, ref64, problem.floored))
        if not set(required) <= ran.symbols or set(forbidden) & ran.symbols:
            failures.append((pattern, "route", sorted(ran.symbols)))
        fwd = ge.rel_err(out, out64)
        if not fwd < TOL:
            failures.append((pattern, "forward", fwd))
        failures += [(pattern, k, e) for k, e in errs.items() if not e < TOL]
    assert not failures, failures


# ---- a / b: sigmoid ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ge.SIGMOID_NARROW, ids=lambda c: f"N{c.N}-L{c.L}-H{c.H}-M{c.M}-D{c.D}-S{c.S0}x{c.S1}")
def test_sigmoid_backward_edges(case, dev, be):
    """dif_sigmoid_attn_bwd_f32, heads up to 64 columns: 32 stationary rows per workgroup, 16-row tiles of the swept side over
    8 waves and sweep_splits() splits, partial results folded by sum_parts_kernel."""
    _sweep(ge.sigmoid_problem(case.N, case.L, case.H, case.M, case.D), _run_attention, {"dif_sigmoid_attn_bwd_f32"}, be, dev)


@pytest.mark.parametrize("N,L,H,M,D", ge.SIGMOID_WIDE)
def test_sigmoid_plane_backward_edges(N, L, H, M, D, dev, be):
    """The same entry point on the split-bfloat16 plane kernels (65 .. 512 columns; never under set_exact_fp32(True))."""
    from difformer_amd import ops
    assert not ops.EXACT_FP32
    _sweep(ge.sigmoid_problem(N, L, H, M, D, family="sigmoid-wide"), _run_attention, {"dif_sigmoid_attn_bwd_f32"}, be, dev)


# ---- c: simple ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,M,D", ge.SIMPLE)
def test_simple_backward_edges(N, H, M, D, dev, be):
    """simple_backward: dif_simple_bwd_prep_f32 (vector / scalar / two-chunk prep, look-ahead fetch clamped at the end, records
    rounded to a multiple of H) + the streaming reduce + three dif_rowgemm_f32 launches."""
    _sweep(ge.simple_problem(N, H, M, D), _run_attention, {"dif_simple_bwd_prep_f32", "dif_rowgemm_f32"}, be, dev)


# ---- d: layer tail -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,H,D,use_x0,use_prev,use_ln,relu", ge.tail_cases())
def test_layer_tail_backward_edges(n, H, D, use_x0, use_prev, use_ln, relu, dev, be):
    """dif_layer_tail_bwd_f32 at 1, R - 1, R, R + 1 and 2 R + 1 rows, R = 256 / tail_group(D) rows per workgroup: the fold of
    the row slots into a workgroup's record and the finalize pass over the records (d_ln_weight, d_ln_bias)."""
    _sweep(ge.tail_problem(n, H, D, use_x0, use_prev, use_ln, relu), _run_tail, {"dif_layer_tail_bwd_f32"}, be, dev)


# ---- e: Linear ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,ci,co", ge.LINEAR)
def test_linear_gradient_edges(n, ci, co, dev, be):
    """_Linear.backward on the reduce kernel at a handful of rows, and ag.linear's own route at the same shapes."""
    problem = ge.linear_problem(n, ci, co)
    _sweep(problem, _run_linear_reduce, {"dif_simple_reduce_f32"}, be, dev, tag=" (reduce kernel)")
    _sweep(problem, _run_linear, (), be, dev, tag=" (ag.linear)")


# ---- g: aggregation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", ge.gcn_problems(), ids=lambda p: p.name)
def test_aggregation_gradient_edges(problem, dev, be):
    """gcn_conv: dx through the adjoint product, d edge_weight through dif_gcn_edge_weight_grad_f32 (16 lanes per edge, 16
    edges per workgroup; NaN exactly where the reference's is)."""
    _sweep(problem, _run_gcn, {"dif_gcn_edge_weight_grad_f32"}, be, dev)


# ---- h: batched attention ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", ge.batched_problems(), ids=lambda p: p.name)
def test_batched_attention_backward_edges(problem, dev, be):
    """TransConv.full_attention of DIFFormer_v2: dif_batched_sigmoid_attn_bwd_f32; dif_batched_simple_raw_f32 (the batched
    `simple` backward: three launches of the forward kernel's raw mode) -- which _BatchedAttention takes from two graphs on:
    a batch of one graph re-derives its gradient with tensor ops by design, and must not reach the kernel."""
    if problem.consts["kernel"] == "sigmoid":
        required, forbidden = {"dif_batched_sigmoid_attn_bwd_f32"}, ()
    elif len(problem.consts["n_nodes"]) > 1:
        required, forbidden = {"dif_batched_simple_raw_f32"}, ()
    else:
        required, forbidden = (), {"dif_batched_simple_raw_f32"}
    _sweep(problem, _run_batched, required, be, dev, forbidden)


# ---- f: closed form ----------------------------------------------------------------------------------------------------
def _closed_form(be, dev, x, coef, dd, dx0, rs, D):
    got = be.closed_form_attn_backward(x.to(dev), coef.to(dev), D, dd.to(dev), None if dx0 is None else dx0.to(dev), rs.to(dev))
    assert got is not None, "closed_form_attn_backward does not cover the shape"
    torch.cuda.synchronize()
    return {k: _np(v) for k, v in zip(ge.CF_TENSORS, got)}


def _coeffs(be, dev, n, C, D):
    """-> (record of dif_gram_f32, gradients of dif_simple_coeffs_bwd_f32, float64 tensor-op gradients from the same record)."""
    from difformer_amd import ops
    x, p, a, dcoef = ge.coeff_operands(n, C, D)
    pd = {k: v.to(dev) for k, v in p.items()}
    args = (pd["Wq"], pd["bq"], pd["Wk"], pd["bk"], pd["Wv"], pd["bv"], a)
    rec, _ = be.gram(x.to(dev))
    coef = be.simple_coeffs(rec, n, C, D, *args)
    dc = dcoef.to(dev)
    got = be.simple_coeffs_backward(rec, n, C, D, *args, coef, dc)
    ref = ops.closed_form_coeffs_backward(rec, n, C, D, *args, dc[: D * C].view(D, C), dc[D * C: D * C + D],
                                          dc[D * C + D: D * C + D + C], dc[D * C + D + C])
    torch.cuda.synchronize()
    return _np(rec), dict(zip(ge.CC_TENSORS, map(_np, got))), {k: _np(v).astype(np.float64) for k, v in zip(ge.CC_TENSORS, ref)}


@pytest.mark.parametrize("n,C,D,with_dx", ge.CLOSED_FORM)
def test_closed_form_backward_edges(n, C, D, with_dx, dev, be):
    """dif_closed_form_attn_bwd_f32 (d_num, d_den, dx and the per-workgroup partial records the host sums: x^T d_den,
    sum d_den, row_sums^T d) and dif_simple_coeffs_bwd_f32 on the record of n rows, with the reference constructions of
    tests/test_gpu_closed_form.py."""
    failures = []
    x, coef, dx0, rs = ge.closed_form_operands(n, C, D, with_dx)
    name = f"closed-form/n{n}-C{C}-D{D}" + ("-dx" if with_dx else "")
    for pattern in ge.PATTERNS:
        dd = ge.cotangent((n, D), pattern, 5)
        ref64 = ge.closed_form_reference(x, coef, dd, dx0, rs, D)
        ref32 = ge.closed_form_reference(x, coef, dd, dx0, rs, D, torch.float32)
        with ge.entry_points(be) as ran:
            got = _closed_form(be, dev, x, coef, dd, dx0, rs, D)
        errs = ge.errors(got, ref64)
        ge.report(name, pattern, errs, ge.errors(ref32, ref64))
        if "dif_closed_form_attn_bwd_f32" not in ran.symbols:
            failures.append((pattern, "route", sorted(ran.symbols)))
        failures += [(pattern, k, e) for k, e in errs.items() if not e < TOL]
    with ge.entry_points(be) as ran:
        rec, got, ref64 = _coeffs(be, dev, n, C, D)
    xc, p, a, dcoef = ge.coeff_operands(n, C, D)
    host_rec = ge.gram_record(xc)
    auto64 = ge.coeffs_autograd(host_rec, n, C, D, p, a, dcoef, torch.float64)
    auto32 = ge.coeffs_autograd(host_rec, n, C, D, p, a, dcoef, torch.float32)
    errs = ge.errors(got, ref64)
    ge.report(f"coeffs/n{n}-C{C}-D{D}", "-", errs, ge.errors(auto32, auto64))
    rec_err = ge.rel_err(rec[: C * C + C], host_rec.numpy())
    print(f"edge | coeffs/n{n}-C{C}-D{D} | - | gram record | hip {rec_err:.2e} | f32-oracle nan")
    if "dif_simple_coeffs_bwd_f32" not in ran.symbols:
        failures.append(("coeffs", "route", sorted(ran.symbols)))
    failures += [("coeffs", k, e) for k, e in errs.items() if not e < TOL]
    if not rec_err < TOL:
        failures.append(("coeffs", "gram record", rec_err))
    assert not failures, failures


# ---- i: whole training step --------------------------------------------------------------------------------------------
def _step(n, kernel, hidden, heads, dev):
    model = ge.step_model(kernel, hidden, heads, n).to(dev)
    x, ei, y = ge.step_graph(n)
    return model, x, ei, y, x.to(dev).requires_grad_(True), ei.to(dev), y.to(dev)


def _step_grads(model, xd):
    got = {k: (np.zeros(tuple(p.shape)) if p.grad is None else _np(p.grad)) for k, p in model.named_parameters()}
    got["x"] = _np(xd.grad)
    return got


@pytest.mark.parametrize("kernel,hidden,heads", ge.STEP_CONFIGS)
@pytest.mark.parametrize("n", ge.STEP_NODES)
def test_whole_training_step_edges(n, kernel, hidden, heads, dev, be):
    """One training step (tests/test_gpu_grad.py _check_step) on 3 .. 65 nodes, every node in the loss: `simple` at one head of
    64 columns trains through the Gram record, everything else on the q / k / v operators; none of them on the whole-model
    kernels for tiny graphs (those stop at 8 hidden columns)."""
    from difformer_amd import tiny
    from test_gpu_grad import _check_step
    cfg = ge.step_cfg(kernel, hidden, heads)
    model, x, ei, y, xd, eid, yd = _step(n, kernel, hidden, heads, dev)
    assert tiny._plan(model, xd, eid, None) is None
    ref64 = ge.step_reference(model.state_dict(), x, ei, y, cfg)
    ref32 = ge.step_reference(model.state_dict(), x, ei, y, cfg, torch.float32)
    with ge.entry_points(be) as ran:
        try:
            _check_step(model, xd, eid, cfg, yd, torch.arange(n, device=dev))
        finally:
            if xd.grad is not None:                      # the figures first, whatever _check_step found
                ge.report(f"step/{kernel}-h{hidden}x{heads}-N{n}", "loss", ge.errors(_step_grads(model, xd), ref64),
                          ge.errors(ref32, ref64))
    assert not {s for s in ran.symbols if s.startswith("dif_tiny_forward") or s.startswith("dif_tiny_backward")}
    if kernel == "simple" and heads == 1 and hidden <= 64:
        assert ran.labels & {"dif_gram_f32", "dif_gram_coeffs_f32"} and "dif_simple_apply_f32" not in ran.labels, ran.labels
        assert {"dif_closed_form_attn_bwd_f32", "dif_simple_coeffs_bwd_f32", "dif_layer_tail_bwd_f32"} <= ran.symbols, ran.symbols
    elif kernel == "simple":
        assert "dif_simple_apply_f32" in ran.labels, ran.labels
        assert {"dif_simple_bwd_prep_f32", "dif_rowgemm_f32", "dif_layer_tail_bwd_f32"} <= ran.symbols, ran.symbols
    else:
        assert {"dif_sigmoid_attn_bwd_f32", "dif_layer_tail_bwd_f32"} <= ran.symbols, ran.symbols


# ---- determinism: every fold of these kernels has a fixed order ---------------------------------------------------------
_TWICE = {
    "sigmoid": (lambda: ge.sigmoid_problem(129, 400, 3, 20, 20), _run_attention),
    "sigmoid-wide": (lambda: ge.sigmoid_problem(63, 129, 1, 300, 300, family="sigmoid-wide"), _run_attention),
    "simple": (lambda: ge.simple_problem(257, 2, 16, 16), _run_attention),
    "tail": (lambda: ge.tail_problem(33, 2, 64, True, True, True, False), _run_tail),
    "linear": (lambda: ge.linear_problem(65, 64, 192), _run_linear_reduce),
    "gcn": (lambda: ge.gcn_problems()[-1], _run_gcn),
    "batched-sigmoid": (lambda: ge.batched_problem("sigmoid", [1, 40, 1, 16, 17], 2, 16), _run_batched),
    "batched-simple": (lambda: ge.batched_problem("simple", [1, 40, 1, 16, 17], 1, 64), _run_batched),
}


@pytest.mark.parametrize("family", sorted(_TWICE))
def test_backward_twice_gives_the_same_bits(family, dev):
    make, run = _TWICE[family]
    problem = make()
    cot = problem.cotangent("dense").to(dev)
    first, second = run(problem, cot, dev), run(problem, cot, dev)
    assert np.array_equal(first[0], second[0])
    for k in first[1]:
        assert np.array_equal(first[1][k], second[1][k], equal_nan=True), k


def test_closed_form_backward_twice_gives_the_same_bits(dev, be):
    n, C, D = 65, 64, 64
    x, coef, dx0, rs = ge.closed_form_operands(n, C, D, True)
    dd = ge.cotangent((n, D), "dense", 5)
    first, second = (_closed_form(be, dev, x, coef, dd, dx0, rs, D) for _ in range(2))
    assert all(np.array_equal(first[k], second[k]) for k in first)
    first, second = (_coeffs(be, dev, n, C, D) for _ in range(2))
    assert np.array_equal(first[0], second[0]) and all(np.array_equal(first[1][k], second[1][k]) for k in first[1])


@pytest.mark.parametrize("kernel,hidden,heads", [("simple", 64, 1), ("sigmoid", 32, 2)])
def test_training_step_twice_gives_the_same_bits(kernel, hidden, heads, dev):
    import torch.nn.functional as F
    n = 65
    model, _, _, _, xd, eid, yd = _step(n, kernel, hidden, heads, dev)
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        xd.grad = None
        F.nll_loss(F.log_softmax(model(xd, eid), dim=1), yd).backward()
        runs.append(_step_grads(model, xd))
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k
