"""The case tables of the backward edge sweep (tests/grad_edges.py), checked without a GPU:
  * every case is well-posed -- the float32 run of the oracle expression sits within TOL / 4 of the float64 run under the
    metric the GPU test uses, so a miss on the GPU is the kernel's and not the arithmetic's;
  * the 1e-2 floor goes to exactly the gradients whose float64 reference vanishes (below 1e-12 of the case's largest);
  * the split pairs annotated in the sigmoid table, and the rows per workgroup of the layer-tail table, are what the
    library's own host functions give: if a launch heuristic changes, the shapes have to be picked again.
"""
import pytest
import torch

import grad_edges as ge

PROBLEMS = ge.op_problems()


@pytest.mark.parametrize("problem", PROBLEMS, ids=repr)
def test_float32_oracle_meets_the_precondition(problem):
    for pattern in ge.PATTERNS:
        cot = problem.cotangent(pattern)
        out64, ref64 = problem.reference(cot)
        out32, ref32 = problem.reference(cot, torch.float32)
        assert ge.rel_err(out32, out64) < ge.PRECONDITION, pattern
        errs = ge.errors(ref32, ref64, problem.floored)
        assert max(errs.values()) < ge.PRECONDITION, (pattern, errs)
        # the floor is no general escape: exactly the identically vanishing gradients have it
        assert ge.vanishing(ref64) == problem.floored, (pattern, sorted(ge.vanishing(ref64)), sorted(problem.floored))


def test_tables_cover_what_they_claim():
    names = [repr(p) for p in PROBLEMS]
    assert len(set(names)) == len(names)
    assert {c[0] for c in ge.SIMPLE} == {1, 2, 3, 15, 16, 17, 63, 64, 65, 257}
    assert {c[1:] for c in ge.SIMPLE} == {(1, 64, 64), (2, 16, 16), (3, 10, 10), (1, 128, 128), (1, 300, 300), (2, 100, 36), (3, 12, 12)}
    tails = ge.tail_cases()
    for D in ge.TAIL_WIDTHS:
        R = ge.tail_rows(D)
        assert {c[0] for c in tails if c[2] == D} == {1, R - 1, R, R + 1, 2 * R + 1}
        assert any(c[5] for c in tails if c[2] == D)                      # a LayerNorm: the record fold and finalize run
        assert {c[1] for c in tails if c[2] == D} == {1, 2}
    assert {c[3:] for c in tails} == set(ge._TAIL_FLAGS)
    assert {c[3] for c in ge.CLOSED_FORM} == {True, False}
    # the spotlight rows: last row, first row of the last 16-row tile
    assert [ge.spot_row(n, "tile") for n in (1, 16, 17, 32, 33, 257)] == [0, 0, 16, 16, 32, 256]
    for pattern in ("last", "tile"):
        g = ge.cotangent((33, 2, 4), pattern, 3)
        assert g[ge.spot_row(33, pattern)].abs().min() > 0 and int((g.abs().sum(dim=(1, 2)) > 0).sum()) == 1


@pytest.mark.parametrize("case", ge.SIGMOID_NARROW, ids=lambda c: f"N{c.N}-L{c.L}-H{c.H}-M{c.M}-D{c.D}")
def test_sigmoid_split_annotations_match_the_library(case):
    """dif_sigmoid_bwd_workspace_bytes is a plain host function: its size for a shape is the launcher's formula for the split
    pair sweep_splits picks.  A mismatch means the heuristic moved and the table no longer reaches the states it names."""
    from difformer_amd import _lib
    got = int(_lib.load().dif_sigmoid_bwd_workspace_bytes(case.N, case.L, case.H, case.M, case.D))
    assert got == ge.sigmoid_workspace_bytes(case), (
        f"{case}: the library sizes its workspace for other split counts than ({case.S0}, {case.S1}): pick the shapes of "
        "tests/grad_edges.py SIGMOID_NARROW again")


@pytest.mark.parametrize("D", ge.TAIL_WIDTHS)
def test_layer_tail_rows_per_workgroup_match_the_library(D):
    """One record of 2 D floats per workgroup, 256 / tail_group(D) rows per workgroup (dif_layer_tail_bwd_workspace_bytes)."""
    from difformer_amd import _lib
    lib, R = _lib.load(), ge.tail_rows(D)
    for n in (1, R - 1, R, R + 1, 2 * R, 2 * R + 1):
        if n > 0:
            assert int(lib.dif_layer_tail_bwd_workspace_bytes(n, D)) == -(-n // R) * 2 * D * 4, (n, D, R)


@pytest.mark.parametrize("n,C,D,with_dx", ge.CLOSED_FORM)
def test_closed_form_cases_are_well_posed(n, C, D, with_dx):
    from difformer_amd import _lib, ops
    assert int(_lib.load().dif_closed_form_attn_bwd_groups(n)) >= 1
    x, coef, dx0, rs = ge.closed_form_operands(n, C, D, with_dx)
    for pattern in ge.PATTERNS:
        dd = ge.cotangent((n, D), pattern, 5)
        ref64 = ge.closed_form_reference(x, coef, dd, dx0, rs, D)
        ref32 = ge.closed_form_reference(x, coef, dd, dx0, rs, D, torch.float32)
        errs = ge.errors(ref32, ref64)
        assert max(errs.values()) < ge.PRECONDITION, (pattern, errs)
        assert not ge.vanishing(ref64), pattern              # nothing vanishes here, n = 1 included: no tensor takes the floor
    # the coefficient stage: its float64 yardstick (ops.closed_form_coeffs_backward, the derivative in closed form) is the
    # autograd derivative of the coefficient formulas, and the float32 run of that derivative meets the precondition
    x, p, a, dcoef = ge.coeff_operands(n, C, D)
    rec = ge.gram_record(x)
    auto64 = ge.coeffs_autograd(rec, n, C, D, p, a, dcoef, torch.float64)
    auto32 = ge.coeffs_autograd(rec, n, C, D, p, a, dcoef, torch.float32)
    closed = ops.closed_form_coeffs_backward(rec, n, C, D, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], a,
                                             dcoef[: D * C].view(D, C), dcoef[D * C: D * C + D], dcoef[D * C + D: D * C + D + C],
                                             dcoef[D * C + D + C])
    closed = {k: v.double().numpy() for k, v in zip(ge.CC_TENSORS, closed)}
    assert max(ge.errors(closed, auto64).values()) < 1e-6            # (the closed form returns float32: one rounding)
    assert max(ge.errors(auto32, auto64).values()) < ge.PRECONDITION
    assert not ge.vanishing(auto64)


@pytest.mark.parametrize("kernel,hidden,heads", ge.STEP_CONFIGS)
@pytest.mark.parametrize("n", ge.STEP_NODES)
def test_whole_step_cases_are_well_posed(n, kernel, hidden, heads):
    """Whole-model steps start at N = 3: at N = 1 and at N = 2 with `simple` the float32 oracle misses the bar itself."""
    cfg = ge.step_cfg(kernel, hidden, heads)
    model = ge.step_model(kernel, hidden, heads, n)
    x, ei, y = ge.step_graph(n)
    ref64 = ge.step_reference(model.state_dict(), x, ei, y, cfg)
    ref32 = ge.step_reference(model.state_dict(), x, ei, y, cfg, torch.float32)
    errs = ge.errors(ref32, ref64)
    assert max(errs.values()) < ge.PRECONDITION, sorted(((e, k) for k, e in errs.items()), reverse=True)[:3]


@pytest.mark.parametrize("n_nodes", [[1], [17]])
def test_single_graph_sigmoid_batches_are_ill_posed(n_nodes):
    """Why BATCHES_SIGMOID leaves out the batches of one graph: every position group then holds one node, the weight is
    s / (s + 1e-9), and dq, dk are ~1e-9 of dv -- not zero (no floor by the rule above), and out of float32's reach
    (s + 1e-9 == s): the float32 run of the oracle is off by 1e-3 .. 1e-1 of the floored scale (measured 7.9e-2 / 8.8e-2 on
    [1] and 1.3e-1 / 1.2e-1 on [17] at one head of 64 columns, dense cotangent)."""
    problem = ge.batched_problem("sigmoid", n_nodes, 1, 64)
    cot = problem.cotangent("dense")
    _, ref64 = problem.reference(cot)
    _, ref32 = problem.reference(cot, torch.float32)
    errs = ge.errors(ref32, ref64)
    assert not ge.vanishing(ref64) and max(errs["q"], errs["k"]) > ge.PRECONDITION and errs["v"] < ge.PRECONDITION, errs


@pytest.mark.parametrize("pattern", ["last", "tile"])
def test_spotlight_patterns_turn_a_dropped_row_into_a_whole_error(pattern):
    """What the spotlight cotangents are for: a backward that drops the lit row (here: the float64 oracle fed a cotangent
    without it) is off by 100 % in every gradient that sums over rows, where the same defect under the dense cotangent of a
    300-row case stays far smaller."""
    problem = ge.sigmoid_problem(300, 17, 1, 64, 64)
    cot = problem.cotangent(pattern)
    _, ref = problem.reference(cot)
    dropped = cot.clone()
    dropped[ge.spot_row(300, pattern)] = 0.0
    _, got = problem.reference(dropped)
    errs = ge.errors(got, ref)
    assert errs["k"] > 0.99 and errs["v"] > 0.99, errs
    dense = problem.cotangent("dense")
    _, ref = problem.reference(dense)
    dropped = dense.clone()
    dropped[ge.spot_row(300, pattern)] = 0.0
    _, got = problem.reference(dropped)
    errs = ge.errors(got, ref)
    assert ge.TOL < errs["v"] < 0.5, errs
