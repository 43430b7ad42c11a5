"""The table of tests/test_gpu_operand_layouts.py against HipBackend itself (no GPU): every method that prepares a row operand
with `_row_major` or `_rows` has a row in the table or a written reason in LEFT_OUT, and every operand the table places is
a parameter of its method.  A method that starts to take strided rows later has to come to the sweep too."""
import ast
import inspect
import textwrap

import test_gpu_operand_layouts as sweep


def _row_operand_methods():
    """{method name: its parameter names} for the HipBackend methods whose body calls _row_major( or _rows(."""
    from difformer_amd.backend_hip import HipBackend
    tree = ast.parse(textwrap.dedent(inspect.getsource(HipBackend)))
    found = {}
    for fn in tree.body[0].body:
        if not isinstance(fn, ast.FunctionDef):
            continue
        calls = {n.func.id for n in ast.walk(fn) if isinstance(n, ast.Call) and isinstance(n.func, ast.Name)}
        if calls & {"_row_major", "_rows"}:
            found[fn.name] = {a.arg for a in fn.args.args + fn.args.kwonlyargs}
    return found


def test_every_method_with_row_operands_is_in_the_table_or_excused():
    methods = _row_operand_methods()
    assert len(methods) >= 25 and {"simple_layer", "layer_tail_mix", "coeffs_bg", "linear", "spmm"} <= set(methods)
    table = {r["method"] for r in sweep.ROWS}
    assert not (table | set(sweep.LEFT_OUT)) - set(methods), f"no such method: {sorted((table | set(sweep.LEFT_OUT)) - set(methods))}"
    assert not table & set(sweep.LEFT_OUT)
    missing = set(methods) - table - set(sweep.LEFT_OUT)
    assert not missing, f"neither swept nor excused: {sorted(missing)}"
    assert all(len(reason) > 10 for reason in sweep.LEFT_OUT.values())
    assert len({r["id"] for r in sweep.ROWS}) == len(sweep.ROWS)


# operands of spmm's fused tail travel inside its `tail` dict
IN_A_DICT = {"spmm": {"x0", "prev"}}


def test_every_placed_operand_is_a_parameter_of_its_method():
    methods = _row_operand_methods()
    for r in sweep.ROWS:
        params = methods[r["method"]] | IN_A_DICT.get(r["method"], set())
        for name in r["operands"]:
            assert name in params, f"{r['id']}: {name} is no parameter of {r['method']}"
        assert (r["copies"] | r["contiguous"]) <= set(r["operands"]), r["id"]


def test_every_row_builds_and_places_its_operands_on_the_host():
    """build() of every row on the CPU: the named operands exist, are row tensors, and come out of a guarded block with the
    promised stride and offset (the placements themselves need no GPU: tests/guarded.py)."""
    import torch
    from guarded import GuardedArena
    for r in sweep.ROWS:
        if r["id"].startswith(("linear-16384", "simple_reduce-4096", "simple_apply-4096", "row_gemm-4096", "sliced_")):
            continue                                             # the threshold shapes: the same builders at more rows (seconds of oracle)
        cpu_ops, run, check = sweep._built(r)
        assert callable(run) and callable(check)
        for name in r["operands"]:
            t = cpu_ops[name]
            assert t.dim() >= 2 and t.is_contiguous(), (r["id"], name)
            for placement in sweep.PLACEMENTS:
                arena = GuardedArena()
                d = sweep._place(arena, "cpu", t, placement)
                assert torch.equal(d, t) and (placement == "off1" or not d.is_contiguous())
                arena.check()
