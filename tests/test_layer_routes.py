"""DIFFormerConv._route: the route of every point of a flag grid against a table recorded from the code BEFORE `_route`
existed (tests/golden/layer_routes.txt), and `_layer` asking `_route` exactly once and going where it says.

The table was recorded at the commit that still had `_closed_form() -> bool`: `observe` below ran `_layer` on every point
of `points()` with the five entry points of the routes replaced by markers and wrote down which one was reached, run-length
coded in grid order.  It is an observation of the old code, not a second statement of the rule.

Host only: the backend is a stub that has nothing but the attribute names `_route` probes for.
"""
import os
import types

import pytest
import torch

from difformer_amd import DIFFormerConv, ops
from difformer_amd import autograd_ops as ag
from difformer_amd import difformer as dif

ROUTES = ("closed_wide", "closed_train", "closed_narrow", "fused_projection", "operator")
TABLE = os.path.join(os.path.dirname(__file__), "golden", "layer_routes.txt")

WIDTHS = (16, 64, 68, 128, 132, 512, 516)
FLAGS = ("bf16", "width", "heads", "rows", "use_weight", "kernel", "use_graph", "world", "grad", "query_is_source", "prev",
         "want_qk", "exact_fp32", "closed_form_training")
GRAD_OPERANDS = (None, "x", "parameter", "x0", "ln_weight", "edge_weight")
CAPABILITIES = ("gram", "gram_sym", "simple_reduce")
# the whole grid with every capability; with one capability missing, the part of the grid where a closed form is in reach
# at all (`simple`, one head, query is source, no q / k wanted) -- elsewhere no capability is ever asked for
SECTIONS = [("all", {})] + [("no " + c, dict(kernels=("simple",), heads=(1,), query_is_source=(True,), want_qk=(False,)))
                            for c in CAPABILITIES]


def stub_backend(section):
    """An object with only the capability names (`section`: "all" or "no <capability>")."""
    be = types.SimpleNamespace()
    for c in CAPABILITIES:
        if section != "no " + c:
            setattr(be, c, None)
    return be


class _Shard:
    def __init__(self, world, n_local):
        self.world, self.rank, self.product = world, 0, "row"
        self.row_begin, self.n_local, self.n_global = 0, n_local, n_local * world


def points(kernels=("simple", "sigmoid"), heads=(1, 2), query_is_source=(True, False), want_qk=(False, True)):
    """Every point of the grid, in the order of the table: -> (the point's FLAGS, conv, arguments of `_route`).  The module-level
    switches (EXACT_FP32, _CLOSED_FORM_TRAINING) are set for the point while it is out and restored at the end."""
    exact_was, cft_was = ops.EXACT_FP32, dif._CLOSED_FORM_TRAINING
    edge_weight = torch.ones(8)
    try:
        for bf16 in (False, True):
            dtype = torch.bfloat16 if bf16 else torch.float32
            for width in WIDTHS:
                ln_w, ln_b = torch.ones(width, dtype=dtype), torch.zeros(width, dtype=dtype)
                for n_heads in heads:
                    convs = {}
                    for use_weight in (True, False):
                        conv = DIFFormerConv(width, width, n_heads, use_weight=use_weight).to(dtype)
                        for p in conv.parameters():
                            p.requires_grad_(False)
                        convs[use_weight] = conv
                    for rows in (40, 4 * width + 4):
                        x, other, x0 = (torch.zeros(rows, width, dtype=dtype) for _ in range(3))
                        for use_weight in (True, False):
                            conv = convs[use_weight]
                            leaves = {"x": x, "parameter": conv.Wq.weight, "x0": x0, "ln_weight": ln_w, "edge_weight": edge_weight}
                            for kernel in kernels:
                                for use_graph in (True, False):
                                    conv.kernel, conv.use_graph = kernel, use_graph
                                    for world in (None, 1, 2):
                                        conv.row_shard = None if world is None else _Shard(world, rows)
                                        for grad in GRAD_OPERANDS:
                                            if grad is not None:
                                                leaves[grad].requires_grad_(True)
                                            for q_is_src in query_is_source:
                                                for prev_name, prev in (("x", x), ("other", other), (None, None)):
                                                    for qk in want_qk:
                                                        for exact in (False, True):
                                                            ops.set_exact_fp32(exact)
                                                            for cft in (True, False):
                                                                dif._CLOSED_FORM_TRAINING = cft
                                                                label = (bf16, width, n_heads, rows, use_weight, kernel, use_graph, world,
                                                                         grad, q_is_src, prev_name, qk, exact, cft)
                                                                yield label, conv, (x if q_is_src else other, x, edge_weight, x0,
                                                                                    prev, ln_w, ln_b, qk)
                                            if grad is not None:
                                                leaves[grad].requires_grad_(False)
    finally:
        ops.set_exact_fp32(exact_was)
        dif._CLOSED_FORM_TRAINING = cft_was


class _Took(Exception):
    pass


def _marker(name):
    def took(*args, **kwargs):
        raise _Took(name)
    return took


def observing(monkeypatch):
    """Replace the entry point of every route by a marker (and what `_layer` builds on the way there by stand-ins)."""
    monkeypatch.setattr(ops, "simple_layer_closed_form_wide", _marker("closed_wide"))
    monkeypatch.setattr(ag, "closed_form_layer", _marker("closed_train"))
    monkeypatch.setattr(ops, "simple_layer_closed_form", _marker("closed_narrow"))
    monkeypatch.setattr(ops, "project_simple_attention", _marker("fused_projection"))
    monkeypatch.setattr(DIFFormerConv, "_project", _marker("operator"))
    monkeypatch.setattr(ops, "WideCoefficients", lambda *a: None)
    monkeypatch.setattr(ops.csr_cache, "get", lambda *a, **k: types.SimpleNamespace(weight_scale=1.0))


def observe(conv, args):
    """The route `_layer` takes for the arguments of `_route` (under `observing`)."""
    query, source, edge_weight, x0, prev, ln_w, ln_b, want_qk = args
    try:
        conv._layer(query, source, torch.zeros(2, 8, dtype=torch.int64), edge_weight, x0, prev, 0.5, ln_w, ln_b, 1e-5, want_qk)
    except _Took as e:
        return e.args[0]
    raise AssertionError("_layer reached none of the five routes")


def read_table():
    """-> {section: [route of every point, in grid order]}"""
    table, section = {}, None
    with open(TABLE) as f:
        for line in f:
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            if line.startswith("["):
                section = table.setdefault(line[1:-1], [])
            else:
                name, count = line.split()
                section.extend([name] * int(count))
    return table


@pytest.fixture(scope="module")
def table():
    return read_table()


@pytest.mark.parametrize("section,fixed", SECTIONS, ids=[s for s, _ in SECTIONS])
def test_route_of_every_grid_point(monkeypatch, table, section, fixed):
    monkeypatch.setattr(ops, "_BACKEND", stub_backend(section))
    expected = table[section]
    assert set(expected) <= set(ROUTES)
    count, wrong = 0, []
    for (label, conv, args), want in zip(points(**fixed), expected):
        got = conv._route(*args)
        count += 1
        if got != want and len(wrong) < 10:
            wrong.append(f"{dict(zip(FLAGS, label))}: {got}, expected {want}")
    assert count == len(expected) and not wrong, "\n".join(wrong)
    if section == "all":
        assert set(expected) == set(ROUTES)            # the grid reaches every route


def test_layer_asks_route_once_and_follows_it(monkeypatch, table):
    """A sample of the grid through `_layer` itself: one `_route` call per `_layer` call, and the entry point reached is
    the one the table names."""
    monkeypatch.setattr(ops, "_BACKEND", stub_backend("all"))
    observing(monkeypatch)
    calls = []
    route = DIFFormerConv._route
    monkeypatch.setattr(DIFFormerConv, "_route", lambda self, *a: calls.append(1) or route(self, *a))
    seen = set()
    for i, ((label, conv, args), want) in enumerate(zip(points(), table["all"])):
        if i % 97 and want in seen:
            continue
        del calls[:]
        assert observe(conv, args) == want, dict(zip(FLAGS, label))
        assert len(calls) == 1, dict(zip(FLAGS, label))
        seen.add(want)
    assert seen == set(ROUTES)
