"""Batched neighbour graphs without a GPU: the oracle of tests/nbr_ref.py against a brute-force loop, the well-posedness of the
GPU tests' inputs, the argument errors of the public functions, the tenth library's header, and its rejections."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import knn_ref
import nbr_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_nbr.h")
NAMES = ["dif_nbr_knn_f32", "dif_nbr_last_error", "dif_nbr_radius_edges", "dif_nbr_radius_lists_f32", "dif_nbr_version",
         "dif_nbr_workspace_bytes"]
KNN_ARGS = ("x", "ldx", "n", "M", "graph_ptr", "edge_ptr", "B", "k", "loop", "metric", "centre_row", "edge_index", "E", "dist", "stream")
LISTS_ARGS = ("x", "ldx", "n", "M", "graph_ptr", "B", "r", "loop", "cap", "deg", "workspace", "workspace_bytes", "stream")
EDGES_ARGS = ("deg_ptr", "n", "cap", "centre_row", "workspace", "workspace_bytes", "edge_index", "E", "dist", "stream")


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def _brute(x, n_nodes, loop, cosine, k=None, r=None, cap=None):
    """Per row: python loops over the rows of its own graph, float64 by direct difference, sorted by (NaN last, distance, index)."""
    x = x.astype(np.float64)
    rows, lo = [], 0
    for nb in n_nodes:
        for i in range(lo, lo + nb):
            cand = []
            for j in range(lo, lo + nb):
                if j == i and not loop:
                    continue
                if cosine:
                    ni, nj = np.sqrt((x[i] * x[i]).sum()), np.sqrt((x[j] * x[j]).sum())
                    d = 1.0 - (x[i] * x[j]).sum() * (0.0 if ni == 0 else 1.0 / ni) * (0.0 if nj == 0 else 1.0 / nj)
                else:
                    d = ((x[i] - x[j]) ** 2).sum()
                if r is not None and not d < np.float64(r) * np.float64(r):
                    continue
                cand.append((np.isnan(d), d if not np.isnan(d) else 0.0, j))
            cand.sort()
            rows.append(np.array([c[2] for c in cand[:k if r is None else cap]], dtype=np.int64))
        lo += nb
    return rows


@pytest.mark.parametrize("name,m", [("edges", 3), ("empties", 4), ("ones", 2), ("tiny", 5), ("one", 1)])
def test_oracle_equals_a_brute_force_loop(name, m):
    n_nodes = nbr_ref.N_NODES[name]
    x = knn_ref.integer_inputs(sum(n_nodes), m, seed=m)       # exact arithmetic: the two restatements agree bit for bit, ties included
    for loop in (False, True):
        for cosine in ((False, True) if m >= nbr_ref.MIN_COSINE_WIDTH and name == "tiny" else (False,)):
            batch = nbr_ref.Batch(x if not cosine else knn_ref.inputs(sum(n_nodes), m, seed=m), n_nodes, cosine)
            for k in knn_ref.KS:
                got = nbr_ref.batched_knn_rows(batch, k, loop)
                want = _brute(batch.x, n_nodes, loop, cosine, k=k)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want) == batch.n, (name, k, loop, cosine)
                for i, nb in zip(range(batch.n), np.repeat(n_nodes, n_nodes)):
                    assert len(got[i]) == min(k, nb - (0 if loop else 1))
        batch = nbr_ref.Batch(x, n_nodes)
        for r in (1.0, 2.0, 3.0):                             # r^2 = 1, 4, 9: distances equal to it exist and stay OUTSIDE
            for cap in nbr_ref.CAPS:
                got = nbr_ref.radius_rows(batch, r, loop, cap)
                want = _brute(x, n_nodes, loop, False, r=r, cap=cap)
                assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == batch.n, (name, r, cap, loop)


def test_oracle_radius_is_strict_caps_to_the_nearest_and_drops_nan_rows():
    x = np.array([[0, 0], [1, 0], [0, 2], [3, 0], [np.nan, 0], [0, 0]], dtype=np.float32)
    batch = nbr_ref.Batch(x, [5, 1])
    rows = nbr_ref.radius_rows(batch, 2.0, loop=True)
    assert rows[0].tolist() == [0, 1]                         # d(0, 2) == r^2 exactly: outside
    assert rows[1].tolist() == [1, 0] and rows[3].tolist() == [3] and rows[5].tolist() == [5]
    assert rows[4].tolist() == []                             # a NaN row: no edges, not even its self-loop
    assert nbr_ref.radius_rows(batch, 2.0, loop=False)[5].tolist() == []
    assert [r.tolist() for r in nbr_ref.radius_rows(batch, 4.0, loop=True, cap=2)[:4]] == [[0, 1], [1, 0], [2, 0], [3, 1]]
    assert nbr_ref.radius_ill_posed(batch, 2.0, True)[[0, 2]].all()          # the boundary decides rows 0 and 2
    ei = nbr_ref.edge_list(rows, 1)
    assert ei[1].tolist() == [0, 0, 1, 1, 2, 3, 5] and ei[0].tolist() == [0, 1, 1, 0, 2, 3, 5]


def test_criterion_discriminates():
    batch = nbr_ref.case("tiny", 3)
    rows, ill = nbr_ref.radius_rows(batch, 2.0, False, 5), nbr_ref.radius_ill_posed(batch, 2.0, False, 5)
    good = nbr_ref.edge_list(rows, 1)
    d = np.concatenate([np.sqrt(batch.distance(i, r)) for i, r in enumerate(rows)]).astype(np.float32)
    nbr_ref.check_edges(good, d, batch, rows, ill)
    full = next(i for i, r in enumerate(rows) if len(r) >= 2)
    swapped = [r.copy() for r in rows]
    swapped[full][[0, 1]] = swapped[full][[1, 0]]
    with pytest.raises(AssertionError, match="differ from the oracle"):
        nbr_ref.check_edges(nbr_ref.edge_list(swapped, 1), None, batch, rows, ill)
    with pytest.raises(AssertionError, match="centres"):
        nbr_ref.check_edges(good[::-1].copy(), None, batch, rows, ill)
    other = [r.copy() for r in rows]
    other[full][0] = (other[full][0] + 20) % batch.n          # a row of another graph
    with pytest.raises(AssertionError, match="outside the centre's graph"):
        nbr_ref.check_edges(nbr_ref.edge_list(other, 1), None, batch, rows, ill)
    dup = [r.copy() for r in rows]
    dup[full][1] = dup[full][0]
    with pytest.raises(AssertionError, match="duplicate"):
        nbr_ref.check_edges(nbr_ref.edge_list(dup, 1), None, batch, rows, ill)
    with pytest.raises(AssertionError, match="distances"):
        nbr_ref.check_edges(good, d * d, batch, rows, ill)


@pytest.mark.parametrize("name", list(nbr_ref.N_NODES))
def test_the_gpu_tests_inputs_are_well_posed(name):
    """The worst share of rows the oracle alone leaves out of the index comparison, over the whole case table, is 0.16 % (`big`,
    M = 1) for k-NN and for the radius alike: far inside knn_ref.MAX_ILL_POSED."""
    worst = 0.0
    for m in nbr_ref.WIDTHS:
        for cosine in ((False, True) if m >= nbr_ref.MIN_COSINE_WIDTH else (False,)):
            batch = nbr_ref.case(name, m, cosine)
            for loop in (False, True):
                for k in knn_ref.KS:
                    worst = max(worst, nbr_ref.knn_ill_posed(batch, k, loop).mean())
                if not cosine:
                    for r in nbr_ref.RADII:
                        for cap in nbr_ref.CAPS:
                            worst = max(worst, nbr_ref.radius_ill_posed(batch, r, loop, cap).mean())
    print(f"{name}: worst ill-posed share {worst:.4%}")
    assert worst <= 0.0017 and worst <= knn_ref.MAX_ILL_POSED
    if name != "big":
        assert worst == 0.0


def test_the_cap_cuts_on_mixed_and_short_rows_occur():
    batch = nbr_ref.case("mixed", 3)
    for r in nbr_ref.RADII:
        for cap in nbr_ref.CAPS:
            full = nbr_ref.radius_rows(batch, r, True, batch.n)
            cut = sum(len(f) > cap for f in full)
            short = sum(len(f) < cap for f in full)
            if (r, cap) == (0.5, 32):
                assert cut == 0
            elif (r, cap) == (1.0, 32):
                assert cut == 47 and short > 0
            else:
                assert 53 <= cut <= 430
    assert batch.n == 431


# ---- argument errors: before the device is touched ------------------------------------------------------------------------------
def test_value_errors_name_the_rule():
    import difformer_amd
    from difformer_amd import knn_graph, radius_graph
    assert {"knn_graph", "radius_graph", "kneighbors_graph"} <= set(difformer_amd.__all__)
    x = torch.zeros(10, 8)
    ids = torch.tensor([0] * 4 + [1] * 6)
    for fn, arg in ((knn_graph, 2), (radius_graph, 1.0)):
        with pytest.raises(ValueError, match="sorted"):
            fn(x, arg, batch=torch.tensor([0, 1] * 5))
        with pytest.raises(ValueError, match="not both"):
            fn(x, arg, batch=ids, n_nodes=torch.tensor([4, 6]))
        with pytest.raises(ValueError, match=r"int64 \[10\]"):
            fn(x, arg, batch=ids[:9])
        with pytest.raises(ValueError, match=r"int64 \[10\]"):
            fn(x, arg, batch=ids.int())
        with pytest.raises(ValueError, match="unknown flow"):
            fn(x, arg, flow="sideways", n_nodes=[4, 6])
        with pytest.raises(ValueError, match="2-d"):
            fn(torch.zeros(4, 2, 8), arg, n_nodes=[4])
        with pytest.raises(ValueError, match="floating point"):
            fn(torch.zeros(10, 8, dtype=torch.int64), arg, n_nodes=[4, 6])
        with pytest.raises(TypeError):
            fn(x, arg, False, "source_to_target", False, False, ids)           # batch is keyword-only
    with pytest.raises(ValueError, match="at least 1"):
        knn_graph(x, 0, n_nodes=[4, 6])
    with pytest.raises(ValueError, match="24"):
        knn_graph(x, 25, batch=ids)
    with pytest.raises(ValueError, match="512"):
        knn_graph(torch.zeros(4, 513), 2, n_nodes=[4])
    with pytest.raises(ValueError, match="at least 1"):
        radius_graph(x, 1.0, max_num_neighbors=0)
    with pytest.raises(ValueError, match="32"):
        radius_graph(x, 1.0, max_num_neighbors=33)
    for r in (-1.0, float("nan")):
        with pytest.raises(ValueError, match=">= 0"):
            radius_graph(x, r)
    with pytest.raises(ValueError, match="64"):
        radius_graph(torch.zeros(4, 65), 1.0)
    with pytest.raises(ValueError, match="64"):
        radius_graph(torch.zeros(4, 68), 1.0, n_nodes=[4])


# ---- header and library ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nbr():
    from difformer_amd import _lib
    if not os.path.exists(_lib.NBR_LIB_PATH):
        pytest.skip("libdifformer_nbr.so not built")
    return _lib.load_nbr()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(nbr):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.NBR_SIGNATURES) == NAMES
    for name in declared:
        assert getattr(nbr, name) is not None
    others = (set(_lib.SIGNATURES) | set(_lib.MAPS_SIGNATURES) | set(_lib.EDGES_SIGNATURES) | set(_lib.KNN_SIGNATURES)
              | set(_lib.SLOTS_SIGNATURES) | set(_lib.METRICS_SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAM_SIGNATURES)
              | set(_lib.READOUT_SIGNATURES))
    assert not set(_lib.NBR_SIGNATURES) & others
    assert len(_lib.NBR_SIGNATURES["dif_nbr_knn_f32"][1]) == len(KNN_ARGS)
    assert len(_lib.NBR_SIGNATURES["dif_nbr_radius_lists_f32"][1]) == len(LISTS_ARGS)
    assert len(_lib.NBR_SIGNATURES["dif_nbr_radius_edges"][1]) == len(EDGES_ARGS)
    assert _lib.NBR_SIGNATURES["dif_nbr_radius_lists_f32"][1][LISTS_ARGS.index("r")] is ctypes.c_double
    assert _lib.NBR_SIGNATURES["dif_nbr_workspace_bytes"] == (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int])
    assert _lib.NBR_SIGNATURES["dif_nbr_last_error"][0] is ctypes.c_char_p
    assert nbr.dif_nbr_version() == _lib.NBR_VERSION == 1
    assert _lib.NBR_CONSTANTS == {"DIF_NBR_MAX_COLUMNS": 64, "DIF_NBR_MAX_K": 24, "DIF_NBR_MAX_CAP": 32}
    from difformer_amd import neighbors
    assert (neighbors.MAX_BATCHED_WIDTH, neighbors.MAX_RADIUS_NEIGHBORS, neighbors.MAX_K) == (64, 32, 24)


def test_the_workspace_is_host_arithmetic(nbr):
    assert nbr.dif_nbr_workspace_bytes(100, 32) == 100 * 32 * 8 and nbr.dif_nbr_workspace_bytes(163925, 5) == 163925 * 5 * 8
    for n, cap in ((0, 5), (-1, 5), (1 << 31, 5), (10, 0), (10, 33)):
        assert nbr.dif_nbr_workspace_bytes(n, cap) == 0


# made-up (never dereferenced) addresses: every rejection happens before any HIP call
def _knn(nbr, **over):
    a = dict(x=0x10000, ldx=64, n=100, M=64, graph_ptr=0x50000, edge_ptr=0x60000, B=3, k=5, loop=0, metric=0, centre_row=1,
             edge_index=0x20000, E=500, dist=0x30000, stream=None)
    a.update(over)
    return nbr.dif_nbr_knn_f32(*[a[n] for n in KNN_ARGS])


def _lists(nbr, **over):
    a = dict(x=0x10000, ldx=64, n=100, M=64, graph_ptr=0x50000, B=3, r=1.0, loop=0, cap=32, deg=0x70000, workspace=0x40000,
             workspace_bytes=1 << 40, stream=None)
    a.update(over)
    return nbr.dif_nbr_radius_lists_f32(*[a[n] for n in LISTS_ARGS])


def _edges(nbr, **over):
    a = dict(deg_ptr=0x80000, n=100, cap=32, centre_row=1, workspace=0x40000, workspace_bytes=1 << 40, edge_index=0x20000, E=500,
             dist=0x30000, stream=None)
    a.update(over)
    return nbr.dif_nbr_radius_edges(*[a[n] for n in EDGES_ARGS])


COMMON = [
    (dict(x=None), "DIF_E_BADARG"), (dict(graph_ptr=None), "DIF_E_BADARG"), (dict(x=0x10004), "DIF_E_BADARG"),
    (dict(graph_ptr=0x50002), "DIF_E_BADARG"), (dict(ldx=66), "DIF_E_BADARG"), (dict(ldx=32), "DIF_E_BADARG"),
    (dict(n=0), "DIF_E_BADARG"), (dict(B=0), "DIF_E_BADARG"), (dict(M=62), "DIF_E_SHAPE"), (dict(M=68, ldx=68), "DIF_E_SHAPE"),
    (dict(n=1 << 31), "DIF_E_RANGE"),
]


@pytest.mark.parametrize("over,code", COMMON + [
    (dict(edge_ptr=None), "DIF_E_BADARG"), (dict(edge_index=None), "DIF_E_BADARG"), (dict(edge_ptr=0x60004), "DIF_E_BADARG"),
    (dict(edge_index=0x20004), "DIF_E_BADARG"), (dict(dist=0x30002), "DIF_E_BADARG"), (dict(k=0), "DIF_E_SHAPE"),
    (dict(k=25), "DIF_E_SHAPE"), (dict(metric=2), "DIF_E_SHAPE"), (dict(centre_row=2), "DIF_E_SHAPE"), (dict(E=-1), "DIF_E_SHAPE"),
    (dict(E=501), "DIF_E_SHAPE"),
])
def test_knn_rejections_return_their_code_without_a_gpu(nbr, over, code):
    from difformer_amd import _lib
    rc = _knn(nbr, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, nbr.dif_nbr_last_error())
    assert b"dif_nbr_knn_f32" in nbr.dif_nbr_last_error()                        # this library's text, not another's


@pytest.mark.parametrize("over,code", COMMON + [
    (dict(deg=None), "DIF_E_BADARG"), (dict(workspace=None), "DIF_E_BADARG"), (dict(deg=0x70002), "DIF_E_BADARG"),
    (dict(workspace=0x40008), "DIF_E_BADARG"), (dict(r=-1.0), "DIF_E_BADARG"), (dict(r=float("nan")), "DIF_E_BADARG"),
    (dict(cap=0), "DIF_E_SHAPE"), (dict(cap=33), "DIF_E_SHAPE"), (dict(workspace_bytes=100 * 32 * 8 - 1), "DIF_E_WORKSPACE"),
])
def test_radius_lists_rejections_return_their_code_without_a_gpu(nbr, over, code):
    from difformer_amd import _lib
    rc = _lists(nbr, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, nbr.dif_nbr_last_error())
    assert b"dif_nbr_radius_lists_f32" in nbr.dif_nbr_last_error()


@pytest.mark.parametrize("over,code", [
    (dict(deg_ptr=None), "DIF_E_BADARG"), (dict(workspace=None), "DIF_E_BADARG"), (dict(edge_index=None), "DIF_E_BADARG"),
    (dict(deg_ptr=0x80004), "DIF_E_BADARG"), (dict(workspace=0x40008), "DIF_E_BADARG"), (dict(edge_index=0x20004), "DIF_E_BADARG"),
    (dict(dist=0x30002), "DIF_E_BADARG"), (dict(n=0), "DIF_E_BADARG"), (dict(cap=0), "DIF_E_SHAPE"), (dict(cap=33), "DIF_E_SHAPE"),
    (dict(centre_row=-1), "DIF_E_SHAPE"), (dict(E=-1), "DIF_E_SHAPE"), (dict(E=3201), "DIF_E_SHAPE"), (dict(n=1 << 31), "DIF_E_RANGE"),
    (dict(workspace_bytes=100 * 32 * 8 - 1), "DIF_E_WORKSPACE"),
])
def test_radius_edges_rejections_return_their_code_without_a_gpu(nbr, over, code):
    from difformer_amd import _lib
    rc = _edges(nbr, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, nbr.dif_nbr_last_error())
    assert b"dif_nbr_radius_edges" in nbr.dif_nbr_last_error()


def test_an_empty_edge_list_is_no_launch(nbr):
    assert _knn(nbr, E=0, edge_index=None, dist=None) == 0                       # no graph has a neighbour to give
    assert _edges(nbr, E=0, edge_index=None, dist=None) == 0                     # no row has a neighbour inside
