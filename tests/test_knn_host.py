"""k-nearest-neighbour graphs without a GPU: the oracle pinned to sklearn, the well-posedness of the GPU tests' inputs, the
argument errors of the public functions, the fourth library's header, and its host arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import knn_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_knn.h")
GRAPH_ARGS = ("x", "ldx", "n", "M", "k", "loop", "metric", "centre_row", "route", "edge_index", "dist", "workspace", "workspace_bytes",
              "stream")


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("include_self", [False, True])
@pytest.mark.parametrize("n,m,k", [(40, 3, 5), (200, 16, 10), (64, 70, 24)])
def test_oracle_equals_sklearn_kneighbors_graph(n, m, k, include_self):
    """`torch.tensor(adj.nonzero())` of image and text/main.py:52-53 on tie-free inputs: rows ascending, and within a row in
    distance order."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    x = knn_ref.inputs(n, m, seed=3)
    assert not knn_ref.ill_posed_rows(knn_ref.distances(x), k, include_self).any()
    adj = neighbors.kneighbors_graph(x, n_neighbors=k, include_self=include_self)
    want = np.stack(adj.nonzero()).astype(np.int64)
    idx, _ = knn_ref.knn_rows(x, k, loop=include_self)
    assert np.array_equal(knn_ref.edge_list(idx, 0), want)


def test_oracle_order_ties_nan_and_self():
    x = np.array([[0, 0], [1, 0], [1, 0], [0, 1], [np.nan, 0]], dtype=np.float32)
    idx, d = knn_ref.knn_rows(x, 3, loop=False)
    assert idx[0].tolist() == [1, 2, 3] and idx[1].tolist() == [2, 0, 3] and idx[2].tolist() == [1, 0, 3]     # ties: lower index
    assert idx[4].tolist() == [0, 1, 2] and np.isnan(d[4]).all()                                             # a NaN row: by index
    idx, _ = knn_ref.knn_rows(x, 24, loop=True)
    assert idx.shape == (5, 5) and (idx[:4, -1] == 4).all() and idx[1].tolist() == [1, 2, 0, 3, 4]           # NaN last
    zero = np.array([[0, 0], [1, 0], [0, 2]], dtype=np.float32)
    assert np.array_equal(knn_ref.distances(zero, cosine=True), np.array([[1, 1, 1], [1, 0, 1], [1, 1, 0.0]]))


@pytest.mark.parametrize("n,m", knn_ref.DIRECT_SHAPES + knn_ref.SWEEP_SHAPES + [(129, 8), (700, 16)])
def test_the_gpu_tests_inputs_are_well_posed(n, m):
    """Every row of every parity shape takes part in the index comparison: the oracle alone leaves out 0 rows."""
    x = knn_ref.inputs(n, m)
    for cosine in (False, True):
        d = knn_ref.distances(x, cosine)
        for loop in (False, True):
            for k in knn_ref.KS:
                assert not knn_ref.ill_posed_rows(d, k, loop).any(), (n, m, cosine, loop, k)


def test_the_tie_inputs_hold_ties_duplicates_and_a_crowd():
    x = knn_ref.integer_inputs(257, 4)
    head = np.sort(knn_ref.distances(x), axis=1)[:, :6]
    assert (np.diff(head, axis=1) == 0).any(axis=1).all()                      # every row: an exact tie in its first six
    assert 257 - len(np.unique(x, axis=0)) == 45                               # duplicate rows
    for m in (4, 20):
        crowd = knn_ref.integer_inputs(257, m, crowd=64)
        copies = np.nonzero((crowd == crowd[0]).all(axis=1))[0]
        assert len(copies) >= 64 and copies.max() > 200                        # more than the sweep's 32 candidates, spread out


def test_criterion_discriminates():
    x = knn_ref.inputs(60, 8, seed=5)
    idx, d = knn_ref.knn_rows(x, 5)
    good = knn_ref.edge_list(idx, 1)
    knn_ref.check_graph(good, np.sqrt(d).astype(np.float32).reshape(-1), x, 5)
    swapped = idx.copy()
    swapped[7, [1, 2]] = swapped[7, [2, 1]]                                    # right set, wrong order
    with pytest.raises(AssertionError, match="differ from the oracle"):
        knn_ref.check_graph(knn_ref.edge_list(swapped, 1), None, x, 5)
    with pytest.raises(AssertionError, match="centres"):
        knn_ref.check_graph(good[::-1].copy(), None, x, 5)                     # the other flow
    dup = idx.copy()
    dup[3, 4] = dup[3, 3]
    with pytest.raises(AssertionError, match="duplicate"):
        knn_ref.check_graph(knn_ref.edge_list(dup, 1), None, x, 5)
    with pytest.raises(AssertionError, match="distances"):
        knn_ref.check_graph(good, d.astype(np.float32).reshape(-1), x, 5)      # squared where the root is due
    # cosine self-loops at k = 1: every reference distance is float64 rounding noise; float32 roundings of it pass, 1e-6 does not
    idx, d = knn_ref.knn_rows(x, 1, loop=True, cosine=True)
    assert (idx[:, 0] == np.arange(60)).all() and np.abs(d).max() < 1e-15
    knn_ref.check_graph(knn_ref.edge_list(idx, 1), np.zeros(60, dtype=np.float32), x, 1, loop=True, cosine=True)
    with pytest.raises(AssertionError, match="distances"):
        knn_ref.check_graph(knn_ref.edge_list(idx, 1), np.full(60, 1e-6, dtype=np.float32), x, 1, loop=True, cosine=True)


# ---- argument errors: before the device is touched ------------------------------------------------------------------------------
def test_value_errors_name_the_limit():
    import difformer_amd
    from difformer_amd import kneighbors_graph, knn_graph
    assert {"knn_graph", "kneighbors_graph"} <= set(difformer_amd.__all__)
    x = torch.zeros(10, 8)
    for fn in (knn_graph, kneighbors_graph):
        with pytest.raises(ValueError, match="at least 1"):
            fn(x, 0)
        with pytest.raises(ValueError, match="24"):
            fn(x, 25)
        with pytest.raises(ValueError, match="512"):
            fn(torch.zeros(4, 513), 2)
        with pytest.raises(ValueError, match="2-d"):
            fn(torch.zeros(4, 2, 8), 2)
        with pytest.raises(ValueError, match="floating point"):
            fn(torch.zeros(10, 8, dtype=torch.int64), 2)
    with pytest.raises(ValueError, match="unknown flow"):
        knn_graph(x, 2, flow="sideways")


# ---- header and library ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def knn():
    from difformer_amd import _lib
    if not os.path.exists(_lib.KNN_LIB_PATH):
        pytest.skip("libdifformer_knn.so not built")
    return _lib.load_knn()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(knn):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.KNN_SIGNATURES) == ["dif_knn_graph_f32", "dif_knn_last_error", "dif_knn_route", "dif_knn_splits",
                                                       "dif_knn_version", "dif_knn_workspace_bytes"]
    for name in declared:
        assert getattr(knn, name) is not None
    assert not set(_lib.KNN_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.MAPS_SIGNATURES) | set(_lib.EDGES_SIGNATURES))
    assert len(_lib.KNN_SIGNATURES["dif_knn_graph_f32"][1]) == len(GRAPH_ARGS)
    assert _lib.KNN_SIGNATURES["dif_knn_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.KNN_SIGNATURES["dif_knn_last_error"][0] is ctypes.c_char_p
    assert knn.dif_knn_version() == _lib.KNN_VERSION == 1


def _call(knn, **over):
    """dif_knn_graph_f32 with made-up (never dereferenced) addresses: every rejection happens before any HIP call."""
    a = dict(x=0x10000, ldx=64, n=100, M=64, k=5, loop=0, metric=0, centre_row=1, route=-1, edge_index=0x20000, dist=0x30000,
             workspace=0x40000, workspace_bytes=1 << 40, stream=None)
    a.update(over)
    return knn.dif_knn_graph_f32(*[a[n] for n in GRAPH_ARGS])


@pytest.mark.parametrize("over,code", [
    (dict(x=None), "DIF_E_BADARG"), (dict(edge_index=None), "DIF_E_BADARG"), (dict(workspace=None), "DIF_E_BADARG"),
    (dict(x=0x10004), "DIF_E_BADARG"), (dict(workspace=0x40008), "DIF_E_BADARG"), (dict(edge_index=0x20004), "DIF_E_BADARG"),
    (dict(dist=0x30002), "DIF_E_BADARG"), (dict(ldx=66), "DIF_E_BADARG"), (dict(ldx=32), "DIF_E_BADARG"), (dict(n=0), "DIF_E_BADARG"),
    (dict(k=0), "DIF_E_SHAPE"), (dict(k=25), "DIF_E_SHAPE"), (dict(M=62), "DIF_E_SHAPE"), (dict(M=516, ldx=516), "DIF_E_SHAPE"),
    (dict(metric=2), "DIF_E_SHAPE"), (dict(centre_row=2), "DIF_E_SHAPE"), (dict(route=2), "DIF_E_SHAPE"),
    (dict(route=0, M=20), "DIF_E_SHAPE"),                                        # the direct route stops at 16 columns
    (dict(workspace_bytes=15), "DIF_E_WORKSPACE"), (dict(n=1 << 31), "DIF_E_RANGE"),
])
def test_every_argument_check_returns_its_code_without_a_gpu(knn, over, code):
    from difformer_amd import _lib
    rc = _call(knn, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, knn.dif_knn_last_error())
    assert b"dif_knn_graph_f32" in knn.dif_knn_last_error()                      # this library's text, not another's


def test_short_workspace_is_one_byte_short_and_no_neighbours_is_no_launch(knn):
    from difformer_amd import _lib
    need = knn.dif_knn_workspace_bytes(100, 64, 5, 0, 0, -1)
    assert _call(knn, workspace_bytes=need - 1) == _lib.ERROR_CODES["DIF_E_WORKSPACE"]
    assert _call(knn, n=1, M=4, ldx=4) == 0                                      # one row, no self-loop: nothing to write


def test_route_splits_and_workspace_are_host_arithmetic(knn):
    for M in (4, 8, 16):
        assert knn.dif_knn_route(1068, M, 5) == 0
    for M in (20, 64, 512):
        assert knn.dif_knn_route(1068, M, 5) == 1
    # the per-snapshot shapes: one key range (one launch) at 20 nodes, several at 1,068
    assert knn.dif_knn_splits(20, 4, 5, 1, -1) == 1 and knn.dif_knn_splits(1068, 8, 5, 1, -1) > 1
    assert knn.dif_knn_splits(33, 64, 5, 0, -1) == 1 and knn.dif_knn_splits(700, 64, 5, 0, -1) > 1
    assert knn.dif_knn_splits(129, 8, 5, 0, 0) > 1 and knn.dif_knn_splits(129, 8, 5, 0, 1) >= 1
    assert knn.dif_knn_splits(100, 62, 5, 0, -1) == 0 and knn.dif_knn_workspace_bytes(100, 64, 25, 0, 0, -1) == 0
    rng = np.random.default_rng(0)
    for _ in range(300):
        n, M = int(10 ** rng.uniform(0, 6)), 4 * int(rng.integers(1, 129))
        k, loop, metric = int(rng.integers(1, 25)), int(rng.integers(0, 2)), int(rng.integers(0, 2))
        for route in ((-1, 0, 1) if M <= 16 else (-1, 1)):
            S = knn.dif_knn_splits(n, M, k, loop, route)
            ws = knn.dif_knn_workspace_bytes(n, M, k, loop, metric, route)
            assert 1 <= S <= 32
            if route == 1 or (route == -1 and M > 16):
                assert ws == S * n * 32 * 8 + (n * M * 4 if metric else 0) + n * 4
            else:
                kk = min(k, n - (0 if loop else 1))
                K = 8 if kk <= 8 else (16 if kk <= 16 else 24)
                assert ws == (0 if S == 1 else S * n * K * 12)


def test_the_workspace_is_linear_in_n_and_far_below_the_dense_matrix(knn):
    # large graphs are swept in ONE key range: the workspace is then linear in N
    for metric in (0, 1):
        sizes = [(n, knn.dif_knn_workspace_bytes(n, 512, 5, 1, metric, -1)) for n in (70000, 140000, 280000)]
        assert all(knn.dif_knn_splits(n, 512, 5, 1, -1) == 1 for n, _ in sizes)
        assert sizes[1][1] == 2 * sizes[0][1] and sizes[2][1] == 4 * sizes[0][1]
    # ... and with the same number of ranges on both sides it is linear too
    assert knn.dif_knn_splits(15000, 512, 5, 1, -1) == knn.dif_knn_splits(14000, 512, 5, 1, -1)
    assert knn.dif_knn_workspace_bytes(15000, 512, 5, 1, 0, -1) * 14 == knn.dif_knn_workspace_bytes(14000, 512, 5, 1, 0, -1) * 15
    for metric in (0, 1):
        ws = knn.dif_knn_workspace_bytes(15000, 512, 5, 1, metric, -1)
        assert 15e6 <= ws <= 50e6 and ws < 90e6 and ws < 15000 * 15000 * 4 / 10
