"""float64 oracle and criterion of the batched neighbour graphs (difformer_amd/neighbors.py with batch= / n_nodes=,
csrc/nbr_batched.hip): `knn_ref`'s distances and total order, applied graph by graph.

A `Batch` holds the features, the row ranges of the graphs and one float64 distance matrix per graph.  `batched_knn_rows` and
`radius_rows` return, per row of the batch, the GLOBAL indices of its neighbours in order; `knn_ill_posed` / `radius_ill_posed`
mark the rows whose list is not decided by more than summation noise; `check_edges` holds an edge list to the oracle.
"""
import numpy as np

from conftest import rel_err
import knn_ref

# ---- the cases the host and the GPU tests share ----------------------------------------------------------------------------
N_NODES = {
    "one": [1],
    "ones": [1, 1, 1],
    "edges": [63, 1, 64, 65, 2],
    "empties": [0, 5, 0, 0, 70, 0],
    "tiny": [20] * 7,
    "mixed": [130, 3, 257, 1, 40],
    "big": [1068, 20, 129],
}
WIDTHS = (1, 2, 3, 4, 5, 16, 17, 64)
RADII = (0.5, 1.0, 2.0, 4.0)
CAPS = (1, 5, 32)
MIN_COSINE_WIDTH = 3        # at M <= 2 every cosine is +-1 (M = 1) or the rows tie in bulk: ill posed by construction of the inputs


class Batch:
    """x [N, M] float32 holding the graphs of `n_nodes` back to back, and per graph (lo, hi, d): its rows and their float64
    distance matrix (knn_ref.distances).  Computed once and left unchanged."""

    def __init__(self, x, n_nodes, cosine=False):
        self.x = np.asarray(x)
        self.n_nodes = [int(v) for v in n_nodes]
        self.cosine = bool(cosine)
        self.ptr = np.concatenate([[0], np.cumsum(self.n_nodes)]).astype(np.int64)
        assert self.ptr[-1] == self.x.shape[0], (self.ptr[-1], self.x.shape)
        self.n = int(self.ptr[-1])
        self.graph_of = np.repeat(np.arange(len(self.n_nodes)), self.n_nodes)
        self.graphs = [(int(lo), int(hi), knn_ref.distances(self.x[lo:hi], cosine))
                       for lo, hi in zip(self.ptr[:-1], self.ptr[1:]) if hi > lo]

    def batch_vector(self):
        return self.graph_of.astype(np.int64)

    def distance(self, i, js):
        """float64 distances (as ranked: squared Euclidean or 1 - cos) of row i to the global rows js of its graph."""
        for lo, hi, d in self.graphs:
            if lo <= i < hi:
                return d[i - lo, np.asarray(js, dtype=np.int64) - lo]
        raise IndexError(i)


def case(name, m, cosine=False):
    """The shared case `name` at width m: inputs knn_ref.inputs(sum(n_nodes), m, seed=m)."""
    n_nodes = N_NODES[name]
    return Batch(knn_ref.inputs(sum(n_nodes), m, seed=m), n_nodes, cosine)


def batched_knn_rows(batch, k, loop=False):
    """-> list of N int64 arrays: per row the global indices of its kk_b = min(k, n_b - (0 if loop else 1)) nearest rows of its
    own graph, nearest first (knn_ref.knn_rows per graph, offset)."""
    rows = [None] * batch.n
    for lo, hi, d in batch.graphs:
        idx, _ = knn_ref.knn_rows(None, k, loop, d=d)
        for i in range(hi - lo):
            rows[lo + i] = idx[i] + lo
    return rows


def knn_ill_posed(batch, k, loop=False):
    """bool [N]: knn_ref.ill_posed_rows per graph."""
    ill = np.zeros(batch.n, dtype=bool)
    for lo, hi, d in batch.graphs:
        ill[lo:hi] = knn_ref.ill_posed_rows(d, k, loop)
    return ill


def _ranked(d, loop):
    order = knn_ref._order(d, loop)
    return order, np.take_along_axis(d, order, axis=1)


def radius_rows(batch, r, loop=False, cap=32):
    """-> list of N int64 arrays: per row the global indices of the rows of its own graph with d < r * r (float64, strict; a NaN
    is never inside; j == i by index only with loop), ranked under the total order and cut at `cap`."""
    r2 = np.float64(r) * np.float64(r)
    rows = [None] * batch.n
    for lo, hi, d in batch.graphs:
        order, ds = _ranked(d, loop)
        with np.errstate(invalid="ignore"):
            keep = np.minimum((ds < r2).sum(axis=1), cap)          # sorted ascending, NaN last: what is inside is a prefix
        for i in range(hi - lo):
            rows[lo + i] = order[i, :keep[i]] + lo
    return rows


def radius_ill_posed(batch, r, loop=False, cap=32):
    """bool [N]: rows whose list is not decided by more than summation noise -- a candidate (a row of the same graph, self only
    with loop) with |d - r^2| <= WELL_POSED r^2 on either side of the boundary, or consecutive distances among the kept
    entries (and the first one cut, where the cap cuts) not separated by more than WELL_POSED of the last kept one."""
    r2 = np.float64(r) * np.float64(r)
    ill = np.zeros(batch.n, dtype=bool)
    for lo, hi, d in batch.graphs:
        _, ds = _ranked(d, loop)
        with np.errstate(invalid="ignore"):
            ill[lo:hi] |= (np.abs(ds - r2) <= knn_ref.WELL_POSED * r2).any(axis=1)
            inside = (ds < r2).sum(axis=1)
        for i in range(hi - lo):
            keep = min(int(inside[i]), cap)
            head = ds[i, :keep + (1 if inside[i] > cap else 0)]
            if keep and head.size > 1 and not np.all(np.diff(head) > knn_ref.WELL_POSED * abs(head[keep - 1])):
                ill[lo + i] = True
    return ill


def edge_list(rows, centre_row):
    """The oracle's rows as int64 [2, E] in the layout of the entry points: row `centre_row` holds the centre."""
    counts = np.array([len(r) for r in rows], dtype=np.int64)
    ei = np.empty((2, int(counts.sum())), dtype=np.int64)
    ei[centre_row] = np.repeat(np.arange(len(rows)), counts)
    ei[1 - centre_row] = np.concatenate(rows) if len(rows) and counts.sum() else np.empty(0, dtype=np.int64)
    return ei


def check_edges(edge_index, dist, batch, rows, ill, loop=False, centre_row=1, what="", exact=False):
    """edge_index int64 [2, E] (+ dist float32 [E] or None) against the oracle's `rows`:
    1. layout: row `centre_row` holds the centres ascending, every centre as often as the oracle lists neighbours for it;
       neighbours inside the centre's graph, distinct, no self without loop;
    2. index equality with the oracle on every well-posed row (all rows with exact=True), at most knn_ref.MAX_ILL_POSED left out;
    3. distances to knn_ref.TOL of the oracle's at the returned indices (conftest.rel_err; see knn_ref.NOISE)."""
    edge_index = np.asarray(edge_index)
    n = batch.n
    counts = np.array([len(r) for r in rows], dtype=np.int64)
    E = int(counts.sum())
    assert edge_index.dtype == np.int64 and edge_index.shape == (2, E), (what, edge_index.dtype, edge_index.shape, E)
    centres = np.repeat(np.arange(n), counts)
    assert np.array_equal(edge_index[centre_row], centres), f"{what}: centres or per-centre counts"
    got = edge_index[1 - centre_row]
    g = batch.graph_of[centres]
    assert ((got >= batch.ptr[g]) & (got < batch.ptr[g + 1])).all(), f"{what}: a neighbour outside the centre's graph"
    if not loop:
        assert (got != centres).all(), f"{what}: self-loop"
    starts = np.concatenate([[0], np.cumsum(counts)])
    ill = np.zeros(n, dtype=bool) if exact else np.asarray(ill, dtype=bool)
    print(f"{what}: {int(ill.sum())} of {n} rows ill posed, {E} edges")
    assert n == 0 or ill.mean() <= knn_ref.MAX_ILL_POSED, f"{what}: {ill.mean():.3f} of the rows are ill posed"
    ref = np.empty(E)
    bad = []
    for i in range(n):
        mine = got[starts[i]:starts[i + 1]]
        assert len(np.unique(mine)) == len(mine), f"{what}: duplicate neighbours of row {i}"
        if len(mine):
            ref[starts[i]:starts[i + 1]] = batch.distance(i, mine)
        if not ill[i] and not np.array_equal(mine, rows[i]):
            bad.append(i)
    assert not bad, f"{what}: {len(bad)} rows differ from the oracle, first {bad[0]}: got " \
                    f"{got[starts[bad[0]]:starts[bad[0] + 1]]}, want {rows[bad[0]]}"
    if dist is not None:
        dist = np.asarray(dist)
        assert dist.dtype == np.float32 and dist.shape == (E,), (what, dist.dtype, dist.shape)
        if E:
            ref = ref if batch.cosine else np.sqrt(ref)
            nan = np.isnan(ref)
            assert np.array_equal(np.isnan(dist), nan), f"{what}: NaN distances"
            if (~nan).any():
                if np.max(np.abs(ref[~nan])) < knn_ref.NOISE:
                    err = float(np.max(np.abs(dist[~nan] - ref[~nan]))) / knn_ref.NOISE
                else:
                    err = rel_err(dist[~nan], ref[~nan])
                print(f"{what}: distances {err:.2e}")
                assert err <= knn_ref.TOL, f"{what}: distances {err:.3e}"
