"""float64 oracle and criterion of the k-nearest-neighbour graphs (difformer_amd/neighbors.py, csrc/knn_graph.hip).

The contract is one total order on float64 distances computed from the float32 rows: the smaller distance first, among equal
distances the lower index first, a NaN after every number.  `knn_rows` restates it with a stable argsort; `check_graph` holds
a result to it by INDEX EQUALITY on every row whose order is decided by more than summation noise.
"""
import numpy as np

from conftest import rel_err

TOL = 1e-4              # the project's bar for values
WELL_POSED = 1e-9       # gap between consecutive distances, relative to the kk-th: far above float64 summation noise (1e-16 per
#                         term), far below any float32 effect (6e-8)
MAX_ILL_POSED = 0.01    # share of rows a test may leave out of the index comparison
NOISE = 1e-9            # conftest.rel_err divides by max|ref|.  Where EVERY reference distance is below this -- cosine self-loops at
#                         k = 1: 1 - cos(x, x) is a few 1e-16 of float64 rounding in the oracle and on the device alike -- that
#                         quotient compares noise with noise; the error is then taken against this scale instead


def inputs(n, m, seed=0):
    """The tests' features: standard normal float32 [n, m]."""
    return np.random.default_rng(seed).standard_normal((n, m)).astype(np.float32)


def distances(x, cosine=False):
    """x [N, M] (float32 values) -> float64 [N, N]: sum_m (x_im - x_jm)^2 by direct difference, or 1 - cos (a zero row has cosine
    0 with every row)."""
    x = np.asarray(x, dtype=np.float64)
    n, m = x.shape
    if cosine:
        norm = np.sqrt((x * x).sum(axis=1))
        with np.errstate(divide="ignore", invalid="ignore"):
            rn = np.where(norm == 0, 0.0, 1.0 / norm)
        return 1.0 - (x @ x.T) * rn[:, None] * rn[None, :]
    d = np.empty((n, n))
    step = max(1, (1 << 22) // max(1, n * m))
    for r in range(0, n, step):
        diff = x[r:r + step, None, :] - x[None, :, :]
        d[r:r + step] = (diff * diff).sum(axis=2)
    return d


def neighbour_count(n, k, loop):
    return min(k, n - (0 if loop else 1))


_ORDERS = {}            # (id(d), loop) -> (d, order): a test asks for the order of one matrix for several k


def _order(d, loop):
    """Row-wise order of the eligible indices under the total order (stable argsort: ties to the lower index, NaN last)."""
    hit = _ORDERS.get((id(d), loop))
    if hit is not None and hit[0] is d:
        return hit[1]
    n = d.shape[0]
    order = np.argsort(d, axis=1, kind="stable")
    if not loop:                                          # self is excluded by index, wherever it ranks
        order = order[order != np.arange(n)[:, None]].reshape(n, n - 1)
    if len(_ORDERS) >= 8:
        _ORDERS.clear()
    _ORDERS[(id(d), loop)] = (d, order)
    return order


def knn_rows(x, k, loop=False, cosine=False, d=None):
    """-> (indices int64 [N, kk], distances float64 [N, kk] as ranked: squared Euclidean or 1 - cos)."""
    d = distances(x, cosine) if d is None else d
    idx = _order(d, loop)[:, :neighbour_count(d.shape[0], k, loop)]
    return idx, np.take_along_axis(d, idx, axis=1)


def ill_posed_rows(d, k, loop):
    """bool [N]: rows whose first kk + 1 distances are NOT separated by more than WELL_POSED of the kk-th."""
    kk = neighbour_count(d.shape[0], k, loop)
    if kk == 0:
        return np.zeros(d.shape[0], dtype=bool)
    head = np.take_along_axis(d, _order(d, loop)[:, :kk + 1], axis=1)
    gaps = np.diff(head, axis=1)
    with np.errstate(invalid="ignore"):
        return ~np.all(gaps > WELL_POSED * np.abs(head[:, kk - 1:kk]), axis=1) if gaps.shape[1] else np.zeros(d.shape[0], dtype=bool)


def edge_list(idx, centre_row):
    """The oracle's rows as int64 [2, N kk] in the layout of the entry points: row `centre_row` holds the centre."""
    n, kk = idx.shape
    ei = np.empty((2, n * kk), dtype=np.int64)
    ei[centre_row] = np.repeat(np.arange(n), kk)
    ei[1 - centre_row] = idx.reshape(-1)
    return ei


def check_graph(edge_index, dist, x, k, loop=False, cosine=False, centre_row=1, what="", d=None, exact=False):
    """edge_index int64 [2, N kk] (+ dist float32 [N kk] or None) against the oracle on x:
    1. layout: row `centre_row` is every centre kk times, ascending; neighbours distinct, in range, no self without loop;
    2. index equality with the oracle on every well-posed row (all rows with exact=True), at most MAX_ILL_POSED left out;
    3. distances to TOL of the oracle's at the returned indices (conftest.rel_err; see NOISE)."""
    edge_index = np.asarray(edge_index)
    n = x.shape[0]
    kk = neighbour_count(n, k, loop)
    d = distances(x, cosine) if d is None else d
    assert edge_index.dtype == np.int64 and edge_index.shape == (2, n * kk), (what, edge_index.dtype, edge_index.shape)
    assert np.array_equal(edge_index[centre_row], np.repeat(np.arange(n), kk)), f"{what}: centres"
    got = edge_index[1 - centre_row].reshape(n, kk)
    assert got.size == 0 or (got.min() >= 0 and got.max() < n), f"{what}: indices out of range"
    srt = np.sort(got, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all(), f"{what}: duplicate neighbours in a row"
    if not loop:
        assert (got != np.arange(n)[:, None]).all(), f"{what}: self-loop"
    want, want_d = knn_rows(x, k, loop, cosine, d=d)
    ill = np.zeros(n, dtype=bool) if exact else ill_posed_rows(d, k, loop)
    print(f"{what}: {int(ill.sum())} of {n} rows ill posed")
    assert ill.mean() <= MAX_ILL_POSED, f"{what}: {ill.mean():.3f} of the rows are ill posed"
    bad = np.nonzero((got != want).any(axis=1) & ~ill)[0]
    assert bad.size == 0, f"{what}: {bad.size} rows differ from the oracle, first {bad[0]}: got {got[bad[0]]}, want {want[bad[0]]}"
    if dist is not None:
        dist = np.asarray(dist)
        assert dist.dtype == np.float32 and dist.shape == (n * kk,), (what, dist.dtype, dist.shape)
        at = np.take_along_axis(d, got, axis=1)
        ref = at if cosine else np.sqrt(at)
        if ref.size and np.nanmax(np.abs(ref)) < NOISE:
            err = float(np.max(np.abs(dist.reshape(n, kk) - ref))) / NOISE
        else:
            err = rel_err(dist.reshape(n, kk), ref)
        print(f"{what}: distances {err:.2e}")
        assert err <= TOL, f"{what}: distances {err:.3e}"


# ---- the cases the host and the GPU tests share ----------------------------------------------------------------------------
DIRECT_SHAPES = [(1, 4), (2, 1), (5, 4), (6, 4), (20, 4), (129, 4), (1068, 8), (33, 16)]
SWEEP_SHAPES = [(15, 20), (16, 20), (17, 20), (31, 64), (32, 64), (33, 64), (700, 64), (600, 300), (257, 512), (1500, 17)]
KS = (1, 5, 24)


def integer_inputs(n, m, seed=0, crowd=0):
    """Integer features in [-2, 2] as float32: every product and sum is exact in float32 and float64, so equal distances are
    equal bit for bit.  crowd: that many rows, spread over the matrix, are copies of row 0."""
    x = np.random.default_rng(seed).integers(-2, 3, size=(n, m)).astype(np.float32)
    if crowd:
        x[np.random.default_rng(seed + 1).permutation(n)[:crowd]] = x[0]
    return x
