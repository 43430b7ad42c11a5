"""Where the oracle's gcn_conv puts non-finite values: exactly where a dense float64 restatement of
`node classification/difformer.py:63-79` puts them.  tests/test_gpu_nonfinite.py holds the HIP products to the oracle's
positions; this file is why the oracle may be the judge.

The restatement is dense in storage, not in arithmetic.  difformer.py:75-77 multiplies a SparseTensor: an entry of x meets
only the STORED entries of its column of A (an entry that :74's nan_to_num set to 0 is still stored, and 0 * inf is NaN there
too), never the structural zeros.  A plain `A @ x` on a dense array would multiply every structural zero with the inf as
well and fill the whole output column with NaN, which the reference does not do -- so the product below runs over a dense
[N, N] value matrix AND the dense [N, N] mask of stored entries."""
import numpy as np
import pytest

from oracle import difformer_oracle as orc


def _dense_restatement(x, edge_index, edge_weight):
    n = x.shape[0]
    row, col = edge_index
    d = np.bincount(col, minlength=n).astype(np.float32)                              # :66, `.float()`
    with np.errstate(divide="ignore", invalid="ignore"):
        d_in, d_out = np.sqrt(np.float32(1.0) / d[col]), np.sqrt(np.float32(1.0) / d[row])     # :67-68, float32 as there
        if edge_weight is None:
            value = (np.ones(row.shape[0], dtype=np.float32) * d_in * d_out).astype(np.float64)  # :71
        else:
            value = edge_weight.astype(np.float64) * d_in * d_out                      # :73
    value = np.nan_to_num(value, nan=0.0, posinf=0.0, neginf=0.0)                     # :74
    A = np.zeros((n, n))
    stored = np.zeros((n, n), dtype=bool)
    np.add.at(A, (col, row), value)                                                   # :75: SparseTensor(row=col, col=row)
    stored[col, row] = True
    out = np.zeros_like(x)
    with np.errstate(invalid="ignore"):
        for h in range(x.shape[1]):                                                   # :76-78
            terms = np.where(stored[:, :, None], A[:, :, None] * x[None, :, h, :], 0.0)
            out[:, h, :] = terms.sum(axis=1)
    return out


def _case(n, e, heads, f, weighted, seed, isolated_source=False):
    rng = np.random.default_rng(seed)
    ei = np.concatenate([rng.integers(0, n, size=(2, e)), np.arange(n)[None].repeat(2, 0)], axis=1)
    if isolated_source:
        # node n-1 sends edges but receives none (no self loop either): its d^-1/2 is inf, :74 turns its entries into 0
        ei = ei[:, (ei[1] != n - 1)]
        ei = np.concatenate([ei, np.array([[n - 1, n - 1], [0, 5]])], axis=1)
    w = rng.uniform(0.5, 1.5, size=ei.shape[1]) if weighted else None
    x = rng.standard_normal((n, heads, f))
    return ei, w, x


@pytest.mark.parametrize("n,e,weighted", [(300, 1500, False), (300, 1500, True), (1500, 120000, False), (1500, 120000, True)])
def test_oracle_puts_non_finite_values_where_the_dense_restatement_does(n, e, weighted):
    """Both code paths of the oracle (numpy below 100,000 edges, the C restatement from there on).  One inf and one NaN in
    single entries of two rows of x whose nodes have in-degree > 0 and finite nonzero weights."""
    ei, w, x = _case(n, e, 2, 3, weighted, seed=n + e)
    x[7, 0, 1] = np.inf
    x[n // 2, 1, 2] = np.nan
    ref = _dense_restatement(x, ei, w)
    got = orc.gcn_conv(x, ei, w)
    bad = ~np.isfinite(ref)
    assert bad.any() and not bad[:, 0, 0].any() and not bad.all(axis=0).any()         # some rows, never a whole column
    assert np.array_equal(~np.isfinite(got), bad) and np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isposinf(got), np.isposinf(ref))
    np.testing.assert_allclose(got[~bad], ref[~bad], rtol=1e-6, atol=1e-9)
    # the positions are the destinations of the two rows' edges, in the one feature column each
    dst_inf, dst_nan = np.unique(ei[1][ei[0] == 7]), np.unique(ei[1][ei[0] == n // 2])
    want = np.zeros_like(bad)
    want[dst_inf, 0, 1] = True
    want[dst_nan, 1, 2] = True
    assert np.array_equal(bad, want)


@pytest.mark.filterwarnings("ignore:invalid value encountered")
def test_stored_zero_entry_times_inf_is_nan_in_both():
    """A source without incoming entries: its entries are stored zeros (:74), and a stored 0 times inf is NaN in the
    reference's sparse product, in the restatement and in the oracle alike."""
    n = 40
    ei, w, x = _case(n, 200, 1, 2, False, seed=3, isolated_source=True)
    x[n - 1, 0, 0] = np.inf
    ref = _dense_restatement(x, ei, w)
    got = orc.gcn_conv(x, ei, w)
    dst = np.unique(ei[1][ei[0] == n - 1])
    assert {0, 5} <= set(dst.tolist()) and n - 1 not in dst
    assert np.isnan(ref[dst, 0, 0]).all() and np.isfinite(np.delete(ref, dst, axis=0)).all() and np.isfinite(ref[:, 0, 1]).all()
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(~np.isfinite(got), ~np.isfinite(ref))
