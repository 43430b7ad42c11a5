"""Non-finite values stay where the reference puts them (gcn_conv, difformer.py:63-79).

One inf and one NaN, each in a single entry of a row j of x whose node has in-degree > 0 and finite nonzero weights: the
output is non-finite exactly at the destinations of j's edges, in that one feature column (tests/test_oracle_nonfinite.py
holds the float64 oracle to a dense restatement of the reference on this).  Every product kernel must agree: the row
kernels, the blocked kernel in natural and degree order (with a hub row that is split over a quad of lanes), and the
feature-sliced product under the strict and the packed schedule.  The sliced schedule's padded steps and idle lanes read "a
zero row": they are right only if that row stays zero and nothing is ever masked by multiplying with 0 -- 0 * inf is NaN,
and it would show up in rows that have no edge from j.  The finite entries keep the usual tolerance (1e-4 norm-wise for the
gather kernels, 1e-5 for the sliced product, as tests/test_gpu_kernel_coverage.py and tests/test_gpu_sliced.py)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from guarded import poisoned_allocations  # noqa: F401  (the fixture)
from oracle import difformer_oracle as orc
from sliced_format import schedule  # noqa: F401  (the fixture that forces DIFFORMER_SLICED_SCHEDULE)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _uniform_graph(n, deg, seed):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, n * deg), generator=g)
    return torch.cat([ei, torch.arange(n).repeat(2, 1)], dim=1)


def _hub_graph(n, deg, seed, hubs=8):
    """A quarter of the entries land on `hubs` rows: far beyond 4x the mean degree (row_order splits those rows)."""
    ei = _uniform_graph(n, deg, seed)
    g = torch.Generator().manual_seed(seed + 1)
    q = ei.shape[1] // 4
    ei[1, :q] = torch.randint(0, hubs, (q,), generator=g) * (n // hubs)
    return ei


def _poisoned_x(n, F, ei, seed):
    """x with +inf in x[j1, 1] and NaN in x[j2, F - 2]; j1 sends to the first hub row (node 0) where the graph has one."""
    x = torch.randn(n, F, generator=torch.Generator().manual_seed(seed))
    src, dst = ei[0], ei[1]
    to_first = src[dst == 0]
    j1 = int(to_first[to_first != 0][0]) if (to_first != 0).any() else int(src[0])
    j2 = int(src[src != j1][len(src) // 2])
    x[j1, 1] = float("inf")
    x[j2, F - 2] = float("nan")
    return x, j1, j2


def _assert_same_positions(out, x, ei, tol, j1, j2):
    ref = orc.gcn_conv(x.double().numpy()[:, None, :], ei.numpy(), None)[:, 0, :]
    out = out.float().cpu().numpy().astype(np.float64)
    bad = ~np.isfinite(ref)
    want = np.zeros_like(bad)                                    # the destinations of j1's and j2's edges, one column each
    want[np.unique(ei[1][ei[0] == j1].numpy()), 1] = True
    want[np.unique(ei[1][ei[0] == j2].numpy()), x.shape[1] - 2] = True
    assert np.array_equal(bad, want) and 2 <= bad.sum() < bad.shape[0]
    got_bad = ~np.isfinite(out)
    extra, missing = np.argwhere(got_bad & ~bad), np.argwhere(~got_bad & bad)
    assert not len(extra) and not len(missing), \
        f"non-finite where the oracle is finite: {extra[:5].tolist()} ({len(extra)}); finite where it is not: " \
        f"{missing[:5].tolist()} ({len(missing)})"
    err = rel_err(np.where(bad, 0.0, out), np.where(bad, 0.0, ref))
    assert err < tol, err


@pytest.mark.parametrize("F", [64, 7])
@pytest.mark.parametrize("deg", [24, 4])
def test_row_kernels_keep_non_finite_values_in_place(deg, F, dev, poisoned_allocations):
    """A wave per row (from 16 entries per row) and a lane group per row, vector rows and rows that are not 4-element aligned."""
    from difformer_amd import ops
    be = ops.get_backend()
    n = 3000
    ei = _uniform_graph(n, deg, F + deg)
    x, j1, j2 = _poisoned_x(n, F, ei, F)
    csr = ops.GraphCSR.build(ei.to(dev), None, n, 1)
    out = be.spmm(csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, n, csr.nnz, x.to(dev), 0, n)
    _assert_same_positions(out, x, ei, 1e-4, j1, j2)


@pytest.mark.parametrize("ordered", [False, True])
def test_blocked_kernel_keeps_non_finite_values_in_place(ordered, dev, poisoned_allocations):
    """Source-blocked CSR (3 blocks), natural order and degree order; in degree order the hub rows -- node 0 among them, which
    receives the inf -- are split over a quad of lanes."""
    from difformer_amd import ops
    be = ops.get_backend()
    n, F = 32768, 64
    ei = _hub_graph(n, 12, 5)
    x, j1, j2 = _poisoned_x(n, F, ei, 6)
    assert (ei[1][ei[0] == j1] == 0).any()
    csr = ops.GraphCSR.build(ei.to(dev), None, n, 3)
    order = csr.row_order(0, n) if ordered else None
    if ordered:
        assert order is not None and order[1] > 0 and 0 in order[0][: order[1]].tolist()      # node 0 is a split row
    out = be.spmm(csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, n, csr.nnz, x.to(dev), 0, n, None, 1.0, 1.0, None, order)
    _assert_same_positions(out, x, ei, 1e-4, j1, j2)


@pytest.mark.parametrize("mode", ["strict", "packed"])
def test_sliced_product_keeps_non_finite_values_in_place(mode, dev, schedule, poisoned_allocations):
    """8,192 nodes with 50 + 1 entries per row: the smallest graph that takes the feature-sliced product.  Its rounds are
    padded to 8-step blocks and its last slot has idle lanes."""
    from difformer_amd import gcn_conv, ops
    schedule(mode)
    n, F = 8192 + 37, 64
    ei = _uniform_graph(n, 50, 11)
    x, j1, j2 = _poisoned_x(n, F, ei, 12)
    eid = ei.to(dev)
    be = ops.get_backend()
    be.kernel_events = {}
    try:
        out = gcn_conv(x[:, None, :].to(dev), eid, None)
    finally:
        names, be.kernel_events = set(be.kernel_events), None
    assert "dif_sliced_spmm_f32" in names
    assert ops.csr_cache.get(eid, None, n, F * 4).sliced(0, n, F).quad_cap == (2 if mode == "packed" else 1)
    _assert_same_positions(out[:, 0, :], x, ei, 1e-5, j1, j2)
