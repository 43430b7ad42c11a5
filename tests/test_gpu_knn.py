"""k-nearest-neighbour graphs on the MI355X (csrc/knn_graph.hip behind include/difformer_knn.h): index equality with the float64
oracle of tests/knn_ref.py through the C ABI on both routes, the tie rule, NaN rows, guard bands, the Python layer, peak memory,
and the per-snapshot step of the spatial-temporal script.

Which case reaches which kernel instantiation (kk <= 8, <= 16, <= 24 give the list lengths K = 8, 16, 24):
  knn_direct_kernel<MQ, K, COS>     MQ = 4: (1..129, 4), (2, 1) padded, (300, 4); MQ = 8: (1068, 8), (129, 8), (300, 8);
                                    MQ = 16: (33, 16), (700, 16), (300, 16), (300, 12) padded; K = 8 at k = 1, 5, K = 24 at k = 24,
                                    K = 16 at k = 12 (test_direct_list_lengths, the tie matrix); both metrics everywhere
  knn_direct_merge_kernel<K, COS>   every direct shape of more than 64 rows (129, 257, 300, 700, 1068): several key ranges
  knn_prepass / knn_rerank <COS>    every sweep case, both metrics
  knn_sweep_kernel<QREG = true>     M <= 64: (15..33, 20 | 64), (700, 64), (1500, 17 -> 20), (129, 8), (700, 16)
  knn_sweep_kernel<QREG = false>    M > 64: (600, 300), (257, 512)
"""
import functools
import gc

import numpy as np
import pytest
import torch

from guarded import GuardedArena, guarded_inputs
import knn_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def knn():
    from difformer_amd import _lib
    return _lib.load_knn()


@functools.lru_cache(maxsize=None)
def _case(n, m):
    """x [n, m] and its oracle distances per metric, computed once and left unchanged."""
    x = knn_ref.inputs(n, m)
    return x, {cosine: knn_ref.distances(x, cosine) for cosine in (False, True)}


def _pad4(x):
    return np.pad(x, ((0, 0), (0, -x.shape[1] % 4)))


def _launch(knn, xd, ldx, n, m, k, loop, metric, centre_row, route, ei, dist, ws):
    from difformer_amd import _lib
    rc = knn.dif_knn_graph_f32(xd.data_ptr(), ldx, n, m, k, int(loop), metric, centre_row, route, ei.data_ptr(),
                               None if dist is None else dist.data_ptr(), ws.data_ptr(), ws.numel(),
                               torch.cuda.current_stream().cuda_stream)
    _lib.check_knn(rc, "dif_knn_graph_f32")


def _graph(knn, x, k, loop, cosine, centre_row=1, route=-1):
    """The entry point on a column slice of a wider device tensor (ldx > M, rows at the minimum alignment: element 4 of a row of
    M + 8), outputs pre-filled with -1 / NaN, the workspace with 0xFF."""
    xp = _pad4(x)
    n, m = xp.shape
    wide = torch.full((n, m + 8), float("nan"))
    wide[:, 4:4 + m] = torch.from_numpy(xp)
    wd = wide.to(DEV)
    kk = knn_ref.neighbour_count(n, k, loop)
    ei = torch.full((2, n * kk), -1, dtype=torch.int64, device=DEV)
    dist = torch.full((n * kk,), float("nan"), device=DEV)
    ws = torch.full((max(16, knn.dif_knn_workspace_bytes(n, m, k, int(loop), int(cosine), route)),), 0xFF, dtype=torch.uint8, device=DEV)
    _launch(knn, wd[:, 4:], wd.stride(0), n, m, k, loop, int(cosine), centre_row, route, ei, dist, ws)
    torch.cuda.synchronize()
    return ei.cpu().numpy(), dist.cpu().numpy()


def _parity(knn, n, m, route):
    x, d = _case(n, m)
    for cosine in (False, True):
        for loop in (False, True):
            for k in knn_ref.KS:
                ei, dist = _graph(knn, x, k, loop, cosine, route=route)
                knn_ref.check_graph(ei, dist, x, k, loop, cosine, 1, f"route {route} N={n} M={m} k={k} loop={loop} cosine={cosine}",
                                    d=d[cosine])


@pytest.mark.parametrize("n,m", knn_ref.DIRECT_SHAPES)
def test_direct_route_equals_the_oracle(knn, n, m):
    assert knn.dif_knn_route(n, -(-m // 4) * 4, 5) == 0
    _parity(knn, n, m, -1)


@pytest.mark.parametrize("n,m", knn_ref.SWEEP_SHAPES)
def test_sweep_route_equals_the_oracle(knn, n, m):
    assert knn.dif_knn_route(n, -(-m // 4) * 4, 5) == 1
    _parity(knn, n, m, -1)


def test_the_grid_has_split_and_unsplit_launches(knn):
    assert knn.dif_knn_splits(33, 64, 5, 0, -1) == 1 and knn.dif_knn_splits(700, 64, 5, 0, -1) > 1
    assert knn.dif_knn_splits(20, 4, 5, 1, -1) == 1 and knn.dif_knn_splits(1068, 8, 5, 1, -1) > 1


@pytest.mark.parametrize("n,m,k", [(300, 4, 12), (300, 8, 12), (300, 16, 12), (300, 12, 24), (40, 16, 5)])
def test_direct_list_lengths(knn, n, m, k):
    """K = 16 at 4, 8 and 16 columns, a row of 12 columns in the 16-column kernel, one tile of 16 columns."""
    x, d = _case(n, m)
    for cosine in (False, True):
        ei, dist = _graph(knn, x, k, False, cosine)
        knn_ref.check_graph(ei, dist, x, k, False, cosine, 1, f"N={n} M={m} k={k} cosine={cosine}", d=d[cosine])


@pytest.mark.parametrize("n,m", [(129, 8), (700, 16), (33, 16), (33, 20)])
def test_both_sides_of_the_route_threshold(knn, n, m):
    """M = 16 and M = 17 (padded to 20) take different routes; forced onto one shape the two routes give IDENTICAL edge lists."""
    assert knn.dif_knn_route(n, 16, 5) == 0 and knn.dif_knn_route(n, 20, 5) == 1
    x, d = _case(n, m)
    for cosine in (False, True):
        for loop in (False, True):
            for k in knn_ref.KS:
                what = f"N={n} M={m} k={k} loop={loop} cosine={cosine}"
                sweep = _graph(knn, x, k, loop, cosine, route=1)
                knn_ref.check_graph(sweep[0], sweep[1], x, k, loop, cosine, 1, "sweep " + what, d=d[cosine])
                if m <= 16:
                    direct = _graph(knn, x, k, loop, cosine, route=0)
                    assert np.array_equal(direct[0], sweep[0]), what
                    assert np.array_equal(direct[1].view(np.int32), sweep[1].view(np.int32)), what


@pytest.mark.parametrize("crowd", [0, 64])
@pytest.mark.parametrize("m,route", [(4, 0), (20, 1), (4, 1)])
def test_exact_ties_go_to_the_lower_index(knn, m, route, crowd):
    """Integer features: every distance is exact, every row has exact ties and 45 rows are duplicates (M = 4); with crowd = 64,
    65 copies of one point -- more than the sweep's 32 candidates.  The WHOLE edge list equals the oracle's."""
    x = knn_ref.integer_inputs(257, m, crowd=crowd)
    d = knn_ref.distances(x)
    for loop in (False, True):
        for k in knn_ref.KS + (12,):
            ei, dist = _graph(knn, x, k, loop, False, route=route)
            idx, _ = knn_ref.knn_rows(x, k, loop, d=d)
            assert np.array_equal(ei, knn_ref.edge_list(idx, 1)), f"M={m} route={route} crowd={crowd} k={k} loop={loop}"
            knn_ref.check_graph(ei, dist, x, k, loop, False, 1, f"ties M={m} route={route}", d=d, exact=True)
            again, _ = _graph(knn, x, k, loop, False, route=route)
            assert np.array_equal(ei, again)


@pytest.mark.parametrize("n,m,route", [(40, 8, 0), (200, 8, 0), (40, 8, 1), (200, 20, 1)])
@pytest.mark.parametrize("cosine", [False, True])
def test_a_nan_row_ranks_last_and_still_gets_its_neighbours(knn, n, m, route, cosine):
    x = knn_ref.inputs(n, m, seed=7).copy()
    bad = 20
    x[bad, 1] = np.nan
    for loop in (False, True):
        k = 24
        kk = knn_ref.neighbour_count(n, k, loop)
        ei, dist = _graph(knn, x, k, loop, cosine, route=route)
        got = ei[0].reshape(n, kk)
        assert np.array_equal(ei[1], np.repeat(np.arange(n), kk))
        # the NaN row: every distance is a NaN, so the order is the index order
        want = [j for j in range(n) if loop or j != bad][:kk]
        assert got[bad].tolist() == want and np.isnan(dist.reshape(n, kk)[bad]).all()
        others = np.delete(np.arange(n), bad)
        assert not np.isnan(dist.reshape(n, kk)[others]).any() and (got[others] != bad).all()
        idx, _ = knn_ref.knn_rows(x, k, loop, cosine)
        assert np.array_equal(got[others], idx[others])
    # N <= k: every row lists everything, the NaN row last
    small = x[bad - 5:bad + 5].copy()
    ei, dist = _graph(knn, small, 24, True, cosine, route=route)
    got = ei[0].reshape(10, 10)
    assert (np.sort(got, axis=1) == np.arange(10)).all() and (np.delete(got, 5, axis=0)[:, -1] == 5).all()
    assert got[5].tolist() == list(range(10))


@pytest.mark.parametrize("n,m,k,route", [(129, 8, 5, 0), (20, 4, 5, 0), (300, 16, 24, 0), (129, 8, 5, 1), (700, 64, 24, 1), (257, 300, 5, 1)])
@pytest.mark.parametrize("cosine", [False, True])
def test_between_guard_bands(knn, n, m, k, route, cosine):
    """The operand between NaN bands at 16-byte alignment (rows padded: the tail of every row is NaN too), outputs and workspace
    poisoned (0xFF) between checked guard bands."""
    x, d = _case(n, m)
    arena = GuardedArena()
    ld = m + 4
    xd, = guarded_inputs(arena, DEV, True, x=(torch.from_numpy(x), ld))
    kk = knn_ref.neighbour_count(n, k, True)
    ei = arena.alloc((2, n * kk), torch.int64, DEV)
    dist = arena.alloc((n * kk,), torch.float32, DEV)
    ws = arena.alloc((max(16, knn.dif_knn_workspace_bytes(n, m, k, 1, int(cosine), route)),), torch.uint8, DEV, offset_bytes=16)
    _launch(knn, xd, ld, n, m, k, True, int(cosine), 0, route, ei, dist, ws)
    arena.check()
    knn_ref.check_graph(ei.cpu().numpy(), dist.cpu().numpy(), x, k, True, cosine, 0, f"guarded N={n} M={m} route={route}", d=d[cosine])


# ---- the Python layer ----------------------------------------------------------------------------------------------------------
def test_knn_graph_flow_distance_dtypes_and_host_tensors():
    from difformer_amd import knn_graph, ops
    x, d = _case(129, 4)
    xt = torch.from_numpy(x)
    be = ops.get_backend()
    be.kernel_events = events = {}
    try:
        ei, dist = knn_graph(xt.to(DEV), 5, return_distance=True)
    finally:
        be.kernel_events = None
    assert "dif_knn_graph_f32" in events and ei.device.type == "cuda" and ei.dtype == torch.int64 and not dist.requires_grad
    knn_ref.check_graph(ei.cpu().numpy(), dist.cpu().numpy(), x, 5, False, False, 1, "source_to_target", d=d[False])
    swapped = knn_graph(xt.to(DEV), 5, flow="target_to_source")
    assert torch.equal(swapped, ei.flip(0)) and torch.equal(knn_graph(xt.to(DEV), 5), ei)
    host_ei, host_dist = knn_graph(xt, 5, return_distance=True)                  # a host tensor is staged and comes back on the host
    assert host_ei.device.type == "cpu" and torch.equal(host_ei, ei.cpu()) and torch.equal(host_dist, dist.cpu())
    ei, dist = knn_graph(xt.to(DEV), 5, loop=True, cosine=True, return_distance=True)
    knn_ref.check_graph(ei.cpu().numpy(), dist.cpu().numpy(), x, 5, True, True, 1, "cosine", d=d[True])
    assert torch.equal(knn_graph(xt.to(DEV), 5, loop=True, cosine=True, _route=1), ei)
    assert knn_graph(torch.zeros(1, 4, device=DEV), 3).shape == (2, 0)           # one node, no self-loop
    assert knn_graph(torch.zeros(1, 4, device=DEV), 3, loop=True).tolist() == [[0], [0]]


@pytest.mark.parametrize("m", [6, 70])
def test_knn_graph_converts_other_dtypes_and_layouts(m):
    """bfloat16 and float64 are rounded to float32 first (the oracle applies the same rounding); a non-contiguous x and an odd
    width are copied / zero-padded."""
    from difformer_amd import knn_graph
    g = torch.Generator().manual_seed(m)
    x64 = torch.randn(150, m, dtype=torch.float64, generator=g)
    for x in (x64, x64.bfloat16(), x64.float().t().contiguous().t(), torch.randn(150, 2 * m, generator=g)[:, ::2]):
        ref = x.float().numpy()
        ei, dist = knn_graph(x.to(DEV), 5, loop=True, cosine=False, return_distance=True)
        knn_ref.check_graph(ei.cpu().numpy(), dist.cpu().numpy(), ref, 5, True, False, 1, f"{x.dtype} {tuple(x.stride())}")
    # views of device tensors: dense rows one element off the boundary, rows at an odd stride, rows at an aligned stride (no copy)
    mp = -(-m // 4) * 4
    flat = torch.randn(150 * m + 1, generator=g).to(DEV)
    odd = torch.randn(150, m + 1, generator=g).to(DEV)
    wide = torch.randn(150, mp + 8, generator=g).to(DEV)
    for x in (flat[1:].view(150, m), odd[:, :m], wide[:, 4:4 + mp]):
        ei, dist = knn_graph(x, 5, loop=True, cosine=False, return_distance=True)
        knn_ref.check_graph(ei.cpu().numpy(), dist.cpu().numpy(), x.cpu().numpy(), 5, True, False, 1, f"view {tuple(x.stride())}")


@pytest.mark.parametrize("n,m", [(129, 4), (700, 64)])
def test_kneighbors_graph_layout(n, m):
    from difformer_amd import kneighbors_graph
    x, d = _case(n, m)
    for include_self in (False, True):
        ei, dist = kneighbors_graph(torch.from_numpy(x).to(DEV), 5, include_self=include_self, return_distance=True)
        idx, _ = knn_ref.knn_rows(x, 5, include_self, d=d[False])
        assert np.array_equal(ei.cpu().numpy(), knn_ref.edge_list(idx, 0))       # what adj.nonzero() gives
        knn_ref.check_graph(ei.cpu().numpy(), dist.cpu().numpy(), x, 5, include_self, False, 0, "kneighbors_graph", d=d[False])


def test_peak_memory_is_the_workspace_and_the_outputs():
    """N = 15,000, M = 64, k = 5: workspace 19.3 MB + outputs 1.5 MB; one [N, N] float32 tensor is 900 MB.  Slack: 1 MiB for the
    caching allocator's rounding of the three allocations to its 512-byte blocks."""
    from difformer_amd import _lib, kneighbors_graph
    n, m, k = 15000, 64, 5
    x = torch.randn(n, m, device=DEV)
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ei, dist = kneighbors_graph(x, k, include_self=True, return_distance=True)
    torch.cuda.synchronize()
    delta = torch.cuda.max_memory_allocated() - before
    budget = _lib.load_knn().dif_knn_workspace_bytes(n, m, k, 1, 0, -1) + ei.numel() * 8 + dist.numel() * 4
    print(f"peak memory delta {delta / 1e6:.1f} MB, workspace + outputs {budget / 1e6:.1f} MB")
    assert delta <= budget + (1 << 20) and delta < n * n * 4 / 10
    assert ei.shape == (2, n * k) and bool((ei[0] == torch.arange(n, device=DEV).repeat_interleave(k)).all())
    assert bool((ei[1].view(n, k)[:, 0] == torch.arange(n, device=DEV)).all()) and bool((dist.view(n, k)[:, 0] == 0).all())


# ---- the script's step ----------------------------------------------------------------------------------------------------------
def test_the_spatial_temporal_knn_step():
    """spatial-temporal/main.py:96-105 with `--special_treat knn`: per snapshot `knn_graph(x, k=5, loop=True, cosine=True)`, then
    the model on that graph with unit edge weights.  The list equals the oracle's; the model on it equals, bit for bit, the
    model on the oracle's list (same graph, same path)."""
    import st_common
    from difformer_amd import DIFFormer, knn_graph
    name = st_common.cases("cumul")[0]
    torch.manual_seed(0)
    for n, m, seed in [(20, 4, 1), (20, 4, 2), (20, 4, 3), (1068, 8, 4)]:
        c = dict(st_common.ST[name])
        x = knn_ref.inputs(n, m, seed=seed)
        d = knn_ref.distances(x, True)
        assert not knn_ref.ill_posed_rows(d, 5, True).any()
        xd = torch.from_numpy(x).to(DEV)
        ei = knn_graph(xd, k=5, loop=True, cosine=True)                          # main.py:98
        idx, _ = knn_ref.knn_rows(x, 5, True, True, d=d)
        want = torch.from_numpy(knn_ref.edge_list(idx, 1))
        assert torch.equal(ei.cpu(), want)
        cfg, _ = st_common.split_model_case(c)
        model = DIFFormer(m, int(cfg["hidden_channels"]), int(cfg["out_channels"]), num_layers=int(cfg["num_layers"]),
                          alpha=float(cfg["alpha"]), dropout=0.0, num_heads=int(cfg["num_heads"]), kernel=str(cfg["kernel"]),
                          use_bn=bool(cfg["use_bn"]), use_residual=bool(cfg["use_residual"]), use_graph=bool(cfg["use_graph"]),
                          use_weight=bool(cfg["use_weight"])).to(DEV).eval()
        with torch.no_grad():
            E = ei.shape[1]
            y = model(xd, ei, torch.ones(E, device=DEV))                         # main.py:105
            y_ref = model(xd, want.to(DEV), torch.ones(E, device=DEV))
        assert y.shape[0] == n and bool(torch.isfinite(y).all()) and torch.equal(y, y_ref)
