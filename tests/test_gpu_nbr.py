"""Batched neighbour graphs on the MI355X (csrc/nbr_batched.hip behind include/difformer_nbr.h; difformer_amd.knn_graph with
batch= / n_nodes=, difformer_amd.radius_graph): index equality with the float64 oracle of tests/nbr_ref.py over the shared case
table, exact ties, equality with the single-graph calls, NaN rows, views and dtypes, guard bands, and the wide-row loop.

Which case reaches which instantiation of nbr_kernel<MQ, K, COS, RADIUS>: MQ = 4 at M = 1..4, 8 at M = 5, 16 at M = 16, 32 at
M = 17, 64 at M = 64; k-NN K = 8 at k = 1, 5 and 24 at k = 24 (16 at k = 12: the tie test); radius K = 8 at cap = 1, 5 and 32 at
cap = 32 (16 at cap = 12: the tie test).  `edges` puts graph boundaries at rows 63, 64, 128 and 193 (inside, at and next to a
wave's first row), `empties` empty graphs at the front, in the middle and at the end, `big` a graph that 17 waves share.
"""
import functools

import numpy as np
import pytest
import torch

from guarded import GuardedArena, guarded_inputs
import knn_ref
import nbr_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLOWS = ("source_to_target", "target_to_source")


@pytest.fixture(scope="module")
def nbr():
    from difformer_amd import _lib
    return _lib.load_nbr()


@functools.lru_cache(maxsize=6)
def _case(name, m, cosine=False):
    """The shared case and its oracle distances, computed once and left unchanged."""
    return nbr_ref.case(name, m, cosine)


def _groups(batch, by_batch):
    """The batch as the public functions take it: batch= (graph ids on the device) or n_nodes= (a host list)."""
    if by_batch:
        return dict(batch=torch.from_numpy(batch.batch_vector()).to(DEV))
    return dict(n_nodes=torch.tensor(batch.n_nodes))


def _np(out, want_dist):
    ei, dist = out if want_dist else (out, None)
    return ei.cpu().numpy(), None if dist is None else dist.cpu().numpy()


# ---- the whole case table through the checker ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m", nbr_ref.WIDTHS)
@pytest.mark.parametrize("name", list(nbr_ref.N_NODES))
def test_batched_knn_graph_equals_the_oracle(name, m):
    from difformer_amd import knn_graph
    turn = 0
    for cosine in ((False, True) if m >= nbr_ref.MIN_COSINE_WIDTH else (False,)):
        batch = _case(name, m, cosine)
        xd = torch.from_numpy(batch.x).to(DEV)
        groups = _groups(batch, by_batch=(m + len(name)) % 2 == 0)
        for loop in (False, True):
            for k in knn_ref.KS:
                flow, want_dist = FLOWS[turn % 2], turn % 3 != 0             # both flows, with and without distances, in every case
                turn += 1
                out = knn_graph(xd, k, loop=loop, flow=flow, cosine=cosine, return_distance=want_dist, **groups)
                ei, dist = _np(out, want_dist)
                nbr_ref.check_edges(ei, dist, batch, nbr_ref.batched_knn_rows(batch, k, loop), nbr_ref.knn_ill_posed(batch, k, loop),
                                    loop, 1 if flow == FLOWS[0] else 0, f"knn {name} M={m} k={k} loop={loop} cosine={cosine}")


@pytest.mark.parametrize("m", nbr_ref.WIDTHS)
@pytest.mark.parametrize("name", list(nbr_ref.N_NODES))
def test_radius_graph_equals_the_oracle(name, m):
    from difformer_amd import radius_graph
    batch = _case(name, m)
    xd = torch.from_numpy(batch.x).to(DEV)
    groups = _groups(batch, by_batch=(m + len(name)) % 2 == 1)
    turn = 0
    for loop in (False, True):
        for r in nbr_ref.RADII:
            for cap in nbr_ref.CAPS:
                flow, want_dist = FLOWS[turn % 2], turn % 3 != 0
                turn += 1
                out = radius_graph(xd, r, loop=loop, max_num_neighbors=cap, flow=flow, return_distance=want_dist, **groups)
                ei, dist = _np(out, want_dist)
                nbr_ref.check_edges(ei, dist, batch, nbr_ref.radius_rows(batch, r, loop, cap),
                                    nbr_ref.radius_ill_posed(batch, r, loop, cap), loop, 1 if flow == FLOWS[0] else 0,
                                    f"radius {name} M={m} r={r} cap={cap} loop={loop}")


def test_radius_graph_without_a_batch_is_one_graph():
    from difformer_amd import radius_graph
    x = knn_ref.inputs(300, 3, seed=3)
    batch = nbr_ref.Batch(x, [300])
    ei, dist = radius_graph(torch.from_numpy(x).to(DEV), 1.0, loop=True, return_distance=True)
    nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), batch, nbr_ref.radius_rows(batch, 1.0, True, 32),
                        nbr_ref.radius_ill_posed(batch, 1.0, True, 32), True, 1, "radius, no batch")
    assert ei.dtype == torch.int64 and ei.device.type == "cuda" and not dist.requires_grad


# ---- exact ties -----------------------------------------------------------------------------------------------------------------
TIE_NODES = [100, 0, 157]


@pytest.mark.parametrize("m", [4, 20])
def test_exact_ties_go_to_the_lower_index_inside_the_graph(m):
    """Integer features: every distance is exact and every row has exact ties; 65 copies of one point lie spread over BOTH
    graphs, so the nearest rows of a copy in one graph are copies in the other.  The WHOLE edge list equals the oracle's."""
    from difformer_amd import knn_graph
    x = knn_ref.integer_inputs(257, m, crowd=64)
    batch = nbr_ref.Batch(x, TIE_NODES)
    copies = np.nonzero((x == x[0]).all(axis=1))[0]
    assert (copies < 100).sum() > 5 and (copies >= 100).sum() > 32
    xd = torch.from_numpy(x).to(DEV)
    for loop in (False, True):
        for k in knn_ref.KS + (12,):
            ei, dist = knn_graph(xd, k, loop=loop, return_distance=True, n_nodes=torch.tensor(TIE_NODES))
            rows = nbr_ref.batched_knn_rows(batch, k, loop)
            assert np.array_equal(ei.cpu().numpy(), nbr_ref.edge_list(rows, 1)), f"M={m} k={k} loop={loop}"
            nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), batch, rows, None, loop, 1, f"ties M={m} k={k}", exact=True)


@pytest.mark.parametrize("m", [4, 20])
def test_radius_is_strict_at_the_boundary_and_keeps_the_nearest_of_a_crowd(m):
    """r^2 = 1, 4, 9 (M = 4) and 49, 64, 81 (M = 20) are distances that occur exactly: the strict `<` is decided AT the boundary.
    A copy in the second graph has 35 other copies around it at distance 0: more than the cap of 32 (and of 12, and of 5)."""
    from difformer_amd import radius_graph
    x = knn_ref.integer_inputs(257, m, crowd=64)
    batch = nbr_ref.Batch(x, TIE_NODES)
    xd = torch.from_numpy(x).to(DEV)
    for r in {4: (1.0, 2.0, 3.0), 20: (7.0, 8.0, 9.0)}[m]:
        at_boundary = sum(int((d == r * r).sum()) for _, _, d in batch.graphs)
        assert at_boundary > 0
        for loop in (False, True):
            for cap in (5, 12, 32):
                rows = nbr_ref.radius_rows(batch, r, loop, cap)
                uncut = nbr_ref.radius_rows(batch, r, loop, batch.n)
                assert any(len(u) > cap for u in uncut), (r, cap)                  # the crowd exceeds the cap
                ei, dist = radius_graph(xd, r, loop=loop, max_num_neighbors=cap, return_distance=True, n_nodes=torch.tensor(TIE_NODES))
                assert np.array_equal(ei.cpu().numpy(), nbr_ref.edge_list(rows, 1)), f"M={m} r={r} cap={cap} loop={loop}"
                nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), batch, rows, None, loop, 1, f"radius ties M={m} r={r}", exact=True)


# ---- equality with the past -------------------------------------------------------------------------------------------------------
def _per_graph(xd, n_nodes, k, loop, cosine):
    """Today's knn_graph graph by graph, indices offset, concatenated."""
    from difformer_amd import knn_graph
    parts, lo = [], 0
    for nb in n_nodes:
        if nb - (0 if loop else 1) > 0:
            ei, dist = knn_graph(xd[lo:lo + nb], k, loop=loop, cosine=cosine, return_distance=True)
            parts.append((ei + lo, dist))
        lo += nb
    return torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts])


@pytest.mark.parametrize("m", [4, 20])
def test_batched_equals_the_per_graph_calls_bitwise_on_integer_inputs(m):
    from difformer_amd import knn_graph
    n_nodes = [100, 0, 157, 1, 70]
    xd = torch.from_numpy(knn_ref.integer_inputs(sum(n_nodes), m, crowd=64)).to(DEV)
    for loop in (False, True):
        for k in knn_ref.KS:
            ei, dist = knn_graph(xd, k, loop=loop, return_distance=True, n_nodes=torch.tensor(n_nodes))
            want_ei, want_dist = _per_graph(xd, n_nodes, k, loop, False)
            assert torch.equal(ei, want_ei) and torch.equal(dist.view(torch.int32), want_dist.view(torch.int32)), (m, k, loop)


@pytest.mark.parametrize("name,m", [("mixed", 3), ("edges", 16), ("big", 5), ("tiny", 64)])
def test_batched_and_per_graph_calls_pass_the_same_checker(name, m):
    for cosine in (False, True):
        batch = _case(name, m, cosine)
        xd = torch.from_numpy(batch.x).to(DEV)
        for loop in (False, True):
            ei, dist = _per_graph(xd, batch.n_nodes, 5, loop, cosine)
            nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), batch, nbr_ref.batched_knn_rows(batch, 5, loop),
                                nbr_ref.knn_ill_posed(batch, 5, loop), loop, 1, f"per graph {name} M={m} loop={loop} cosine={cosine}")


def test_without_a_batch_knn_graph_is_bitwise_what_it_was():
    from difformer_amd import knn_graph, ops
    be = ops.get_backend()
    for n, m in ((129, 4), (700, 64)):
        xd = torch.from_numpy(knn_ref.inputs(n, m)).to(DEV)
        for loop, cosine in ((False, False), (True, True)):
            be.kernel_events = events = {}
            try:
                ei, dist = knn_graph(xd, 5, loop=loop, cosine=cosine, return_distance=True)
            finally:
                be.kernel_events = None
            assert set(events) == {"dif_knn_graph_f32"}                          # today's path, not the batched kernel
            want_ei, want_dist = be.knn_graph(xd, 5, loop, 1 if cosine else 0, 1, want_dist=True)
            assert torch.equal(ei, want_ei) and torch.equal(dist.view(torch.int32), want_dist.view(torch.int32))


# ---- NaN rows -------------------------------------------------------------------------------------------------------------------
def test_a_nan_feature_stays_inside_its_graph():
    from difformer_amd import knn_graph, radius_graph
    n_nodes = [40, 20, 60]
    x = knn_ref.inputs(120, 3, seed=9)
    bad = 50                                                                    # a row of the middle graph
    xn = x.copy()
    xn[bad, 1] = np.nan
    clean, dirty = torch.from_numpy(x).to(DEV), torch.from_numpy(xn).to(DEV)
    nn = torch.tensor(n_nodes)
    for loop in (False, True):
        a, da = _np(knn_graph(clean, 24, loop=loop, return_distance=True, n_nodes=nn), True)
        b, db = _np(knn_graph(dirty, 24, loop=loop, return_distance=True, n_nodes=nn), True)
        assert a.shape == b.shape
        outside = (a[1] < 40) | (a[1] >= 60)
        assert np.array_equal(a[:, outside], b[:, outside]) and np.array_equal(da[outside].view(np.int32), db[outside].view(np.int32))
        mine = b[0][b[1] == bad]                                                # every distance a NaN: the index order
        assert mine.tolist() == [j for j in range(40, 60) if loop or j != bad] and np.isnan(db[b[1] == bad]).all()
        for i in range(40, 60):                                                 # 20 nodes, k = 24: every list holds the whole graph,
            row = b[0][b[1] == i]                                               # the NaN row last
            if i != bad:
                assert row[-1] == bad and len(row) == (20 if loop else 19) and not np.isnan(db[b[1] == i][:-1]).any()
        a, da = _np(radius_graph(clean, 2.0, loop=loop, return_distance=True, n_nodes=nn), True)
        b, db = _np(radius_graph(dirty, 2.0, loop=loop, return_distance=True, n_nodes=nn), True)
        assert np.array_equal(a[:, (a[1] < 40) | (a[1] >= 60)], b[:, (b[1] < 40) | (b[1] >= 60)])
        assert not (b == bad).any() and not np.isnan(db).any()                  # never inside a radius: no edge, not even its self-loop
        keep = (a != bad).all(axis=0)                                           # the clean graph without the row's edges
        assert np.array_equal(a[:, keep], b) and np.array_equal(da[keep].view(np.int32), db.view(np.int32))


# ---- views, widths, dtypes, host tensors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [6, 17])
def test_views_dtypes_and_host_tensors(m):
    """bfloat16 and float64 are rounded to float32 first (the oracle applies the same rounding); a strided or offset x and an odd
    width are copied / zero-padded; a host tensor is staged and its result comes back on the host, equal to the device's."""
    from difformer_amd import knn_graph, radius_graph
    n_nodes = [70, 1, 79]
    nn = torch.tensor(n_nodes)
    g = torch.Generator().manual_seed(m)
    x64 = torch.randn(150, m, dtype=torch.float64, generator=g)
    mp = -(-m // 4) * 4
    flat = torch.randn(150 * m + 1, generator=g).to(DEV)
    odd = torch.randn(150, m + 1, generator=g).to(DEV)
    wide = torch.randn(150, mp + 8, generator=g).to(DEV)
    r = 0.8 * float(np.sqrt(2 * m))                                             # about a fifth of a graph inside: the cap of 5 cuts most rows
    for x in (x64.to(DEV), x64.bfloat16().to(DEV), x64.float().t().contiguous().t().to(DEV),
              torch.randn(150, 2 * m, generator=g).to(DEV)[:, ::2], flat[1:].view(150, m), odd[:, :m], wide[:, 4:4 + mp]):
        batch = nbr_ref.Batch(x.float().cpu().numpy(), n_nodes)
        what = f"{x.dtype} {tuple(x.stride())}"
        ei, dist = knn_graph(x, 5, loop=True, return_distance=True, n_nodes=nn)
        nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), batch, nbr_ref.batched_knn_rows(batch, 5, True),
                            nbr_ref.knn_ill_posed(batch, 5, True), True, 1, "knn " + what)
        ei, dist = radius_graph(x, r, loop=False, max_num_neighbors=5, return_distance=True, n_nodes=nn)
        assert sum(len(v) for v in nbr_ref.radius_rows(batch, r, False, 5)) > 150          # the inputs: not a vacuous case
        nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), batch, nbr_ref.radius_rows(batch, r, False, 5),
                            nbr_ref.radius_ill_posed(batch, r, False, 5), False, 1, "radius " + what)
    host = x64.float()
    ids = torch.from_numpy(batch.batch_vector())
    for fn, arg in ((knn_graph, 5), (radius_graph, r)):
        on_dev = fn(host.to(DEV), arg, return_distance=True, batch=ids.to(DEV))
        on_host = fn(host, arg, return_distance=True, batch=ids)
        assert all(h.device.type == "cpu" and torch.equal(h, d.cpu()) for h, d in zip(on_host, on_dev))
        again = fn(host.to(DEV), arg, return_distance=True, n_nodes=nn)         # two calls (and the two ways to name the batch): bitwise equal
        assert torch.equal(again[0], on_dev[0]) and torch.equal(again[1].view(torch.int32), on_dev[1].view(torch.int32))


def test_launches_and_the_layout_cache():
    """One launch for the batched k-NN, two for the radius; the layout is the one `ops.layout_cache` holds for the tensor."""
    from difformer_amd import knn_graph, ops, radius_graph
    batch = _case("tiny", 3)
    xd = torch.from_numpy(batch.x).to(DEV)
    nn = torch.tensor(batch.n_nodes)
    be = ops.get_backend()
    be.kernel_events = events = {}
    try:
        ei = knn_graph(xd, 5, loop=True, n_nodes=nn)
        radius_graph(xd, 1.0, loop=True, n_nodes=nn)
    finally:
        be.kernel_events = None
    assert {k: len(v) for k, v in events.items()} == {"dif_nbr_knn_f32": 1, "dif_nbr_radius_lists_f32": 1, "dif_nbr_radius_edges": 1}
    assert ei.shape == (2, batch.n * 5) and ops.layout_cache.get(nn, xd.device) is ops.layout_cache.get(nn, xd.device)


# ---- wide rows: the per-graph loop ----------------------------------------------------------------------------------------------
def test_rows_wider_than_the_batched_kernel_loop_over_the_graphs():
    from difformer_amd import knn_graph, ops, radius_graph
    n_nodes = [33, 1, 0, 40]
    batch = nbr_ref.Batch(knn_ref.inputs(74, 68, seed=68), n_nodes)
    xd = torch.from_numpy(batch.x).to(DEV)
    be = ops.get_backend()
    for loop in (False, True):
        be.kernel_events = events = {}
        try:
            ei, dist = knn_graph(xd, 5, loop=loop, return_distance=True, n_nodes=torch.tensor(n_nodes))
        finally:
            be.kernel_events = None
        assert set(events) == {"dif_knn_graph_f32"} and len(events["dif_knn_graph_f32"]) == (3 if loop else 2)
        nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), batch, nbr_ref.batched_knn_rows(batch, 5, loop),
                            nbr_ref.knn_ill_posed(batch, 5, loop), loop, 1, f"M=68 loop={loop}")
    with pytest.raises(ValueError, match="64"):
        radius_graph(xd, 1.0, n_nodes=torch.tensor(n_nodes))


# ---- guard bands and poison: every entry point through the C ABI -------------------------------------------------------------------
def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("min_align", [False, True])
@pytest.mark.parametrize("m", [4, 64])
@pytest.mark.parametrize("name", ["edges", "empties"])
def test_between_guard_bands(nbr, name, m, min_align):
    """Operands between NaN / -1 bands (rows padded: the tail of every row is NaN too), outputs and workspace poisoned (0xFF)
    between checked guard bands, at 512-byte alignment and at the minimum each operand documents (x and workspace 16 bytes,
    int64 tables and edge_index 8, int32 tables, deg and distances 4)."""
    from difformer_amd import _lib
    batch = _case(name, m)
    n, B = batch.n, len(batch.n_nodes)
    ld = m + 4
    arena = GuardedArena()
    off = (lambda b: b) if min_align else (lambda b: 0)
    ptr32 = torch.from_numpy(batch.ptr.astype(np.int32))
    xd, = guarded_inputs(arena, DEV, off(16), x=(torch.from_numpy(batch.x), ld))
    gp, = guarded_inputs(arena, DEV, off(4), graph_ptr=ptr32)
    for k, loop, cosine in ((5, True, False), (24, False, True)):
        cb = _case(name, m, cosine)
        rows = nbr_ref.batched_knn_rows(cb, k, loop)
        counts = np.array([len(r) for r in rows])
        per_graph = np.array([counts[lo:hi].sum() for lo, hi in zip(batch.ptr[:-1], batch.ptr[1:])])
        ep, = guarded_inputs(arena, DEV, off(8), edge_ptr=torch.from_numpy(np.concatenate([[0], np.cumsum(per_graph)]).astype(np.int64)))
        E = int(counts.sum())
        ei = arena.alloc((2, E), torch.int64, DEV, offset_bytes=off(8))
        dist = arena.alloc((E,), torch.float32, DEV, offset_bytes=off(4))
        rc = nbr.dif_nbr_knn_f32(xd.data_ptr(), ld, n, m, gp.data_ptr(), ep.data_ptr(), B, k, int(loop), int(cosine), 0, ei.data_ptr(), E,
                                 dist.data_ptr(), _stream())
        _lib.check_nbr(rc, "dif_nbr_knn_f32")
        arena.check()
        nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), cb, rows, nbr_ref.knn_ill_posed(cb, k, loop), loop, 0,
                            f"guarded knn {name} M={m} k={k}")
        xd, = guarded_inputs(arena, DEV, off(16), x=(torch.from_numpy(batch.x), ld))          # checked blocks are forgotten: again
        gp, = guarded_inputs(arena, DEV, off(4), graph_ptr=ptr32)
    r = {4: 2.5, 64: 10.5}[m]                                                      # rows at the cap and rows below it, both caps
    for cap, loop in ((5, True), (32, False)):
        rows = nbr_ref.radius_rows(batch, r, loop, cap)
        counts = np.array([len(x) for x in rows])
        assert counts.max() == cap and counts.min() < cap
        ws_bytes = nbr.dif_nbr_workspace_bytes(n, cap)
        deg = arena.alloc((n,), torch.int32, DEV, offset_bytes=off(4))
        ws = arena.alloc((ws_bytes,), torch.uint8, DEV, offset_bytes=off(16))
        rc = nbr.dif_nbr_radius_lists_f32(xd.data_ptr(), ld, n, m, gp.data_ptr(), B, r, int(loop), cap, deg.data_ptr(), ws.data_ptr(),
                                          ws_bytes, _stream())
        _lib.check_nbr(rc, "dif_nbr_radius_lists_f32")
        torch.cuda.synchronize()
        assert np.array_equal(deg.cpu().numpy(), counts)
        E = int(counts.sum())
        dp, = guarded_inputs(arena, DEV, off(8), deg_ptr=torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)))
        ei = arena.alloc((2, E), torch.int64, DEV, offset_bytes=off(8))
        dist = arena.alloc((E,), torch.float32, DEV, offset_bytes=off(4))
        rc = nbr.dif_nbr_radius_edges(dp.data_ptr(), n, cap, 1, ws.data_ptr(), ws_bytes, ei.data_ptr(), E, dist.data_ptr(), _stream())
        _lib.check_nbr(rc, "dif_nbr_radius_edges")
        arena.check()
        nbr_ref.check_edges(ei.cpu().numpy(), dist.cpu().numpy(), batch, rows, nbr_ref.radius_ill_posed(batch, r, loop, cap), loop, 1,
                            f"guarded radius {name} M={m} cap={cap}")
        xd, = guarded_inputs(arena, DEV, off(16), x=(torch.from_numpy(batch.x), ld))
        gp, = guarded_inputs(arena, DEV, off(4), graph_ptr=ptr32)
    arena.check()
