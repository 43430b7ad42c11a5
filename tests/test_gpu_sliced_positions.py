"""Position records of the feature-sliced product (csrc/gcn_sliced.hip): one 8-byte record
{row, deg^-1/2} per row position, written by the cold build in front of the entry blocks, read by the product's epilogue
instead of order[pos], two gathers of rowptr and a divide and square root per (position, slice).

DIFFORMER_SLICED_POSITIONS=0 builds the format without records and runs the gathering epilogue.  The record holds the value of
the same expression, so every product here is computed under both settings and the two outputs must be equal bit for bit; with
the records the output is held to the float64 oracle at 1e-5, the bound of test_gpu_sliced.py.  A product that brings its own
dinv vector (the adjoint) never reads the records.

Shapes: 8,205 rows (one tile, 129 slots: a partial last slot, and a last round of one slot on 128 (panel, wave) pairs); 40,000
rows (4 tiles, 3 rounds) and its 2-way row shard (source splits: the records are read by the combine kernel, row_begin > 0);
a skewed graph whose hub rows are split into parts and leave empty positions; one row without incoming entries (scale 0)."""
import numpy as np
import pytest
import torch

from conftest import rel_err
from guarded import poisoned_allocations  # noqa: F401  (the fixture)
from oracle import difformer_oracle as orc
from sliced_format import check_format, dev, env, ragged_graph, records, skewed_graph  # noqa: F401  (dev, env: fixtures)

D = 64


_CASES = {}


def _case(name):
    """(n, edge_index, x [n, 1, D], float64 oracle [n, D]) -- built once, shared, never modified."""
    if name not in _CASES:
        n, ei = {"one_tile": lambda: (8205, ragged_graph(8205, 47, 59, 1)),
                 "four_tiles": lambda: (40000, ragged_graph(40000, 59, 59, 2)),
                 # half of the entries of a 64-per-row graph go to 40 hub rows
                 "skewed": lambda: (12000, skewed_graph(12000, None, 3, base=ragged_graph(12000, 63, 63, 3))),
                 "orphan": lambda: (8205, ragged_graph(8205, 47, 59, 4, orphan=4321))}[name]()
        x = torch.randn(n, 1, D, generator=torch.Generator().manual_seed(n))
        ref = orc.gcn_conv(x.double().numpy(), ei.numpy(), None)[:, 0, :]
        _CASES[name] = (n, ei, x, ref)
    return _CASES[name]


def _check_records(sl, csr, lo, cnt):
    """Rows: order (or the natural order) padded with -1 to whole slots; scales: deg^-1/2 of the CSR's row lengths."""
    G = int(sl.plan[2])
    row, scale = records(sl)
    want = torch.full((G * 64,), -1, dtype=torch.int32, device=row.device)
    n_pos = cnt if sl.n_pos is None else sl.n_pos
    want[:n_pos] = sl.order if sl.order is not None else torch.arange(cnt, dtype=torch.int32, device=row.device)
    assert torch.equal(row, want)
    live = row >= 0
    deg = (csr.rowptr[1:] - csr.rowptr[:-1])[lo + row[live].long()].double()
    ref = torch.where(deg > 0, deg.clamp(min=1).rsqrt(), torch.zeros_like(deg))
    assert float((scale[live].double() - ref).abs().max()) <= 2.0 ** -23          # one rounding of a value <= 1, twice over
    assert bool((scale[~live] == 0).all())


def _forward(name, dev, env, schedule=None, slots=None):
    """gcn_conv of a case with the records and without -> (out_on, format_on, format_off); asserts the two are bit-identical."""
    from difformer_amd import gcn_conv, ops
    n, ei, x, ref = _case(name)
    eid, xd = ei.to(dev), x.to(dev)
    got = {}
    for positions in ("1", "0"):
        env(schedule, slots, positions)
        csr = ops.csr_cache.get(eid, None, n, D * 4)
        sl = csr.sliced(0, n, D)
        assert sl is not None and sl.positions == (positions == "1")
        if sl.positions:
            _check_records(sl, csr, 0, n)
        got[positions] = (gcn_conv(xd, eid, None)[:, 0, :], sl)
    assert torch.equal(got["1"][0], got["0"][0])
    assert torch.equal(got["1"][1].entries, got["0"][1].entries) and torch.equal(got["1"][1].table, got["0"][1].table)
    assert rel_err(got["1"][0].cpu().numpy(), ref) < 1e-5
    return got["1"][0], got["1"][1], got["0"][1]


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["strict", "packed"])
def test_one_tile_partial_slot_and_partly_empty_last_round(schedule, dev, env):
    _, sl, _ = _forward("one_tile", dev, env, schedule)
    slices, panels, G, PW, W, R, T, NT = (int(v) for v in sl.plan)
    assert NT == 1 and G == 129 and 8205 % 64 != 0 and R >= 2 and G < R * PW
    assert sl.quad_cap == (2 if schedule == "packed" else 1)


@pytest.mark.gpu
def test_four_tiles_three_rounds_packed_and_dealt(dev, env):
    _, sl, _ = _forward("four_tiles", dev, env, "packed", "dealt")
    slices, panels, G, PW, W, R, T, NT = (int(v) for v in sl.plan)
    assert NT == 4 and R == 3 and sl.quad_cap == 2 and sl.order is not None


@pytest.mark.gpu
def test_skewed_graph_with_split_rows_and_empty_positions(dev, env):
    _, sl, _ = _forward("skewed", dev, env)
    assert sl.parts is not None and sl.n_pos is not None
    assert int((sl.parts.to(torch.int32) >> 8).max()) > 1, "no row was split into parts"
    assert int((sl.order < 0).sum()) > 0, "no empty position"


@pytest.mark.gpu
def test_row_without_incoming_entries_is_zero(dev, env):
    out, sl, _ = _forward("orphan", dev, env)
    row, scale = records(sl)
    assert float(scale[row == 4321]) == 0.0
    assert bool((out[4321] == 0).all()) and bool(torch.isfinite(out).all())


@pytest.mark.gpu
def test_both_ranks_of_a_two_way_row_shard(dev, env):
    """Source splits (S > 1): the partial sums meet in sliced_combine_kernel, which reads the records; rank 1 has row_begin > 0."""
    from difformer_amd import ops
    from difformer_amd.dist import RowShard
    n, ei, x, ref = _case("four_tiles")
    eid, x2 = ei.to(dev), x[:, 0, :].to(dev).contiguous()
    for rank in (0, 1):
        sh = RowShard(n, rank=rank, world=2)
        lo, cnt = sh.row_begin, sh.n_local
        got = {}
        for positions in ("1", "0"):
            env("packed", "dealt", positions)
            be = ops.get_backend()
            csr = ops.csr_cache.get(eid, None, n, D * 4, sh)
            sl = csr.sliced(lo, cnt, D)
            assert sl is not None and sl.positions == (positions == "1")
            assert be.lib.dif_sliced_spmm_workspace_bytes(n, cnt, D) > 0, "this shard should take source splits"
            if sl.positions:
                _check_records(sl, csr, lo, cnt)
            ys = be.sliced_prescale(x2, csr.rowptr, n, sl.plan)
            got[positions] = be.sliced_spmm(sl, ys, csr.rowptr, n, lo, cnt, D)
        assert lo > 0 or rank == 0
        assert torch.equal(got["1"], got["0"]), rank
        assert rel_err(got["1"].cpu().numpy(), ref[lo: lo + cnt]) < 1e-5, rank


@pytest.mark.gpu
def test_a_product_with_its_own_dinv_keeps_the_gathering_epilogue(dev, env):
    """The adjoint product passes the forward graph's dinv: same bits with and without records, through the backward pass and
    through a direct call on a format that HAS records with a dinv that is not the one of the row lengths."""
    from difformer_amd import gcn_conv, ops
    n, ei, x, _ = _case("one_tile")
    eid = ei.to(dev)
    gout = torch.randn(n, 1, D, generator=torch.Generator().manual_seed(9)).to(dev)
    dinv = (0.5 + torch.rand(n, generator=torch.Generator().manual_seed(10))).to(dev)
    grads, direct = {}, {}
    for positions in ("1", "0"):
        env(positions=positions)
        xd = x.to(dev).requires_grad_(True)
        gcn_conv(xd, eid, None).backward(gout)
        grads[positions] = xd.grad.clone()
        be = ops.get_backend()
        csr = ops.csr_cache.get(eid, None, n, D * 4)
        adj = csr.adjoint().sliced(0, n, D)
        assert adj is not None and not adj.positions
        sl = csr.sliced(0, n, D)
        assert sl.positions == (positions == "1")
        ys = be.sliced_prescale(x[:, 0, :].to(dev).contiguous(), csr.rowptr, n, sl.plan)
        direct[positions] = (be.sliced_spmm(sl, ys, csr.rowptr, n, 0, n, D, dinv=dinv), be.sliced_spmm(sl, ys, csr.rowptr, n, 0, n, D))
    assert torch.equal(grads["1"], grads["0"])
    assert torch.equal(direct["1"][0], direct["0"][0]) and torch.equal(direct["1"][1], direct["0"][1])
    assert not torch.equal(direct["1"][0], direct["1"][1])             # the caller's dinv was used, not the records


@pytest.mark.gpu
def test_two_calls_and_a_graph_replay_of_a_two_layer_forward_agree(dev, env):
    from difformer_amd import DIFFormer, GraphedForward, ops
    env(positions="1")
    torch.manual_seed(7)
    n, ei, _, _ = _case("one_tile")
    model = DIFFormer(24, D, 5, num_layers=2, kernel="simple").to(dev).eval()
    x = torch.randn(n, 24, generator=torch.Generator().manual_seed(8)).to(dev)
    eid = ei.to(dev)
    be = ops.get_backend()
    be.kernel_events = {}
    with torch.no_grad():
        a = model(x, eid).clone()
    launched, be.kernel_events = set(be.kernel_events), None
    assert "dif_sliced_spmm_f32" in launched
    assert ops.csr_cache.get(eid, None, n, D * 4).sliced(0, n, D).positions
    with torch.no_grad():
        b = model(x, eid).clone()
    fwd = GraphedForward(model, x, eid)
    assert torch.equal(a, b) and torch.equal(fwd(x), a) and torch.equal(fwd(x), a)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_tile", "skewed"])
def test_records_between_guard_bands(name, dev, env, poisoned_allocations):
    """The allocation that carries the records and the blocks comes poisoned and between guard bands (tests/guarded.py): every
    record the product reads was written by the build (a poisoned one is row -1 / scale NaN: rows would be missing from the
    output, which is itself poisoned), and nothing is written outside the allocation."""
    out, sl, _ = _forward(name, dev, env)
    assert bool(torch.isfinite(out).all())
    row, scale = records(sl)
    assert bool(torch.isfinite(scale).all())
    poisoned_allocations.check()


@pytest.mark.gpu
@pytest.mark.parametrize("schedule", ["strict", "packed"])
def test_the_format_checker_fails_on_a_corrupted_format(schedule, dev, env):
    """check_format (tests/sliced_format.py) on host copies of the smallest format there is -- one tile, a partial last slot,
    a partly empty last round: it passes on the copy as built and raises for each of five single corruptions.  Every
    corruption keeps what the other rules look at (a cell that changes keeps its bank quad where the content is the point,
    and its content where the bank rule is), so each rule is shown to fail on its own.  No kernel sees the corrupted data."""
    from types import SimpleNamespace

    from difformer_amd import ops
    from sliced_format import HW_GROUPS
    n, ei, _, _ = _case("one_tile")
    env(schedule)
    csr = ops.csr_cache.get(ei.to(dev), None, n, D * 4)
    sl = csr.sliced(0, n, D)
    cap = 2 if schedule == "packed" else 1
    assert list(sl.plan) == [16, 16, 129, 80, 5, 2, 8208, 1] and sl.quad_cap == cap and sl.parts is None
    R, T = int(sl.plan[5]), int(sl.plan[6])
    host_csr = SimpleNamespace(n_blocks=csr.n_blocks, rowptr=csr.rowptr.cpu(), src=csr.src.cpu(), blkptr=None)
    entries, table = sl.entries.cpu().numpy(), sl.table.cpu().numpy()
    order = None if sl.order is None else sl.order.cpu()

    def check(e=entries, t=table):
        copy = SimpleNamespace(plan=sl.plan, entries=torch.from_numpy(e), table=torch.from_numpy(t), order=order, parts=None,
                               n_pos=None, quad_cap=cap)
        return check_format(copy, ei, n, host_csr)

    def cells(a):                                   # [block, lane, step] view of a flat entry array
        return a.view(np.uint16).reshape(-1, 64, 8)[: int(table[-1])]
    check()                                         # as built
    ent0, grp = cells(entries), HW_GROUPS[0]
    # (a) / (b): `cap` zero-row reads of a lane group move onto the quad of one more of its lanes -> cap + 1 lanes on it
    b, s = np.argwhere((ent0[:, grp, :] >= T).sum(axis=1) >= cap)[0]
    moved = [k for k in grp if ent0[b, k, s] >= T][:cap]
    other = next(k for k in grp if k not in moved)
    e = entries.copy()
    cells(e)[b, moved, s] = T + (ent0[b, other, s] & 15)
    with pytest.raises(AssertionError, match="more than two lanes" if cap == 2 else "bank conflict"):
        check(e)

    def alone(b, k, s):                             # no other lane of its lane group reads this cell's quad in this step
        lanes = next(g for g in HW_GROUPS if k in g)
        return int(((ent0[b, lanes, s] & 15) == (ent0[b, k, s] & 15)).sum()) == 1
    # (c) one real entry becomes a zero-row read of the same quad
    b, k, s = next(c for c in np.argwhere(ent0 < T) if alone(*c))
    e = entries.copy()
    cells(e)[b, k, s] = T + (ent0[b, k, s] & 15)
    with pytest.raises(AssertionError):
        check(e)
    # (d) two lanes of a lane group exchange their entries of one step
    k0, k1 = grp[:2]
    b, s = next((b, s) for b, s in np.argwhere((ent0[:, [k0, k1], :] < T).all(axis=1)) if ent0[b, k0, s] != ent0[b, k1, s])
    e = entries.copy()
    cells(e)[b, [k0, k1], s] = ent0[b, [k1, k0], s]
    with pytest.raises(AssertionError):
        check(e)
    # (e) a table row whose round lengths increase
    t = table.copy()
    rows = t[:-1].reshape(-1, R + 1)
    i = int(np.argwhere(rows[:, 1] > rows[:, R])[0, 0])
    rows[i, [1, R]] = rows[i, [R, 1]]
    with pytest.raises(AssertionError, match="round lengths"):
        check(t=t)


def test_switch_rejects_unknown_values(monkeypatch):
    from difformer_amd import sliced
    for v, want in (("1", True), ("0", False), ("", True), (" 1 ", True)):
        monkeypatch.setenv("DIFFORMER_SLICED_POSITIONS", v)
        assert sliced.sliced_positions() is want
    monkeypatch.delenv("DIFFORMER_SLICED_POSITIONS")
    assert sliced.sliced_positions() is True
    for v in ("2", "on", "true", "-1"):
        monkeypatch.setenv("DIFFORMER_SLICED_POSITIONS", v)
        with pytest.raises(ValueError):
            sliced.sliced_positions()


def test_backend_sizes_the_record_section_from_the_plan():
    from difformer_amd.sliced import SlicedPlan
    plan = SlicedPlan(16 | 1 << 16, 16, 2071, 240, 15, 9, 10208, 13)
    assert plan.record_elems == 0                                              # no bit: no records
    run = plan.with_records(True)
    assert list(plan) == [16 | 1 << 16, 16, 2071, 240, 15, 9, 10208, 13]       # the caller's plan stays as it is
    assert run[0] == 16 | 1 << 16 | 1 << 18 and list(run)[1:] == list(plan)[1:]
    assert run.record_elems * 2 == 2071 * 64 * 8                               # 8 bytes per position of every slot, int16 elements
    assert run.record_elems * 2 % 512 == 0                                     # the blocks behind them keep their alignment
    assert list(run.with_records(False)) == list(plan)
    assert (plan.slices, plan.panels, plan.G, plan.PW, plan.W, plan.R, plan.T, plan.NT) == (16, 16, 2071, 240, 15, 9, 10208, 13)
