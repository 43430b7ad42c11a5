"""The PACKED schedule of the feature-sliced product (csrc/gcn_sliced.hip): slots formed by tile profile
(sliced.packed_slot_order) and a quad capacity of 2 in the colouring (asked for in the plan record, include/difformer_hip.h).

The schedule is forced through DIFFORMER_SLICED_SCHEDULE so that nothing here depends on the threshold of `auto`, which has
its own test.  Integer work is checked exactly: the format holds every (row, tile) group of the CSR exactly once, in every
step a hardware lane group puts at most 2 lanes on one bank quad, and a zero-row read never shares a quad
(tests/sliced_format.py, check_format at capacity 2).  The product is
held to the float64 oracle at 1e-5, the bound of test_gpu_sliced.py.

Bounds at the headline shape, both from the counts of the graph and not from what the colouring gives:
  * built lane-steps per entry <= 1.05 x the row-envelope prediction (longest row per round, 8-step blocks, non-increasing
    rounds): the quad columns must no longer bind;
  * shared cells <= 2 x their minimum for that build, sum over (slot, tile, lane group, quad) of max(0, column - K) with
    K the built length of the round: a column of C entries needs C - K cells of a K-step round to be second reads.
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import difformer_oracle as orc
from sliced_format import (check_format, dense_graph, dev, headline_stats, product_vs_oracle, schedule,  # noqa: F401
                           skewed_graph)                                   # (dev, schedule: the fixtures)

pytestmark = pytest.mark.gpu

HEADLINE = (132534, 39561252)           # bench.py, workload ogbn-proteins-s


def test_packed_format_holds_the_csr_with_at_most_two_lanes_on_a_quad(dev, schedule):
    from difformer_amd import ops
    schedule("packed")
    n, deg, F = 84000, 48, 64
    ei = dense_graph(n, deg, seed=n + F)
    csr = ops.csr_cache.get(ei.to(dev), None, n, F * 4)
    sl = csr.sliced(0, n, F)
    assert sl is not None and sl.quad_cap == 2 and int(sl.plan[7]) >= 8
    assert sl.parts is None and sl.n_pos is None and sl.order is not None
    shared = check_format(sl, ei, n, csr)
    print(f"packed format of {n} rows x {deg}: {int(sl.table[-1])} blocks, {shared} shared cells")
    assert shared > 0, "the packed schedule of this graph shares quads (else this test checks nothing new)"
    # the schedule is static: a second build gives the same bits
    again = csr._build_sliced(0, n, F)
    assert torch.equal(again.entries, sl.entries) and torch.equal(again.table, sl.table) and torch.equal(again.order, sl.order)


def _old_builder(be, csr, n, F, plan, order):
    """dif_sliced_measure / dif_sliced_emit called the way every caller did before the plan record could hold a capacity:
    with the plan as dif_sliced_plan wrote it."""
    from difformer_amd import backend_hip as bh
    dev = csr.rowptr.device
    slices, panels, G, PW, W, R, T, NT = (int(v) for v in plan)
    i32 = dict(dtype=torch.int32, device=dev)
    srt = torch.empty(max(csr.nnz, 1), dtype=torch.int16, device=dev)
    counts = torch.empty(n * NT * 32, dtype=torch.uint8, device=dev)
    lengths = torch.empty(G * NT * 4, **i32)
    table = torch.empty((R + 1) * panels * NT * W + 1, **i32)
    status = torch.empty(1, **i32)
    p, st = bh._ptr, bh._stream(dev)
    rc = be.lib.dif_sliced_measure(p(csr.rowptr), p(csr.blkptr), p(csr.src), n, csr.nnz, 0, n, F, plan, p(order), None, n,
                                   p(srt), p(counts), p(lengths), p(table), p(status), st)
    assert rc == 0 and int(status[0]) == 0
    n_blocks = int(table[-1])
    entries = torch.empty(512 * max(n_blocks, 1), dtype=torch.int16, device=dev)
    rc = be.lib.dif_sliced_emit(p(csr.rowptr), p(csr.blkptr), n, 0, n, F, plan, p(order), None, n, p(srt), p(counts), p(table),
                                max(n_blocks, 1), p(entries), st)
    assert rc == 0
    return entries, table


@pytest.mark.parametrize("ordered", [False, True])
def test_capacity_one_is_the_strict_builder_bit_for_bit(ordered, dev, schedule):
    from difformer_amd import ops, sliced
    schedule("strict")
    n, deg, F = 40000, 60, 64
    ei = dense_graph(n, deg, seed=7).to(dev)
    csr = ops.csr_cache.get(ei, None, n, F * 4)
    be = ops.get_backend()
    plan = be.sliced_plan(n, n, F)
    order = sliced.packed_slot_order(csr.rowptr, csr.blkptr, n, int(plan[7]), 0, n) if ordered else None
    old = _old_builder(be, csr, n, F, plan, order)
    new = be.sliced_build(csr.rowptr, csr.blkptr, csr.src, n, csr.nnz, 0, n, F, plan, order, None, None, quad_cap=1)
    assert torch.equal(old[0], new[0]) and torch.equal(old[1], new[1])
    if not ordered:
        sl = csr.sliced(0, n, F)
        assert sl.quad_cap == 1 and sl.order is None and torch.equal(sl.entries, new[0]) and torch.equal(sl.table, new[1])
    packed = be.sliced_build(csr.rowptr, csr.blkptr, csr.src, n, csr.nnz, 0, n, F, plan, order, None, None, quad_cap=2)
    assert int(packed[1][-1]) <= int(new[1][-1])
    with pytest.raises(Exception):
        be.sliced_build(csr.rowptr, csr.blkptr, csr.src, n, csr.nnz, 0, n, F, plan, order, None, None, quad_cap=3)


def test_headline_graph_packs_to_the_row_envelope_and_shares_near_the_minimum(dev, schedule):
    """`auto` gives the headline graph (bench.make_graph(132534, 39561252)) the packed schedule.  Measured on the MI355X
    (profiles/r07_experiments.md): built 193,426 blocks = the row-envelope prediction exactly (1.2496 lane-steps per entry;
    strict: 240,827 blocks, 1.556), 897,152 shared cells against a minimum of 563,870 (1.59 x)."""
    import bench
    from difformer_amd import ops
    schedule(None)                                            # auto
    n, pairs = HEADLINE
    ei = bench.make_graph(n, pairs, dev)
    csr = ops.csr_cache.get(ei, None, n, 256)
    sl = csr.sliced(0, n, 64)
    assert sl is not None and sl.quad_cap == 2 and sl.order is not None and sl.parts is None
    built, predicted, shared, minimum = headline_stats(sl, csr, n, dev)
    print(f"headline: built {built * 512 / csr.nnz:.4f} lane-steps per entry ({built} blocks), row-envelope prediction "
          f"{predicted * 512 / csr.nnz:.4f} ({predicted}), shared cells {shared}, minimum {minimum}")
    assert built <= 1.05 * predicted
    assert shared <= 2 * minimum
    schedule("strict")
    strict = ops.csr_cache.get(ei, None, n, 256).sliced(0, n, 64)
    assert strict.quad_cap == 1 and strict.order is None and int(strict.table[-1]) > built


@pytest.mark.parametrize("mode", ["packed", "strict"])
def test_product_vs_oracle_forward_adjoint_and_row_shard(mode, dev, schedule):
    product_vs_oracle(mode, dev, schedule)


@pytest.mark.parametrize("n,deg,F", [(20000, 60, 64), (9000, 70, 64), (33000, 50, 128), (12000, 64, 32)])
def test_auto_keeps_the_strict_format_for_small_uniform_graphs(n, deg, F, dev, schedule):
    from difformer_amd import ops
    schedule(None)
    ei = dense_graph(n, deg, seed=n + F).to(dev)
    csr = ops.csr_cache.get(ei, None, n, F * 4)
    sl = csr.sliced(0, n, F)
    assert sl is not None and sl.quad_cap == 1 and sl.order is None
    be = ops.get_backend()
    plan = be.sliced_plan(n, n, F)
    old = _old_builder(be, csr, n, F, plan, None)
    assert torch.equal(old[0], sl.entries) and torch.equal(old[1], sl.table)


@pytest.mark.parametrize("mode", [None, "packed"])
def test_skewed_graphs_keep_the_descending_degree_order_and_hub_split(mode, dev, schedule):
    from difformer_amd import ops
    n, deg, F = 12000, 64, 64
    ei = skewed_graph(n, deg, seed=n).to(dev)
    schedule("strict")
    ref = ops.csr_cache.get(ei, None, n, F * 4).sliced(0, n, F)
    schedule(mode)
    sl = ops.csr_cache.get(ei, None, n, F * 4).sliced(0, n, F)
    assert sl.quad_cap == 1 and sl.parts is not None and torch.equal(sl.order, ref.order)
    assert torch.equal(sl.entries, ref.entries) and torch.equal(sl.table, ref.table)


def test_schedule_switch_rejects_unknown_values(dev, schedule):
    from difformer_amd import ops
    schedule("fastest")
    n = 12000
    ei = dense_graph(n, 64, seed=1).to(dev)
    with pytest.raises(ValueError):
        ops.csr_cache.get(ei, None, n, 256)
