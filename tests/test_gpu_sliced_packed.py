"""The PACKED schedule of the feature-sliced product (csrc/gcn_sliced.hip): slots formed by tile profile
(ops.packed_slot_order) and a quad capacity of 2 in the colouring (asked for in the plan record, include/difformer_hip.h).

The schedule is forced through DIFFORMER_SLICED_SCHEDULE so that nothing here depends on the threshold of `auto`, which has
its own test.  Integer work is checked exactly: the format holds every (row, tile) group of the CSR exactly once, in every
step a hardware lane group puts at most 2 lanes on one bank quad, and a zero-row read never shares a quad.  The product is
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

pytestmark = pytest.mark.gpu

# lane sets that share one LDS cycle of ds_read_b128 (MI355X_MICROARCH.md, LDS table)
HW_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
    [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63],
]
HEADLINE = (132534, 39561252)           # bench.py, workload ogbn-proteins-s


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def schedule(monkeypatch):
    def set_(mode):
        from difformer_amd import ops
        if mode is None:
            monkeypatch.delenv("DIFFORMER_SLICED_SCHEDULE", raising=False)
        else:
            monkeypatch.setenv("DIFFORMER_SLICED_SCHEDULE", mode)
        ops.csr_cache.clear()
    yield set_
    from difformer_amd import ops
    ops.csr_cache.clear()


def _dense_graph(n, deg, seed):
    g = torch.Generator().manual_seed(seed)
    e = n * deg
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[:, : e // 50] = ei[:, e // 50: 2 * (e // 50)]         # repeated edges must be summed twice
    return torch.cat([ei, torch.arange(n).repeat(2, 1)], dim=1)


def _skewed_graph(n, deg, seed, hubs=40):
    ei = _dense_graph(n, deg, seed)
    g = torch.Generator().manual_seed(seed + 1)
    half = ei.shape[1] // 2
    ei[1, :half] = torch.randint(0, hubs, (half,), generator=g) * (n // hubs)
    return ei


def _check_packed_format(sl, ei, n, csr):
    """test_gpu_sliced.py::_check_format for a format without parts, with its bank rule replaced by the packed one."""
    slices, panels, G, PW, W, R, T, NT = (int(v) for v in sl.plan)
    assert sl.parts is None and sl.n_pos is None and sl.order is not None
    assert NT == csr.n_blocks and T % 16 == 0 and PW == panels * W and G == -(-n // 64) and (R - 1) * PW < G <= R * PW
    order = sl.order.cpu().numpy().astype(np.int64)
    assert order.size == n and np.array_equal(np.sort(order), np.arange(n)), "order is a permutation of the rows"
    table = sl.table.cpu().numpy()
    n_ptw = panels * NT * W
    n_blocks = int(table[-1])
    rows = table[:-1].reshape(n_ptw, R + 1)
    ent = sl.entries.cpu().numpy().view(np.uint16).reshape(-1, 64, 8)[:n_blocks]
    assert ent.max() < T + 16
    # every step of every block: a hardware lane group puts at most 2 lanes on a bank quad; a zero-row read shares none
    quads = (ent & 15).transpose(0, 2, 1).astype(np.int64)       # [block, step, lane]
    zero = (ent >= T).transpose(0, 2, 1)
    shared = 0
    for grp in HW_GROUPS:
        q = quads[:, :, grp]
        per_quad = (q[..., None] == np.arange(16)).sum(axis=2)   # [block, step, quad]
        assert per_quad.max() <= 2, "more than two lanes of a lane group on one bank quad"
        own = np.take_along_axis(per_quad, q, axis=2)            # lanes on the quad each lane reads
        assert np.all(own[zero[:, :, grp]] == 1), "a zero-row read shares its bank quad"
        shared += int((per_quad == 2).sum())
    # the real entries of (row, tile) == the CSR group
    src, dst = ei[0].numpy(), ei[1].numpy()
    perm = np.lexsort((src, dst))
    src_s, dst_s = src[perm], dst[perm]
    rowptr = np.searchsorted(dst_s, np.arange(n + 1))
    assert np.array_equal(rowptr, csr.rowptr.cpu().numpy())
    csr_src = csr.src.cpu().numpy().astype(np.int64)
    blkptr = csr.blkptr.cpu().numpy().reshape(NT + 1, n) if NT > 1 else None
    total_real, expect_start, seen_slots = 0, 0, 0
    for p in range(panels):
        for t in range(NT):
            for w in range(W):
                start, nb = int(rows[(p * NT + t) * W + w, 0]), rows[(p * NT + t) * W + w, 1:].astype(np.int64)
                assert start == expect_start and np.all(nb[:-1] >= nb[1:]), "round lengths must not increase"
                expect_start += int(nb.sum())
                pw = w * panels + p
                for j in range(R):
                    g = j * PW + (PW - 1 - pw if j & 1 else pw)
                    if g >= G:
                        assert nb[j] == 0
                        continue
                    seen_slots += (t == 0)
                    blocks = [start + int(np.minimum(nb, k).sum()) + j for k in range(int(nb[j]))]
                    lists = ent[blocks].transpose(1, 0, 2).reshape(64, -1) if blocks else np.zeros((64, 0), np.uint16)
                    for lane in range(64):
                        pos = g * 64 + lane
                        got = np.sort(lists[lane][lists[lane] < T].astype(np.int64))
                        if pos >= n:
                            assert got.size == 0
                            continue
                        row = order[pos]
                        seg = src_s[rowptr[row]: rowptr[row + 1]]
                        e0, e1 = (rowptr[row], rowptr[row + 1]) if NT == 1 else (blkptr[t, row], blkptr[t + 1, row])
                        want = np.sort(csr_src[e0:e1] - t * T)
                        assert np.array_equal(want, seg[(seg >= t * T) & (seg < (t + 1) * T)] - t * T)
                        assert np.array_equal(got, want), (p, t, w, j, lane)
                        total_real += got.size
    assert expect_start == n_blocks and seen_slots == G and total_real == ei.shape[1]
    return shared


def test_packed_format_holds_the_csr_with_at_most_two_lanes_on_a_quad(dev, schedule):
    from difformer_amd import ops
    schedule("packed")
    n, deg, F = 84000, 48, 64
    ei = _dense_graph(n, deg, seed=n + F)
    csr = ops.csr_cache.get(ei.to(dev), None, n, F * 4)
    sl = csr.sliced(0, n, F)
    assert sl is not None and sl.quad_cap == 2 and int(sl.plan[7]) >= 8
    shared = _check_packed_format(sl, ei, n, csr)
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
    from difformer_amd import ops
    schedule("strict")
    n, deg, F = 40000, 60, 64
    ei = _dense_graph(n, deg, seed=7).to(dev)
    csr = ops.csr_cache.get(ei, None, n, F * 4)
    be = ops.get_backend()
    plan = be.sliced_plan(n, n, F)
    order = ops.packed_slot_order(csr.rowptr, csr.blkptr, n, int(plan[7]), 0, n) if ordered else None
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


def _headline_stats(sl, csr, n, dev):
    """-> (built blocks, row-envelope prediction in blocks, shared cells, their minimum for this build)"""
    slices, panels, G, PW, W, R, T, NT = (int(v) for v in sl.plan)
    order = sl.order.long()
    cnt = csr.blkptr.view(NT + 1, n)
    cnt = (cnt[1:] - cnt[:-1]).t().contiguous()                                   # [row, tile]
    o = torch.full((G * 64,), -1, dtype=torch.int64, device=dev)
    o[:n] = order
    c = torch.where(o[:, None] >= 0, cnt[o.clamp(min=0)], torch.zeros_like(cnt[:1])).view(G, 64, NT)
    nb = (c.max(dim=1).values + 7) // 8
    j = torch.arange(R, device=dev)[:, None]
    pw = torch.arange(PW, device=dev)[None, :]
    s = j * PW + torch.where(j % 2 == 1, PW - 1 - pw, pw)
    r = torch.where((s < G)[..., None], nb[s.clamp(max=G - 1)], torch.zeros_like(nb[:1]))
    predicted = int(torch.flip(torch.cummax(torch.flip(r, [0]), 0).values, [0]).sum())
    n_blocks = int(sl.table[-1])
    # shared cells of the built format: per (block, step, lane group) the lanes beyond the first on a quad, real reads only
    ent = sl.entries[: n_blocks * 512].view(n_blocks, 64, 8).to(torch.int32) & 0xFFFF
    groups = torch.tensor(HW_GROUPS, device=dev)
    shared = 0
    for b0 in range(0, n_blocks, 16384):
        e = ent[b0: b0 + 16384][:, groups, :]                                      # [block, group, 16 lanes, step]
        q = torch.where(e < T, e & 15, 16 + torch.arange(16, device=dev)[None, None, :, None])      # zero rows never match
        qs = torch.sort(q, dim=2).values
        shared += int((qs[:, :, 1:, :] == qs[:, :, :-1, :]).sum())
    # minimum: columns of every (slot, tile, lane group) against the built length of the round
    rows = sl.table[:-1].view(panels * NT * W, R + 1).long()
    g = torch.arange(G, device=dev)
    jj, idx = g // PW, g % PW
    pwg = torch.where(jj % 2 == 1, PW - 1 - idx, idx)
    p, w = pwg % panels, pwg // panels
    t = torch.arange(NT, device=dev)
    K = 8 * rows[(p[:, None] * NT + t[None, :]) * W + w[:, None], 1 + jj[:, None]]          # [slot, tile] steps
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    inv[order] = torch.arange(n, device=dev)
    group_of = torch.empty(64, dtype=torch.int64, device=dev)
    group_of[groups.flatten()] = torch.arange(64, device=dev) // 16
    dst = torch.repeat_interleave(torch.arange(n, device=dev), (csr.rowptr[1:] - csr.rowptr[:-1]).long())
    pos = inv[dst]
    srcl = csr.src.long()
    key = (((pos // 64) * NT + srcl // T) * 4 + group_of[pos % 64]) * 16 + (srcl % T) % 16
    col = torch.bincount(key, minlength=G * NT * 64).view(G, NT, 4, 16)
    minimum = int((col - K[:, :, None, None]).clamp(min=0).sum())
    return n_blocks, predicted, shared, minimum


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
    built, predicted, shared, minimum = _headline_stats(sl, csr, n, dev)
    print(f"headline: built {built * 512 / csr.nnz:.4f} lane-steps per entry ({built} blocks), row-envelope prediction "
          f"{predicted * 512 / csr.nnz:.4f} ({predicted}), shared cells {shared}, minimum {minimum}")
    assert built <= 1.05 * predicted
    assert shared <= 2 * minimum
    schedule("strict")
    strict = ops.csr_cache.get(ei, None, n, 256).sliced(0, n, 64)
    assert strict.quad_cap == 1 and strict.order is None and int(strict.table[-1]) > built


@pytest.mark.parametrize("mode", ["packed", "strict"])
def test_product_vs_oracle_forward_adjoint_and_row_shard(mode, dev, schedule):
    from difformer_amd import gcn_conv, ops
    from difformer_amd.dist import RowShard
    schedule(mode)
    cap = 2 if mode == "packed" else 1
    n, deg, d = 50000, 60, 64
    ei = _dense_graph(n, deg, seed=3 * n + d)
    # out-degrees != in-degrees, both near-uniform (the first half of the nodes sends ~2 more entries each)
    ei[0, : n] = torch.randint(0, n // 2, (n,), generator=torch.Generator().manual_seed(3))
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 1, d, generator=g)
    gout = torch.randn(n, 1, d, generator=g)
    eid = ei.to(dev)
    xd = x.to(dev).requires_grad_(True)
    csr = ops.csr_cache.get(eid, None, n, d * 4)
    assert csr.sliced(0, n, d).quad_cap == cap
    out = gcn_conv(xd, eid, None)
    ref = orc.gcn_conv(x.double().numpy(), ei.numpy(), None)
    assert rel_err(out.detach().cpu().numpy(), ref) < 1e-5
    assert torch.equal(gcn_conv(xd, eid, None), out)                                           # deterministic
    out.backward(gout.to(dev))
    adj = csr.adjoint()
    assert adj.sliced(0, n, d) is not None and adj.sliced(0, n, d).quad_cap == cap
    row, col = ei[0].numpy(), ei[1].numpy()                       # difformer.py:63-75 in float64
    degs = np.bincount(col, minlength=n).astype(np.float64)
    dinv = np.where(degs > 0, 1.0 / np.sqrt(np.maximum(degs, 1)), 0.0)
    want = np.zeros((n, d))
    np.add.at(want, row, (dinv[col] * dinv[row])[:, None] * gout[:, 0, :].double().numpy()[col])
    assert rel_err(xd.grad[:, 0, :].cpu().numpy(), want) < 1e-5
    # a 2-way row shard: each rank's rows through the same builder and the same rule
    be = ops.get_backend()
    x2 = x[:, 0, :].to(dev).contiguous()
    for rank in (0, 1):
        sh = RowShard(n, rank=rank, world=2)
        lo, cnt = sh.row_begin, sh.n_local
        scsr = ops.csr_cache.get(eid, None, n, d * 4, sh)
        sl = scsr.sliced(lo, cnt, d)
        assert sl is not None and sl.quad_cap == cap
        ys = be.sliced_prescale(x2, scsr.rowptr, n, sl.plan)
        got = be.sliced_spmm(sl, ys, scsr.rowptr, n, lo, cnt, d)
        assert rel_err(got.cpu().numpy(), ref[lo: lo + cnt, 0, :]) < 1e-5, rank
        assert torch.equal(be.sliced_spmm(sl, ys, scsr.rowptr, n, lo, cnt, d), got)
        again = scsr._build_sliced(lo, cnt, d)
        assert torch.equal(again.entries, sl.entries) and torch.equal(again.table, sl.table)


@pytest.mark.parametrize("n,deg,F", [(20000, 60, 64), (9000, 70, 64), (33000, 50, 128), (12000, 64, 32)])
def test_auto_keeps_the_strict_format_for_small_uniform_graphs(n, deg, F, dev, schedule):
    from difformer_amd import ops
    schedule(None)
    ei = _dense_graph(n, deg, seed=n + F).to(dev)
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
    ei = _skewed_graph(n, deg, seed=n).to(dev)
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
    ei = _dense_graph(n, 64, seed=1).to(dev)
    with pytest.raises(ValueError):
        ops.csr_cache.get(ei, None, n, 256)
