"""Slot order and quad capacity of the feature-sliced product on the C4 graph: strict and packed schedules built and timed back to
back in one process (A/B/A/B), with the UNCHANGED product kernel.
  natural order, cap 1   today's strict schedule
  ordered slots, cap 1   r06's experiment: rows that share a 64-row slot chosen by (largest per-tile block count, set of tiles that
                         reach it).  Cuts the ROW envelope from 1.52 to 1.25 lane-steps per entry and the built format does not
                         move (1.556 -> 1.569): the fullest bank-quad COLUMN of a lane group binds (profiles/r06_experiments.md 3)
  natural order, cap 2   two lanes of a lane group may share a quad: the column bound halves, the row envelope (natural) binds
  ordered slots, cap 2   the packed schedule: both together (profiles/r07_experiments.md)
Prints per variant: the block count the row envelopes alone predict, the block count built, the cold build time of the format
(measure + emit, after the CSR) and the product's time.
    python scripts/exp_slot_order.py [n pairs]     (GPU)        python scripts/exp_sliced_slots.py    (the offline statistics)"""
import os, sys, time, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import make_graph
from difformer_amd import ops, sliced
dev = torch.device("cuda:0")
n, pairs, F = 132534, 39561252, 64
if len(sys.argv) > 2:
    n, pairs = int(sys.argv[1]), int(sys.argv[2])
ei = make_graph(n, pairs, dev)
be = ops.get_backend()
x = torch.randn(n, F, device=dev)
csr = ops.csr_cache.get(ei, None, n, F * 4, build_format=False)        # the CSR only: the formats are built below
plan = be.sliced_plan(n, n, F)
slices, panels, G, PW, W, R, T, NT = (int(v) for v in plan)


def slot_order():
    return sliced.packed_slot_order(csr.rowptr, csr.blkptr, n, NT, 0, n)


def predicted(order):
    """blocks of the format if a round were as long as its longest ROW only"""
    cnt = csr.blkptr.view(NT + 1, n)
    cnt = (cnt[1:] - cnt[:-1]).t().contiguous()
    o = torch.full((G * 64,), -1, dtype=torch.int64, device=dev)
    o[:n] = order.long() if order is not None else torch.arange(n, device=dev)
    c = torch.where(o[:, None] >= 0, cnt[o.clamp(min=0)], torch.zeros_like(cnt[:1])).view(G, 64, NT)
    nb = (c.max(dim=1).values + 7) // 8
    j = torch.arange(R, device=dev)[:, None]
    pw = torch.arange(PW, device=dev)[None, :]
    s = j * PW + torch.where(j % 2 == 1, PW - 1 - pw, pw)
    r = torch.where((s < G)[..., None], nb[s.clamp(max=G - 1)], torch.zeros_like(nb[:1]))
    r = torch.flip(torch.cummax(torch.flip(r, [0]), 0).values, [0])
    return int(r.sum())


if __name__ == "__main__":
    variants = (("natural order, cap 1", False, 1), ("ordered slots, cap 2", True, 2), ("ordered slots, cap 1", True, 1),
                ("natural order, cap 2", False, 2))
    print(f"{n} rows, {csr.nnz} entries, {NT} tiles of {T} rows, {G} slots, {PW} pairs x {R} rounds", flush=True)
    for rep in range(3):
        for name, ordered, cap in variants[: 2 if rep else 4]:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            order = slot_order() if ordered else None
            built = be.sliced_build(csr.rowptr, csr.blkptr, csr.src, n, csr.nnz, 0, n, F, plan, order, None, None, cap)
            torch.cuda.synchronize()
            build_ms = (time.perf_counter() - t0) * 1e3
            sl = sliced.SlicedAdjacency(plan, built[0], built[1], order, None, None, cap)
            nb = int(sl.table[-1])
            ys = be.sliced_prescale(x, csr.rowptr, n, sl.plan)
            for _ in range(5):
                out = be.sliced_spmm(sl, ys, csr.rowptr, n, 0, n, F, None, 1.0, 1.0)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(30):
                out = be.sliced_spmm(sl, ys, csr.rowptr, n, 0, n, F, None, 1.0, 1.0)
            e1.record(); torch.cuda.synchronize()
            print(f"{name}: row envelopes alone {predicted(order) * 512 / csr.nnz:.3f} lane-steps per entry, built format "
                  f"{nb * 512 / csr.nnz:.3f} ({nb} blocks), format build {build_ms:.2f} ms, product "
                  f"{e0.elapsed_time(e1) / 30 * 1e3:.1f} us", flush=True)
