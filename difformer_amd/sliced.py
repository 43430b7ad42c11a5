"""Host side of the feature-sliced gcn_conv format (csrc/gcn_sliced.hip, csrc/sliced_slots.hip; DESIGN.md sections 2-3):
the plan record (SlicedPlan), which graphs the product is for (candidate), the three switches with their thresholds and row
orders, and the build of a CSR shard's format (build; rows_format for the rows of a call).  ops.py and backend_hip.py import
from here, never the other way round: the backend is passed in where a call is needed."""
import ctypes
import os

import torch


class SlicedPlan(ctypes.c_int32 * 8):
    """The int32[8] plan record (include/difformer_hip.h) as dif_sliced_plan writes it: iterable as its eight ints,
    indexable, and taken as it is by every C call with a plan argument.  plan[0] holds F / 4 in its low 16 bits, the quad
    capacity - 1 of a build in bits 16-17 and the announcement of the position records in bit 18; dif_sliced_plan leaves
    both zero.  Three flagged copies go to the C side, each made once when a format is built: with_capacity(quad_cap) to
    dif_sliced_measure, that .with_records(positions) to dif_sliced_emit, and SlicedAdjacency.run_plan to the product."""
    slices = property(lambda self: self[0] & 0xFFFF)
    panels, G, PW, W, R, T, NT = (property(lambda self, i=i: self[i]) for i in range(1, 8))

    def with_capacity(self, quad_cap):     # a copy that asks the two build calls for this capacity (C rejects 3 and 4)
        if not 1 <= int(quad_cap) <= 4:
            raise ValueError(f"difformer_amd: quad_cap={quad_cap!r}: expected 1 (strict) or 2 (packed)")
        return SlicedPlan(self[0] & ~(3 << 16) | (int(quad_cap) - 1) << 16, *self[1:])

    def with_records(self, positions):     # a copy with (positions) or without the bit that announces the position records
        return SlicedPlan(self[0] | 1 << 18 if positions else self[0] & ~(1 << 18), *self[1:])

    # int16 elements the position records take in front of the entry blocks: 8 bytes for each of the 64 positions of the
    # G slots when plan[0] announces them, else 0.  A multiple of 256 elements, so the blocks keep their alignment.
    record_elems = property(lambda self: self.G * 64 * 4 if self[0] & 1 << 18 else 0)


SLICED_MIN_DEGREE = 48      # entries per row from which the LDS-staged product beats the gather kernels
SLICED_MIN_ROWS = 8192
SLICED_SPLIT_FACTOR = 4.0   # rows beyond this multiple of the mean degree are split into lock-step parts (Zipf C4: 2-6 within 4 %)
SLICED_MAX_PARTS = 64       # one slot


def candidate(num_nodes, nnz, F=None, weighted=False, elem_size=4):
    """Is the feature-sliced product for this graph (and, where the caller knows it, for rows of F columns)?"""
    return (not weighted and elem_size == 4 and num_nodes >= SLICED_MIN_ROWS and nnz >= SLICED_MIN_DEGREE * num_nodes and
            (F is None or (F % 4 == 0 and F <= 256)))


# Two schedules of the format.  strict: natural row order, no two lanes of a hardware lane group on
# one bank quad in a step.  packed (near-uniform degrees only): rows with equal per-tile block counts share a slot and a
# quad may be read by two lanes of a step -- fewer padded steps for a few 2-way shared LDS reads, a longer cold build.
# DIFFORMER_SLICED_SCHEDULE = strict | packed | auto (default); auto packs where the build is paid back within 64
# launches (one short training run, or a few evaluations of a 4-layer model).  Measured on the MI355X at F = 64
# (profiles/r07_experiments.md, profiles/r12_experiments.md): against the strict schedule a launch saves
#    2.4 M entries: 1.4 us    10 M: 8 us    30 M: 15 us    79 M (headline): 35 us, 41 us with the dealt slot order
# and the cold build of CSR + format, as `bench.py --full` times it on the headline graph, goes from 9.1 ms (strict) to
# 10.0 ms (packed_slot_order) and 11.6 ms (the dealt order: 1.9 ms of device time for its two sorts, the greedy windows and
# the deal).  2.45 ms / 64 = 38 us per launch: linear between the 30 M point (17 us with the dealt order's share) and the
# 79 M point (41 us) that is ~73 M entries.
SLICED_PACKED_MIN_ENTRIES = 72_000_000
SLICED_PACKED_MAX_TILES = 40  # the slot order's key holds one bit per tile in an int64


def _switch(name, default, allowed):
    mode = os.environ.get(name, default).strip().lower() or default
    if mode not in allowed:
        raise ValueError(f"{name}={mode!r}: expected {', '.join(allowed[:-1])} or {allowed[-1]}")
    return mode


def sliced_schedule():
    return _switch("DIFFORMER_SLICED_SCHEDULE", "auto", ("strict", "packed", "auto"))


# Which rows share a slot of the packed schedule, and which slots share a wave:
# DIFFORMER_SLICED_SLOTS = dealt (default): greedy slots by tile profile, dealt to the waves against their running envelope,
# all on the device (csrc/sliced_slots.hip); profile: packed_slot_order below, slots dealt in order -- also what a geometry
# the device call does not cover gets.
def sliced_slots():
    return _switch("DIFFORMER_SLICED_SLOTS", "dealt", ("profile", "dealt"))


# DIFFORMER_SLICED_POSITIONS = 1 (default): the format carries one 8-byte record {row, deg^-1/2} per row position, written
# by the cold build, and the product's epilogue reads it as one coalesced line per (wave, round) instead of gathering
# rowptr and taking the divide and square root again in each of the 16 slice-workgroups of a panel.
# 0: no records, the gathering epilogue -- the same results bit for bit.
def sliced_positions():
    return _switch("DIFFORMER_SLICED_POSITIONS", "1", ("0", "1")) == "1"


def packed_order(be, rowptr, blkptr, n_src, NT, row_begin, n_rows, plan):
    """The row order of the packed schedule under DIFFORMER_SLICED_SLOTS: int32 [n_rows] on the device."""
    dealt = sliced_slots() == "dealt" and hasattr(be, "sliced_slot_order")
    order = be.sliced_slot_order(rowptr, blkptr, n_src, row_begin, n_rows, plan) if dealt else None
    return packed_slot_order(rowptr, blkptr, n_src, NT, row_begin, n_rows) if order is None else order


def packed_slot_order(rowptr, blkptr, n_src, NT, row_begin, n_rows):
    """Rows of a near-uniform graph in the order that forms the slots of the packed schedule: by the largest per-tile
    block count (8-step blocks, descending), then by the set of tiles that reach it, stable -- the 64 lock-step rows of
    a slot then end their rounds in the same block in (nearly) every tile.  int32 [n_rows], on the device."""
    if NT > 1:
        cnt = blkptr.view(NT + 1, n_src)[:, row_begin: row_begin + n_rows]
        blocks = (cnt[1:] - cnt[:-1] + 7) // 8
    else:
        blocks = ((rowptr[row_begin + 1: row_begin + n_rows + 1] - rowptr[row_begin: row_begin + n_rows] + 7) // 8)[None, :]
    top = blocks.max(dim=0).values.to(torch.int64)
    weights = torch.ones(NT, dtype=torch.int64, device=blocks.device) << torch.arange(NT, device=blocks.device)
    hot = ((blocks == top[None, :]).to(torch.int64) * weights[:, None]).sum(dim=0)
    key = (top.max() - top) * (1 << NT) + hot
    return torch.argsort(key, stable=True).to(torch.int32)


class SlicedAdjacency:
    """Entry blocks + table + geometry of the feature-sliced product (include/difformer_hip.h, dif_sliced_*).
    order: rows by descending degree (skewed graphs) or by tile profile (packed schedule); parts / n_pos: hub rows split
    into lock-step parts ("row positions" in the header) -- then order has n_pos entries (-1 = padding) and plan is the
    geometry of n_pos positions; quad_cap: 1 = strict schedule, 2 = packed; positions: the allocation of `entries`
    holds the position records in front of them (backend sliced_build) and run_plan, the plan the product is called
    with, says so.  The slice-major source copy is written with the same plan (its tiling)."""

    def __init__(self, plan, entries, table, order=None, parts=None, n_pos=None, quad_cap=1, positions=False):
        self.plan, self.entries, self.table, self.order = plan, entries, table, order
        self.parts, self.n_pos, self.quad_cap, self.positions = parts, n_pos, int(quad_cap), bool(positions)
        self.run_plan = plan.with_records(True) if self.positions else plan


def split_positions(deg_sorted, order, cap, max_parts=SLICED_MAX_PARTS):
    """Row positions for rows sorted by descending degree `deg_sorted` (their ids in `order`): a row of degree d takes
    P = min(ceil(d / cap), max_parts) consecutive positions of ONE 64-position slot.  Rows with the same P are packed
    64 // P to a slot (every P-class starts on a fresh slot), the unsplit rows follow in order.
    -> (order2 int32 [n_pos] with -1 = empty, parts uint16-as-int16 [n_pos] = p | P << 8, n_pos).  Device tensor ops;
    one host sync for the sizes (cold path)."""
    dev = deg_sorted.device
    d = deg_sorted.to(torch.int64)
    P = torch.clamp((d + cap - 1) // cap, 1, max_parts)
    n_hub = int((P > 1).sum())                                   # a prefix: the degrees are sorted
    n = d.numel()
    Ph = P[:n_hub]
    vals, counts = torch.unique_consecutive(Ph, return_counts=True)
    per_slot = 64 // vals
    class_slots = (counts + per_slot - 1) // per_slot
    class_base = torch.cumsum(class_slots, 0) - class_slots      # first slot of every class
    class_first = torch.cumsum(counts, 0) - counts               # first hub row of every class
    cls = torch.repeat_interleave(torch.arange(vals.numel(), device=dev), counts)
    k = torch.arange(n_hub, device=dev) - class_first[cls]
    pos0 = (class_base[cls] + k // per_slot[cls]) * 64 + (k % per_slot[cls]) * Ph
    hub_slots = int(class_slots.sum())
    n_pos = hub_slots * 64 + (n - n_hub)
    order2 = torch.full((n_pos,), -1, dtype=torch.int32, device=dev)
    parts = torch.full((n_pos,), 0x0100, dtype=torch.int16, device=dev)
    row_of_part = torch.repeat_interleave(torch.arange(n_hub, device=dev), Ph)
    p_idx = torch.arange(row_of_part.numel(), device=dev) - (torch.cumsum(Ph, 0) - Ph)[row_of_part]
    pos = pos0[row_of_part] + p_idx
    order2[pos] = order[:n_hub][row_of_part].to(torch.int32)
    parts[pos] = (p_idx + (Ph[row_of_part] << 8)).to(torch.int16)
    order2[hub_slots * 64:] = order[n_hub:].to(torch.int32)
    return order2, parts, n_pos


def build(be, csr, row_begin, n_rows, F):
    """The feature-sliced LDS format of rows [row_begin, row_begin + n_rows) of `csr` (ops.GraphCSR) for F fp32 feature
    columns -- or None when this graph keeps the gather kernels: edge weights, an adjoint CSR, a blocking that is not the
    format's tiling, or a (row, tile) group beyond the 16-bit counters.  With skewed degrees (max > 2x mean) the 64-row
    slots are formed in descending-degree order, so that the lock-step lanes of a slot carry lists of similar length."""
    if csr.nnz == 0 or (csr.transposed and csr.dinv is None) or not candidate(csr.num_nodes, csr.nnz, weighted=csr.weighted):
        return None
    plan = be.sliced_plan(csr.num_nodes, n_rows, F) if hasattr(be, "sliced_plan") else None
    if plan is None or plan.NT != csr.n_blocks or (plan.NT > 1 and plan.T != csr.block_rows):
        return None
    T, NT = plan.T, plan.NT
    deg = csr.rowptr[row_begin + 1: row_begin + n_rows + 1] - csr.rowptr[row_begin: row_begin + n_rows]
    max_deg, total = (int(v) for v in torch.stack([deg.max(), deg.sum()]).tolist())       # one sync, cold path
    order = parts = n_pos = None
    quad_cap, mode = 1, sliced_schedule()
    if max_deg * n_rows > 2 * total:
        order = be.row_order(csr.rowptr, row_begin, n_rows)[0]
        cap = max(int(SLICED_SPLIT_FACTOR * total / n_rows), 64)
        if max_deg > cap:
            # hub rows run as several lock-step lanes of one slot instead of one long lane
            order, parts, n_pos = split_positions(deg[order.long()], order, cap)
            plan = be.sliced_plan(csr.num_nodes, n_pos, F)
            if plan is None or plan.T != T or plan.NT != NT:
                return None
    elif NT <= SLICED_PACKED_MAX_TILES and (mode == "packed" or (mode == "auto" and total >= SLICED_PACKED_MIN_ENTRIES)):
        order = packed_order(be, csr.rowptr, csr.blkptr, csr.num_nodes, NT, row_begin, n_rows, plan)
        quad_cap = 2
    # the records hold deg^-1/2 of this CSR's row lengths: not for an adjoint CSR, whose products bring the forward dinv
    positions = sliced_positions() and csr.dinv is None
    built = be.sliced_build(csr.rowptr, csr.blkptr, csr.src, csr.num_nodes, csr.nnz, row_begin, n_rows, F, plan, order,
                            parts, n_pos, quad_cap, positions)
    return None if built is None else SlicedAdjacency(plan, built[0], built[1], order, parts, n_pos, quad_cap, positions)


def rows_format(csr, dtype, n, F, shard=None):
    """csr.sliced(...) for n float32 rows that are the whole graph's or this rank's shard of it, else None.  (Once per layer
    of every forward: it takes the caller's dtype and n as they are.)"""
    sharded = shard is not None and shard.world > 1
    if csr is None or dtype != torch.float32 or not (sharded or n == csr.num_nodes):
        return None
    return csr.sliced(shard.row_begin if sharded else 0, n, F)
