"""Snapshot batches: all snapshots of an epoch in one launch per pass (csrc/tiny_batched.hip; include/difformer_snapshots.h).

`spatial-temporal/main.py:94-121` forwards 104 / 50 / 146 tiny graphs one after another and, for every dataset but wikimath, sums
their costs before ONE backward; `eval.py:9-22` forwards them all under no_grad.  Through difformer_amd/tiny.py that is two
Python-driven launches of ONE workgroup and an autograd node per snapshot.  Given the weights the snapshots are independent and
their gradients add:

    batch = difformer_amd.SnapshotBatch(xs, edge_index, edge_weight)        # once per split
    Y = model.forward_snapshots(batch)                                       # [sum n_b, out_channels]: one launch of T workgroups

and `Y`'s backward is one launch of T workgroups plus one ordered sum of the T gradient slabs, under ONE autograd node that hands
`batch.x` and every parameter their gradient.  Taken for exactly the configurations `tiny._plan` accepts; everything else is a plain
loop over `model.forward` (counted in `stats["fallback"]`).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib, ops, tiny
from .backend_hip import _stream

stats = {"forward": 0, "backward": 0, "fallback": 0}          # calls that took the batched kernels / the loop (tests assert on them)


def _as_list(what, name, T):
    """One tensor (or None) shared by all snapshots, or a list with one entry per snapshot -> (list of T, shared?)."""
    if isinstance(what, (list, tuple)):
        if len(what) != T:
            raise ValueError(f"difformer_amd: {name} has {len(what)} entries for {T} snapshots")
        return list(what), False
    return [what] * T, True


class SnapshotBatch:
    """The snapshots of one split, stored back to back.

    xs: a list of [n_b, F] float32 tensors or one [T, n, F] tensor; `batch.x` is ONE contiguous [N_total, F] copy (set
    `batch.x.requires_grad_()` to get dx back).  edge_index / edge_weight: one tensor pair shared by all snapshots, or lists with
    one entry per snapshot; node ids are local to the snapshot.  On the GPU the tiny CSR and its transpose of every DISTINCT graph
    (by tensor identity) are built here by `tiny.build_graph`, and the deferred index check is read once: a bad edge_index raises
    here.  Construction is the only place that synchronises with the device."""

    def __init__(self, xs, edge_index=None, edge_weight=None):
        if torch.is_tensor(xs):
            if xs.dim() != 3:
                raise ValueError("difformer_amd: SnapshotBatch takes a list of [n_b, F] tensors or one [T, n, F] tensor")
            xs = list(xs.unbind(0))
        xs = list(xs)
        if not xs:
            raise ValueError("difformer_amd: SnapshotBatch needs at least one snapshot")
        for x in xs:
            if not torch.is_tensor(x) or x.dtype != torch.float32:
                raise TypeError("difformer_amd: SnapshotBatch features must be float32 tensors")
            if x.dim() != 2 or x.shape[1] != xs[0].shape[1] or x.device != xs[0].device:
                raise ValueError("difformer_amd: every snapshot is [n_b, F] with the same F on the same device")
        T = len(xs)
        self.edge_index, shared_ei = _as_list(edge_index, "edge_index", T)
        self.edge_weight, shared_ew = _as_list(edge_weight, "edge_weight", T)
        for ei, ew in ((self.edge_index[0], self.edge_weight[0]),) if (shared_ei and shared_ew) else zip(self.edge_index, self.edge_weight):
            if ei is None:
                if ew is not None:
                    raise ValueError("difformer_amd: edge_weight without an edge_index")
                continue
            if ei.dtype != torch.int64 or ei.dim() != 2 or ei.shape[0] != 2:
                raise TypeError("difformer_amd: edge_index must be an int64 tensor of shape [2, E]")
            if ew is not None and ew.numel() != ei.shape[1]:
                raise ValueError("difformer_amd: edge_weight must have one entry per edge")
        self.x = torch.cat(xs, dim=0).contiguous()
        if self.x.data_ptr() == xs[0].data_ptr() and self.x.numel():                # T = 1: cat of one tensor may return it
            self.x = self.x.clone()
        self.sizes = [int(x.shape[0]) for x in xs]
        self.node_ptr = [0]
        for n in self.sizes:
            self.node_ptr.append(self.node_ptr[-1] + n)
        self.max_n = max(self.sizes)
        dev = self.x.device
        self.node_ptr_dev = torch.tensor(self.node_ptr, dtype=torch.int64, device=dev)
        # the snapshot with the most entries stands for the batch in tiny._plan (its limits are upper bounds)
        self._widest = max(range(T), key=lambda b: -1 if self.edge_index[b] is None else int(self.edge_index[b].shape[1]))
        self._tables = {}                    # (padded width, layers) -> (device table, tape floats, scratch floats)
        self.graphs = None                   # TinyGraph per snapshot (shared objects for shared tensors), or None: not buildable
        if dev.type == "cuda" and tiny.ENABLED and all(e is not None for e in self.edge_index) and min(self.sizes) >= 1 and \
                self.max_n <= tiny.MAX_NODES and int(self.edge_index[self._widest].shape[1]) <= tiny.MAX_EDGES and \
                getattr(ops.get_backend(), "has_tiny", False):
            built, self.graphs = {}, []
            for ei, ew, n in zip(self.edge_index, self.edge_weight, self.sizes):
                key = (id(ei), id(ew), n)
                if key not in built:
                    built[key] = tiny.build_graph(ei, ew, n)
                self.graphs.append(built[key])
            tiny._poll_status(wait=True)

    def __len__(self):
        return len(self.sizes)

    def split(self, Y):
        """Per-snapshot views of a [N_total, ...] tensor."""
        return [Y[a:b] for a, b in zip(self.node_ptr[:-1], self.node_ptr[1:])]

    def _table(self, DP, L, use_graph):
        """The device record table of include/difformer_snapshots.h for this padded width and layer count (uploaded once)."""
        key = (DP, L, bool(use_graph))
        hit = self._tables.get(key)
        if hit is None:
            lib = _lib.load_snapshots()
            per_n = {n: (int(lib.dif_snap_tape_floats(n, DP, L)), int(lib.dif_snap_scratch_floats(n, DP, L))) for n in set(self.sizes)}
            rows, tape, scratch = [], 0, 0
            for b, n in enumerate(self.sizes):
                g = self.graphs[b] if use_graph else None
                ptrs = [0] * 6 if g is None else [g.rowptr, g.src, g.val, g.rowptr_t, g.dst_t, g.val_t]
                rows.append([n, self.node_ptr[b]] + ptrs + [tape, scratch, 0, 0])
                tape += per_n[n][0]
                scratch += per_n[n][1]
            assert len(rows[0]) == _lib.SNAPSHOTS_CONSTANTS["DIF_SNAP_RECORD_FIELDS"]
            hit = self._tables[key] = (torch.tensor(rows, dtype=torch.int64).to(self.x.device), tape, scratch)
        return hit


def _plan(model, batch):
    """tiny._plan for the whole batch -> (cfg fields, parameters) or None: the loop."""
    x = batch.x
    if not x.is_cuda or not getattr(ops.get_backend(), "has_tiny", False):
        return None
    use_graph = bool(model._modules["convs"][0].use_graph) if len(model._modules["convs"]) else False
    if use_graph and batch.graphs is None:
        return None
    b = batch._widest
    if use_graph and any(w is not None and w.requires_grad for w in batch.edge_weight) and torch.is_grad_enabled():
        return None                              # differentiable in edge_weight: the layer-by-layer path, per snapshot
    big = batch.sizes.index(batch.max_n)
    if min(batch.sizes) < 1:
        return None
    return tiny._plan(model, x[batch.node_ptr[big]: batch.node_ptr[big + 1]], batch.edge_index[b], batch.edge_weight[b])


class _Snapshots(torch.autograd.Function):
    """DIFFormer.forward of every snapshot as one launch; backward = one launch of the same grid + the ordered slab sum."""

    @staticmethod
    def forward(ctx, state, x, *live):
        fields, params, batch, p_drop, training, rnd = state
        lib = _lib.load_snapshots()
        dev = x.device
        d, L, c = fields["hidden"], fields["num_layers"], fields["out_channels"]
        table, tape_floats, scratch_floats = batch._table(4 if d <= 4 else 8, L, fields["use_graph"])
        cfg = _lib.TinyCfg(training=int(training), dropout=float(p_drop), nnz=0, launch_plan=1, **fields)
        tape = torch.empty(tape_floats, dtype=torch.float32, device=dev)
        y = torch.empty((x.shape[0], c), dtype=torch.float32, device=dev)
        pa = tiny._ptr_array(params)
        rc = lib.dif_snap_forward_f32(ctypes.byref(cfg), len(batch), table.data_ptr(), x.data_ptr(), x.shape[1], pa,
                                      None if rnd is None else rnd.data_ptr(), tape.data_ptr(), y.data_ptr(), _stream(dev))
        _lib.check_snapshots(rc, "dif_snap_forward_f32")
        stats["forward"] += 1
        ctx.cfg, ctx.batch, ctx.rnd, ctx.tape, ctx.table, ctx.scratch_floats = cfg, batch, rnd, tape, table, scratch_floats
        ctx.slots = [p is not None for p in params]
        ctx.save_for_backward(x, *live)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = _lib.load_snapshots()
        x, *live = ctx.saved_tensors
        dev = x.device
        cfg, T = ctx.cfg, len(ctx.batch)
        offs, P = tiny._layout(live)
        slabs = torch.empty(T * P, dtype=torch.float32, device=dev)
        flat = torch.empty(P, dtype=torch.float32, device=dev)
        dx = torch.empty((x.shape[0], cfg.in_channels), dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        scratch = torch.empty(ctx.scratch_floats, dtype=torch.float32, device=dev)
        base, it = slabs.data_ptr(), iter(offs)
        grads = (ctypes.c_void_p * len(ctx.slots))(*[base + 4 * next(it) if has else None for has in ctx.slots])
        li = iter(live)
        pa = tiny._ptr_array([next(li) if has else None for has in ctx.slots])
        gyc = gy if gy.is_contiguous() else gy.contiguous()
        rc = lib.dif_snap_backward_f32(ctypes.byref(cfg), T, ctx.table.data_ptr(), x.data_ptr(), x.shape[1], pa,
                                       None if ctx.rnd is None else ctx.rnd.data_ptr(), ctx.tape.data_ptr(), gyc.data_ptr(), grads,
                                       slabs.data_ptr(), P, flat.data_ptr(), None if dx is None else dx.data_ptr(),
                                       scratch.data_ptr(), _stream(dev))
        _lib.check_snapshots(rc, "dif_snap_backward_f32")
        stats["backward"] += 1
        return (None, dx) + tuple(flat[o: o + p.numel()].view(p.shape) for o, p in zip(offs, live))


def forward_snapshots(model, batch, *, _uniforms=None):
    """-> Y [sum n_b, out_channels]: the rows of model(x_b, edge_index_b, edge_weight_b) for b = 0 .. T - 1, stacked."""
    plan = _plan(model, batch)
    if plan is None:
        stats["fallback"] += 1
        return torch.cat([model(x, ei, ew) for x, ei, ew in zip(batch.split(batch.x), batch.edge_index, batch.edge_weight)], dim=0)
    fields, params = plan
    fields["n"] = batch.max_n
    live = [p for p in params if p is not None]
    training = bool(model.training)
    p_drop = float(model.__dict__["dropout"]) if training else 0.0           # eval: dropout is the identity
    rnd = None
    if training and p_drop > 0.0:
        # ONE draw for the whole batch: snapshot b's [(L + 1), n_b, d] block at (L + 1) * d * node_ptr[b]
        count = (fields["num_layers"] + 1) * batch.node_ptr[-1] * fields["hidden"]
        rnd = torch.rand(count, device=batch.x.device) if _uniforms is None else _uniforms
        if rnd.numel() != count or rnd.dtype != torch.float32 or rnd.device != batch.x.device or not rnd.is_contiguous():
            raise ValueError(f"difformer_amd: _uniforms must be {count} contiguous float32 values on the batch's device")
    return _Snapshots.apply((fields, params, batch, p_drop, training, rnd), batch.x, *live)
