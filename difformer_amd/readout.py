"""The graph read-out of the reference's graph-level model (physical particle/models.py:13-36): one row per graph from the node
rows of a batch, and the model that puts it behind a node-level network.

    global_add_pool(x, batch=None, size=None, *, n_nodes=None)      global_mean_pool(...)      global_max_pool(...)
    GraphGNN(in_channels, out_channels, gnn, graph_pooling='mean')

x is [N, H], all graphs of the batch back to back; the result is [B, H].  The graphs are given either as torch_geometric's
`batch` (int64 [N], the graph id of every row, with the optional `size` = B) or as `n_nodes` ([B], the node count per graph:
what `DIFFormer_v2.forward` takes).  Exactly one of the two.  `n_nodes` goes through `ops.layout_cache`, so a read-out behind
the model re-uses the model's layout and adds no host synchronisation; a sorted `batch` is converted once per tensor (a
bincount and one sortedness check) and remembered by the tensor's identity.

Device tensors (float32 or bfloat16, H <= 1,024, rows sorted by graph) go through csrc/graph_readout.hip (C ABI
include/difformer_readout.h): one launch forward, one backward.  Sums run in float64 in a fixed order and are rounded once, so
two calls on equal operands are bitwise equal -- the scatter of torch_geometric adds with floating-point atomics and is not.  An
empty graph gives a row of +0 in all three modes (the count of `mean` is clamped to 1) and `max` splits the gradient evenly
among tied rows, both as current torch_geometric; NaN in a column of `max` gives NaN, as torch.amax.  First derivatives only.

Everything else -- CPU tensors, float64 / float16, H > 1,024, an unsorted `batch`, no rows at all -- takes the tensor expression
(`index_add_` / `scatter_reduce(amax, include_self=False)`) with the same values for empty graphs.
"""
from __future__ import annotations

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from . import ops
from .tensor_cache import MISS, TensorCache

__all__ = ["global_add_pool", "global_mean_pool", "global_max_pool", "GraphGNN"]

MAX_COLUMNS = 1024          # DIF_READOUT_MAX_COLUMNS of include/difformer_readout.h
_DEVICE_DTYPES = (torch.float32, torch.bfloat16)


class _BatchCache(TensorCache):
    """`batch` tensor, size -> (n_nodes int64 [B], sorted?): one bincount and one sortedness check (one host read) per tensor."""

    def get(self, batch, size):
        extras = (size,)
        hit = self.lookup((batch,), extras)
        if hit is MISS:
            counts = torch.bincount(batch, minlength=size or 0)
            if size is not None and counts.shape[0] > size:
                raise ValueError(f"difformer_amd: batch holds graph ids up to {counts.shape[0] - 1} for size = {size}")
            is_sorted = bool((batch[1:] >= batch[:-1]).all()) if batch.shape[0] > 1 else True
            hit = self.insert((batch,), extras, (counts, is_sorted))
        return hit


batch_cache = _BatchCache(16, unversioned=True)


class _Readout(torch.autograd.Function):
    """One pool of csrc/graph_readout.hip over the row ranges of `graph_ptr` (int32 [B + 1]); mode 'add' | 'mean' | 'max'."""

    @staticmethod
    def forward(ctx, x, graph_ptr, mode):
        xd = x.detach()
        out = ops.get_backend().readout_fwd(xd, graph_ptr, mode)
        ctx.mode, ctx.n_rows = mode, x.shape[0]
        if mode == "max":
            ctx.save_for_backward(graph_ptr, xd, out)
        else:
            ctx.save_for_backward(graph_ptr)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        graph_ptr, *rest = ctx.saved_tensors
        x, pooled = rest if rest else (None, None)
        grad = ops.get_backend().readout_bwd(grad_out.detach(), graph_ptr, ctx.mode, ctx.n_rows, x, pooled)
        return grad, None, None


def _expression(mode, x, batch, B):
    """The pool as tensor operations; empty graphs are rows of zeros."""
    H = x.shape[1]
    zeros = torch.zeros((B, H), dtype=x.dtype, device=x.device)
    if mode == "max":
        return zeros.scatter_reduce(0, batch[:, None].expand(-1, H), x, "amax", include_self=False)
    out = zeros.index_add_(0, batch, x)
    if mode == "mean":
        out = out / torch.bincount(batch, minlength=B).clamp(min=1).to(x.dtype)[:, None]
    return out


def _pool(who, mode, x, batch, size, n_nodes):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{who}: x must be a tensor [N, H] (got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__})")
    if (batch is None) == (n_nodes is None):
        raise ValueError(f"{who}: give exactly one of batch (the graph id of every row) and n_nodes (the node count per graph)")
    N, H = x.shape
    on_device = x.is_cuda and x.dtype in _DEVICE_DTYPES and 1 <= H <= MAX_COLUMNS and N > 0
    if n_nodes is not None:
        if on_device:
            layout = ops.layout_cache.get(n_nodes, x.device)
            if layout.n_rows != N or (size is not None and size != layout.n_graphs):
                raise ValueError(f"{who}: n_nodes describes {layout.n_graphs} graphs of {layout.n_rows} rows; x has {N} rows"
                                 + (f", size = {size}" if size is not None else ""))
            return _Readout.apply(x, layout.graph_ptr, mode)
        counts = torch.as_tensor(n_nodes).to(device=x.device, dtype=torch.int64).reshape(-1)
        B = counts.shape[0]
        if int(counts.sum()) != N or (size is not None and size != B):
            raise ValueError(f"{who}: n_nodes describes {B} graphs of {int(counts.sum())} rows; x has {N} rows"
                             + (f", size = {size}" if size is not None else ""))
        return _expression(mode, x, torch.repeat_interleave(torch.arange(B, device=x.device), counts), B)
    if not torch.is_tensor(batch) or batch.dtype != torch.int64 or tuple(batch.shape) != (N,) or batch.device != x.device:
        raise ValueError(f"{who}: batch must be int64 [{N}] on {x.device} (got "
                         f"{(batch.dtype, tuple(batch.shape), batch.device) if torch.is_tensor(batch) else type(batch).__name__})")
    if size is not None:
        size = int(size)
    if on_device:
        counts, is_sorted = batch_cache.get(batch, size)
        if is_sorted:
            return _Readout.apply(x, ops.layout_cache.get(counts, x.device).graph_ptr, mode)
        return _expression(mode, x, batch, counts.shape[0])
    B = size if size is not None else (int(batch.max()) + 1 if N else 0)
    if N and int(batch.max()) >= B:
        raise ValueError(f"difformer_amd: batch holds graph ids up to {int(batch.max())} for size = {B}")
    return _expression(mode, x, batch, B)


def global_add_pool(x, batch=None, size=None, *, n_nodes=None):
    """out[b] = the sum of the rows of graph b.  x [N, H]; batch int64 [N] (with size = B) or n_nodes [B] -> [B, H]."""
    return _pool("global_add_pool", "add", x, batch, size, n_nodes)


def global_mean_pool(x, batch=None, size=None, *, n_nodes=None):
    """out[b] = the mean of the rows of graph b (+0 for a graph without rows).  Operands as global_add_pool."""
    return _pool("global_mean_pool", "mean", x, batch, size, n_nodes)


def global_max_pool(x, batch=None, size=None, *, n_nodes=None):
    """out[b] = the column-wise maximum of the rows of graph b (+0 for a graph without rows; the gradient is split evenly among
    tied rows).  Operands as global_add_pool."""
    return _pool("global_max_pool", "max", x, batch, size, n_nodes)


_POOLS = {"sum": global_add_pool, "mean": global_mean_pool, "max": global_max_pool}


class GraphGNN(nn.Module):
    """Reference: physical particle/models.py:13-36 -- `lin(pool(gnn_node(...)))`, one row of logits per graph.  `gnn` is the
    node-level model (DIFFormer_v2: `gnn(x, edge_index, n_nodes)` -> [N, in_channels]); graph_pooling 'sum' | 'mean' | 'max'.

    forward takes both call forms the reference contains: `model(x, edge_index, n_nodes)` (main.py:85) and
    `model(batched_data)` (models.py:28) with `.x`, `.edge_index` and `.n_nodes` or a sorted `.batch`."""

    def __init__(self, in_channels, out_channels, gnn, graph_pooling='mean'):
        super().__init__()
        if graph_pooling not in _POOLS:
            raise ValueError(f"difformer_amd: graph_pooling must be 'sum', 'mean' or 'max' (got {graph_pooling!r})")
        self.graph_pooling = graph_pooling
        self.pool = _POOLS[graph_pooling]
        self.gnn_node = gnn
        self.lin = nn.Linear(in_channels, out_channels)

    def reset_parameters(self):
        self.lin.reset_parameters()
        self.gnn_node.reset_parameters()

    def forward(self, x, edge_index=None, n_nodes=None):
        if not torch.is_tensor(x):                                   # models.py:28: one batched_data object
            data = x
            x, edge_index = data.x, getattr(data, "edge_index", None)
            n_nodes = getattr(data, "n_nodes", None)
            if n_nodes is None:
                batch = getattr(data, "batch", None)
                if batch is None:
                    raise ValueError("difformer_amd: GraphGNN needs batched_data.n_nodes or batched_data.batch")
                n_nodes, is_sorted = batch_cache.get(batch, None)
                if not is_sorted:
                    raise ValueError("difformer_amd: GraphGNN takes the graphs of a batch back to back; batched_data.batch is not sorted")
        elif n_nodes is None:
            raise ValueError("difformer_amd: GraphGNN.forward(x, edge_index, n_nodes) needs n_nodes")
        h_node = self.gnn_node(x, edge_index, n_nodes)
        return self.lin(self.pool(h_node, n_nodes=n_nodes))
