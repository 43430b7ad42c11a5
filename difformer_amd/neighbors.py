"""k-nearest-neighbour and radius graphs of a feature matrix, built on the device and exact to the float64 order.

Two of the reference's task folders make their graph from the features: `spatial-temporal/main.py:96-98` and `eval.py:11-12`
(`--special_treat knn`) call `torch_cluster.knn_graph(snapshot.x, k=5, loop=True, cosine=True)` for every snapshot of every
epoch, and `image and text/main.py:52-53` calls `sklearn.neighbors.kneighbors_graph(node_feat, n_neighbors=args.k,
include_self=True)` once per dataset on the host.  `knn_graph` and `kneighbors_graph` return the same graphs as int64 edge
lists from csrc/knn_graph.hip (C ABI include/difformer_knn.h): no [N, N] tensor exists, and nothing of torch_cluster or
sklearn is used.

A graph is a discrete object, so the contract is on the neighbour SET AND ORDER, not on values.  Every distance is computed
in float64 from the float32 rows (bfloat16 / float64 / float16 inputs are converted to float32 first):

    Euclidean   d(i, j) = sum_m (x[i, m] - x[j, m])^2          (returned as its square root)
    cosine      d(i, j) = 1 - (x_i . x_j) / (|x_i| |x_j|)

and per node the kk = min(k, N - (0 if loop else 1)) smallest come first under one total order: the smaller distance first,
among equal distances the lower index first, a NaN distance after every number.  A zero row has cosine 0 with every row, so
its cosine distance is 1 (the reference divides by zero there).  Without self-loops j == i is excluded by index only:
duplicates of a point stay eligible.  Outputs are detached: there is no gradient through a selection.

Stated deviations from the originals: torch_cluster with loop=False takes k + 1 neighbours and drops row == col, which leaves
k + 1 for a node that a duplicate displaced -- here it is always kk; neither original specifies ties -- here they are; and
torch_cluster's `radius_graph` keeps an ARBITRARY subset when more than max_num_neighbors nodes lie inside the radius -- here
the max_num_neighbors nearest under the same order are kept.

Batches.  The `physical particle` datasets build one graph per sample (synmol.py:117, actstrack.py:178, plbind.py:224:
`knn_graph(pos, k=5, loop=True)`; tau3mu.py:95: `radius_graph(pos, r=1.0, loop=True)`), and the spatial-temporal loop one per
snapshot.  With `batch=` (int64 [N] of non-decreasing graph ids) or `n_nodes=` ([B] node counts; one or the other, the rules of
readout.py) `knn_graph` and `radius_graph` build the graphs of all samples stored back to back in one launch of
csrc/nbr_batched.hip (C ABI include/difformer_nbr.h): neighbours are searched inside a node's own graph only, indices are
global row numbers, and the layout comes from `ops.layout_cache`, which the model's forward over the same batch shares.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from . import staging

__all__ = ["knn_graph", "kneighbors_graph", "radius_graph", "MAX_K", "MAX_WIDTH", "MAX_BATCHED_WIDTH", "MAX_RADIUS_NEIGHBORS"]

MAX_K = 24          # the lists the direct kernel keeps in registers (kMaxK of csrc/knn_graph.hip)
MAX_WIDTH = 512     # columns the kernels contract over (kMaxM)
MAX_BATCHED_WIDTH = 64        # DIF_NBR_MAX_COLUMNS of include/difformer_nbr.h: the rows the batched kernel holds in registers
MAX_RADIUS_NEIGHBORS = 32     # DIF_NBR_MAX_CAP
_FLOWS = ("source_to_target", "target_to_source")


def _rows_for_kernel(x):
    """x [N, M] -> float32 rows as the kernels read them, four columns at a time: M zero-padded to a multiple of 4 (zero columns
    change no distance: exact), unit column stride, 16-byte aligned rows a multiple of 4 elements apart.  A view that already is
    all that is not copied."""
    xs = x.detach().float()
    N, M = xs.shape
    if M % 4:
        xs = F.pad(xs, (0, 4 - M % 4))
    ld = xs.stride(0) if N > 1 else xs.shape[1]
    if xs.stride(1) != 1 or ld < xs.shape[1] or ld % 4 or xs.data_ptr() % 16:
        xs = xs.clone(memory_format=torch.contiguous_format)
    return xs


def _graph(who, x, k, loop, cosine, centre_row, return_distance, route):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{who}: x must be a 2-d tensor [N, M] (got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__})")
    if not x.is_floating_point():
        raise ValueError(f"{who}: x must be floating point (got {x.dtype})")
    k = int(k)
    if k < 1:
        raise ValueError(f"{who}: k must be at least 1 (got {k})")
    if k > MAX_K:
        raise ValueError(f"{who}: k = {k} exceeds the limit of {MAX_K} neighbours per node")
    N, M = x.shape
    if N < 1 or M < 1:
        raise ValueError(f"{who}: x must hold at least 1 row and 1 column (got {tuple(x.shape)})")
    if M > MAX_WIDTH:
        raise ValueError(f"{who}: rows of {M} columns exceed the limit of {MAX_WIDTH}")
    if route not in (None, 0, 1):
        raise ValueError(f"{who}: unknown route {route!r}")
    dev = staging.staging_device(None, (x,))
    if dev is not None:      # a host tensor: computed on the GPU, returned on the host
        out = _graph(who, x.to(dev), k, loop, cosine, centre_row, return_distance, route)
        return tuple(o.to(x.device) for o in out) if return_distance else out.to(x.device)
    with torch.no_grad():
        if N - (0 if loop else 1) == 0:                              # one node, no self-loop
            edge_index = torch.empty((2, 0), dtype=torch.int64, device=x.device)
            dist = torch.empty(0, dtype=torch.float32, device=x.device)
        else:
            edge_index, dist = ops.get_backend().knn_graph(_rows_for_kernel(x), k, bool(loop), 1 if cosine else 0, centre_row,
                                                           want_dist=bool(return_distance), route=-1 if route is None else route)
    return (edge_index, dist) if return_distance else edge_index


def _check_points(who, x):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f"{who}: x must be a 2-d tensor [N, M] (got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__})")
    if not x.is_floating_point():
        raise ValueError(f"{who}: x must be floating point (got {x.dtype})")
    N, M = x.shape
    if N < 1 or M < 1:
        raise ValueError(f"{who}: x must hold at least 1 row and 1 column (got {tuple(x.shape)})")
    return N, M


def _check_batch(who, x, batch, n_nodes):
    """The argument rules of readout.py for `batch` / `n_nodes`, checked where the tensors live (no device needed)."""
    N = x.shape[0]
    if batch is not None and n_nodes is not None:
        raise ValueError(f"{who}: give one of batch (the graph id of every row) and n_nodes (the node count per graph), not both")
    if batch is not None:
        if not torch.is_tensor(batch) or batch.dtype != torch.int64 or tuple(batch.shape) != (N,) or batch.device != x.device:
            raise ValueError(f"{who}: batch must be int64 [{N}] on {x.device} (got "
                             f"{(batch.dtype, tuple(batch.shape), batch.device) if torch.is_tensor(batch) else type(batch).__name__})")
        if not batch.is_cuda and N > 1 and not bool((batch[1:] >= batch[:-1]).all()):      # on the device: _layout, with the counts
            raise ValueError(f"{who}: batch must be sorted (non-decreasing graph ids): the graphs are stored back to back")
        return
    if torch.is_tensor(n_nodes) and (n_nodes.is_floating_point() or n_nodes.dim() != 1):
        raise ValueError(f"{who}: n_nodes must be integers [B] (got {n_nodes.dtype}, {tuple(n_nodes.shape)})")


def _layout(who, x, batch, n_nodes):
    """-> the ops.BatchLayout of the batch on x's device (x is on the GPU here)."""
    N = x.shape[0]
    if batch is not None:
        from .readout import batch_cache                      # one bincount and one sortedness check (one host read) per tensor
        n_nodes, is_sorted = batch_cache.get(batch, None)
        if not is_sorted:
            raise ValueError(f"{who}: batch must be sorted (non-decreasing graph ids): the graphs are stored back to back")
    layout = ops.layout_cache.get(n_nodes, x.device)
    if layout.n_rows != N:
        raise ValueError(f"{who}: n_nodes describes {layout.n_graphs} graphs of {layout.n_rows} rows; x has {N} rows")
    return layout


def _to_host(out, device):
    return tuple(o.to(device) for o in out) if isinstance(out, tuple) else out.to(device)


def _knn_edges(layout, k, loop):
    """-> (edge_ptr int64 [B + 1], E): edge_ptr[b] = sum over b' < b of n_b' kk_b', kk_b = min(k, n_b - (0 if loop else 1)).  B-sized
    integer bookkeeping, kept on the layout; E is known without a host read when every graph has at least k candidates."""
    memo = layout.__dict__.setdefault("_knn_edges", {})
    hit = memo.get((k, loop))
    if hit is None:
        n_b = (layout.graph_ptr[1:] - layout.graph_ptr[:-1]).to(torch.int64)
        kk_b = (n_b - (0 if loop else 1)).clamp(min=0, max=k)
        edge_ptr = torch.zeros(layout.n_graphs + 1, dtype=torch.int64, device=n_b.device)
        torch.cumsum(n_b * kk_b, 0, out=edge_ptr[1:])
        E = layout.n_rows * k if layout.min_nodes - (0 if loop else 1) >= k else int(edge_ptr[-1])
        hit = memo[(k, loop)] = (edge_ptr, E)
    return hit


def _batched_knn(x, k, loop, cosine, centre_row, return_distance, batch, n_nodes):
    who = "knn_graph"
    N, M = _check_points(who, x)
    k = int(k)
    if k < 1:
        raise ValueError(f"{who}: k must be at least 1 (got {k})")
    if k > MAX_K:
        raise ValueError(f"{who}: k = {k} exceeds the limit of {MAX_K} neighbours per node")
    if M > MAX_WIDTH:
        raise ValueError(f"{who}: rows of {M} columns exceed the limit of {MAX_WIDTH}")
    _check_batch(who, x, batch, n_nodes)
    dev = staging.staging_device(None, (x,))
    if dev is not None:      # host tensors: computed on the GPU, returned on the host
        out = _batched_knn(x.to(dev), k, loop, cosine, centre_row, return_distance, None if batch is None else batch.to(dev),
                           n_nodes)
        return _to_host(out, x.device)
    with torch.no_grad():
        layout = _layout(who, x, batch, n_nodes)
        loop = bool(loop)
        if M > MAX_BATCHED_WIDTH:
            # wider rows than the batched kernel holds: the single-graph entry point per graph, indices offset
            ptr = layout.graph_ptr.tolist()
            parts = []
            for lo, hi in zip(ptr[:-1], ptr[1:]):
                if hi - lo - (0 if loop else 1) > 0:
                    ei, dist = _graph(who, x[lo:hi], k, loop, cosine, centre_row, True, None)
                    parts.append((ei + lo, dist))
            if parts:
                edge_index, dist = torch.cat([p[0] for p in parts], dim=1), torch.cat([p[1] for p in parts])
            else:
                edge_index = torch.empty((2, 0), dtype=torch.int64, device=x.device)
                dist = torch.empty(0, dtype=torch.float32, device=x.device)
        else:
            edge_ptr, E = _knn_edges(layout, k, loop)
            edge_index, dist = ops.get_backend().nbr_knn(_rows_for_kernel(x), layout.graph_ptr, edge_ptr, E, k, loop,
                                                         1 if cosine else 0, centre_row, want_dist=bool(return_distance))
    return (edge_index, dist) if return_distance else edge_index


def knn_graph(x, k, loop=False, flow="source_to_target", cosine=False, return_distance=False, *, batch=None, n_nodes=None,
              _route=None):
    """torch_cluster's `knn_graph`: x [N, M] -> int64 [2, N kk] on x's device, kk = min(k, N - (0 if loop else 1)).  Edges are
    grouped by centre node ascending, nearest first.  flow='source_to_target': row 0 is the neighbour and row 1 the centre (what
    `gcn_conv` aggregates at); 'target_to_source': the rows swapped.  cosine=True ranks by 1 - cos, and a zero row has cosine 0
    with every row (distance 1; the reference divides by zero there).  Ties go to the lower index, a NaN distance after every
    number.  return_distance=True: -> (that, float32 [N kk]) with the Euclidean distance or 1 - cos per edge.  1 <= k <= 24,
    M <= 512.

    batch (int64 [N], non-decreasing graph ids) or n_nodes ([B] node counts), keyword-only and one or the other: x holds B
    graphs back to back, neighbours are searched inside a node's own graph only, and indices are global row numbers.  Node i
    of graph b (n_b nodes) gets kk_b = min(k, n_b - (0 if loop else 1)) neighbours -- an empty graph, or a one-node graph
    without loop, contributes no edges -- so the result is int64 [2, sum_b n_b kk_b], still grouped by centre ascending, nearest
    first, under the same order and metrics.  One launch for M <= 64 (csrc/nbr_batched.hip); wider rows run the single-graph
    kernels graph by graph.  The layout comes from `ops.layout_cache`; when every graph has more than k nodes the call adds no
    host wait of its own (E = N k).  An unsorted batch raises ValueError.  With neither argument the call is the single-graph
    one, unchanged."""
    if flow not in _FLOWS:
        raise ValueError(f"knn_graph: unknown flow {flow!r} (expected 'source_to_target' or 'target_to_source')")
    centre_row = 1 if flow == "source_to_target" else 0
    if batch is None and n_nodes is None:
        return _graph("knn_graph", x, k, loop, cosine, centre_row, return_distance, _route)
    return _batched_knn(x, k, loop, cosine, centre_row, return_distance, batch, n_nodes)


def radius_graph(x, r, loop=False, max_num_neighbors=32, flow="source_to_target", return_distance=False, *, batch=None,
                 n_nodes=None):
    """torch_cluster's `radius_graph` (Euclidean): x [N, M] -> int64 [2, E] on x's device, an edge for every pair of nodes of the
    same graph closer than r.  This package's rule, stated: node j is a neighbour of i when the float64 squared distance
    d(i, j) = sum_m (x[i, m] - x[j, m])^2 satisfies d(i, j) < r * r -- r held as a double, the comparison STRICT.  j == i is
    excluded by index unless loop (duplicates of a point stay eligible); a NaN distance is never inside, so a row with a NaN has
    no edges, not even its self-loop.  When more than max_num_neighbors nodes are inside, the max_num_neighbors NEAREST are kept,
    under the order of `knn_graph` (smaller distance, then lower index); torch_cluster documents its subset as arbitrary, so
    one deterministic choice keeps its contract.  1 <= max_num_neighbors <= 32 (torch_cluster's default), M <= 64.

    Edges are grouped by centre ascending, nearest first; flow as in `knn_graph`.  return_distance=True: -> (that, float32 [E]
    Euclidean distances).  batch / n_nodes (keyword-only, one or the other) as in `knn_graph`; with neither, x is one graph.
    E depends on the data, so the call reads ONE integer back from the device -- its only host wait beyond the layout's own.
    Host tensors are staged to the GPU and the result comes back on the host.  Outputs are detached."""
    who = "radius_graph"
    if flow not in _FLOWS:
        raise ValueError(f"{who}: unknown flow {flow!r} (expected 'source_to_target' or 'target_to_source')")
    N, M = _check_points(who, x)
    try:
        r = float(r)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: r must be a number (got {type(r).__name__})") from None
    if not r >= 0.0:
        raise ValueError(f"{who}: r must be a number >= 0 (got {r})")
    cap = int(max_num_neighbors)
    if cap < 1:
        raise ValueError(f"{who}: max_num_neighbors must be at least 1 (got {cap})")
    if cap > MAX_RADIUS_NEIGHBORS:
        raise ValueError(f"{who}: max_num_neighbors = {cap} exceeds the limit of {MAX_RADIUS_NEIGHBORS} neighbours per node")
    if M > MAX_BATCHED_WIDTH:
        raise ValueError(f"{who}: rows of {M} columns exceed the limit of {MAX_BATCHED_WIDTH}")
    _check_batch(who, x, batch, n_nodes)
    dev = staging.staging_device(None, (x,))
    if dev is not None:      # host tensors: computed on the GPU, returned on the host
        out = radius_graph(x.to(dev), r, loop, cap, flow, return_distance, batch=None if batch is None else batch.to(dev),
                           n_nodes=n_nodes)
        return _to_host(out, x.device)
    centre_row = 1 if flow == "source_to_target" else 0
    with torch.no_grad():
        if batch is None and n_nodes is None:
            graph_ptr = torch.tensor([0, N], dtype=torch.int32, device=x.device)
        else:
            graph_ptr = _layout(who, x, batch, n_nodes).graph_ptr
        be = ops.get_backend()
        deg, ws = be.nbr_radius_lists(_rows_for_kernel(x), graph_ptr, r, bool(loop), cap)
        deg_ptr = torch.zeros(N + 1, dtype=torch.int64, device=x.device)
        torch.cumsum(deg, 0, dtype=torch.int64, out=deg_ptr[1:])    # integer, exact
        E = int(deg_ptr[-1])                                     # the one value the host reads
        edge_index, dist = be.nbr_radius_edges(deg_ptr, E, cap, centre_row, ws, want_dist=bool(return_distance))
    return (edge_index, dist) if return_distance else edge_index


def kneighbors_graph(x, n_neighbors, include_self=False, return_distance=False, *, _route=None):
    """sklearn's `kneighbors_graph` (Euclidean, connectivity) as the edge list `image and text/main.py:52-53` makes of it,
    `torch.tensor(adj.nonzero())`: x [N, M] -> int64 [2, N kk], row 0 the centre and row 1 the neighbour, centres ascending,
    nearest first.  Ties go to the lower index.  return_distance=True: -> (that, float32 [N kk] Euclidean distances).
    1 <= n_neighbors <= 24, M <= 512."""
    return _graph("kneighbors_graph", x, n_neighbors, include_self, False, 0, return_distance, _route)
