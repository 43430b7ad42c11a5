"""k-nearest-neighbour graphs of a feature matrix, built on the device and exact to the float64 order.

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
k + 1 for a node that a duplicate displaced -- here it is always kk; and neither original specifies ties -- here they are.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from . import staging

__all__ = ["knn_graph", "kneighbors_graph", "MAX_K", "MAX_WIDTH"]

MAX_K = 24          # the lists the direct kernel keeps in registers (kMaxK of csrc/knn_graph.hip)
MAX_WIDTH = 512     # columns the kernels contract over (kMaxM)


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
        xs = x.detach().float()                                      # the kernels read float32
        if N - (0 if loop else 1) == 0:                              # one node, no self-loop
            edge_index = torch.empty((2, 0), dtype=torch.int64, device=x.device)
            dist = torch.empty(0, dtype=torch.float32, device=x.device)
        else:
            if M % 4:                                                # zero columns change no distance: exact
                xs = F.pad(xs, (0, 4 - M % 4))
            ld = xs.stride(0) if N > 1 else xs.shape[1]
            if xs.stride(1) != 1 or ld < xs.shape[1] or ld % 4 or xs.data_ptr() % 16:
                xs = xs.clone(memory_format=torch.contiguous_format)  # the kernels read rows four columns at a time, 16-byte aligned
            edge_index, dist = ops.get_backend().knn_graph(xs, k, bool(loop), 1 if cosine else 0, centre_row,
                                                           want_dist=bool(return_distance), route=-1 if route is None else route)
    return (edge_index, dist) if return_distance else edge_index


def knn_graph(x, k, loop=False, flow="source_to_target", cosine=False, return_distance=False, *, _route=None):
    """torch_cluster's `knn_graph` without `batch`: x [N, M] -> int64 [2, N kk] on x's device, kk = min(k, N - (0 if loop else
    1)).  Edges are grouped by centre node ascending, nearest first.  flow='source_to_target': row 0 is the neighbour and row 1
    the centre (what `gcn_conv` aggregates at); 'target_to_source': the rows swapped.  cosine=True ranks by 1 - cos, and a zero
    row has cosine 0 with every row (distance 1; the reference divides by zero there).  Ties go to the lower index, a NaN
    distance after every number.  return_distance=True: -> (that, float32 [N kk]) with the Euclidean distance or 1 - cos per
    edge.  1 <= k <= 24, M <= 512."""
    if flow not in ("source_to_target", "target_to_source"):
        raise ValueError(f"knn_graph: unknown flow {flow!r} (expected 'source_to_target' or 'target_to_source')")
    return _graph("knn_graph", x, k, loop, cosine, 1 if flow == "source_to_target" else 0, return_distance, _route)


def kneighbors_graph(x, n_neighbors, include_self=False, return_distance=False, *, _route=None):
    """sklearn's `kneighbors_graph` (Euclidean, connectivity) as the edge list `image and text/main.py:52-53` makes of it,
    `torch.tensor(adj.nonzero())`: x [N, M] -> int64 [2, N kk], row 0 the centre and row 1 the neighbour, centres ascending,
    nearest first.  Ties go to the lower index.  return_distance=True: -> (that, float32 [N kk] Euclidean distances).
    1 <= n_neighbors <= 24, M <= 512."""
    return _graph("kneighbors_graph", x, n_neighbors, include_self, False, 0, return_distance, _route)
