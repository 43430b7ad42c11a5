"""Attention maps without the dense [N, L, H] map: per node and head the k keys it attends to most (`attention_topk`), and the
attention at the edges of a graph with its per-node sum (`attention_on_edges`).

The reference's interpretability output is the dense attention (`full_attention_conv(..., output_attn=True)`,
`DIFFormer.get_attentions`; node classification/difformer.py:42-43 `simple`, :47-55 `sigmoid`, :211-226).  That tensor is
900 MB per layer and head at 15,000 nodes and does not exist at the sizes this package is built for; what is read off it is
the handful of strongest keys of a row.  `attention_topk` returns exactly those, from one sweep over key tiles that keeps a
running top-k per query row in registers (csrc/attn_topk.hip, C ABI include/difformer_maps.h).  Outputs are detached: there
is no gradient through a selection.

`attention_on_edges` answers the question a graph model raises next: how much attention does a node put on each of the
neighbours it was given, and how much of its attention row lies on the input graph at all (a layer diffuses along the graph
or across it).  One dot product per edge, rows gathered by index (csrc/attn_edges.hip, C ABI include/difformer_edges.h).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from . import staging

__all__ = ["attention_topk", "attention_on_edges", "MAX_K", "MAX_WIDTH"]

MAX_K = 32          # the lists the kernel keeps in registers (kMaxTopk of csrc/attn_topk.hip)
MAX_WIDTH = 512     # columns per head the kernel contracts over (kMaxM)


def _simple_scale(qs, ks):
    """[N,H,1]: 1 / (|q| |k| den[n,h]) with den = q^.sum_l k^ + N (difformer.py:20-22,32-38): folded into the query rows, the
    score q'.k IS the attention weight of :43 -- the visualisation numerator has no `+ 1`, as in the reference."""
    inv = 1.0 / (torch.linalg.vector_norm(qs) * torch.linalg.vector_norm(ks))
    den = torch.einsum("nhm,hm->nh", qs, ks.sum(dim=0)) * inv + qs.shape[0]
    return (inv / den).unsqueeze(-1)


def attention_topk(qs, ks, kernel, k):
    """qs [N,H,M], ks [L,H,M] -> (values float32 [N,H,k], indices int64 [N,H,k]): for every query row and head the k
    largest attention weights a[n,:,h] of the reference's dense map, descending, and the keys they belong to.  One total
    order: the larger weight first, among equal weights the lower key index.  For `sigmoid` the rank is taken on the score
    q.k (sigma is monotone, and the score stays decisive where sigma saturates in float32).  1 <= k <= min(L, 32)."""
    if kernel not in ("simple", "sigmoid"):
        raise ValueError(f"unknown attention kernel {kernel!r} (expected 'simple' or 'sigmoid')")
    if qs.dim() != 3 or ks.dim() != 3 or qs.shape[1:] != ks.shape[1:]:
        raise ValueError(f"attention_topk: qs [N,H,M] and ks [L,H,M] expected (got {tuple(qs.shape)} and {tuple(ks.shape)})")
    k = int(k)
    L, M = ks.shape[0], ks.shape[2]
    if k < 1:
        raise ValueError(f"attention_topk: k must be at least 1 (got {k})")
    if k > MAX_K:
        raise ValueError(f"attention_topk: k = {k} exceeds the limit of {MAX_K} keys per row")
    if k > L:
        raise ValueError(f"attention_topk: k = {k} exceeds the number of keys L = {L}")
    if M > MAX_WIDTH:
        raise ValueError(f"attention_topk: heads of {M} columns exceed the limit of {MAX_WIDTH}")
    dev = staging.staging_device(None, (qs, ks))
    if dev is not None:      # host operands: computed on the GPU, returned on the host
        values, indices = attention_topk(qs.to(dev), ks.to(dev), kernel, k)
        return values.to(qs.device), indices.to(qs.device)
    with torch.no_grad():
        qs, ks = qs.detach().float(), ks.detach().float()        # bfloat16 is storage only: scores and ranks in float32
        if kernel == "simple":
            qs = qs * _simple_scale(qs, ks)
        if M % 4:                                                # zero columns add nothing to a score: exact
            qs, ks = F.pad(qs, (0, 4 - M % 4)), F.pad(ks, (0, 4 - M % 4))
        values, indices = ops.get_backend().attn_topk(qs, ks, 0 if kernel == "simple" else 1, k)
        return values, indices.long()


def _check_edges(edge_index):
    if not torch.is_tensor(edge_index) or edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.shape[0] != 2:
        raise TypeError("attention_on_edges: edge_index must be an int64 tensor of shape [2, E]")


def _edges_of(qs, ks, mode, scale, edge_index, csr):
    """qs / ks float32 (any M), scale [N,H] -> (values [E,H], mass [N,H] | None) through the backend; raises IndexError for an
    id out of range.  csr: None (no mass) or a one-element list holding the target-row CSR of the edge list, built here -- after
    the edge kernel, which names the side of a bad id where the build could only say that there is one -- when it holds None."""
    N, H, M = qs.shape
    L, E = ks.shape[0], edge_index.shape[1]
    if M % 4:                                                    # zero columns add nothing to a product: exact
        qs, ks = F.pad(qs, (0, 4 - M % 4)), F.pad(ks, (0, 4 - M % 4))
    be = ops.get_backend()
    if E == 0:                                                   # (the entry points take at least one edge)
        values = torch.zeros((0, H), dtype=torch.float32, device=qs.device)
        return values, (None if csr is None else torch.zeros((N, H), dtype=torch.float32, device=qs.device))
    values, status = be.edge_attention(qs, ks, scale, edge_index, mode)
    _, bad_key, bad_query = status.tolist()
    if bad_key or bad_query:
        sides = [f"source (key) ids outside [0, {L})"] * bool(bad_key) + [f"target (query) ids outside [0, {N})"] * bool(bad_query)
        raise IndexError("attention_on_edges: edge_index holds " + " and ".join(sides))
    if csr is None:
        return values, None
    if csr[0] is None:                                           # unweighted; rowptr and src are all that is read of it
        csr[0] = ops.GraphCSR.build(edge_index, None, max(N, L), 1)
    return values, be.edge_attention_mass(qs, ks, scale, csr[0].rowptr, csr[0].src, mode)


def attention_on_edges(qs, ks, kernel, edge_index, mass=False, *, _den=None, _csr=None):
    """qs [N,H,M], ks [L,H,M], edge_index int64 [2,E] (row 0 the source = key id, row 1 the target = query id, as gcn_conv
    reads it) -> float32 [E,H]: the attention weight a[col_e, row_e, h] of the reference's dense map at every edge, in the
    caller's edge order -- `full_attention_conv(..., output_attn=True)[1][col, row, :]` without the [N, L] map.  Duplicate edges
    and self-loops are ordinary edges.  mass=True: -> (that, float32 [N,H]), the sum of a node's weights over its in-edges:
    the share of its attention row that lies on the graph."""
    if kernel not in ("simple", "sigmoid"):
        raise ValueError(f"unknown attention kernel {kernel!r} (expected 'simple' or 'sigmoid')")
    if qs.dim() != 3 or ks.dim() != 3 or qs.shape[1:] != ks.shape[1:]:
        raise ValueError(f"attention_on_edges: qs [N,H,M] and ks [L,H,M] expected (got {tuple(qs.shape)} and {tuple(ks.shape)})")
    _check_edges(edge_index)
    if qs.shape[2] > MAX_WIDTH:
        raise ValueError(f"attention_on_edges: heads of {qs.shape[2]} columns exceed the limit of {MAX_WIDTH}")
    dev = staging.staging_device(None, (qs, ks, edge_index))
    if dev is not None:      # host operands: computed on the GPU, returned on the host
        out = attention_on_edges(qs.to(dev), ks.to(dev), kernel, staging.operands.get(edge_index, dev), mass)
        return tuple(o.to(qs.device) for o in out) if mass else out.to(qs.device)
    with torch.no_grad():
        qs, ks = qs.detach().float(), ks.detach().float()        # bfloat16 is storage only: products and sums in float32
        if kernel == "simple":
            scale = _simple_scale(qs, ks).squeeze(-1)            # an operand of the kernel, not folded into a copy of qs
        else:
            if _den is None:                                     # the row sums of the library's forward; any narrow v does
                _den = ops.get_backend().sigmoid_attention(qs, ks, ks[:, :, :4], want_den=True)[1]
            scale = 1.0 / _den
        values, m = _edges_of(qs, ks, 0 if kernel == "simple" else 1, scale.contiguous(), edge_index,
                              (_csr if _csr is not None else [None]) if mass else None)
        return (values, m) if mass else values
