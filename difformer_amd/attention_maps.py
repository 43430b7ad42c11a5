"""Streaming top-k attention maps: per node and head the k keys it attends to most, without the dense [N, L, H] map.

The reference's interpretability output is the dense attention (`full_attention_conv(..., output_attn=True)`,
`DIFFormer.get_attentions`; node classification/difformer.py:42-43 `simple`, :47-55 `sigmoid`, :211-226).  That tensor is
900 MB per layer and head at 15,000 nodes and does not exist at the sizes this package is built for; what is read off it is
the handful of strongest keys of a row.  `attention_topk` returns exactly those, from one sweep over key tiles that keeps a
running top-k per query row in registers (csrc/attn_topk.hip, C ABI include/difformer_maps.h).  Outputs are detached: there
is no gradient through a selection.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from . import staging

__all__ = ["attention_topk", "MAX_K", "MAX_WIDTH"]

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
