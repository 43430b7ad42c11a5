"""Operators of the DIFFormer propagation layer on MI355X (shard-aware, no arithmetic of their own).

    simple_attention / sigmoid_attention  <- full_attention_conv   (difformer.py:10-61)
    GraphCSR + gcn_aggregate              <- gcn_conv              (difformer.py:63-79)
    layer_tail                            <- difformer.py:137-140, :200-203

Each function drives the HIP kernels through `backend_hip.HipBackend`; with a `RowShard` it
adds the single exchange step the operator needs (dist.py).
"""
from __future__ import annotations

import weakref
from typing import Optional

import math
import os

import torch

from . import sliced
from .dist import RowShard
from .tensor_cache import MISS, TensorCache, param_key, tensor_version      # (both functions are part of this module's surface)

_BACKEND = None


def get_backend():
    """The HIP backend (created on first use; import fails loudly if the .so is missing)."""
    global _BACKEND
    if _BACKEND is None:
        from .backend_hip import HipBackend
        _BACKEND = HipBackend()
    return _BACKEND


# ------------------------------------------------------------------------------------------
# a1 / a2
# ------------------------------------------------------------------------------------------
def simple_attention(qs, ks, vs, shard: Optional[RowShard] = None):
    """qs, ks [n,H,M], vs [n,H,D] (this rank's rows) -> [n,H,D].  difformer.py:18-39."""
    if qs.shape[0] != vs.shape[0] or ks.shape[0] != vs.shape[0]:
        # difformer.py:29 adds a [L,H,D] tensor to a [N,H,D] one: the reference raises too
        raise RuntimeError(f"simple kernel needs as many queries as sources (N={qs.shape[0]}, L={vs.shape[0]}; "
                           "difformer.py:29)")
    be = get_backend()
    reduced = be.simple_reduce(qs, ks, vs)
    n_global = qs.shape[0]
    if shard is not None and shard.world > 1:
        shard.all_reduce_sum(reduced)          # the one exchange step: H*(M*D+M+D)+2 floats
        n_global = shard.n_global
    return be.simple_apply(qs, reduced, n_global, vs.shape[2])


def project_simple_attention(x, Wq, bq, Wk, bk, Wv, bv, H, D, shard: Optional[RowShard] = None,
                             gather_values=False):
    """x [n,C] (local rows) -> (attn [n,H,D], v [n,H,D]).  Projections (difformer.py:115-118) fused with
    stage 1 of the simple kernel; k never reaches HBM.  Needs C <= 64 and D <= 64."""
    be = get_backend()
    q, v, reduced = be.project_reduce(x, Wq, bq, Wk, bk, Wv, bv, H, D)
    n_global = x.shape[0]
    if shard is not None and shard.world > 1:
        n_global = shard.n_global
        if gather_values:
            # start moving the value rows now, and the record all-reduce on the second communicator; the part of the
            # SpMM that needs only this rank's own rows runs under both (gcn_aggregate), then `apply`, then the rest
            v = GatheredRows(v, shard.all_gather_rows_async(v.reshape(v.shape[0], H * D)))
            work = shard.all_reduce_sum_async(reduced)

            def finish():
                if work is not None:
                    work.wait()
                return be.simple_apply(q, reduced, n_global, D)
            return LazyAttention(finish, q.shape[0], H, D), v
        shard.all_reduce_sum(reduced)
    return be.simple_apply(q, reduced, n_global, D), v


class LazyAttention:
    """The `simple` attention of a row-sharded layer whose record all-reduce is still in flight: materialize() waits
    for it and runs the apply kernel.  gcn_aggregate calls it after part 0 of the SpMM, which needs neither."""

    def __init__(self, finish, n, H, D):
        self._finish, self._value = finish, None
        self.shape = (n, H, D)

    def materialize(self):
        if self._value is None:
            self._value = self._finish()
            self._finish = None
        return self._value


class GatheredRows:
    """Local value rows [n,H,D] plus the in-flight all-gather of them (row-sharded runs)."""

    def __init__(self, local, handle):
        self.local, self.handle = local, handle
        self.shape = local.shape


def sigmoid_attention(qs, ks, vs, shard: Optional[RowShard] = None):
    """qs [n,H,M] local queries; ks, vs local sources -> [n,H,D].  difformer.py:45-56."""
    if shard is not None and shard.world > 1:
        ks = shard.all_gather_rows(ks)
        vs = shard.all_gather_rows(vs)
    return get_backend().sigmoid_attention(qs, ks, vs)


# ------------------------------------------------------------------------------------------
# a3
# ------------------------------------------------------------------------------------------
L2_SLICE_BYTES = 2.5 * 2 ** 20   # target size of the x slice one source block covers (L2 is 4 MiB / XCD)


def choose_source_blocks(num_nodes, row_bytes, nnz):
    """Source blocks for the blocked SpMM: 1 (plain CSR) when x fits L2 or rows are too sparse for
    the per-(row, block) groups to amortise; otherwise ~2.5 MiB of x per block, at most 64."""
    total = float(num_nodes) * float(row_bytes)
    if total <= 4 * 2 ** 20 or nnz < 64 * num_nodes:
        return 1
    nb = int(round(total / L2_SLICE_BYTES))
    # the sweep prefetches up to 64 entries of a (row, block) group; longer groups fall off that fast path
    nb = max(nb, -(-int(nnz) // (int(num_nodes) * 48)))
    nb = max(2, min(nb, 64))
    # keep >= ~24 entries per (row, block) group on average
    while nb > 2 and nnz / (num_nodes * nb) < 24:
        nb -= 1
    return nb


def choose_shard_blocks(num_nodes, row_bytes, nnz, shard):
    """(n_blocks, block_rows) whose block boundaries fall on the rank boundaries of `shard`, or None.  The blocked SpMM
    of a row-sharded run can then sweep the blocks holding this rank's OWN value rows while the all-gather of the
    others is still in flight (gcn_aggregate).  Every rank's c rows (a multiple of 8, dist.split_rows) are cut into
    m in {1, 2, 4, 8} blocks of c / m rows, ~2.5 MiB of x each."""
    if shard is None or shard.world <= 1 or choose_source_blocks(num_nodes, row_bytes, nnz) <= 1:
        return None
    c = shard.counts[0]
    if any(shard.offsets[r] != r * c for r in range(shard.world)) or c % 8 != 0:
        return None
    for m in (1, 2, 4, 8):
        rows = c // m
        n_blocks = -(-int(num_nodes) // rows)
        if rows * row_bytes <= 1.15 * L2_SLICE_BYTES and n_blocks <= 64:
            # the sweep prefetches up to 64 entries of a (row, block) group: keep the average group at <= ~48 entries
            if nnz / (float(num_nodes) * n_blocks) <= 48 or m == 8:
                return n_blocks, rows
    return None


def sliced_tiling(num_nodes, F, nnz, edge_weight, shard, elem_size):
    """(n_tiles, tile_rows) the feature-sliced product would use for this graph, or None when it is not a candidate
    (sliced.candidate: edge weights, non-fp32 rows, sparse or small graph).  csr_cache builds the CSR with that blocking.
    A row shard has its own tiling (source splits: a multiple of 2, 4 or 8 tiles, include/difformer_hip.h)."""
    if not sliced.candidate(num_nodes, nnz, F, edge_weight is not None, elem_size):
        return None
    be = get_backend()
    n_rows = shard.n_local if (shard is not None and shard.world > 1) else num_nodes
    plan = be.sliced_plan(num_nodes, n_rows, F) if hasattr(be, "sliced_plan") else None
    return None if plan is None else (plan.NT, plan.T)


class GraphCSR:
    """Normalised adjacency in CSR over destination rows (built once per graph, on device)."""

    def __init__(self, rowptr, blkptr, n_blocks, src, val, num_nodes, nnz, block_rows=0):
        self.rowptr, self.blkptr, self.n_blocks, self.src, self.val = rowptr, blkptr, int(n_blocks), src, val
        self.num_nodes, self.nnz = int(num_nodes), int(nnz)
        self.block_rows = int(block_rows) or -(-int(num_nodes) // int(n_blocks))     # source rows per block
        self._edges = None          # weak references to (edge_index, edge_weight) for the lazily built adjoint
        self._adjoint = None
        self._orders = {}           # (row_begin, n_rows) -> rows by descending degree (blocked SpMM load balance)
        self.weighted = self.transposed = False
        self.dinv = None            # adjoint CSR only: deg^-1/2 of the FORWARD graph (its own row lengths are out-degrees)
        self._sliced = {}           # (row_begin, n_rows, F) -> SlicedAdjacency | None
        self._row_sums = None
        self._row_scale = False      # not computed yet (None = this graph has none: row_scale)
        self._format_checked = False # csr_cache.get(build_format=True) has built (or ruled out) the sliced format for this CSR
        self.weight_scale = 1.0      # a CONSTANT edge_weight (every entry equal: `--special_treat dense` / knn, spatial-temporal/
                                     # main.py:99,103) is not in `val`: the CSR is the unweighted one and every caller multiplies
                                     # its gcn_scale by this (csr_cache.get)
        self._max_degree = None      # longest row: known from the build (status[1] of dif_csr_build) ...
        self._max_source = None      # ... or (graph_utils._LongestRows, batch) for the batches of one subgraph_batches call

    def row_order(self, row_begin, n_rows):
        """(order, n_split) for the blocked SpMM over a shard: its rows by descending degree, the first n_split of them
        (degree > 4x mean) to be split over a whole quad.  Built once per shard on the device (one host sync for the two
        statistics).  None when the order would not help: unblocked kernels (they map rows to waves / lane groups one by
        one), or degrees about equal (max <= 2x mean: contiguous panels are faster then)."""
        if self.n_blocks <= 1 or self.nnz == 0:
            return None
        key = (int(row_begin), int(n_rows))
        if key not in self._orders:
            order, stats = get_backend().row_order(self.rowptr, *key)
            n_split, max_deg = (int(v) for v in stats.tolist())
            total = int(self.rowptr[key[0] + key[1]]) - int(self.rowptr[key[0]])
            skewed = max_deg * key[1] > 2 * total
            self._orders[key] = (order, n_split) if skewed else None
        return self._orders[key]

    @classmethod
    def build(cls, edge_index, edge_weight, num_nodes, n_blocks=1, transpose=False, block_rows=0):
        rowptr, blkptr, src, val, longest = get_backend().csr_build(edge_index, edge_weight, int(num_nodes), int(n_blocks),
                                                                    transpose, int(block_rows))
        csr = cls(rowptr, blkptr, n_blocks, src, val, num_nodes, edge_index.shape[1], block_rows)
        csr._max_degree = int(longest)
        csr.weighted, csr.transposed = edge_weight is not None, bool(transpose)
        if not transpose:
            csr._edges = (weakref.ref(edge_index), None if edge_weight is None else weakref.ref(edge_weight))
        return csr

    def sliced(self, row_begin, n_rows, F):
        """sliced.build of rows [row_begin, row_begin + n_rows) for F fp32 feature columns (a SlicedAdjacency, or None when
        this graph keeps the gather kernels), built on first use and kept with the CSR."""
        key = (int(row_begin), int(n_rows), int(F))
        if key not in self._sliced:
            self._sliced[key] = self._build_sliced(*key)
        return self._sliced[key]

    def _build_sliced(self, row_begin, n_rows, F):     # (uncached)
        return sliced.build(get_backend(), self, row_begin, n_rows, F)

    def row_sums(self):
        """A_hat 1 (float32 [N]): what the bias of the value projection turns into under the aggregation,
        A_hat (x Wv^T + 1 bv^T) = (A_hat x) Wv^T + (A_hat 1) bv^T.  One small product per graph, cached."""
        if self._row_sums is None:
            ones = torch.ones((self.num_nodes, 4), dtype=torch.float32, device=self.rowptr.device)
            self._row_sums = _aggregate_rows(get_backend(), self, None, ones, 0, self.num_nodes)[:, 0].contiguous()
        return self._row_sums

    def row_scale(self):
        """rscale = deg^1/2 (float32 [N]), the inverse of the deg^-1/2 the slice-major copy of the sliced product is scaled
        by: with it a closed-form layer recovers its input rows from that copy, x[r] = ys[r] * rscale[r], and the rows need
        no row-major copy (single-copy mode of simple_layer_closed_form).  None when a row cannot be recovered -- some node
        has no incoming entry (deg = 0: its ys row is zero whatever x was) -- or the product does not factor this way
        (edge weights, an adjoint CSR).  One pass over rowptr and one host read per graph, kept with the CSR."""
        if self._row_scale is False:
            self._row_scale = None
            if not self.weighted and not self.transposed and self.num_nodes > 0 and self.nnz > 0:
                deg = self.rowptr[1:] - self.rowptr[:-1]
                if int(deg.min()) > 0:                     # cold path: once per graph
                    self._row_scale = deg.to(torch.float32).sqrt().contiguous()
        return self._row_scale

    def max_degree(self):
        """Longest row (entries).  `build` gets it from the CSR kernels with the host read a build has anyway
        (dif_csr_build status[1]) and graph_utils.subgraph_batches sets it for the batches it registers, so the kernel
        choice that depends on it (the closed-form layer kernel aggregates inside only when no row is long: its 16 rows of a
        tile walk in lock step) is a function of the graph alone -- identical calls launch identical kernels.  A CSR put
        together by hand pays one reduction and one host read here, once."""
        if self._max_degree is None and self._max_source is not None:
            rows, b = self._max_source
            self._max_degree, self._max_source = int(rows.resolve()[b]), None
        if self._max_degree is None:
            self._max_degree = int((self.rowptr[1:] - self.rowptr[:-1]).max().item()) if self.num_nodes > 0 else 0
        return self._max_degree

    def weight_leaf(self):
        """The edge_weight tensor this CSR was built from when the caller wants its gradient (difformer.py:73 is
        differentiable in it), else None."""
        if not self.weighted or not self._edges or self._edges[1] is None or not torch.is_grad_enabled():
            return None
        w = self._edges[1]()
        return w if (w is not None and w.requires_grad) else None

    def hold_edges(self):
        """Strong references to the tensors this CSR was built from (None if already freed).  The autograd node of the
        aggregation keeps them until backward(), so callers may pass temporaries (`model(x, ei.to(dev))`)."""
        if not self._edges:
            return None
        return (self._edges[0](), self._edges[1]() if self._edges[1] is not None else None)

    def adjoint(self):
        """CSR of A_hat^T (entries filed under their source row): the SpMM over it is the gradient of the
        aggregation.  Built on first use (training only) from the same edge tensors."""
        if self._adjoint is None:
            ei = self._edges[0]() if self._edges else None
            ew = self._edges[1]() if self._edges and self._edges[1] is not None else None
            if ei is None or (self._edges[1] is not None and ew is None):
                raise RuntimeError("difformer_amd: the edge_index this CSR was built from has been freed; keep it alive "
                                   "until backward()")
            self._adjoint = GraphCSR.build(ei, ew, self.num_nodes, self.n_blocks, transpose=True,
                                           block_rows=self.block_rows)
            if not self.weighted:
                # value_e = dinv[col] * dinv[row] with dinv from the in-degree (difformer.py:66-68): the adjoint product
                # factors the same way, grad_x[s] = dinv[s] * sum_{e: src = s} (dinv * g)[dst_e] -> the sliced kernel
                deg = (self.rowptr[1:] - self.rowptr[:-1]).to(torch.float32)
                self._adjoint.dinv = torch.where(deg > 0, (1.0 / deg).sqrt(), torch.zeros_like(deg))
        return self._adjoint


class _CSRCache(TensorCache):
    """The reference rebuilds degree / values / SparseTensor in every layer of every forward
    (difformer.py:66-75).  We key the built CSR on the identity *and* version of the tensors the
    caller passes (TensorCache: edge_index and the edge_weight GIVEN, with num_nodes and the blocking), so
    `forward(x, edge_index)` keeps its signature and in-place edits or new tensors still trigger a rebuild."""

    def __init__(self, capacity=8):
        super().__init__(capacity, unversioned=True)
        self._uniform = TensorCache(64)           # edge_weight tensor -> the constant all its entries equal, or None

    def get(self, edge_index, edge_weight, num_nodes, row_bytes=256, shard=None, elem_size=4, build_format=True):
        """`row_bytes` = bytes of one feature row the SpMM will gather (H*D*elem_size); picks the blocking -- the
        tiling of the feature-sliced product for dense unweighted fp32 graphs, else ~2.5 MiB source blocks, aligned
        with the rank boundaries of `shard` when the run is row-sharded."""
        if edge_weight is not None and edge_weight.requires_grad and torch.is_grad_enabled() and shard is not None \
                and shard.world > 1:
            # the reference's gcn_conv is differentiable in edge_weight (value = w * d_in * d_out through
            # torch_sparse.matmul).  One GPU: autograd_ops._GcnAggregate returns that gradient (csrc/gcn_edge_grad.hip);
            # row-sharded it would need the gathered rows of both operands on every rank
            raise NotImplementedError("difformer_amd: gradients with respect to edge_weight are not implemented for "
                                      "row-sharded runs; detach() it or keep it a constant of the graph")
        # entries of freed edge tensors go NOW: a mini-batch loop (main-batch.py:126-131) makes a new edge_index per batch,
        # and a dead entry would otherwise pin its CSR (and sliced format) in HBM until the next build
        self.purge()
        # every weight equal (one reduction, read with the host read a build has anyway): value_e = w d_in d_out
        # (difformer.py:73) = w x the unweighted value, so the graph takes every UNWEIGHTED kernel (feature-sliced product,
        # in-layer aggregation) and w rides in the callers' gcn_scale.  Keyed like a weighted graph, built like an unweighted one.
        given_weight, scale = edge_weight, 1.0
        if edge_weight is not None:
            u = self._uniform_weight(edge_weight, edge_index.shape[1], num_nodes)
            if u is not None:
                edge_weight, scale = None, u
        n_blocks, block_rows = self.blocking(edge_index, edge_weight, num_nodes, row_bytes, shard, elem_size)
        tensors, extras = (edge_index, given_weight), (int(num_nodes), int(n_blocks), int(block_rows))
        csr = self.lookup(tensors, extras)
        if csr is not MISS and edge_weight is not None and not csr.weighted:
            # built through the uniform-weight shortcut (an eval pass before the first step of learnable weights
            # initialised to a constant): this call wants the weighted CSR, whose values autograd differentiates
            csr = MISS
        if csr is MISS:
            csr = GraphCSR.build(edge_index, edge_weight, num_nodes, n_blocks, block_rows=block_rows)
            csr.weight_scale = scale
        elif csr._format_checked or not build_format:
            return csr
        F = row_bytes // elem_size
        if build_format:
            # (also the first `build_format` request for a CSR that a pointers-only probe left here: _MixCache.get)
            csr._format_checked = True
        if build_format and sliced_tiling(num_nodes, F, edge_index.shape[1], edge_weight, shard, elem_size) is not None:
            # the blocking above is the tiling of the sliced product: build its format now, and if the graph turns out not
            # to fit it (a (row, tile) group beyond the 16-bit counters, a split plan with another tiling), fall back to a
            # CSR blocked for the gather kernels instead of running them on a blocking that was never tuned for them
            sharded = shard is not None and shard.world > 1
            rb, nr = (shard.row_begin, shard.n_local) if sharded else (0, num_nodes)
            if csr.sliced(rb, nr, F) is None:
                aligned = choose_shard_blocks(num_nodes, row_bytes, edge_index.shape[1], shard)
                nb2, br2 = aligned if aligned else (choose_source_blocks(num_nodes, row_bytes, edge_index.shape[1]), 0)
                if (nb2, br2 or -(-int(num_nodes) // nb2)) != (csr.n_blocks, csr.block_rows):
                    global _SLICED_FALLBACK_WARNED
                    if not _SLICED_FALLBACK_WARNED:
                        _SLICED_FALLBACK_WARNED = True
                        import warnings
                        warnings.warn("difformer_amd: this graph does not fit the feature-sliced product (see "
                                      "sliced.build); using the gather kernels on their own blocking")
                    csr = GraphCSR.build(edge_index, edge_weight, num_nodes, nb2, block_rows=br2)
                    csr._format_checked = True
                    csr.weight_scale = scale
        return self.insert(tensors, extras, csr)

    UNIFORM_ALWAYS = False       # tests: run the check on graphs of any size
    UNIFORM_MIN_EDGES = 4096     # below this the CSR build is a handful of launches and the check would double its host cost
    # ... and it only buys something where the unweighted graph takes kernels the weighted one cannot: the feature-sliced
    # product (sliced.candidate: SLICED_MIN_ROWS nodes, SLICED_MIN_DEGREE entries per row).  A 1,068-node snapshot with fresh tensors per forward
    # (spatial-temporal/main.py:96-105) would pay two reductions and a host read per snapshot for the same gather kernels.

    def _uniform_weight(self, edge_weight, n_edges, num_nodes=None):
        """The constant all entries of `edge_weight` are equal to (0.0 when that constant is not finite: nan_to_num,
        difformer.py:74), or None: weights that vary, that want a gradient, or a graph too small for the check to pay.
        Remembered per weight tensor (identity + version)."""
        if n_edges < self.UNIFORM_MIN_EDGES or edge_weight.numel() != n_edges or not edge_weight.is_floating_point():
            return None
        if num_nodes is not None and not sliced.candidate(num_nodes, n_edges) and not self.UNIFORM_ALWAYS:
            return None
        if edge_weight.requires_grad and torch.is_grad_enabled():
            return None
        u = self._uniform.lookup((edge_weight,), (n_edges,))
        if u is not MISS:
            return u
        w = edge_weight.detach()
        lo, hi = torch.stack([w.min(), w.max()]).tolist()            # NaN anywhere -> both NaN -> lo == hi is False
        if lo == hi:
            u = float(lo) if math.isfinite(lo) else 0.0
        elif math.isnan(lo) and bool(torch.isnan(w).all()):
            u = 0.0
        else:
            u = None
        return self._uniform.insert((edge_weight,), (n_edges,), u)

    @staticmethod
    def blocking(edge_index, edge_weight, num_nodes, row_bytes=256, shard=None, elem_size=4):
        """(n_blocks, block_rows) of the CSR `get` builds for this graph: the tiling of the feature-sliced product for
        dense unweighted fp32 graphs, else ~2.5 MiB source blocks (aligned with the rank boundaries of a row shard)."""
        tiling = sliced_tiling(num_nodes, row_bytes // elem_size, edge_index.shape[1], edge_weight, shard, elem_size)
        if tiling is not None:
            return tiling if tiling[0] > 1 else (1, 0)
        aligned = choose_shard_blocks(num_nodes, row_bytes, edge_index.shape[1], shard)
        return aligned if aligned else (choose_source_blocks(num_nodes, row_bytes, edge_index.shape[1]), 0)

    def put(self, edge_index, edge_weight, num_nodes, csr):
        """Register a CSR built elsewhere (graph_utils.subgraph_batches: all batches of an epoch from one sort) under the
        key `get` would use for these tensors, so that `model(x_i, edge_index_i)` finds it without building anything."""
        self.insert((edge_index, edge_weight), (int(num_nodes), int(csr.n_blocks), 0), csr)

    # From TensorCache: drop(edge_index) forgets every CSR built from that tensor (its HBM is freed once no autograd node
    # holds it), reserve(n) keeps an epoch's worth of registered batches from evicting one another, values() are the CSRs
    # held (what a hipGraph capture keeps alive).


_SLICED_FALLBACK_WARNED = False
csr_cache = _CSRCache()


# ------------------------------------------------------------------------------------------
# graphs with community structure: the model runs in a MIXED node order
# ------------------------------------------------------------------------------------------
MIX_THRESHOLD = 2.5     # mean over rows of (largest per-tile share of the row's entries) x tiles: 1.3 on a uniform graph,
                        # ~8 when every row's entries sit in one or two source tiles


class MixedGraph:
    """A graph relabelled by a fixed random permutation of its nodes.  The sliced product sweeps the SOURCE rows tile by
    tile with all rows of a slot in lock step; when a row's entries sit in one or two tiles (the real ogbn-proteins: 8
    species that interact almost only among themselves, node ids grouped by species) most rounds of a wave are empty in
    any given tile and the rest are padded to them: 3.4-4.6 slots per entry instead of 1.56, 2-3x the time
    (profiles/r02_experiments.md).  Every per-node operation of the model is equivariant under a relabelling, so the model
    permutes x once on the way in and the logits once on the way out and runs everything else on `edge_index` = the
    relabelled graph: perm[i] = original node at position i, inv[perm] = arange."""

    def __init__(self, edge_index, num_nodes):
        dev = edge_index.device
        g = torch.Generator(device=dev).manual_seed(0x5EED)
        self.perm = torch.randperm(num_nodes, generator=g, device=dev)
        self.inv = torch.empty_like(self.perm)
        self.inv[self.perm] = torch.arange(num_nodes, device=dev)
        self.edge_index = self.inv[edge_index]              # same edges, same order, nodes renamed


class _MixCache(TensorCache):
    """MixedGraph (or None: the decision not to mix) per edge_index tensor, num_nodes and width."""

    def get(self, edge_index, num_nodes, F):
        mix = self.lookup((edge_index,), (int(num_nodes), int(F)))
        if mix is not MISS:
            return mix
        mix = None
        if sliced_tiling(num_nodes, F, edge_index.shape[1], None, None, 4) is not None:
            csr = csr_cache.get(edge_index, None, num_nodes, F * 4, build_format=False)     # probe: pointers only
            if csr.n_blocks > 1 and csr.blkptr is not None:
                cnt = csr.blkptr.view(csr.n_blocks + 1, num_nodes)
                cnt = (cnt[1:] - cnt[:-1]).to(torch.float32)                    # entries per (tile, row)
                share = float((cnt.max(dim=0).values.sum() * csr.n_blocks / max(csr.nnz, 1)).item())     # one sync, cold path
                if share > MIX_THRESHOLD:
                    mix = MixedGraph(edge_index, num_nodes)
                    csr_cache.drop(edge_index)      # the forward runs on the relabelled graph: the probe CSR is dead weight
        return self.insert((edge_index,), (int(num_nodes), int(F)), mix)


mix_cache = _MixCache(8, unversioned=True)


def _aggregate_rows(be, csr, sl, x_src, row_begin, n_rows, attn=None, attn_scale=1.0, gcn_scale=1.0, tail=None, ys=None):
    """gcn_scale * A_hat[row_begin : row_begin + n_rows] x_src (+ attn_scale * attn) (-> tail): the one call sequence of
    the aggregation, x_src [num_nodes, F] -> [n_rows, F].
    sl = csr.sliced(row_begin, n_rows, F) of a dense unweighted graph: the sources pre-scaled (`ys`: that copy, when a layer
    kernel has written it already) and staged slice by slice in LDS (csrc/gcn_sliced.hip); the LayerNorm of the tail needs
    whole rows, which the slice workgroups do not have: it runs as its own pass.
    sl = None: the gather kernels, the tail in their epilogue."""
    if sl is None:
        return be.spmm(csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, csr.num_nodes, csr.nnz, x_src, row_begin, n_rows,
                       attn, attn_scale, gcn_scale, tail, csr.row_order(row_begin, n_rows))
    F = x_src.shape[1]
    if ys is None:
        ys = be.sliced_prescale(x_src, csr.rowptr, csr.num_nodes, sl.plan, csr.dinv)
    out = be.sliced_spmm(sl, ys, csr.rowptr, csr.num_nodes, row_begin, n_rows, F, attn, attn_scale, gcn_scale, csr.dinv)
    if tail is not None:                       # (one head: F = D)
        out = be.layer_tail(out.reshape(n_rows, 1, F), tail.get("x0"), tail.get("prev"), tail.get("alpha", 0.5),
                            tail.get("ln_weight"), tail.get("ln_bias"), tail.get("eps", 1e-5), tail.get("relu", False))
    return out


def gcn_aggregate(csr: GraphCSR, x, attn=None, attn_scale=1.0, gcn_scale=1.0, shard: Optional[RowShard] = None,
                  tail=None):
    """x [n,H,D] (this rank's rows of the value tensor) -> gcn_scale * A_hat x (+ attn_scale * attn).

    difformer.py:75-78 plus the combine of :130-134.  Sharded: all-gather x, SpMM over the local
    destination rows.  `tail` (H == 1 only) = dict(x0, prev, alpha, ln_weight, ln_bias, eps) fuses the
    layer tail of :139-140 / :200-203 into the SpMM epilogue; the result is then [n, 1, D]."""
    n, H, D = x.shape
    be = get_backend()
    flat = lambda a: None if a is None else (a.materialize() if isinstance(a, LazyAttention) else a).reshape(n, H * D)
    if shard is None or shard.world <= 1:
        sl = sliced.rows_format(csr, x.dtype, n, H * D)
        out = _aggregate_rows(be, csr, sl, x.reshape(n, H * D), 0, n, flat(attn), attn_scale, gcn_scale, tail)
        return out.reshape(n, -1, D)           # [n, H, D]; [n, 1, D] after a tail
    # row-sharded: the one exchange step of this operator is the all-gather of the value rows (N*H*D elements)
    if isinstance(x, GatheredRows):            # already started by project_simple_attention
        local, handle = x.local.reshape(n, H * D), x.handle
    else:
        local = x.reshape(n, H * D)
        handle = shard.all_gather_rows_async(local)
    row_begin, n_rows = shard.row_begin, shard.n_local
    F = H * D
    # dense unweighted graph: the shard's feature-sliced product (source tiles split over the workgroups of a panel) over
    # the gathered rows, as in the single-GPU branch above
    sl = sliced.rows_format(csr, local.dtype, n_rows, F, shard)
    order = csr.row_order(row_begin, n_rows) if sl is None else None      # (built here, under the collective, on first use)
    rows = csr.block_rows
    split = (sl is None and csr.n_blocks > 1 and csr.nnz > 0 and F % 4 == 0 and F <= 256 and row_begin % rows == 0 and
             (row_begin + n_rows == csr.num_nodes or (row_begin + n_rows) % rows == 0))
    if split:
        # blocks [own_lo, own_hi) hold exactly this rank's own value rows: sweep them now, under the collective, and
        # park the accumulators; the rest of the sweep and the epilogue follow once the other ranks' rows have landed
        own_lo, own_hi = row_begin // rows, -(-(row_begin + n_rows) // rows)
        local = local if local.is_contiguous() else local.contiguous()
        args = (csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, csr.num_nodes, csr.nnz)
        scratch = be.spmm(*args, local, row_begin, n_rows, None, attn_scale, gcn_scale, None, order,
                          (0, own_lo, own_hi, None, row_begin))
        a2 = flat(attn)                        # waits for the record all-reduce, runs `apply` -- after part 0 is queued
        x2 = handle.wait()
        out = be.spmm(*args, x2, row_begin, n_rows, a2, attn_scale, gcn_scale, tail, order,
                      (1, own_lo, own_hi, scratch, 0))
    else:
        a2 = flat(attn)                        # waits for the record all-reduce, runs `apply` under the all-gather
        out = _aggregate_rows(be, csr, sl, handle.wait(), row_begin, n_rows, a2, attn_scale, gcn_scale, tail)
    return out.reshape(n_rows, -1, D)          # [n_rows, H, D]; [n_rows, 1, D] after a tail


class NarrowFactors:
    """Weight-only factors of the background coefficient chain (csrc/side_chain.hip), float32 [80 x 80] zero padded,
    augmented index 64: pt = W~q^T W~k, vtt = [W~v^T | e]^T, st = [W~q^T W~q ; W~k^T W~k] with W~ = [W | b].  Computed in
    float64 once per parameter version (the module caches the object)."""

    def __init__(self, Wq, bq, Wk, bk, Wv, bv):
        f64, B, A = torch.float64, 80, 64
        D, C = Wq.shape
        dev = Wq.device

        def aug(W, b):
            M = torch.zeros((W.shape[0], B), dtype=f64, device=dev)
            M[:, : W.shape[1]] = W.to(f64)
            M[:, A] = b.to(f64)
            return M
        Wq_, Wk_ = aug(Wq, bq), aug(Wk, bk)
        if Wv is not None:
            Wv_ = aug(Wv, bv)
        else:                                                           # use_weight = False: v = x (difformer.py:120)
            Wv_ = torch.zeros((C, B), dtype=f64, device=dev)
            Wv_[torch.arange(C), torch.arange(C)] = 1.0
        self.pt = (Wq_.t() @ Wk_).to(torch.float32).contiguous().reshape(-1)
        self.st = torch.stack([(Wq_.t() @ Wq_).reshape(-1), (Wk_.t() @ Wk_).reshape(-1)]).to(torch.float32).contiguous().reshape(-1)
        vtt = torch.zeros((B, B), dtype=f64, device=dev)
        vtt[: Wv_.shape[0]] = Wv_
        vtt[A, A] = 1.0
        self.vtt = vtt.to(torch.float32).contiguous().reshape(-1)


_SIDE_STREAMS = {}


def side_stream(dev):
    """The second stream the background coefficient chain runs on (one per device)."""
    key = (dev.type, dev.index)
    if key not in _SIDE_STREAMS:
        _SIDE_STREAMS[key] = torch.cuda.Stream(dev)
    return _SIDE_STREAMS[key]


SIDE_CHAIN = os.environ.get("DIFFORMER_SIDE_CHAIN", "1") != "0"
# DIFFORMER_SINGLE_COPY=0: every closed-form layer keeps its rows row-major AND slice-major (the two-copy path), as before the
# single-copy mode existed -- same kernels, same bits.
SINGLE_COPY = os.environ.get("DIFFORMER_SINGLE_COPY", "1") != "0"
# DIFFORMER_EXACT_FP32=1: no product of the forward runs on split-bfloat16 operands -- the long-row input Linear takes the
# fp32 MFMA (the library reads the same variable), and the output Linear is not folded into the last layer kernel (whose
# extra product is a split-bfloat16 one) but runs as its own fp32-MFMA launch.  Results move by ~4e-6 of the logits' scale.
EXACT_FP32 = os.environ.get("DIFFORMER_EXACT_FP32", "0") == "1"

_F32_PARAMS = TensorCache(256)


def f32_param(t):
    """Exact float32 copy of a bfloat16 parameter, cached until the parameter changes (TensorCache); float32 tensors
    pass through.  The closed-form kernels take their coefficients in float32."""
    if t is None or t.dtype == torch.float32:
        return t
    c = _F32_PARAMS.lookup((t,))
    if c is MISS:
        c = _F32_PARAMS.insert((t,), (), t.detach().to(torch.float32).contiguous())
    return c


def invalidate_param_caches():
    """Forget the cached float32 copies of bfloat16 parameters and the packed weights of the long-row Linear (see
    param_key for when this is needed)."""
    _F32_PARAMS.clear()
    packed = getattr(_BACKEND, "_packed", None)      # (HipBackend's; a host-side test backend packs nothing and has none)
    if packed is not None:
        packed.clear()


def slice_sharded(shard, C, dtype=torch.float32):
    """True when a closed-form layer of width C on this shard splits its aggregation by feature slices (dist.py)."""
    return (shard is not None and shard.world > 1 and getattr(shard, "product", "row") == "slice" and
            dtype == torch.float32 and shard.slice_width(C) > 0)


class LayerChain:
    """What the model loop and the closed-form layers of ONE forward hand each other (the `carry` argument; single GPU).
        want_next  in.   Set by the model loop (DIFFormer._forward_eager) before every layer: another layer follows over
                         the same graph, so the layer kernel may also write the slice-major pre-scaled copy of its output
                         (the next layer's SpMM operand) from its registers.  Read by simple_layer_closed_form.
        head       in.   Set by the model loop before every layer: (weight, bias) of the model's output Linear when this is
                         the last layer and it may apply the Linear in its own pass, else None.  Read by
                         DIFFormerConv._closed_narrow, which hands the pair on as `head=` if the kernel takes it.
        products   layer -> layer.  dict(x, sl, record, ys): what is already known about the rows `x` -- their Gram record
                         and / or their slice-major copy `ys` for the sliced format `sl`.  Left by
                         DIFFormer._input_with_products and by a layer kernel asked through `want_next`; consumed by the
                         next simple_layer_closed_form, which clears it whether it could use it or not.
                         Single copy: the dict also has rscale (GraphCSR.row_scale) and `x` is only a stand-in
                         (rows_stand_in): the rows exist as ys alone and the next layer reads them from there.
        single_copy in.  Set once by the model loop (DIFFormer._single_copy): every reader of the layers' rows in this forward
                         is a closed-form layer kernel over the same dense graph, so a layer asked through `want_next` may
                         leave its rows as the slice-major copy alone.  simple_layer_closed_form chooses the mode per layer.
        single     out.  How many layer kernels of this forward read their input from the slice-major copy.
        head_done  out.  Set by DIFFormerConv._closed_narrow once `head` was applied: the layer's output is the model's
                         logits already.  Read by the model loop after the last layer."""

    def __init__(self, want_next=False, head=None, products=None):
        self.want_next, self.head, self.products, self.head_done = want_next, head, products, False
        self.single_copy, self.single = False, 0


def rows_stand_in(ys, n, C):
    """What a single-copy layer returns in place of its rows: a float32 [n, C] view of ONE element (strides 0) on the rows'
    device.  It carries what the routing looks at (shape, dtype, device, identity) and no data: the rows are in `ys`, and only
    the simple_layer_closed_form that finds them in LayerChain.products may consume them -- any other call is refused there."""
    return ys.new_empty(1).expand(n, C)


def _simple_layer_kernel(be, x, coef, D, ax, Wv, bv, rs, gcn_scale, x0, residual, alpha, ln_weight, ln_bias, eps, relu,
                         next_operand=None, head=None, gather=None, rscale=None, rows=True):
    """The layer kernel of the closed form: the one be.simple_layer call.  Optional: next_operand = (rowptr, plan) -> the
    kernel also returns the slice-major copy of its output; head = (weight, bias) of the model's output Linear -> logits;
    gather = (rowptr, src, val) -> the kernel aggregates by itself.  Only the ones that are set are passed, so a stand-in
    backend with a narrower signature keeps working."""
    optional = {}
    if next_operand is not None:
        optional["next_rowptr"], optional["next_plan"] = next_operand
    if head is not None:
        optional["head"] = head
    if gather is not None:
        optional["gather"] = gather
    if rscale is not None:                         # single copy: x is the slice-major copy of the rows
        optional["rscale"] = rscale
    if not rows:
        optional["rows"] = False
    return be.simple_layer(x, coef, D, ax, Wv, bv, rs, gcn_scale, x0, residual, alpha, ln_weight, ln_bias, eps, relu, **optional)


def _closed_form_slice_sharded(be, x, Wq, bq, Wk, bk, Wv, bv, csr, attn_scale, gcn_scale, x0, residual, alpha, ln_weight,
                               ln_bias, eps, relu, shard, head):
    """The closed-form layer on a row shard with the aggregation split by FEATURE SLICES: this rank multiplies all
    n_global destination rows of its C / world columns (the sliced product of the whole graph at that width -- or the
    gather kernel where the graph does not take it), between two all-to-alls; Gram record, coefficients and the layer
    kernel stay on the rank's own rows exactly as in the row-sharded layer.  `csr` is the FULL graph's (built without a
    shard: csr_cache.get(..., shard=None) at the slice width)."""
    n, C = x.shape
    D = Wq.shape[0]
    N, w = shard.n_global, shard.slice_width(C)
    xs = shard.all_to_all_columns(x)                                        # [N, w]: my columns of every row
    record, _ = be.gram(x, None, None)                                      # local rows; runs while the exchange lands
    shard.all_reduce_sum(record)
    coef = be.simple_coeffs(record, N, C, D, Wq, bq, Wk, bk, Wv, bv, attn_scale)
    axs = _aggregate_rows(be, csr, csr.sliced(0, N, w), xs, 0, N, gcn_scale=gcn_scale)
    ax = shard.all_to_all_rows(axs)                                         # [n, C]: every column block of my rows
    rs = None
    if Wv is not None:
        rs = csr.row_sums()[shard.row_begin: shard.row_begin + n]
    return _simple_layer_kernel(be, x, coef, D, ax, Wv, bv, rs, gcn_scale, x0, residual, alpha, ln_weight, ln_bias, eps, relu,
                                head=head)


def _record_and_coeffs(be, x, proj, csr, sl, have, shard, factors, attn_scale):
    """Stage a of simple_layer_closed_form: where the Gram record and the coefficients come from.
    have = the carried products of x (LayerChain.products) or None; proj = (Wq, bq, Wk, bk, Wv, bv) in float32.
    -> (record, ys, coef, side): ys = the slice-major copy of x for `sl` if one exists now, else None; side = None, or
    (enqueue, join) when the coefficients come from the background chain -- then coef is None until `enqueue()` (to be
    called right after the product is enqueued) has returned them and `join(coef)` has made the main stream wait."""
    n, C = x.shape
    D = proj[0].shape[0]
    sharded = shard is not None and shard.world > 1
    n_global = shard.n_global if sharded else n
    record = have["record"] if have is not None else None
    ys = have["ys"] if have is not None else None
    rscale = have.get("rscale") if have is not None else None      # single copy: x is a stand-in, the rows are ys * rscale
    # With the sliced product ahead (0.3 ms that does not need the coefficients) the chain Gram -> coefficients runs as
    # single-wave background kernels on a second stream, UNDER the product (csrc/side_chain.hip).
    if (SIDE_CHAIN and factors is not None and sl is not None and not sharded and x.dtype == torch.float32 and
            C % 4 == 0 and D % 4 == 0 and x.is_cuda and hasattr(be, "coeffs_bg")):
        if record is None and ys is None:          # first layer: the Gram pass also writes the slice-major copy the product reads
            record, ys = be.gram(x, csr.rowptr, sl.plan)
        main, side = torch.cuda.current_stream(x.device), side_stream(x.device)
        side.wait_stream(main)                     # the chain may start once x (and the record) exist ...

        def enqueue():
            # ... but is ENQUEUED after the product: its workgroups then take the wave slot the product leaves free on
            # every CU instead of delaying the product's start
            with torch.cuda.stream(side):
                if record is None and rscale is not None:
                    return be.coeffs_bg(ys, None, n_global, factors, C, D, attn_scale, rscale=rscale)
                return be.coeffs_bg(None if record is not None else x, record, n_global, factors, C, D, attn_scale)

        def join(coef):                            # the layer kernel needs the coefficients: the side stream joins
            main.wait_stream(side)
            coef.record_stream(main)
        return record, ys, None, (enqueue, join)
    if rscale is not None:
        raise RuntimeError("difformer_amd: rows kept as their slice-major copy alone need the background coefficient chain "
                           "(DIFFORMER_SIDE_CHAIN=0 and DIFFORMER_SINGLE_COPY=1 do not go together)")
    need_ys = sl is not None and ys is None and not sharded
    if (record is None and not need_ys and not sharded and x.dtype == torch.float32 and C % 4 == 0 and
            n <= GRAM_COEFFS_MAX_ROWS and hasattr(be, "gram_coeffs")):
        # small graphs (node classification/run.sh: Cora ... PubMed): the few partial records of the Gram pass are summed
        # inside the coefficient kernel -- one launch (and one host call) less in a chain of four dependent ones
        record, coef = be.gram_coeffs(x, n_global, C, D, *proj, attn_scale)
        return record, ys, coef, None
    if record is None:
        record, ys2 = be.gram(x, csr.rowptr if need_ys else None, sl.plan if need_ys else None)
        ys = ys2 if need_ys else ys
    if sharded:
        shard.all_reduce_sum(record)
    return record, ys, be.simple_coeffs(record, n_global, C, D, *proj, attn_scale), None


def _graph_term(be, x, csr, sl, ys, handle, shard, gcn_scale, want_row_sums, may_gather, after_product):
    """Stage b of simple_layer_closed_form: how the graph term is produced -> (ax, row sums, gather, late).  Inside the
    layer kernel (gather = (rowptr, src, val), ax None), by the aggregation kernels (ax = gcn_scale * A_hat x, row sums when
    there is a Wv whose bias they carry), or not at all (csr None).  handle = the all-gather of x started by the caller
    (row-sharded) or None; late = what after_product() (stage a's `enqueue`, or None) returned, called as soon as the
    product is enqueued."""
    n = x.shape[0]
    sharded = shard is not None and shard.world > 1
    row_begin = shard.row_begin if sharded else 0
    if csr is None:
        return None, None, None, None
    if (sl is None and not sharded and may_gather and LAYER_GATHER and csr.n_blocks == 1 and n == csr.num_nodes and
            0 < csr.nnz <= LAYER_GATHER_MAX_DEGREE * n and hasattr(be, "_simple_layer_gather") and
            csr.max_degree() <= LAYER_GATHER_MAX_ROW):
        # a few entries per row: the layer kernel walks the CSR itself, no separate SpMM launch and no `ax` round trip
        return None, None, (csr.rowptr, csr.src, csr.val), None
    x_src = handle.wait() if sharded else x
    ax = _aggregate_rows(be, csr, sl, x_src, row_begin, n, gcn_scale=gcn_scale, ys=ys)
    late = after_product() if after_product is not None else None
    rs = None
    if want_row_sums:
        rs = csr.row_sums()
        if sharded:
            rs = rs[row_begin: row_begin + n]
    return ax, rs, None, late


def simple_layer_closed_form(x, Wq, bq, Wk, bk, Wv, bv, csr, attn_scale, gcn_scale, x0, residual, alpha, ln_weight,
                             ln_bias, eps, relu=False, carry=None, shard: Optional[RowShard] = None, factors=None, head=None,
                             keep=None):
    """One DIFFormer layer with the `simple` kernel, query == source == x [n, C] (this rank's rows), one head
    (csrc/simple_layer.hip): Gram record -> coefficients -> SpMM on x -> the layer kernel.  q, k, v and the attention
    output never reach memory.  csr = None: use_graph = False.  Wv = None: use_weight = False.
    Row-sharded: the two exchange steps of SURVEY 8e keep their place -- ONE all-reduce of the 4,160-float Gram record
    (instead of the KtV record) and ONE all-gather of the source rows (x instead of v), started first so that the
    Gram pass and the coefficients run under it.
    `carry` (LayerChain, optional; single GPU) chains layers over the same graph: with carry.want_next the layer kernel also
    writes the slice-major pre-scaled copy of its output (the next layer's SpMM operand) from its registers; the next layer
    picks it up.
    `keep` (dict, optional; the training forward, autograd_ops._ClosedFormLayer): receives the record, the coefficients, the
    aggregated rows and the row sums the backward pass starts from (the aggregation then stays a launch of its own)."""
    be = get_backend()
    n, C = x.shape
    D = Wq.shape[0]
    # bfloat16 activations (BASELINE config C5): the parameters go in as exact float32 copies, all arithmetic is float32
    Wq, bq, Wk, bk, Wv, bv, ln_weight, ln_bias = (f32_param(t) for t in (Wq, bq, Wk, bk, Wv, bv, ln_weight, ln_bias))
    tail = (x0, residual, alpha, ln_weight, ln_bias, eps, relu)
    sharded = shard is not None and shard.world > 1
    if sharded and csr is not None and slice_sharded(shard, C, x.dtype):
        return _closed_form_slice_sharded(be, x, Wq, bq, Wk, bk, Wv, bv, csr, attn_scale, gcn_scale, *tail, shard, head)
    sl = sliced.rows_format(csr, x.dtype, n, C, shard)
    handle = shard.all_gather_rows_async(x) if (sharded and csr is not None) else None
    have = carry.products if (carry is not None and not sharded) else None
    if have is not None and not (have["x"] is x and have["sl"] is sl):
        if have["x"] is x and have.get("rscale") is not None:
            raise RuntimeError("difformer_amd: these rows exist as a slice-major copy for another sliced format only")
        have = None
    rscale = have.get("rscale") if have is not None else None      # single copy in: x is rows_stand_in, the rows are have["ys"]
    if rscale is not None and (x0 is not None or keep is not None or have["ys"] is None or sl is None):
        raise RuntimeError("difformer_amd: rows kept as their slice-major copy alone cannot feed this layer")
    record, ys, coef, side = _record_and_coeffs(be, x, (Wq, bq, Wk, bk, Wv, bv), csr, sl, have, shard, factors, attn_scale)
    ax, rs, gather, late = _graph_term(be, x, csr, sl, ys, handle, shard, gcn_scale, Wv is not None, keep is None,
                                       side[0] if side is not None else None)
    if side is not None:
        coef = late
        side[1](coef)
    if carry is not None:
        carry.products = None
    if keep is not None:
        keep.update(record=record, coef=coef, ax=ax, row_sums=rs)
    if head is not None:                           # last layer: the model's output Linear rides in the same pass -> logits
        head = tuple(f32_param(t) for t in head)   # bfloat16 storage: exact float32 copies, as for the other parameters
    want_next = (carry is not None and not sharded and carry.want_next and D % 4 == 0 and D == C and
                 x.dtype == torch.float32 and sl is not None and head is None and gather is None)
    # the mode: this layer's rows may exist as the slice-major copy alone when the model loop has said that only closed-form
    # layer kernels over this graph read them (carry.single_copy) and the graph lets a row be recovered from the copy
    rscale_out = csr.row_scale() if (want_next and carry.single_copy and SINGLE_COPY and side is not None) else None
    out = _simple_layer_kernel(be, ys if rscale is not None else x, coef, D, ax, Wv, bv, rs, gcn_scale, *tail,
                               next_operand=(csr.rowptr, sl.plan) if want_next else None, head=head, gather=gather,
                               rscale=rscale, rows=rscale_out is None)
    if rscale is not None:
        carry.single += 1
    if want_next:
        out, ys2 = out
        if out is None:
            out = rows_stand_in(ys2, n, D)
        carry.products = dict(x=out, sl=sl, record=None, ys=ys2, rscale=rscale_out)
    return out


# The closed-form layer aggregates inside its own kernel (dif_simple_layer_gather_*) up to this many entries per row on
# average; above, the separate SpMM kernels (rows split over lanes, long rows over quads) balance the work better.
LAYER_GATHER = os.environ.get("DIFFORMER_LAYER_GATHER", "1") != "0"
LAYER_GATHER_MAX_DEGREE = int(os.environ.get("DIFFORMER_LAYER_GATHER_MAX_DEGREE", "12"))
# ... and only without long rows: the 16 rows of a tile walk in lock step to the longest (GraphCSR.max_degree); from ~64
# entries on the SpMM kernel, which hands long rows to a whole block, is faster (profiles/r03_experiments.md, 5b)
LAYER_GATHER_MAX_ROW = int(os.environ.get("DIFFORMER_LAYER_GATHER_MAX_ROW", "64"))

def closed_form_coeffs_backward(record, n_global, C, D, Wq, bq, Wk, bk, Wv, bv, attn_scale, d_MnT, d_cn, d_u, d_cd):
    """Backward of the coefficient stage (backend.simple_coeffs): gradients of a loss with respect to the Gram record and
    the projection parameters, given its gradients with respect to MnT [D, C], cn [D], u [C] and cd.  float64 tensor ops on
    (C + 1)-square matrices.  With the augmented matrices W~ = [W | b] and G~ = [[G, sx], [sx^T, N]] (difformer.py:18-38):
        KtV = W~k G~ W~v^T,  sum k = W~k G~ e,  sum v = W~v G~ e,  |Q|^2 = <W~q G~, W~q>,  |K|^2 = <W~k G~, W~k>,  s = (|Q|^2 |K|^2)^-1/2
        [Mn; cn - a sum v] = a s W~q^T KtV,    [u; cd - N] = s W~q^T sum k
    -> (S [C, C], t [C]) with d x = x S + 1 t^T (S, t = the symmetrised gradient of G~), d_Wq, d_bq, d_Wk, d_bk, d_Wv, d_bv
    (float32; the last two None when Wv is None: use_weight = False)."""
    f64 = torch.float64
    dev = record.device
    N = float(n_global)
    r = record.to(f64)
    Gt = torch.empty((C + 1, C + 1), dtype=f64, device=dev)
    Gt[:C, :C] = r[: C * C].view(C, C)
    Gt[:C, C] = r[C * C: C * C + C]
    Gt[C, :C] = r[C * C: C * C + C]
    Gt[C, C] = N
    aug = lambda W, b: torch.cat([W.to(f64), b.to(f64)[:, None]], dim=1)
    Wq_, Wk_ = aug(Wq, bq), aug(Wk, bk)
    if Wv is not None:
        Wv_ = aug(Wv, bv)
    else:
        Wv_ = torch.cat([torch.eye(D, C, dtype=f64, device=dev), torch.zeros(D, 1, dtype=f64, device=dev)], dim=1)
    a = float(attn_scale)
    Aq, Ak, Av = Wq_ @ Gt, Wk_ @ Gt, Wv_ @ Gt
    ktv, ksum = Ak @ Wv_.t(), Ak[:, C]
    q2, k2 = (Aq * Wq_).sum(), (Ak * Wk_).sum()
    s = (q2 * k2) ** -0.5
    P, rr = Wq_.t() @ ktv, Wq_.t() @ ksum
    Dm = torch.cat([d_MnT.to(f64).t(), d_cn.to(f64)[None, :]], dim=0)                   # [C + 1, D]
    Du = torch.cat([d_u.to(f64).reshape(-1), d_cd.to(f64).reshape(1)])                  # [C + 1]
    dP, dr = a * s * Dm, s * Du
    ds = a * (Dm * P).sum() + (Du * rr).sum()
    dvsum = a * d_cn.to(f64)
    dktv, dksum = Wq_ @ dP, Wq_ @ dr
    dq2, dk2 = -0.5 * ds * s / q2, -0.5 * ds * s / k2
    e_col = Gt[:, C]
    dWq_ = ktv @ dP.t() + torch.outer(ksum, dr) + 2.0 * dq2 * Aq
    dWk_ = 2.0 * dk2 * Ak + dktv @ Av + torch.outer(dksum, e_col)
    dWv_ = dktv.t() @ Ak + torch.outer(dvsum, e_col)
    dGt = dq2 * (Wq_.t() @ Wq_) + dk2 * (Wk_.t() @ Wk_) + Wk_.t() @ dktv @ Wv_
    dGt[:, C] += Wk_.t() @ dksum + Wv_.t() @ dvsum
    S = dGt + dGt.t()
    f32 = torch.float32
    out = [S[:C, :C].to(f32).contiguous(), S[C, :C].to(f32).contiguous(), dWq_[:, :C].to(f32), dWq_[:, C].to(f32),
           dWk_[:, :C].to(f32), dWk_[:, C].to(f32)]
    out += [dWv_[:, :C].to(f32), dWv_[:, C].to(f32)] if Wv is not None else [None, None]
    return out


XWIDE_MAX = int(os.environ.get("DIFFORMER_XWIDE_MAX", "416"))   # widest layer of the one-pass kernel with streamed weights (0: library GEMMs)
CLOSED_FORM_WIDE_MAX = 512      # widest layer the Gram-record formulation is used for (record = C x C floats)
# Layers wider than this take the Gram-record formulation at the scripts' widths: from 65 columns with the one-pass layer kernel
# of csrc/simple_layer_wide.hip (up to 128 columns: pokec-batch-h128 0.95 -> see profiles/r04_experiments.md); under
# DIFFORMER_EXACT_FP32=1 (that kernel runs split-bfloat16 products) from 129, where the library GEMMs around the tail pass win
# over the q / k / v operator path (at 128 they cost the same: 1.01 vs 1.02 ms)
CLOSED_FORM_WIDE_MIN = 128 if EXACT_FP32 else 64


def set_exact_fp32(flag):
    """Switch DIFFORMER_EXACT_FP32 at run time (bench.py's second pass) -> the previous setting.  What was made under the
    old setting follows the switch by itself: a captured forward (DIFFormer's auto-graph) is keyed on it and runs eagerly,
    then is captured afresh; the backward of a sigmoid head whose forward ran on the plane kernels takes the tensor-op
    gradient once exact mode is on.  The packed weights and the weight-only factors of the closed form do not depend on it
    (only the launchers that read them do), and CLOSED_FORM_WIDE_MIN below is read at every call."""
    global EXACT_FP32, CLOSED_FORM_WIDE_MIN
    was = EXACT_FP32
    EXACT_FP32 = bool(flag)
    be = _BACKEND
    if be is not None and hasattr(be, "set_exact_fp32"):
        be.set_exact_fp32(EXACT_FP32)                       # the launchers' own choices (dif_set_exact_fp32)
    CLOSED_FORM_WIDE_MIN = 128 if EXACT_FP32 else 64
    return was


class WideCoefficients:
    """Weight-only factors of the closed form at the scripts' widths, float64, rebuilt when a parameter changes.
    With the augmented matrices  X~ = [X | 1],  W~ = [W | b]  (so q = X~ W~q^T etc.) and  G~ = X~^T X~ = [[G, sx], [sx^T, N]]:
        |Q|^2 = <W~q^T W~q, G~>,   |K|^2 = <W~k^T W~k, G~>                       (difformer.py:20-21)
        T = G~ V~,    V~ = [W~v^T | e_last | 0 0 0]     -> last row of T = [sum v | N | 0 0 0]
        R = P~ T,     P~ = W~q^T W~k                     -> rows 0..C-1 = [Mn | u] / s,  last row = [bq KtV | bq.ksum] / s
    num = x Mn + cn, den = x.u + cd  with  [cn | cd] = s R[C] + T[C]              (:25-38)"""

    def __init__(self, Wq, bq, Wk, bk, Wv, bv):
        f64 = torch.float64
        aug = lambda W, b: torch.cat([W.to(f64), b.to(f64)[:, None]], dim=1)
        Wq_, Wk_ = aug(Wq, bq), aug(Wk, bk)
        D, C1 = Wq_.shape
        if Wv is not None:
            Wv_ = aug(Wv, bv)
        else:                                                           # use_weight = False: v = x (difformer.py:120)
            Wv_ = torch.cat([torch.eye(C1 - 1, dtype=f64, device=Wq.device), torch.zeros(C1 - 1, 1, dtype=f64, device=Wq.device)], 1)
        self.D = Wv_.shape[0]
        self.S = torch.stack([(Wq_.t() @ Wq_).reshape(-1), (Wk_.t() @ Wk_).reshape(-1)])           # [2, (C+1)^2]
        self.P = (Wq_.t() @ Wk_).contiguous()                                                      # [(C+1), (C+1)]
        V = torch.zeros((C1, self.D + 4), dtype=f64, device=Wq.device)
        V[:, : self.D] = Wv_.t()
        V[C1 - 1, self.D] = 1.0
        self.V = V


def simple_layer_closed_form_wide(x, coeffs: WideCoefficients, Wv, bv, csr, attn_scale, gcn_scale, x0, residual, alpha,
                                  ln_weight, ln_bias, eps):
    """The closed form of simple_layer_closed_form at the widths the reference's scripts train with (hidden 128 / 300 /
    400: run.sh): query == source == x [n, C] fp32, one head, single GPU, inference.
        G~ = [X | 1]^T [X | 1]             one streaming pass (dif_gram_sym_f32: the upper 64-blocks of X^T X on the fp32 MFMA)
        [Mn | u], [cn | cd]                the float64 (C + 1)-square products of WideCoefficients (dif_wide_coeffs_f64)
        Z = x [Mn | u] + [cn | cd]         ONE row GEMM: numerator | denominator
        gcn = (A_hat x) Wv^T               SpMM on x, one row GEMM  (+ (A_hat 1) bv^T inside the tail)
        tail                               num / den, combine, + x0, residual, LayerNorm in one pass (dif_layer_tail_mix_f32)
    instead of three projections (3 N C D), the K^T V reduce (N D^2) and the Q-side apply (N D^2): 2-3x fewer FLOPs and
    q, k, v never written."""
    be = get_backend()
    n, C = x.shape
    D = coeffs.D
    x3 = x.reshape(n, 1, C)
    rec = be.gram_sym(x)                                                # [X^T X (upper blocks) | sum x | ...]
    B, bias = be.wide_coeffs(rec, C, n, coeffs.S, coeffs.V, coeffs.P)   # both float64 products + bookkeeping: two launches
    one_pass = None
    if max(C, D) <= 128 and not EXACT_FP32 and hasattr(be, "simple_layer_wide"):
        # hidden 128 (node classification/run.sh:42-44): both row products, the division, the combine, the residual and the
        # LayerNorm in ONE pass over the rows (csrc/simple_layer_wide.hip) -- no library GEMM, no [n, D + 4] intermediate
        one_pass = be.simple_layer_wide
    elif max(C, D) <= XWIDE_MAX and not EXACT_FP32 and hasattr(be, "simple_layer_xwide"):
        # hidden 300 / 400 (image and text/run.sh:27): the same one pass with the rows in registers and the weights streamed
        # through LDS (csrc/simple_layer_xwide.hip) instead of a library GEMM per product around a tail pass
        one_pass = be.simple_layer_xwide
    if one_pass is not None:
        ax = rs = None
        if csr is not None:
            ax = gcn_aggregate(csr, x3, None, 1.0, 1.0).reshape(n, C)
            rs = csr.row_sums() if Wv is not None else None
        return one_pass(x, B, bias, D, attn_scale, ax, Wv if csr is not None else None, bv if csr is not None else None, rs,
                        gcn_scale, x0, residual, alpha, ln_weight, ln_bias, eps)
    Z = torch.addmm(bias, x, B)                                         # [n, D + 4]: numerator | denominator
    gcn = rs = None
    if csr is not None:
        ax = gcn_aggregate(csr, x3, None, 1.0, 1.0).reshape(n, C)       # sliced or gather kernels, whichever the graph takes
        if Wv is not None:
            gcn, rs = torch.mm(ax, Wv.t()), csr.row_sums()
        else:
            gcn = ax
    return be.layer_tail_mix(Z, D, D, attn_scale, gcn, gcn_scale, rs, bv if rs is not None else None, x0,
                             x if residual else None, alpha, ln_weight, ln_bias, eps)


# ------------------------------------------------------------------------------------------
# f4: batch of graphs stored back to back (physical particle/difformer-v2.py:71-137)
# ------------------------------------------------------------------------------------------
class BatchLayout:
    """Index tables of a batch, derived once from `n_nodes` [B] (node count per graph), all on the device:
        graph_ptr    int32 [B+1]   graph b = rows [graph_ptr[b], graph_ptr[b+1])
        ranked_first int32 [B]     first row of the r-th largest graph        (sigmoid kernel)
        pos_count    int32 [maxn]  number of graphs with more than p nodes    (sigmoid kernel)
    They replace the reference's padding machinery (make_batch_mask / make_batch / to_pad, difformer-v2.py:8-27).
    Only B-sized integer bookkeeping happens here; the node-sized work is in the kernels."""

    def __init__(self, n_nodes, device):
        n = n_nodes.to(device=device, dtype=torch.int64).reshape(-1)
        if n.numel() == 0:
            raise ValueError("difformer_amd: n_nodes is empty")
        ptr = torch.zeros(n.numel() + 1, dtype=torch.int64, device=device)
        torch.cumsum(n, 0, out=ptr[1:])
        self.n_graphs = int(n.numel())
        total, biggest, smallest = (int(v) for v in torch.stack([ptr[-1], n.max(), n.min()]).tolist())   # one sync
        if smallest < 0:
            raise ValueError("difformer_amd: negative entry in n_nodes")
        if total >= 2 ** 31:
            raise ValueError("difformer_amd: batches are limited to 2^31 - 1 nodes")
        self.n_rows, self.max_nodes, self.min_nodes = total, biggest, smallest
        self.graph_ptr = ptr.to(torch.int32)
        order = torch.argsort(n, descending=True, stable=True)
        self.ranked_first = ptr[:-1][order].to(torch.int32).contiguous()
        le = torch.cumsum(torch.bincount(n, minlength=biggest + 1), 0)        # le[p] = #{graphs with n <= p}
        self.pos_count = (self.n_graphs - le[:biggest]).to(torch.int32).contiguous()


class _LayoutCache(TensorCache):
    """One BatchLayout per `n_nodes` tensor and device, so the per-layer calls of one forward and repeated forwards over
    the same batch do the bookkeeping (and its host sync) once."""

    def get(self, n_nodes, device):
        if not torch.is_tensor(n_nodes):
            n_nodes = torch.as_tensor(n_nodes)
            return BatchLayout(n_nodes, device)
        extras = (str(device),)
        lay = self.lookup((n_nodes,), extras)
        if lay is MISS:
            lay = self.insert((n_nodes,), extras, BatchLayout(n_nodes, device))
        return lay


layout_cache = _LayoutCache(16, unversioned=True)


def _check_batch(qs, ks, vs, layout):
    if not (qs.shape[0] == ks.shape[0] == vs.shape[0] == layout.n_rows):
        raise RuntimeError(f"difformer_amd: n_nodes sums to {layout.n_rows} but q/k/v have "
                           f"{qs.shape[0]}/{ks.shape[0]}/{vs.shape[0]} rows (difformer-v2.py:26 would raise too)")


def batched_simple_attention(qs, ks, vs, layout: BatchLayout):
    """qs, ks [N,H,M], vs [N,H,D] -> [N,H,D]; attention inside each graph.  difformer-v2.py:80-111."""
    _check_batch(qs, ks, vs, layout)
    if layout.n_graphs == 1:          # one graph: exactly a1, whose reduce spreads the rows over the whole chip
        return simple_attention(qs, ks, vs)
    return get_backend().batched_simple_attention(qs, ks, vs, layout.graph_ptr)


def batched_sigmoid_attention(qs, ks, vs, layout: BatchLayout):
    """Attention among the nodes at equal positions of the graphs.  difformer-v2.py:113-135."""
    _check_batch(qs, ks, vs, layout)
    return get_backend().batched_sigmoid_attention(qs, ks, vs, layout.ranked_first, layout.pos_count)


# ------------------------------------------------------------------------------------------
# a4 / a5 tail
# ------------------------------------------------------------------------------------------
def layer_tail(conv, x0=None, prev=None, alpha=0.5, ln_weight=None, ln_bias=None, eps=1e-5, relu=False):
    """conv [n,H,D] -> [n,D]: head mean (+x0) -> alpha-residual with prev -> LayerNorm (-> ReLU)."""
    return get_backend().layer_tail(conv, x0, prev, alpha, ln_weight, ln_bias, eps, relu)


def linear(x, weight, bias, ln_weight=None, ln_bias=None, eps=1e-5, relu=False):
    """x W^T + b (-> LayerNorm) (-> ReLU) (difformer.py:188-191, :208; csrc/skinny_linear.hip: C_in <= 128, long rows into
    <= 64 features; csrc/simple_layer_xwide.hip: wide rows into 65..416 features, see linear_xwide_covers)."""
    return get_backend().linear(x, weight, bias, ln_weight, ln_bias, eps, relu)


GRAM_COEFFS_MAX_ROWS = 24576        # 48 partial Gram records: beyond, the separate finalize launch is the cheaper sum
LINEAR_XWIDE_MIN_ROWS = 16384       # below: too few 128-row blocks for the chip (15,000 x 512 -> 300: 64 us against 62 for GEMM + tail)


def linear_xwide_covers(x, weight):
    """Shapes dif_linear_xwide_f32 takes (float32, split-bf16 products: not under DIFFORMER_EXACT_FP32): more than 128 input
    channels in one product (<= 416) or two halves (C_in % 8 == 0, C_in / 2 <= 416), 65..416 output features, both multiples
    of 4, enough rows to fill the chip (a workgroup owns 128 rows)."""
    if EXACT_FP32 or x.dtype != torch.float32 or weight.dtype != torch.float32 or x.dim() != 2:
        return False
    n, c_in = x.shape
    d = weight.shape[0]
    if n < LINEAR_XWIDE_MIN_ROWS or not (64 < d <= XWIDE_MAX) or d % 4 or c_in <= 128 or c_in % 4:
        return False
    return c_in <= XWIDE_MAX or (c_in % 8 == 0 and c_in // 2 <= XWIDE_MAX)
