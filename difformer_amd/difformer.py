"""Drop-in replacement for the reference module `difformer` on MI355X.

Same public names, constructor arguments, defaults, `forward` signatures and `state_dict` keys
as `node classification/difformer.py` (the superset of the three task-folder copies), so
`from difformer import *` in the reference's parse.py (`node classification/parse.py:2`) keeps
working once `difformer.py` in a task folder is replaced by `dropin/difformer.py`.

What differs is where the arithmetic runs: every propagation operator is a hand-written gfx950
kernel behind the C ABI of include/difformer_hip.h (see ops.py); this file only sequences them.
There is no CPU arithmetic: tensors must be float32 (or bfloat16) on the GPU.  Callers that keep the model AND its
operands in host memory (`test_large_dataset.py:69,91-93`, `eval.py::evaluate_cpu`) are staged onto the GPU and get their
result back on the host (staging.py); without a GPU such a call raises.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from . import sliced
from . import autograd_ops as ag
from . import staging
from . import tiny
from .tensor_cache import remembered, same_tensors, tensor_key, weak_refs

__all__ = ["full_attention_conv", "gcn_conv", "DIFFormerConv", "DIFFormer"]

_AUTO_GRAPH = os.environ.get("DIFFORMER_AUTO_GRAPH", "1") != "0"
_CLOSED_FORM_TRAINING = os.environ.get("DIFFORMER_CLOSED_FORM_TRAINING", "1") != "0"
# wide layers (> 64 columns) train on the operator path: a backward through the record was slower there (hidden-128 step
# 5.86 ms against 3.41; profiles/r06_experiments.md section 5)
# A forward is captured and replayed as one hipGraph only while it is LAUNCH-bound: the capture keeps a private pool with one
# forward's intermediates for the model's lifetime (~0.5 GB at the ogbn-proteins size, ~3 GB on the full Pokec graph) and
# replay buys <= 2 % there (profiles/r04_e_bench_small_configs.json), against 2x at Cora size.  The gate is the forward's
# estimated HBM traffic, layers x (4 N hidden s + 8 nnz) bytes: 1.5 GB is ~0.4 ms of kernels -- Cora, CIFAR-50k and Pokec
# mini-batches (also at hidden 128 / 300) replay, the ogbn-proteins graph and the full Pokec graph run kernel by kernel.
_AUTO_GRAPH_MAX_BYTES = float(os.environ.get("DIFFORMER_AUTO_GRAPH_MAX_BYTES", "1.5e9"))


def _dense_attention(qs, ks, kernel):
    """Dense [N,L,H] attention weights for visualisation (`output_attn`, difformer.py:42-43 /
    :47-55).  O(N*L) by definition and outside the timed path: plain device-side tensor ops."""
    if kernel == "simple":
        qn = qs / torch.linalg.vector_norm(qs)
        kn = ks / torch.linalg.vector_norm(ks)
        den = torch.einsum("nhm,hm->nh", qn, kn.sum(dim=0)).unsqueeze(-1) + qs.shape[0]
        return torch.einsum("nhm,lhm->nlh", qn, kn) / den
    s = torch.sigmoid(torch.einsum("nhm,lhm->nlh", qs, ks))
    return s / s.sum(dim=1, keepdim=True)


def full_attention_conv(qs, ks, vs, kernel, output_attn=False):
    """qs [N,H,M], ks [L,H,M], vs [L,H,D] -> [N,H,D]  (reference: difformer.py:10-61)."""
    dev = staging.staging_device(None, (qs, ks, vs))
    if dev is not None:      # host operands: computed on the GPU, returned on the host (`.to` is differentiable)
        out = full_attention_conv(qs.to(dev), ks.to(dev), vs.to(dev), kernel, output_attn)
        return tuple(o.to(qs.device) for o in out) if output_attn else out.to(qs.device)
    if kernel == "simple":
        out = ag.simple_attention(qs, ks, vs)
    elif kernel == "sigmoid":
        out = ag.sigmoid_attention(qs, ks, vs)
    else:
        raise ValueError(f"unknown attention kernel {kernel!r} (expected 'simple' or 'sigmoid')")
    if output_attn:
        return out, _dense_attention(qs, ks, kernel)
    return out


def gcn_conv(x, edge_index, edge_weight):
    """x [N,H,D], edge_index [2,E] int64, edge_weight [E] or None -> [N,H,D]
    (reference: difformer.py:63-79).  The normalised CSR is built on first use and cached."""
    dev = staging.staging_device(None, (x, edge_index, edge_weight))
    if dev is not None:      # host operands: the device copy of edge_index is kept, so the cached CSR is found again
        ew = edge_weight
        if ew is not None:
            ew = ew.to(dev) if ew.requires_grad else staging.operands.get(ew, dev)
        return gcn_conv(x.to(dev), staging.operands.get(edge_index, dev), ew).to(x.device)
    csr = ops.csr_cache.get(edge_index, edge_weight, x.shape[0], x.shape[1] * x.shape[2] * x.element_size(),
                            elem_size=x.element_size())
    return ag.gcn_aggregate(csr, x, None, 1.0, csr.weight_scale)


def mix_scales(graph_weight, use_graph, csr):
    """(attention scale, graph scale) of the combine, difformer.py:130-136: (1 - w, w) for graph_weight = w > 0, else
    (1, 1); the graph scale also carries a constant edge_weight (csr.weight_scale: ops._CSRCache.get).  Without a graph
    the mix does not exist: the attention scale is 1 (and the graph scale multiplies nothing)."""
    a_s, g_s = (1.0 - graph_weight, float(graph_weight)) if graph_weight > 0 else (1.0, 1.0)
    if not use_graph:
        return 1.0, g_s
    return a_s, g_s * csr.weight_scale


_NO_WV = {"weight": None, "bias": None}


def _present(params):
    return [t for t in params if t is not None]


def _ln_args(bn):
    """(weight, bias, eps) of a LayerNorm for the kernels that apply it in their tail; (None, None, 1e-5) without one."""
    return (bn.weight, bn.bias, bn.eps) if bn is not None else (None, None, 1e-5)


class DIFFormerConv(nn.Module):
    """One DIFFormer propagation layer (reference: difformer.py:81-145)."""

    def __init__(self, in_channels, out_channels, num_heads, kernel='simple', use_graph=True, use_weight=True,
                 graph_weight=-1, use_source=False):
        super().__init__()
        # creation order Wk, Wq, Wv as in the reference so seeded initialisation matches
        self.Wk = nn.Linear(in_channels, out_channels * num_heads)
        self.Wq = nn.Linear(in_channels, out_channels * num_heads)
        if use_weight:
            self.Wv = nn.Linear(in_channels, out_channels * num_heads)
        self.out_channels = out_channels
        self.num_heads = num_heads
        self.kernel = kernel
        self.use_graph = use_graph
        self.use_weight = use_weight
        self.graph_weight = graph_weight
        self.use_source = use_source
        self.row_shard = None  # set through DIFFormer.set_row_shard for multi-GPU runs
        self._fused_wb = None  # (key, (weight, bias)) of the concatenated projections (inference only)
        self._wide = None      # (key, ops.WideCoefficients): weight-only factors of the closed form at hidden > 64
        self._narrow = None    # (key, ops.NarrowFactors): weight-only factors of the background coefficient chain

    def __getstate__(self):
        # copy.deepcopy / torch.save(model): the inference caches are rebuilt on demand and must not travel
        state = super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__.copy()
        state = dict(state)
        state.update(_fused_wb=None, _wide=None, _narrow=None, row_shard=None)
        return state

    def __deepcopy__(self, memo):
        # a best-checkpoint / EMA copy of a row-sharded model keeps the shard BY REFERENCE (it describes the process group,
        # not the parameters); pickling (torch.save(model)) still drops it -- a process group does not travel
        import copy as _copy
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__.update(_copy.deepcopy(self.__getstate__(), memo))
        new.row_shard = self.row_shard
        return new

    def reset_parameters(self):
        self.Wk.reset_parameters()
        self.Wq.reset_parameters()
        if self.use_weight:
            self.Wv.reset_parameters()
        self.invalidate_caches()

    def invalidate_caches(self):
        """Drop the inference-time caches derived from the parameters (concatenated projections, weight-only factors of
        the closed form).  They are keyed on (data_ptr, _version) of the parameters, which in-place optimiser steps,
        `copy_` and `load_state_dict` bump -- but writes through `.data` (EMA, weight averaging, manual loading) do not:
        call this (or `DIFFormer.invalidate_caches()`) after such an update."""
        self._fused_wb = self._wide = self._narrow = None

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_caches()
        return out

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_caches()
        return out

    def _qkv_params(self):
        """(Wq.weight, Wq.bias, Wk.weight, Wk.bias, Wv.weight | None, Wv.bias | None): the projections as the closed-form
        kernels take them, None for a missing Wv (use_weight=False).  Plain dict reads, as in DIFFormer._graph_key: this
        runs in every layer call, and nn.Module.__getattr__ costs about a microsecond per name."""
        m = self._modules
        q, k, v = m["Wq"]._parameters, m["Wk"]._parameters, m["Wv"]._parameters if self.use_weight else _NO_WV
        return (q["weight"], q["bias"], k["weight"], k["bias"], v["weight"], v["bias"])

    def _qkv_list(self):
        """The parameters that exist, for `ag._needs_grad` and the parameter-version memos."""
        return _present(self._qkv_params())

    # -- projections: one fused GEMM when query and source are the same tensor -----------------
    def _project(self, query_input, source_input):
        H, D = self.num_heads, self.out_channels
        if query_input is source_input:
            mods = [self.Wq, self.Wk] + ([self.Wv] if self.use_weight else [])
            params = self._qkv_list()
            if ag._needs_grad(*params):
                w = torch.cat([m.weight for m in mods], dim=0)
                b = torch.cat([m.bias for m in mods], dim=0)
            else:
                # inference: the concatenation is rebuilt only when a parameter changes (in-place optimiser steps and
                # load_state_dict bump _version; .to() replaces the tensors) -- two concat kernels per layer otherwise
                self._fused_wb = remembered(self._fused_wb, params, lambda: (torch.cat([m.weight for m in mods], dim=0),
                                                                             torch.cat([m.bias for m in mods], dim=0)))
                w, b = self._fused_wb[1]
            # [n, (2|3)*H*D]; q/k/v are column slices.  Narrow inputs take the hand-written Linear kernel (one launch,
            # x read once), wide ones the vendor GEMM (autograd_ops.linear decides).
            if w.shape[0] <= 256:
                qkv = ag.linear(source_input, w, b)
            elif ag._needs_grad(source_input, w, b):
                qkv = ag._row_linear(source_input, w, b)       # training at hidden 128: weight gradient on the streaming reduce
            else:
                qkv = F.linear(source_input, w, b)
            cols = ag.split_columns(qkv, *([H * D] * (3 if self.use_weight else 2)))
            q, k = cols[0].reshape(-1, H, D), cols[1].reshape(-1, H, D)
            v = cols[2].reshape(-1, H, D) if self.use_weight else None
        else:
            q = self.Wq(query_input).reshape(-1, H, D)
            k = self.Wk(source_input).reshape(-1, H, D)
            v = self.Wv(source_input).reshape(-1, H, D) if self.use_weight else None
        if v is None:
            v = source_input.reshape(-1, 1, D)                # difformer.py:120
        return q, k, v

    def _route(self, query_input, source_input, edge_weight, x0, prev, ln_weight, ln_bias, want_qk):
        """Which kernels run this layer: the single statement of the rule.  Evaluated once per `_layer` call; the methods
        of the routes rely on it and test none of this again.  x = source_input [n, C], D = out_channels, `wide` = C > 64
        or D > 64, `training` = a gradient is wanted for x, a projection parameter, x0 or a LayerNorm parameter -- ANY
        operand of the layer makes it a training call.

        Everything but "operator" needs: the `simple` kernel, query_input IS source_input, x two-dimensional, no q / k
        wanted back (`want_qk`: the dense attention map is made from them) and no gradient for edge_weight
        (difformer.py:73 is differentiable in it; only the operator path's aggregation has that backward).

        The three closed forms (the whole layer through the Gram record, csrc/simple_layer.hip: q, k, v never exist)
        need on top of that
          * one head, float32 or bfloat16 rows, C a multiple of 4 (the kernels read rows as float4);
          * bfloat16 rows only for the narrow single-GPU layer with bfloat16 parameters (BASELINE config C5): not wide,
            no row shard, Wq stored as bfloat16;
          * wide only without a row shard, up to ops.CLOSED_FORM_WIDE_MAX columns (the record is C x C floats), above
            ops.CLOSED_FORM_WIDE_MIN input columns and with n >= 4 C: the record only pays with many more rows than
            columns, and from hidden ~256 up (at 128 the two row GEMMs cost what the operator path does; with the
            one-pass kernel of csrc/simple_layer_wide.hip the threshold is 64 -- see ops.CLOSED_FORM_WIDE_MIN, which
            DIFFORMER_EXACT_FP32 moves, so it is read here at every call);
          * C == D without Wv (v = x, difformer.py:120), and with a residual (`prev`): it must be x itself -- the kernel
            mixes the residual from the rows it already holds;
          * a backend with `gram`, and with `gram_sym` when wide (a host-side test backend without the record passes:
            operator path).
        Then
          closed_wide       not training, wide: ops.simple_layer_closed_form_wide (Gram-record formulation at the
                            scripts' widths, hidden 128 / 300 / 400, inference).
          closed_narrow     not training, not wide: ops.simple_layer_closed_form.
          closed_train      training, not wide, float32, no row shard (or a world of one), `_CLOSED_FORM_TRAINING` on and a
                            backend with `simple_reduce`: ag.closed_form_layer, forward and backward through the record
                            (ag._ClosedFormLayer has that backward up to 64 columns; wide layers train on the operator
                            path, where a backward through the record was slower: hidden-128 step 5.86 ms against 3.41,
                            profiles/r06_experiments.md section 5).
        Otherwise
          fused_projection  Wv present, C <= 64 and D <= 64, no gradient wanted for x or a projection parameter (x0 and
                            the LayerNorm live in the tail, which has its own backward): projection + reduce in one
                            kernel (csrc/project_reduce.hip), ops.project_simple_attention.
          operator          everything else: q / k / v projections, the attention operator, aggregation with the tail."""
        x = source_input
        if (self.kernel != 'simple' or query_input is not source_input or x.dim() != 2 or want_qk or
                ag._needs_grad(edge_weight)):
            return "operator"
        C, D, shard = x.shape[1], self.out_channels, self.row_shard
        wide = C > 64 or D > 64
        params = self._qkv_list()
        if (self.num_heads == 1 and x.dtype in (torch.float32, torch.bfloat16) and C % 4 == 0
                and not (x.dtype == torch.bfloat16 and (wide or shard is not None or self.Wq.weight.dtype != torch.bfloat16))
                and not (wide and (shard is not None or max(C, D) > ops.CLOSED_FORM_WIDE_MAX or
                                   C <= ops.CLOSED_FORM_WIDE_MIN or x.shape[0] < 4 * C))
                and (self.use_weight or C == D) and (prev is None or (prev is x and C == D))
                and hasattr(ops.get_backend(), "gram") and (not wide or hasattr(ops.get_backend(), "gram_sym"))):
            if not ag._needs_grad(x, *params, x0, ln_weight, ln_bias):
                return "closed_wide" if wide else "closed_narrow"
            if (not wide and _CLOSED_FORM_TRAINING and x.dtype == torch.float32 and (shard is None or shard.world <= 1)
                    and hasattr(ops.get_backend(), "simple_reduce")):
                return "closed_train"
        if self.use_weight and C <= 64 and D <= 64 and not ag._needs_grad(x, *params):
            return "fused_projection"
        return "operator"

    def _layer(self, query_input, source_input, edge_index, edge_weight, x0=None, prev=None, alpha=0.5,
               ln_weight=None, ln_bias=None, eps=1e-5, want_qk=False, carry=None):
        """Propagation (:115-136) followed by the tail (:137-140 and, when given, :200-203) -> ([n,D], q, k)."""
        route = self._route(query_input, source_input, edge_weight, x0, prev, ln_weight, ln_bias, want_qk)
        tail = (x0, prev, alpha, ln_weight, ln_bias, eps)
        if route == "fused_projection":
            attn, v = ops.project_simple_attention(source_input, *self._qkv_params(), self.num_heads, self.out_channels,
                                                   self.row_shard, gather_values=self.use_graph)
            return self._graph_term_and_tail(attn, v, edge_index, edge_weight, tail), None, None
        if route == "operator":
            q, k, attn, v = self._operator(query_input, source_input, edge_index, edge_weight)
            return self._graph_term_and_tail(attn, v, edge_index, edge_weight, tail), q, k
        x = source_input
        csr = self._closed_form_csr(x, edge_index, edge_weight)
        a_s, g_s = mix_scales(self.graph_weight, self.use_graph, csr)
        closed = {"closed_wide": self._closed_wide, "closed_train": self._closed_train, "closed_narrow": self._closed_narrow}
        return closed[route](x, csr, a_s, g_s, tail, carry), None, None

    def _closed_form_csr(self, x, edge_index, edge_weight):
        """The CSR a closed-form layer aggregates x [n, C] with (None without a graph)."""
        if not self.use_graph:
            return None
        if edge_index is None:
            raise ValueError("use_graph=True needs an edge_index")
        shard, esz = self.row_shard, x.element_size()
        n_global = shard.n_global if shard is not None else x.shape[0]
        if ops.slice_sharded(shard, x.shape[1], x.dtype) and x.shape[1] <= 64 and self.out_channels <= 64:
            # slice-sharded product: every rank multiplies the WHOLE graph at its C / world columns
            return ops.csr_cache.get(edge_index, edge_weight, n_global, shard.slice_width(x.shape[1]) * esz, None, esz)
        return ops.csr_cache.get(edge_index, edge_weight, n_global, x.shape[1] * esz, shard, esz)

    def _closed_wide(self, x, csr, a_s, g_s, tail, carry):
        x0, prev, alpha, ln_weight, ln_bias, eps = tail
        params = self._qkv_params()
        # weight-only factors: rebuilt when a parameter changes
        self._wide = remembered(self._wide, _present(params), lambda: ops.WideCoefficients(*params))
        return ops.simple_layer_closed_form_wide(x, self._wide[1], params[4], params[5], csr, a_s, g_s, x0, prev is not None,
                                                 alpha, ln_weight, ln_bias, eps)

    def _closed_train(self, x, csr, a_s, g_s, tail, carry):
        x0, prev, alpha, ln_weight, ln_bias, eps = tail
        return ag.closed_form_layer(x, *self._qkv_params(), csr, a_s, g_s, x0, prev is not None, alpha, ln_weight, ln_bias, eps)

    def _closed_narrow(self, x, csr, a_s, g_s, tail, carry):
        x0, prev, alpha, ln_weight, ln_bias, eps = tail
        params = self._qkv_params()
        factors = None
        # (`coeffs_bg` is no route condition: it says whether the factors of the background chain are worth keeping;
        # ops.simple_layer_closed_form decides whether the chain runs)
        if csr is not None and self.row_shard is None and x.dtype == torch.float32 and hasattr(ops.get_backend(), "coeffs_bg"):
            self._narrow = remembered(self._narrow, _present(params), lambda: ops.NarrowFactors(*params))
            factors = self._narrow[1]
        head = carry.head if carry is not None else None
        if head is not None and not (head[0].dtype == x.dtype and head[0].shape[0] <= 128 and head[1] is not None):
            head = None
        out = ops.simple_layer_closed_form(x, *params, csr, a_s, g_s, x0, prev is not None, alpha, ln_weight, ln_bias, eps,
                                           carry=carry, shard=self.row_shard, factors=factors, head=head)
        if head is not None:
            carry.head_done = True             # `out` is already the model's logits (difformer.py:208)
        return out

    def _operator(self, query_input, source_input, edge_index, edge_weight):
        """q / k / v projections and the attention operator -> (q, k, attn, v)."""
        H, shard = self.num_heads, self.row_shard
        q, k, v = self._project(query_input, source_input)
        v_att = v if v.shape[1] == H else v.expand(-1, H, -1).contiguous()
        if self.kernel == 'simple':
            attn = ag.simple_attention(q, k, v_att, shard)
        elif self.kernel == 'sigmoid':
            attn = ag.sigmoid_attention(q, k, v_att, shard)
        else:
            raise ValueError(f"unknown attention kernel {self.kernel!r}")
        if (self.use_graph and not v.is_contiguous() and v.shape[0] >= 65536 and edge_index is not None and
                edge_index.shape[1] >= 32 * v.shape[0] and
                ops.sliced_tiling(v.shape[0], v.shape[1] * v.shape[2], edge_index.shape[1], edge_weight, shard, v.element_size()) is None):
            v = v.contiguous()   # the blocked SpMM gathers whole rows: contiguous rows are ~8 % faster on big dense
                                 # graphs; small or sparse graphs (a Pokec batch: 18 us of copy for a 55-us product)
                                 # take the strided view as it is (every kernel has a leading dimension)
        return q, k, attn, v

    def _graph_term_and_tail(self, attn, v, edge_index, edge_weight, tail):
        """What follows the attention on the fused_projection and operator routes: mix with the aggregated values
        (:130-136), then the tail."""
        H, shard = self.num_heads, self.row_shard
        x0, prev, alpha, ln_weight, ln_bias, eps = tail
        if not self.use_graph:
            if isinstance(attn, ops.LazyAttention):
                attn = attn.materialize()
            return ag.layer_tail(attn, x0, prev, alpha, ln_weight, ln_bias, eps)
        if edge_index is None:
            raise ValueError("use_graph=True needs an edge_index")
        n_global = shard.n_global if shard is not None else v.shape[0]
        esize = (v.local if isinstance(v, ops.GatheredRows) else v).element_size()
        csr = ops.csr_cache.get(edge_index, edge_weight, n_global, v.shape[1] * v.shape[2] * esize, shard, esize)
        a_s, g_s = mix_scales(self.graph_weight, True, csr)
        if v.shape[1] == H:
            return ag.gcn_aggregate_tail(csr, v, attn, a_s, g_s, shard, x0, prev, alpha, ln_weight, ln_bias, eps)
        # use_weight=False with several heads: the [n,1,D] aggregate broadcasts over heads
        conv = a_s * attn + g_s * ag.gcn_aggregate(csr, v, None, 1.0, 1.0, shard)
        return ag.layer_tail(conv, x0, prev, alpha, ln_weight, ln_bias, eps)

    def forward(self, query_input, source_input, edge_index=None, edge_weight=None, x_0=None, output_attn=False):
        out, q, k = self._layer(query_input, source_input, edge_index, edge_weight,
                                x_0 if self.use_source else None, want_qk=output_attn)   # head mean (+ x_0), :137-140
        if output_attn:
            return out, _dense_attention(q, k, self.kernel)
        return out


class DIFFormer(nn.Module):
    """DIFFormer model (reference: difformer.py:147-226).
    x: node features [N, in_channels]; edge_index [2, E] int64 (or None when use_graph=False);
    returns logits [N, out_channels]."""

    def __init__(self, in_channels, hidden_channels, out_channels, num_layers=2, num_heads=1, kernel='simple',
                 alpha=0.5, dropout=0.5, use_bn=True, use_residual=True, use_weight=True, use_graph=True,
                 graph_weight=-1, use_source=False):
        super().__init__()
        self.convs = nn.ModuleList()
        self.fcs = nn.ModuleList()
        self.fcs.append(nn.Linear(in_channels, hidden_channels))
        self.bns = nn.ModuleList()
        self.bns.append(nn.LayerNorm(hidden_channels))
        for _ in range(num_layers):
            self.convs.append(DIFFormerConv(hidden_channels, hidden_channels, num_heads=num_heads, kernel=kernel,
                                            use_graph=use_graph, use_weight=use_weight, graph_weight=graph_weight,
                                            use_source=use_source))
            self.bns.append(nn.LayerNorm(hidden_channels))
        self.fcs.append(nn.Linear(hidden_channels, out_channels))
        self.dropout = dropout
        self.activation = F.relu
        self.use_bn = use_bn
        self.residual = use_residual
        self.alpha = alpha
        self.auto_graph = True     # repeated inference forwards over the same operands replay as one hipGraph (_forward_graphed)
        self._ag_state = None
        self.last_single_copy = 0  # layer kernels of the last eager forward that read their rows from the slice-major copy alone

    def __getstate__(self):
        # copy.deepcopy(model) for a best-checkpoint / EMA copy and torch.save(model) must keep working after eval calls:
        # the hipGraph capture, its weak references and the device twin of a host-resident model stay behind
        state = super().__getstate__() if hasattr(super(), "__getstate__") else self.__dict__.copy()
        state = dict(state)
        state.update(_ag_state=None)
        state.pop("_staged", None)
        return state

    def reset_parameters(self):
        for conv in self.convs:
            conv.reset_parameters()
        for bn in self.bns:
            bn.reset_parameters()
        for fc in self.fcs:
            fc.reset_parameters()
        self._ag_state = None

    def invalidate_caches(self):
        """Forget everything cached from the parameters (see DIFFormerConv.invalidate_caches): needed only after
        updates that bypass the version counter (`p.data.copy_()`, `p.data.mul_()`, ...)."""
        for conv in self.convs:
            conv.invalidate_caches()
        ops.invalidate_param_caches()
        self._ag_state = None
        staging.drop(self)

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self.invalidate_caches()
        return out

    def train(self, mode=True):
        """model.train() / model.eval() (once per epoch in the reference's loops): also the point where the whole-model path for
        tiny graphs reads its deferred edge_index checks (tiny._poll_status): a node id outside [0, n) seen by an earlier forward
        raises ValueError here at the latest (DIFFORMER_DEBUG=1: at the offending call)."""
        tiny._poll_status(wait=True)
        return super().train(mode)

    def load_state_dict(self, *args, **kwargs):
        out = super().load_state_dict(*args, **kwargs)
        self.invalidate_caches()
        return out

    def set_row_shard(self, shard):
        """Multi-GPU: `shard` (dist.RowShard) says which contiguous block of node rows this rank
        holds; forward() then takes the LOCAL rows of x and the GLOBAL edge_index."""
        for conv in self.convs:
            conv.row_shard = shard
        return self

    def _input_layer(self, x, training):
        bn = self.bns[0] if self.use_bn else None                     # :188-191 in one kernel
        x = ag.linear(x, self.fcs[0].weight, self.fcs[0].bias, *_ln_args(bn), relu=True)
        return F.dropout(x, p=self.dropout, training=training)

    def _single_copy(self, x, hidden, csr):
        """True when every reader of the hidden rows in this forward is a closed-form layer kernel over the same dense graph,
        so that the rows may exist ONCE, as the slice-major copy the sliced product reads (ops.LayerChain.single_copy; the
        layers choose per call).  That needs: inference; every layer on the `closed_narrow` route at hidden -> hidden with
        the graph term, without use_source (layer_[0] would have to exist row-major) and without a row shard; the background
        coefficient chain (it reads the rows beside the product); a graph whose rows can be recovered from the copy
        (GraphCSR.row_scale: every node has an incoming entry); neither DIFFORMER_SINGLE_COPY=0 nor DIFFORMER_EXACT_FP32=1."""
        if (not ops.SINGLE_COPY or not ops.SIDE_CHAIN or ops.EXACT_FP32 or self.training or not len(self.convs) or
                not hasattr(ops.get_backend(), "coeffs_bg")):
            return False
        probe = x.new_empty(1).expand(x.shape[0], hidden)               # what the route looks at: shape, dtype, no gradient
        for i, conv in enumerate(self.convs):
            if conv.use_source or not conv.use_graph or conv.row_shard is not None or conv.out_channels != hidden:
                return False
            ln = _ln_args(self.bns[i + 1] if self.use_bn else None)
            if conv._route(probe, probe, None, None, probe if self.residual else None, ln[0], ln[1], False) != "closed_narrow":
                return False
        return csr.row_scale() is not None

    def _input_with_products(self, x, edge_index, edge_weight, conv0):
        """Narrow input features in front of a closed-form first layer on a dense graph (BASELINE config C4: 8 -> 64): the
        input layer's kernel also leaves the Gram record of its output and the slice-major copy the sliced product reads
        (dif_input_gram_f32), so the hidden rows are written once and never read back before the product.
        -> (h, products for ops.simple_layer_closed_form) or None when the shapes / flags take the separate kernels."""
        if (self.training or conv0 is None or edge_index is None or edge_weight is not None or not conv0.use_graph or
                conv0.row_shard is not None or conv0.kernel != 'simple' or conv0.num_heads != 1 or not self.use_bn or
                x.dim() != 2 or x.dtype != torch.float32 or not x.is_cuda or x.shape[1] > 64):
            return None
        fc, bn = self.fcs[0], self.bns[0]
        hidden = fc.weight.shape[0]
        if hidden > 64 or hidden % 4 or conv0.out_channels != hidden or fc.weight.dtype != torch.float32:
            return None
        be = ops.get_backend()
        if not hasattr(be, "input_gram"):
            return None
        if ag._needs_grad(x, fc.weight, fc.bias, bn.weight, bn.bias, *conv0._qkv_list()):
            return None
        csr = ops.csr_cache.get(edge_index, None, x.shape[0], hidden * 4)
        sl = sliced.rows_format(csr, x.dtype, x.shape[0], hidden)
        if sl is None:
            return None
        if self._single_copy(x, hidden, csr):                  # the hidden rows are left as the slice-major copy alone
            _, record, ys = be.input_gram(x, fc.weight, fc.bias, bn.weight, bn.bias, bn.eps, True, csr.rowptr, sl.plan, rows=False)
            h = ops.rows_stand_in(ys, x.shape[0], hidden)
            return h, dict(x=h, sl=sl, record=record, ys=ys, rscale=csr.row_scale())
        h, record, ys = be.input_gram(x, fc.weight, fc.bias, bn.weight, bn.bias, bn.eps, True, csr.rowptr, sl.plan)
        return h, dict(x=h, sl=sl, record=record, ys=ys)

    # ---- repeated inference forwards over the same operands replay as ONE hipGraph -------------------------------------
    def _graph_key(self, x, edge_index, edge_weight):
        """Identity of everything a captured forward has baked in, or None when this call must run eagerly."""
        if self.training or torch.is_grad_enabled() or not self.auto_graph or not _AUTO_GRAPH:
            return None
        be = ops._BACKEND
        if (be is None or getattr(be, "kernel_events", None) is not None or not x.is_cuda or x.dim() != 2 or
                torch.cuda.is_current_stream_capturing()):
            return None
        # everything the capture bakes in: the operands, the model's and every layer's flags, and the parameters as they are
        # NOW (walked afresh through the registration dicts -- plain dict reads, this runs on every replayed call -- so a
        # module swapped in after the first call does not leave a stale list behind)
        mods = self._modules
        convs = mods["convs"]._modules.values()
        hidden = mods["fcs"]._modules["0"].weight.shape[0]
        nnz = edge_index.shape[1] if edge_index is not None else 0
        if len(convs) * (4.0 * x.shape[0] * hidden * x.element_size() + 8.0 * nnz) > _AUTO_GRAPH_MAX_BYTES:
            return None                  # GPU-bound: nothing to gain from a replay, gigabytes to hold for it
        key = [x.data_ptr(), x.shape, x.stride(), x.dtype, torch.cuda.current_stream(x.device).cuda_stream,
               self.alpha, self.use_bn, self.residual, ops.SIDE_CHAIN, ops.EXACT_FP32, ops.SINGLE_COPY, len(convs)]
        lin = []
        for m in mods["fcs"]._modules.values():
            lin.append(m)
        for m in mods["bns"]._modules.values():
            lin.append(m)
        for c in convs:
            if c.row_shard is not None:
                return None
            key.append((id(c), c.kernel, c.use_graph, c.use_weight, c.use_source, c.graph_weight, c.num_heads, c.out_channels))
            lin.extend(c._modules.values())              # Wk, Wq (, Wv)
        key.append(tensor_key(edge_index))
        key.append(tensor_key(edge_weight))
        for m in lin:
            for p in m._parameters.values():
                key.append(tensor_key(p))
        return tuple(key)

    def _forward_graphed(self, x, edge_index, edge_weight):
        """A Cora-sized forward is a dozen kernels of a few microseconds and ~0.2 ms of Python: launch-bound.  Every C-ABI
        entry point only enqueues on the stream it is given, so the whole forward can be captured once and replayed with one
        launch.  The third consecutive eval / no_grad call with the SAME operands (x at the same address and shape, the same
        edge_index / edge_weight tensors, unchanged parameters) captures it; later calls replay and return a copy of the
        captured output.  The graph reads x, the graph tensors and the parameters in place, so new VALUES at the same
        addresses are seen; anything else (another shape, another tensor, an optimiser step, train mode, gradients, a row
        shard, a flag of the model or of a layer flipped, a sub-module replaced) runs eagerly and drops the capture.
        Derived caches (concatenated projections, weight-only factors, float32 copies of bfloat16 parameters) are frozen
        into the capture; they are keyed on the same parameter versions as the capture itself.  The capture keeps a private
        memory pool with every intermediate of one forward for as long as it lives (about a second forward's worth of HBM),
        so only launch-bound forwards are captured (`_AUTO_GRAPH_MAX_BYTES`: the ogbn-proteins graph and the full Pokec graph
        run kernel by kernel) and a capture whose key no longer matches is dropped, pool included, at the next call.
        DIFFORMER_AUTO_GRAPH=0 or `model.auto_graph = False` turns it off;
        `invalidate_caches()` drops it (needed after parameter writes through `.data`, as for the other caches)."""
        key = self._graph_key(x, edge_index, edge_weight)
        if key is None:
            return None
        st = self._ag_state
        # the key of a freed graph tensor can come back with a NEW tensor: weak references tell the tensors the capture was
        # made for from look-alikes (tensor_cache)
        if st is None or st[0] != key or not same_tensors(st[5], (edge_index, edge_weight)):
            refs = weak_refs((edge_index, edge_weight))
            self._ag_state = [key, 1, None, None, None, refs]        # key, calls seen, graph, static output, CSR refs, tensors
            return None
        if st[2] is None:
            st[1] += 1
            if st[1] < 3:
                return None
            be = ops._BACKEND
            pins = []
            try:
                be.capture_pins = pins      # packed weight buffers the captured kernels read: kept alive with the capture
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    out = self._forward_eager(x, edge_index, edge_weight)
            except Exception as e:          # something in this configuration cannot be captured: stay eager for good
                self.auto_graph = False
                self._ag_state = None
                import warnings
                warnings.warn(f"difformer_amd: hipGraph capture of the forward failed ({e}); running eagerly")
                return None
            finally:
                be.capture_pins = None
            # the captured kernels hold raw pointers into the cached CSR / formats: they live as long as the capture
            st[2], st[3] = graph, out
            st[4] = (ops.csr_cache.values() if edge_index is not None else []) + pins
        st[2].replay()
        return st[3].clone()

    def forward(self, x, edge_index, edge_weight=None):
        dev = staging.staging_device(self, (x, edge_index, edge_weight))
        if dev is not None:      # model and operands in host memory (test_large_dataset.py:91-93, eval.py:38-41)
            return staging.staged_forward(self, dev, lambda m, *a: m.forward(*a), x, edge_index, edge_weight)
        out = tiny.forward(self, x, edge_index, edge_weight)      # tiny graphs (spatial-temporal/): the whole model in one launch
        if out is not None:
            return out
        out = self._forward_graphed(x, edge_index, edge_weight)
        return out if out is not None else self._forward_eager(x, edge_index, edge_weight)

    def forward_snapshots(self, batch, *, _uniforms=None):
        """The rows of `self(x_b, edge_index_b, edge_weight_b)` for every snapshot b of a `SnapshotBatch`, stacked: on tiny graphs
        ONE launch of one workgroup per snapshot and ONE autograd node (difformer_amd/snapshots.py); a plain loop otherwise."""
        from . import snapshots
        return snapshots.forward_snapshots(self, batch, _uniforms=_uniforms)

    def _forward_eager(self, x, edge_index, edge_weight=None):
        layer_ = []
        # A graph with community structure (every row's entries in one or two source tiles) runs in a mixed node order:
        # x is permuted once here, the logits once at the end, everything in between sees the relabelled graph
        mix = None
        conv0 = self.convs[0] if len(self.convs) else None
        if (conv0 is not None and conv0.use_graph and edge_index is not None and edge_weight is None and conv0.row_shard is None
                and x.dtype == torch.float32 and x.is_cuda):
            # columns the aggregation runs on: the value tensor [n, H, D] (or the layer input itself without Wv)
            width = conv0.out_channels * (conv0.num_heads if conv0.use_weight else 1)
            mix = ops.mix_cache.get(edge_index, x.shape[0], width)
        if mix is not None:
            x, edge_index = x[mix.perm], mix.edge_index
        # closed-form layers write the slice-major copy of their output (the next layer's SpMM operand) from their registers
        carry = ops.LayerChain()
        first = self._input_with_products(x, edge_index, edge_weight, conv0)
        if first is not None:                                  # :188-192 and the first layer's Gram record / SpMM operand
            x, carry.products = first
            carry.single_copy = carry.products.get("rscale") is not None
        else:
            x = self._input_layer(x, self.training)            # difformer.py:188-192
        layer_.append(x)
        for i, conv in enumerate(self.convs):
            bn = self.bns[i + 1] if self.use_bn else None
            carry.want_next = (not self.training) and i + 1 < len(self.convs)
            # the last closed-form layer applies the output Linear (:208) to its rows in the same pass (inference)
            last = i + 1 == len(self.convs)
            fc = self.fcs[-1]
            carry.head = (fc.weight, fc.bias) if (last and not self.training and not ops.EXACT_FP32 and
                                                  not ag._needs_grad(x, fc.weight, fc.bias)) else None
            # head mean, + layer_[0] (use_source), alpha-residual, LayerNorm ride in the last kernel of the
            # layer (:137-140, :200-203)
            x, _, _ = conv._layer(x, x, edge_index, edge_weight, layer_[0] if conv.use_source else None,
                                  layer_[i] if self.residual else None, self.alpha, *_ln_args(bn), carry=carry)
            if self.training:
                x = F.dropout(x, p=self.dropout, training=True)
            layer_.append(x)
        self.last_single_copy = carry.single           # layer kernels of this forward that read the slice-major copy (0: two-copy path)
        out = x if carry.head_done else ag.linear(x, self.fcs[-1].weight, self.fcs[-1].bias)   # :208
        return out[mix.inv] if mix is not None else out

    def get_attentions(self, x):
        """Dense per-layer attention [layers, N, N, H] (difformer.py:211-226; no graph term,
        as in the reference, which passes no edge_index here)."""
        dev = staging.staging_device(self, (x,))
        if dev is not None:
            return staging.staged_forward(self, dev, lambda m, a: m.get_attentions(a), x)
        layer_, attentions = [], []
        x = self._input_layer(x, False)
        layer_.append(x)
        for i, conv in enumerate(self.convs):
            q, k, v = conv._project(x, x)
            attentions.append(_dense_attention(q, k, conv.kernel))
            v_att = v if v.shape[1] == conv.num_heads else v.expand(-1, conv.num_heads, -1).contiguous()
            c = full_attention_conv(q, k, v_att, conv.kernel)
            bn = self.bns[i + 1] if self.use_bn else None
            x = ag.layer_tail(c, None, layer_[i] if self.residual else None, self.alpha, *_ln_args(bn))
            layer_.append(x)
        return torch.stack(attentions, dim=0)

    def top_attentions(self, x, k):
        """Per layer, node and head the k keys a node attends to most: (values float32 [layers,N,H,k], indices int64
        [layers,N,H,k]) = the k largest entries of every row of `get_attentions(x)`, descending, ties to the lower node
        index -- from a sweep that never forms the [N, N] map (attention_maps.attention_topk), so it runs at the sizes
        where get_attentions cannot.  Same layers as get_attentions (no graph term); outputs are detached."""
        from .attention_maps import attention_topk
        if any(conv.row_shard is not None for conv in self.convs):
            raise NotImplementedError("difformer_amd: top_attentions of a row-sharded model is not implemented (every rank "
                                      "holds the top-k over its own keys only)")
        dev = staging.staging_device(self, (x,))
        if dev is not None:      # model and x in host memory: the device twin's result, returned on the host
            twin = staging.twin_of(self, dev)
            twin.refresh(self)
            values, indices = twin.module.top_attentions(staging.operands.get(x, dev), k)
            return values.to(x.device), indices.to(x.device)
        with torch.no_grad():
            layer_, values, indices = [], [], []
            x = self._input_layer(x, False)
            layer_.append(x)
            for i, conv in enumerate(self.convs):
                q, kk, v = conv._project(x, x)
                val, idx = attention_topk(q, kk, conv.kernel, k)
                values.append(val)
                indices.append(idx)
                v_att = v if v.shape[1] == conv.num_heads else v.expand(-1, conv.num_heads, -1).contiguous()
                c = full_attention_conv(q, kk, v_att, conv.kernel)
                bn = self.bns[i + 1] if self.use_bn else None
                x = ag.layer_tail(c, None, layer_[i] if self.residual else None, self.alpha, *_ln_args(bn))
                layer_.append(x)
            return torch.stack(values, dim=0), torch.stack(indices, dim=0)

    def edge_attentions(self, x, edge_index, mass=False):
        """Per layer the attention ON THE EDGES of a graph: float32 [layers,E,H] with
        `edge_attentions(x, ei)[l, e, h] == get_attentions(x)[l, ei[1, e], ei[0, e], h]` (row 0 of edge_index the source = key,
        row 1 the target = query, as gcn_conv reads it), in the caller's edge order; mass=True: -> (that, float32 [layers,N,H]),
        per node the sum over its in-edges -- the share of its attention row that lies on the graph.  One dot product per
        edge (attention_maps.attention_on_edges): nothing of size N x N exists.  Same layers as get_attentions (no graph term
        in the propagation, as in the reference); outputs are detached."""
        from .attention_maps import _check_edges, attention_on_edges
        if any(conv.row_shard is not None for conv in self.convs):
            raise NotImplementedError("difformer_amd: edge_attentions of a row-sharded model is not implemented (a rank holds "
                                      "the key rows of its own shard only)")
        _check_edges(edge_index)
        dev = staging.staging_device(self, (x, edge_index))
        if dev is not None:      # model and operands in host memory: the device twin's result, returned on the host
            twin = staging.twin_of(self, dev)
            twin.refresh(self)
            out = twin.module.edge_attentions(staging.operands.get(x, dev), staging.operands.get(edge_index, dev), mass)
            return tuple(o.to(x.device) for o in out) if mass else out.to(x.device)
        with torch.no_grad():
            layer_, values, masses = [], [], []
            csr = [None]                                       # one CSR of the edge list for all layers: built by the first
            x = self._input_layer(x, False)
            layer_.append(x)
            for i, conv in enumerate(self.convs):
                q, kk, v = conv._project(x, x)
                v_att = v if v.shape[1] == conv.num_heads else v.expand(-1, conv.num_heads, -1).contiguous()
                den = None
                if conv.kernel == "sigmoid" and q.dtype == torch.float32:
                    # ONE forward: its output is the layer's, its row sums the denominators of the map
                    c, den = ops.get_backend().sigmoid_attention(q, kk, v_att, want_den=True)
                else:
                    c = full_attention_conv(q, kk, v_att, conv.kernel)
                out = attention_on_edges(q, kk, conv.kernel, edge_index, mass, _den=den, _csr=csr)
                values.append(out[0] if mass else out)
                if mass:
                    masses.append(out[1])
                bn = self.bns[i + 1] if self.use_bn else None
                x = ag.layer_tail(c, None, layer_[i] if self.residual else None, self.alpha, *_ln_args(bn))
                layer_.append(x)
            values = torch.stack(values, dim=0)
            return (values, torch.stack(masses, dim=0)) if mass else values
