"""Autograd glue so the reference's unchanged training scripts (`main.py:130` loss.backward())
keep working: the FORWARD of every operator is the HIP kernel; the BACKWARD of the simple and the sigmoid
attention, the aggregation (adjoint product on the same SpMM kernels), the layer tail (LayerNorm / residual /
head mean) and the weight gradients of the Linear layers are HIP kernels too;
the batched (v2) attentions too (simple: raw mode of the forward kernel; sigmoid: the sweep kernels per position group); only
heads wider than 512 columns re-derive their gradient on the device with tensor ops.
Under torch.no_grad() / eval these wrappers are pass-throughs to ops.py.  Nothing here touches the CPU.
"""
from __future__ import annotations

import torch

from . import ops


def _needs_grad(*tensors):
    return torch.is_grad_enabled() and any(t is not None and getattr(t, "requires_grad", False) for t in tensors)


def _sharded(shard):
    return shard if (shard is not None and shard.world > 1) else None


class _AllReduceSum(torch.autograd.Function):
    """y = sum over ranks of x, every rank gets y.  With L = sum over ranks of the local losses, dL/dx on a rank is the
    sum over ranks of their dL_r/dy: the backward is the same collective on the gradient."""

    @staticmethod
    def forward(ctx, x, shard):
        ctx.shard = shard
        return shard.all_reduce_sum(x.detach().clone().contiguous())

    @staticmethod
    def backward(ctx, g):
        return ctx.shard.all_reduce_sum(g.contiguous().clone()), None


def _own_rows_of_sum(shard, t):
    """Every rank holds a partial [n_global, ...] gradient of gathered rows: sum over ranks, keep this rank's rows.
    (all-reduce + slice rather than reduce-scatter: the blocks may be uneven, and gloo has no reduce-scatter.)"""
    return shard.local_rows(shard.all_reduce_sum(t.contiguous())).contiguous()


def _grad_by_recompute(fn, inputs, grad_out):
    """d(fn)/d(inputs) . grad_out with fn expressed in differentiable device-side tensor ops."""
    leaves = [None if t is None else t.detach().requires_grad_(True) for t in inputs]
    with torch.enable_grad():
        out = fn(*leaves)
    live = [t for t in leaves if t is not None]
    grads = torch.autograd.grad(out, live, grad_out, allow_unused=True)
    it = iter(grads)
    return tuple(None if t is None else next(it) for t in leaves)


# ---- differentiable restatements used ONLY inside backward() --------------------------------------
def _simple_expr(q, k, v):
    s = 1.0 / (torch.linalg.vector_norm(q) * torch.linalg.vector_norm(k))
    ktv = torch.einsum("lhm,lhd->hmd", k, v)
    num = s * torch.einsum("nhm,hmd->nhd", q, ktv) + v.sum(dim=0)
    den = s * torch.einsum("nhm,hm->nh", q, k.sum(dim=0)) + q.shape[0]
    return num / den.unsqueeze(-1)


def _simple_expr_sharded(shard):
    """_simple_expr over a rank's rows: the sums over nodes are all-reduced (one record), N is the global count."""
    def fn(q, k, v):
        H, M, D = k.shape[1], k.shape[2], v.shape[2]
        rec = torch.cat([torch.einsum("lhm,lhd->hmd", k, v).reshape(-1), k.sum(dim=0).reshape(-1), v.sum(dim=0).reshape(-1),
                         (q * q).sum().reshape(1), (k * k).sum().reshape(1)])
        rec = _AllReduceSum.apply(rec, shard)
        ktv = rec[: H * M * D].reshape(H, M, D)
        ksum = rec[H * M * D: H * M * D + H * M].reshape(H, M)
        vsum = rec[H * M * D + H * M: H * M * D + H * M + H * D].reshape(H, D)
        s = 1.0 / (torch.sqrt(rec[-2]) * torch.sqrt(rec[-1]))
        num = s * torch.einsum("nhm,hmd->nhd", q, ktv) + vsum
        den = s * torch.einsum("nhm,hm->nh", q, ksum) + shard.n_global
        return num / den.unsqueeze(-1)
    return fn


def _sigmoid_expr(q, k, v):
    s = torch.sigmoid(torch.einsum("nhm,lhm->nlh", q, k))
    return torch.einsum("nlh,lhd->nhd", s / s.sum(dim=1, keepdim=True), v)


def _tail_expr(alpha, eps, has_ln):
    def fn(conv, x0, prev, w, b):
        z = conv.mean(dim=1)
        if x0 is not None:
            z = z + x0
        if prev is not None:
            z = alpha * z + (1.0 - alpha) * prev
        if has_ln:
            z = torch.nn.functional.layer_norm(z, (z.shape[-1],), w, b, eps)
        return z
    return fn


class _SimpleAttention(torch.autograd.Function):
    """Forward and (for fp32, M, D <= 512: every head width of the reference's scripts) backward on the HIP kernels; other
    shapes re-derive the gradient with differentiable device ops."""

    @staticmethod
    def forward(ctx, q, k, v, shard=None):
        if q.shape[0] != v.shape[0] or k.shape[0] != v.shape[0]:
            # the kernels take the row count from q: L < N would read past the end of k / v (difformer.py:29 raises too)
            raise RuntimeError(f"simple kernel needs as many queries as sources (N={q.shape[0]}, L={v.shape[0]}; "
                               "difformer.py:29)")
        be = ops.get_backend()
        ctx.shard = shard = _sharded(shard)
        reduced = be.simple_reduce(q, k, v)
        if shard is not None:
            shard.all_reduce_sum(reduced)                      # the one exchange step of the forward
        out = be.simple_apply(q, reduced, shard.n_global if shard is not None else q.shape[0], v.shape[2])
        ctx.save_for_backward(q, k, v, reduced, out)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, reduced, out = ctx.saved_tensors
        hip_ok = (q.dtype == torch.float32 and q.shape[2] <= 512 and v.shape[2] <= 512 and q.shape[1] * q.shape[2] < 12000 and
                  hasattr(ops.get_backend(), "simple_backward"))
        if hip_ok:
            # row-sharded: two small all-reduces inside (the sums over nodes of the backward, then the scalar T)
            return ops.get_backend().simple_backward(q, k, v, reduced, out, g, ctx.shard) + (None,)
        expr = _simple_expr if ctx.shard is None else _simple_expr_sharded(ctx.shard)
        return _grad_by_recompute(expr, (q, k, v), g.contiguous()) + (None,)


class _SigmoidAttention(torch.autograd.Function):
    """Forward and (fp32, M, D <= 512) backward on the HIP kernels: the forward leaves the row sums, the backward
    recomputes sigma tile by tile (csrc/sigmoid_attn_bwd.hip up to 64 columns, csrc/sigmoid_wide.hip beyond).  Other shapes
    (bfloat16 storage, heads wider than 512) re-derive the gradient with tensor ops.
    Row-sharded: the key / value rows are all-gathered (queries stay local); their gradients are partial sums over the
    ranks' queries and come back as the sum over ranks of this rank's rows."""

    @staticmethod
    def forward(ctx, q, k, v, shard=None):
        be = ops.get_backend()
        ctx.shard = shard = _sharded(shard)
        if shard is not None:
            k, v = shard.all_gather_rows(k), shard.all_gather_rows(v)
        # heads up to 64 columns: the fp32 sweep kernels; 65 .. 512 (image and text/run.sh: hidden 300 / 400): the split-bfloat16
        # plane kernels of csrc/sigmoid_wide.hip -- not under ops.set_exact_fp32(True), where wide heads keep the tensor-op gradient
        width = max(q.shape[2], v.shape[2])
        ctx.hip = (q.dtype == torch.float32 and k.dtype == torch.float32 and v.dtype == torch.float32 and
                   (width <= 64 or (width <= 512 and not ops.EXACT_FP32)) and hasattr(be, "sigmoid_backward"))
        ctx.planes = ctx.hip and width > 64          # the backward may take the plane kernels -- while exact mode stays off
        if ctx.hip:
            out, den = be.sigmoid_attention(q, k, v, want_den=True)
            ctx.save_for_backward(q, k, v, out, den)
            return out
        ctx.save_for_backward(q, k, v)
        return be.sigmoid_attention(q, k, v)

    @staticmethod
    def backward(ctx, g):
        if ctx.hip:
            q, k, v, out, den = ctx.saved_tensors
            if ctx.planes and ops.EXACT_FP32:
                # ops.set_exact_fp32(True) between forward and backward: the split-bfloat16 planes are no longer allowed
                # (csrc/sigmoid_attn_bwd.hip refuses wide heads then) -- the tensor-op gradient of a forward made in exact mode
                dq, dk, dv = _grad_by_recompute(_sigmoid_expr, (q, k, v), g.contiguous())
            else:
                dq, dk, dv = ops.get_backend().sigmoid_backward(q, k, v, out, den, g)
        else:
            dq, dk, dv = _grad_by_recompute(_sigmoid_expr, ctx.saved_tensors, g.contiguous())
        if ctx.shard is not None:
            dk, dv = _own_rows_of_sum(ctx.shard, dk), _own_rows_of_sum(ctx.shard, dv)
        return dq, dk, dv, None


class _GcnAggregate(torch.autograd.Function):
    """edge_weight is an input only when the caller wants its gradient (the CSR values are built from it outside
    autograd); the product itself always runs on the cached CSR."""

    @staticmethod
    def forward(ctx, csr, x, attn, attn_scale, gcn_scale, shard=None, edge_weight=None):
        ctx.csr, ctx.attn_scale, ctx.gcn_scale, ctx.has_attn = csr, attn_scale, gcn_scale, attn is not None
        ctx.edges = csr.hold_edges() if (csr._adjoint is None or edge_weight is not None) else None
        ctx.shard = _sharded(shard)
        if edge_weight is not None:
            if ctx.shard is not None:
                raise NotImplementedError("difformer_amd: edge_weight gradients are single-GPU only")
            ctx.save_for_backward(x)
        return ops.gcn_aggregate(csr, x, attn, attn_scale, gcn_scale, ctx.shard)

    @staticmethod
    def backward(ctx, g):
        # adjoint product on the same SpMM kernels: grad_x = gcn_scale * A_hat^T g.  Row-sharded it is the forward
        # pattern again on the transposed CSR: all-gather the rows of g, product over this rank's (source) rows.
        g = g.contiguous()
        gx = gw = None
        if ctx.needs_input_grad[1]:
            gx = ops.gcn_aggregate(ctx.csr.adjoint(), g, None, 1.0, ctx.gcn_scale, ctx.shard)
        if ctx.needs_input_grad[6]:
            # d value_e = <g[col_e], x[row_e]>, chained through value = w * d_in * d_out and nan_to_num (difformer.py:73-74)
            (x,) = ctx.saved_tensors
            n = x.shape[0]
            gw = ops.get_backend().edge_weight_grad(ctx.edges[0], ctx.edges[1], ctx.csr.rowptr, n, g.reshape(n, -1),
                                                    x.reshape(n, -1), ctx.gcn_scale)
        return None, gx, (ctx.attn_scale * g if ctx.has_attn else None), None, None, None, gw


class _LayerTail(torch.autograd.Function):
    """Forward and backward are one HIP pass each (csrc/layer_tail.hip, csrc/layer_tail_bwd.hip); shapes the backward
    kernel does not cover (D % 4 != 0, D > 512, bf16 storage) re-derive the gradient with tensor ops."""

    @staticmethod
    def forward(ctx, conv, x0, prev, alpha, w, b, eps, relu):
        ctx.save_for_backward(conv, x0, prev, w, b)
        ctx.alpha, ctx.eps, ctx.relu = alpha, eps, bool(relu)
        return ops.layer_tail(conv, x0, prev, alpha, w, b, eps, relu)

    @staticmethod
    def backward(ctx, g):
        conv, x0, prev, w, b = ctx.saved_tensors
        need = ctx.needs_input_grad
        got = ops.get_backend().layer_tail_bwd(conv, x0, prev, ctx.alpha, w, b, ctx.eps, ctx.relu, g,
                                               (need[0], need[1], need[2]))
        if got is None:
            expr = _tail_expr(ctx.alpha, ctx.eps, w is not None)
            fn = (lambda *a: torch.relu(expr(*a))) if ctx.relu else expr
            got = _grad_by_recompute(fn, (conv, x0, prev, w, b), g.contiguous())
        return got[0], got[1], got[2], None, got[3], got[4], None, None


class _Linear(torch.autograd.Function):
    """x W^T + b on many rows.  The weight gradient g^T x contracts over the ROWS (K = n, a 64 x 192 result): the
    vendor GEMM takes ~0.3 ms for it at 132k rows; it is exactly stage 1 of the simple kernel (K^T V and sum K of
    difformer.py:25-28 with K = g, V = x), one streaming pass that also yields the bias gradient."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        # the narrow-Linear kernel keeps up to 256 output features per workgroup in LDS for C_in <= 64 (the fused q | k | v
        # projection 64 -> 192: one launch, x read once), 128 for C_in <= 128
        if bias is not None and ((x.shape[1] <= 64 and weight.shape[0] <= 256) or (x.shape[1] <= 128 and weight.shape[0] <= 64)):
            return ops.linear(x, weight, bias)
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = g @ weight
        if ctx.needs_input_grad[1] or (len(ctx.needs_input_grad) > 2 and ctx.needs_input_grad[2]):
            n, co = g.shape
            ci = x.shape[1]
            g3 = g.reshape(n, 1, co)
            red = ops.get_backend().simple_reduce(g3, g3, x.detach().reshape(n, 1, ci))     # one pass yields both
            if ctx.needs_input_grad[1]:
                gw = red[: co * ci].view(co, ci)
            if ctx.needs_input_grad[2]:
                gb = red[co * ci: co * ci + co]
        return gx, gw, gb


def _row_gemm(be, A, mat, bias=None, accumulate=None):
    """A mat (+ bias) (+ accumulate) on many rows: one pass on the row-GEMM kernel where the backend has it (K <= 512)."""
    got = be.row_gemm(A, mat, bias, accumulate) if hasattr(be, "row_gemm") else None
    if got is not None:
        return got
    out = A @ mat
    if bias is not None:
        out = out.add_(bias)
    return out if accumulate is None else out.add_(accumulate)


def _weighted_column_sum(be, rows, w):
    """sum_r w[r] rows[r, :] as K^T V of the streaming reduce with K = w (one column): the vendor GEMV on the transposed
    operand takes 0.9 ms for 132,534 x 64 floats, the reduce kernel reads the rows once."""
    n, c = rows.shape
    w3 = w.reshape(n, 1, 1)
    return be.simple_reduce(w3, w3, rows.reshape(n, 1, c))[:c]


class _ClosedFormLayer(torch.autograd.Function):
    """One DIFFormer layer with the `simple` kernel through the Gram record (ops.simple_layer_closed_form), under autograd:
    q, k, v are never formed, forward or backward.  With  att = (x Mn + cn) / (x u + cd)  and the coefficients
    (Mn, cn, u, cd) = f(G~, W~)  of the record  G~ = [x | 1]^T [x | 1]  (difformer.py:18-39):
        forward   Gram pass -> coefficients -> aggregation of x -> layer kernel (attention + graph term + tail)
        backward  tail (LayerNorm, residual, + x0)                  dif_layer_tail_bwd on the recomputed pre-tail rows
                  graph term  g_s (A x Wv^T + (A 1) bv^T)            d ax = d Wv, d Wv = d^T ax (one streaming reduce),
                                                                    d x += g_s A^T d ax (adjoint product)
                  attention   d num = d / den, d den = -<d num, att>  d x += d num Mn^T + d den u^T;
                              d Mn = x^T d num, d cn = sum d num (one streaming reduce), d u = x^T d den, d cd = sum d den
                  coefficients -> d G~, d W~                         ops.closed_form_coeffs_backward (C + 1 square matrices)
                  record      d x += x (dG + dG^T) + 1 d sx^T
    Single GPU, one head, query == source, float32, C, D <= 64 (DIFFormerConv._closed_form)."""

    @staticmethod
    def forward(ctx, x, Wq, bq, Wk, bk, Wv, bv, x0, ln_w, ln_b, csr, attn_scale, gcn_scale, residual, alpha, eps):
        keep = {}
        out = ops.simple_layer_closed_form(x, Wq, bq, Wk, bk, Wv, bv, csr, attn_scale, gcn_scale, x0, residual, alpha, ln_w,
                                           ln_b, eps, keep=keep)
        ctx.save_for_backward(x, Wq, bq, Wk, bk, Wv, bv, x0, ln_w, ln_b, keep["record"], keep["coef"], keep["ax"],
                              keep["row_sums"])
        ctx.csr, ctx.scales, ctx.tail = csr, (float(attn_scale), float(gcn_scale)), (bool(residual), float(alpha), float(eps))
        # the adjoint CSR is built from the edge list on first use (in backward): keep the caller's tensors alive until then
        ctx.edges = csr.hold_edges() if (csr is not None and csr._adjoint is None) else None
        return out

    @staticmethod
    def backward(ctx, g):
        x, Wq, bq, Wk, bk, Wv, bv, x0, ln_w, ln_b, record, coef, ax, rs = ctx.saved_tensors
        (a_s, g_s), (residual, alpha, eps), csr = ctx.scales, ctx.tail, ctx.csr
        be = ops.get_backend()
        n, C = x.shape
        D = Wq.shape[0]
        g = g.contiguous()
        # tail: the pre-tail rows come out of the layer kernel once more (no tail), then one backward pass
        conv = be.simple_layer(x, coef, D, ax, Wv, bv, rs, g_s).view(n, 1, D)
        prev = x if residual else None
        want = (True, x0 is not None and ctx.needs_input_grad[7], residual)
        got = be.layer_tail_bwd(conv, x0, prev, alpha, ln_w, ln_b, eps, False, g, want)
        if got is None:
            got = _grad_by_recompute(_tail_expr(alpha, eps, ln_w is not None), (conv, x0, prev, ln_w, ln_b), g)
        d, d_x0, dx, d_lnw, d_lnb = got
        d = d.reshape(n, D)
        del conv
        # graph term
        d_Wv = d_bv = None
        need_rs_d = False
        if csr is not None:
            if Wv is not None:
                d_ax = _row_gemm(be, d, Wv)
                d3 = d.view(n, 1, D)
                red = be.simple_reduce(d3, d3, ax.view(n, 1, C))                    # K^T V with K = d, V = ax
                d_Wv = red[: D * C].view(D, C).clone()
                need_rs_d = True                      # d_bv of this branch = g_s rs^T d: from the attention pass below
            else:
                d_ax = d
            # g_s A^T d_ax, added to what dx already holds in the product's epilogue (its `attn` operand)
            dx = ops.gcn_aggregate(csr.adjoint(), d_ax.reshape(n, 1, C), None if dx is None else dx.reshape(n, 1, C), 1.0, g_s,
                                   None).reshape(n, C)
            del d_ax
        # attention term
        MnT, cn = coef[: D * C].view(D, C), coef[D * C: D * C + D]
        u, cd = coef[D * C + D: D * C + D + C], coef[D * C + D + C]
        got = (be.closed_form_attn_backward(x, coef, D, d, dx, rs if need_rs_d else None)
               if hasattr(be, "closed_form_attn_backward") else None)
        d_u = d_cd = None
        if got is not None:                           # one pass (csrc/simple_layer.hip): also x^T d_den, sum d_den, rs^T d
            d_num, d_den, dx, d_u, d_cd, rs_d = got
            if need_rs_d:
                d_bv = g_s * rs_d
        else:
            if need_rs_d:
                d_bv = g_s * _weighted_column_sum(be, d, rs)
            att = be.simple_layer(x, coef, D)                                       # (x Mn + cn) / (x u + cd)
            den = torch.mul(x, u).sum(dim=1).add_(cd)
            d_num = d / den[:, None]
            d_den = (d_num * att).sum(dim=1).neg_()
            del att, den
            dx = torch.mm(d_num, MnT) if dx is None else dx.addmm_(d_num, MnT)
            dx.addr_(d_den, u)
        dn3 = d_num.view(n, 1, D)
        red = be.simple_reduce(dn3, dn3, x.view(n, 1, C))                           # K^T V = d_num^T x, sum K = sum d_num
        # red = [d_num^T x: D x C][sum d_num: D][...]: with d u and d cd written behind them it IS the gradient of coef
        red[D * C + D: D * C + D + C] = d_u if d_u is not None else _weighted_column_sum(be, x, d_den)
        if d_cd is not None:
            red[D * C + D + C] = d_cd
        else:
            torch.sum(d_den, dim=0, out=red[D * C + D + C])
        if hasattr(be, "simple_coeffs_backward"):
            S, t, d_Wq, d_bq, d_Wk, d_bk, d_Wv_a, d_bv_a = be.simple_coeffs_backward(record, n, C, D, Wq, bq, Wk, bk, Wv, bv,
                                                                                     a_s, coef, red)
        else:
            S, t, d_Wq, d_bq, d_Wk, d_bk, d_Wv_a, d_bv_a = ops.closed_form_coeffs_backward(
                record, n, C, D, Wq, bq, Wk, bk, Wv, bv, a_s, red[: D * C].view(D, C), red[D * C: D * C + D],
                red[D * C + D: D * C + D + C], red[D * C + D + C])
        dx = _row_gemm(be, x, S, t, dx)                                             # dx + x S + 1 t^T in one pass
        if Wv is not None:
            d_Wv = d_Wv_a if d_Wv is None else d_Wv.add_(d_Wv_a)
            d_bv = d_bv_a if d_bv is None else d_bv.add_(d_bv_a)
        return dx, d_Wq, d_bq, d_Wk, d_bk, d_Wv, d_bv, d_x0, d_lnw, d_lnb, None, None, None, None, None, None


def closed_form_layer(x, Wq, bq, Wk, bk, Wv, bv, csr, attn_scale, gcn_scale, x0, residual, alpha, ln_weight, ln_bias, eps):
    return _ClosedFormLayer.apply(x, Wq, bq, Wk, bk, Wv, bv, x0, ln_weight, ln_bias, csr, attn_scale, gcn_scale, residual,
                                  alpha, eps)


def _adjacent_columns(grads, n, sizes):
    """The contiguous [n, sum(sizes)] tensor whose column blocks the gradients are, or None.  backend.simple_backward writes
    dq | dk | dv as views of one such buffer; a slice whose gradient was accumulated with another consumer's (v also feeds the
    aggregation: autograd hands over a new tensor for dv) is copied into its block -- a third of the concatenation."""
    base = None
    for g in grads:
        b = None if g is None else g._base
        if (b is not None and getattr(b, "_difformer_fused_grad", False) and b.dim() == 2 and tuple(b.shape) == (n, sum(sizes))
                and b.is_contiguous()):      # the tag: never a tensor that autograd or the caller owns (retain_grad, hooks)
            base = b
            break
    if base is None:
        return None
    off, fill = base.storage_offset(), []
    for g, w in zip(grads, sizes):
        if g is None or g.dim() != 2 or tuple(g.shape) != (n, w) or g.dtype != base.dtype or g.device != base.device:
            return None
        in_place = g._base is base and g.stride() == (base.stride(0), 1) and g.storage_offset() == off
        if not in_place:
            if g._base is base:          # another view of the same buffer: not the layout this shortcut is for
                return None
            fill.append((off - base.storage_offset(), w, g))
        off += w
    if len(fill) == len(sizes):
        return None
    for o, w, g in fill:
        base[:, o: o + w].copy_(g)
    return base


class _SplitColumns(torch.autograd.Function):
    """q | k | v as column slices of the fused projection [n, (2|3) H D].  Plain slicing would have autograd build one
    zero-filled [n, 3 H D] buffer per slice gradient and add them up (three fills, three copies, two adds of 102 MB at
    C4); the gradients of the slices are simply the columns of the gradient, so backward is one concatenation."""

    @staticmethod
    def forward(ctx, t, *sizes):
        ctx.sizes, ctx.n = sizes, t.shape[0]
        return tuple(t.split(list(sizes), dim=1))

    @staticmethod
    def backward(ctx, *grads):
        whole = _adjacent_columns(grads, ctx.n, ctx.sizes)
        if whole is not None:            # the backward kernels wrote the slices side by side already (backend.simple_backward)
            return (whole,) + (None,) * len(ctx.sizes)
        ref = next(g for g in grads if g is not None)
        parts = [g if g is not None else ref.new_zeros((ctx.n, w)) for g, w in zip(grads, ctx.sizes)]
        return (torch.cat(parts, dim=1),) + (None,) * len(ctx.sizes)


def split_columns(t, *sizes):
    if _needs_grad(t):
        return _SplitColumns.apply(t, *sizes)
    return t.split(list(sizes), dim=1)


def _row_linear(x, weight, bias):
    # up to 512 columns either way (hidden 128: the fused q | k | v projection 128 -> 384): torch's own backward of F.linear
    # forms g^T x on a library GEMM that contracts over the rows -- 505 us for 100,000 x 384 x 128 against 159 us for the
    # streaming reduce of _Linear.backward, bias gradient included (scripts/exp_linear_dx.py)
    ok = (x.dim() == 2 and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.shape[0] >= 1024
          and x.shape[1] <= 512 and weight.shape[0] <= 512 and bias is not None)
    return _Linear.apply(x, weight, bias) if ok else torch.nn.functional.linear(x, weight, bias)


# ---- public wrappers -----------------------------------------------------------------------------
def simple_attention(q, k, v, shard=None):
    if _needs_grad(q, k, v):
        return _SimpleAttention.apply(q, k, v, shard)
    return ops.simple_attention(q, k, v, shard)


def sigmoid_attention(q, k, v, shard=None):
    if _needs_grad(q, k, v):
        return _SigmoidAttention.apply(q, k, v, shard)
    return ops.sigmoid_attention(q, k, v, shard)


# ---- f4: batch of graphs (physical particle/difformer-v2.py:71-137) -------------------------------
def _pad(t, layout):
    """[N,H,D] -> [B, max_nodes, H, D] (zeros beyond each graph) -- backward-only helper."""
    ptr = layout.graph_ptr.long()
    batch = torch.repeat_interleave(torch.arange(layout.n_graphs, device=t.device), ptr[1:] - ptr[:-1])
    pos = torch.arange(layout.n_rows, device=t.device) - ptr[:-1][batch]
    out = t.new_zeros((layout.n_graphs, layout.max_nodes) + tuple(t.shape[1:]))
    out[batch, pos] = t
    return out, batch, pos


def _batched_simple_expr(layout):
    def fn(q, k, v):
        s = 1.0 / (torch.linalg.vector_norm(q) * torch.linalg.vector_norm(k))
        qp, batch, pos = _pad(q, layout)
        kp, _, _ = _pad(k, layout)
        vp, _, _ = _pad(v, layout)
        ktv = torch.einsum("blhm,blhd->bhmd", kp, vp)
        num = s * torch.einsum("bnhm,bhmd->bnhd", qp, ktv) + vp.sum(dim=1, keepdim=True)
        n_b = (layout.graph_ptr[1:] - layout.graph_ptr[:-1]).to(q.dtype).view(-1, 1, 1)
        den = s * torch.einsum("bnhm,bhm->bnh", qp, kp.sum(dim=1)) + n_b
        return (num / den.unsqueeze(-1))[batch, pos]
    return fn


def _batched_sigmoid_expr(layout):
    def fn(q, k, v):
        qp, batch, pos = _pad(q, layout)
        kp, _, _ = _pad(k, layout)
        vp, _, _ = _pad(v, layout)
        sg = torch.sigmoid(torch.einsum("aphm,ephm->aeph", qp, kp))
        att = sg / (sg.sum(dim=1, keepdim=True) + 1e-9)
        return torch.einsum("aeph,ephd->aphd", att, vp)[batch, pos]
    return fn


class _BatchedAttention(torch.autograd.Function):
    """'simple' (fp32, widths up to 256, more than one graph): forward with the row denominators kept, backward as three
    launches of the forward kernel's raw mode (csrc/batched_attn.hip).  'sigmoid' (fp32, heads up to 64 wide): forward with
    the full denominators kept, backward on the sweep kernel of csrc/sigmoid_attn_bwd.hip with the position groups' row
    mapping.  Other shapes re-derive the gradient with tensor ops on the padded batch."""

    @staticmethod
    def forward(ctx, q, k, v, layout, kernel):
        ctx.layout, ctx.kernel = layout, kernel
        be = ops.get_backend()
        ctx.hip = (kernel == "simple" and layout.n_graphs > 1 and hasattr(be, "batched_simple_backward") and
                   all(t.dtype == torch.float32 for t in (q, k, v)) and q.shape[2] <= 256 and v.shape[2] <= 256)
        if ctx.hip:
            ops._check_batch(q, k, v, layout)
            out, den, sumsq = be.batched_simple_attention(q, k, v, layout.graph_ptr, want_den=True)
            ctx.save_for_backward(q, k, v, out, den, sumsq)
            return out
        ctx.hip_sigmoid = (kernel == "sigmoid" and hasattr(be, "batched_sigmoid_backward") and
                           all(t.dtype == torch.float32 for t in (q, k, v)) and q.shape[2] <= 64 and v.shape[2] <= 64)
        if ctx.hip_sigmoid:
            ops._check_batch(q, k, v, layout)
            out, den = be.batched_sigmoid_attention(q, k, v, layout.ranked_first, layout.pos_count, want_den=True)
            ctx.save_for_backward(q, k, v, out, den)
            return out
        ctx.save_for_backward(q, k, v)
        fwd = ops.batched_simple_attention if kernel == "simple" else ops.batched_sigmoid_attention
        return fwd(q, k, v, layout)

    @staticmethod
    def backward(ctx, g):
        if ctx.hip:
            q, k, v, out, den, sumsq = ctx.saved_tensors
            return ops.get_backend().batched_simple_backward(q, k, v, out, den, sumsq, g, ctx.layout.graph_ptr) + (None, None)
        if getattr(ctx, "hip_sigmoid", False):
            q, k, v, out, den = ctx.saved_tensors
            return ops.get_backend().batched_sigmoid_backward(q, k, v, out, den, g, ctx.layout.ranked_first,
                                                              ctx.layout.pos_count) + (None, None)
        expr = _batched_simple_expr if ctx.kernel == "simple" else _batched_sigmoid_expr
        return _grad_by_recompute(expr(ctx.layout), ctx.saved_tensors, g.contiguous()) + (None, None)


def batched_attention(q, k, v, layout, kernel):
    if kernel not in ("simple", "sigmoid"):
        raise ValueError(f"unknown attention kernel {kernel!r} (expected 'simple' or 'sigmoid')")
    if _needs_grad(q, k, v):
        return _BatchedAttention.apply(q, k, v, layout, kernel)
    fwd = ops.batched_simple_attention if kernel == "simple" else ops.batched_sigmoid_attention
    return fwd(q, k, v, layout)


def gcn_aggregate(csr, x, attn=None, attn_scale=1.0, gcn_scale=1.0, shard=None):
    w = csr.weight_leaf()
    if w is not None or _needs_grad(x, attn):
        return _GcnAggregate.apply(csr, x, attn, attn_scale, gcn_scale, shard, w)
    return ops.gcn_aggregate(csr, x, attn, attn_scale, gcn_scale, shard)


def gcn_aggregate_tail(csr, x, attn, attn_scale, gcn_scale, shard, x0, prev, alpha, ln_weight, ln_bias, eps,
                       relu=False):
    """SpMM + combine + layer tail -> [n, D].  One fused kernel when nothing needs a gradient and the
    layer has a single head; otherwise the two operators run back to back."""
    d = x.shape[2]
    fused = (x.shape[1] == 1 and (d <= 64 or (d % 4 == 0 and d <= 256)) and
             not _needs_grad(x, attn, x0, prev, ln_weight, ln_bias) and csr.weight_leaf() is None)
    if fused:
        tail = dict(x0=x0, prev=prev, alpha=alpha, ln_weight=ln_weight, ln_bias=ln_bias, eps=eps, relu=relu)
        return ops.gcn_aggregate(csr, x, attn, attn_scale, gcn_scale, shard, tail)[:, 0, :]
    conv = gcn_aggregate(csr, x, attn, attn_scale, gcn_scale, shard)
    return layer_tail(conv, x0, prev, alpha, ln_weight, ln_bias, eps, relu)


def layer_tail(conv, x0=None, prev=None, alpha=0.5, ln_weight=None, ln_bias=None, eps=1e-5, relu=False):
    if _needs_grad(conv, x0, prev, ln_weight, ln_bias):
        return _LayerTail.apply(conv, x0, prev, alpha, ln_weight, ln_bias, eps, relu)
    return ops.layer_tail(conv, x0, prev, alpha, ln_weight, ln_bias, eps, relu)


def norm_relu(x, ln_weight, ln_bias, eps):
    """LayerNorm -> ReLU of the input layer (difformer.py:189-191) in one kernel when no gradient is needed."""
    if _needs_grad(x, ln_weight, ln_bias):
        return _LayerTail.apply(x.unsqueeze(1), None, None, 0.5, ln_weight, ln_bias, eps, True)
    return ops.layer_tail(x.unsqueeze(1), None, None, 0.5, ln_weight, ln_bias, eps, relu=True)


def linear(x, weight, bias, ln_weight=None, ln_bias=None, eps=1e-5, relu=False):
    """nn.Linear (-> LayerNorm) (-> ReLU).  Narrow inputs (C_in <= 128) and long rows into a narrow layer (C_in up to 8192 ->
    C_out <= 64: 512 -> 64 at CIFAR scale, 1,433 -> 64 on Cora) and wide rows into a wide layer (up to 832 -> 416: 512 -> 300 of
    the image scripts) run the fused HIP kernels when no gradient is needed; the rest uses the vendor GEMM (rocBLAS via F.linear) followed by the fused LayerNorm/ReLU kernel."""
    fn = torch.nn.functional
    grad = _needs_grad(x, weight, bias, ln_weight, ln_bias)
    # 65-128 input columns keep only 128 output features per workgroup in LDS: beyond that x is re-read per 128 features
    # and the vendor GEMM wins on big inputs (100,000 x 128 -> 256: 91 vs 68 us; -> 128: 46 vs 62 us;
    # scripts/exp_linear_wide_out.py); small inputs stay on the one-launch kernel (host-bound there)
    narrow_ok = x.dim() == 2 and (x.shape[1] <= 64 or weight.shape[0] <= 128 or x.shape[0] < 16384)
    if not grad and x.dim() == 2 and x.shape[1] <= 128 and narrow_ok and (ln_weight is None or weight.shape[0] <= 128):
        return ops.linear(x, weight, bias, ln_weight, ln_bias, eps, relu)
    if (not grad and x.dim() == 2 and 128 < x.shape[1] <= 8192 and weight.shape[0] <= 64 and bias is not None and
            (x.dtype == torch.float32 or (x.shape[1] % 4 == 0 and x.shape[0] >= 16384))):
        # float32: any row count and any width (Cora's 1,433 features: rows only 4-byte aligned) -- few or unaligned rows take
        # the kernel that splits K over the waves of a workgroup; bfloat16 storage: the chunked kernel's shapes only
        return ops.linear(x, weight, bias, ln_weight, ln_bias, eps, relu)
    if not grad and x.dim() == 2 and bias is not None and ops.linear_xwide_covers(x, weight):
        # wide rows into a wide layer (image and text/run.sh:27: 512 -> 300): the hidden-300 layer kernel with the two halves of
        # the input channels as its two accumulating products, LayerNorm / ReLU in the same pass
        return ops.linear(x, weight, bias, ln_weight, ln_bias, eps, relu)
    y = _row_linear(x, weight, bias) if grad else fn.linear(x, weight, bias)
    if ln_weight is not None:
        if grad:
            return _LayerTail.apply(y.unsqueeze(1), None, None, 0.5, ln_weight, ln_bias, eps, relu)
        return ops.layer_tail(y.unsqueeze(1), None, None, 0.5, ln_weight, ln_bias, eps, relu=relu)
    return torch.relu(y) if relu else y
