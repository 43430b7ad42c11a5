"""Every entry point of include/difformer_hip.h with its OPERANDS between NaN bands (tests/guarded.py).

The hot kernels issue raw loads from clamped addresses a step ahead and mask them where they are used; idle lanes of the
sliced product read "a zero row".  That is right only if every clamp and every mask is right in every instantiation, and a
missing one reads the neighbouring tensor -- in an ordinary test process another finite N(0, 1) array, which moves a norm-wise
error by little or nothing.  Here every tensor a call is handed, integer operands included, is copied into a block of its
own whose surroundings are 0xFF bytes: a float read outside [base, base + rows * ld) is NaN, an integer read is -1 (as a row
index: one row before its array, inside the leading band), and the NaN reaches the result.  Outputs and workspaces come
poisoned and guarded from the `poisoned_allocations` fixture, so intermediate results that one entry point hands to the next
sit between bands as well.  Each case runs twice: payloads 512-byte aligned, and at the minimum alignment the header
promises (16 bytes; 4 bytes for the rows of dif_linear_packed_f32).

Table: CASES = (name, entry points the case must launch, run(P, be) -> [(label, got, float64 reference, tolerance)]); P copies
CPU operands into guarded blocks.  References and tolerances are those of the existing tests of the same entry points
(oracle.difformer_oracle, the numpy restatements of tests/test_gpu_parity.py and tests/fake_backend.py): 1e-4 (float32) and
1e-2 (bfloat16 storage) norm-wise plus np.isfinite(out).all(); integer results exactly (tolerance 0).

Shapes: rows 1, T - 1 and T + 1 for the rows T of a workgroup -- waves per workgroup x the 16 rows of an MFMA tile, from the
kernel files' wave counts: 64 (simple_attn / simple_layer / project_reduce: 4 waves), 128 (row GEMM, xwide, packed linear,
sigmoid: 8 waves), 256 (simple_layer_wide, blocked SpMM: 16 waves) -- and widths from the lists of
tests/test_gpu_kernel_coverage.py (3, 7, 13, 30, 50, 70, 300 and each family's largest).  Paths that only dispatch from a
threshold run at that threshold: 8,192 nodes x 48 entries per row (sliced product), 16,384 rows (xwide / long-row Linear)."""
import re

import numpy as np
import pytest
import torch

from conftest import rel_err
from fake_backend import OracleBackend
from guarded import GuardedArena, guarded_inputs, poisoned_allocations  # noqa: F401
from oracle import difformer_oracle as orc
from sliced_format import schedule  # noqa: F401  (forces DIFFORMER_SLICED_SCHEDULE)

TOL, BF16_TOL = 1e-4, 1e-2
F32, BF16 = torch.float32, torch.bfloat16
FAKE = OracleBackend()

# Entry points with a pointer parameter that no case launches, and why.
LEFT_OUT = {
    "dif_sliced_plan": "host-side arithmetic only: `plan` is a host array of 8 ints, no device memory is touched",
}

CASES = []


def case(name, *symbols, min_align=16):
    def add(fn):
        CASES.append((name, symbols, fn, min_align))
        return fn
    return add


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(g, *shape, dt=F32, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(dt)


def _d(t):
    """exact float64 numpy value of a (CPU or device) tensor"""
    return t.detach().to(torch.float64).cpu().numpy()


def _tol(dt):
    return TOL if dt == F32 else BF16_TOL


def _graph(n, deg, seed, hubs=0):
    g = _g(seed)
    ei = torch.randint(0, n, (2, n * deg), generator=g)
    if hubs:
        q = ei.shape[1] // 4
        ei[1, :q] = torch.randint(0, hubs, (q,), generator=g) * (n // hubs)
    return torch.cat([ei, torch.arange(n).repeat(2, 1)], dim=1)


def _csr(ei, w, n, n_blocks=1, block_rows=0, transpose=False):
    """CPU CSR of the oracle in the backend's layout -> (rowptr, blkptr | None, src, val, nnz)"""
    rp, blk, src, val, _ = FAKE.csr_build(ei, w, n, n_blocks, transpose, block_rows)
    return rp, blk, src, val, int(src.numel())


# ================================================================== a1: simple attention in two stages
def _simple_record(q, k, v):
    return np.concatenate([np.einsum("lhm,lhd->hmd", k, v).ravel(), k.sum(0).ravel(), v.sum(0).ravel(), [(q * q).sum(), (k * k).sum()]])


def _simple_stages(P, be, dt, shapes):
    res = []
    for n, h, m, d, ld_pad in shapes:
        g = _g(n + m)
        q, k, v = _rn(g, n, h, m, dt=dt), _rn(g, n, h, m, dt=dt), _rn(g, n, h, d, dt=dt, shift=0.2)
        qd, kd, vd = P(q=(q, h * m + ld_pad) if ld_pad else q, k=k, v=v)
        rec = be.simple_reduce(qd, kd, vd)
        ref = _simple_record(_d(q), _d(k), _d(v))
        res.append((f"record n={n} m={m} d={d}", rec[: ref.size], ref, _tol(dt)))
        rec_in, = P(rec=torch.from_numpy(ref.astype(np.float32)))
        out = be.simple_apply(qd, rec_in, n + 5, d)
        res.append((f"apply n={n} m={m} d={d}", out, _d(FAKE.simple_apply(q.float(), rec_in.cpu(), n + 5, d)), _tol(dt)))
    return res


@case("simple_reduce_apply_f32", "dif_simple_reduce_f32", "dif_simple_apply_f32")
def _(P, be):
    return _simple_stages(P, be, F32, [(1, 2, 10, 7, 0), (63, 1, 64, 64, 4), (65, 3, 33, 65, 0), (65, 1, 70, 130, 0), (63, 1, 516, 13, 0)])


@case("simple_reduce_apply_bf16", "dif_simple_reduce_bf16", "dif_simple_apply_bf16")
def _(P, be):
    return _simple_stages(P, be, BF16, [(1, 2, 10, 7, 0), (63, 1, 64, 64, 8), (65, 3, 33, 65, 0), (65, 1, 70, 130, 0)])


def _project_reduce(P, be, dt):
    res = []
    for n, c, h, d in [(1, 20, 3, 10), (63, 64, 1, 64), (65, 30, 2, 33)]:
        g = _g(c + d + n)
        x = _rn(g, n, c, dt=dt)
        W = [_rn(g, h * d, c, dt=dt, scale=c ** -0.5) for _ in range(3)]
        b = [_rn(g, h * d, dt=dt, scale=0.3) for _ in range(3)]
        xd, *wb = P(x=x, Wq=W[0], bq=b[0], Wk=W[1], bk=b[1], Wv=W[2], bv=b[2])
        q, v, rec = be.project_reduce(xd, *wb, h, d)
        q64, k64, v64 = ((_d(x) @ _d(W[i]).T + _d(b[i])).reshape(n, h, d) for i in range(3))
        ktv = np.einsum("lhm,lhd->hmd", k64, v64)
        res += [(f"q n={n} c={c}", q, q64, _tol(dt)), (f"v n={n} c={c}", v, v64, _tol(dt)),
                (f"KtV n={n} c={c}", rec[: ktv.size], ktv.ravel(), _tol(dt))]
    return res


@case("project_reduce_f32", "dif_project_reduce_f32")
def _(P, be):
    return _project_reduce(P, be, F32)


@case("project_reduce_bf16", "dif_project_reduce_bf16")
def _(P, be):
    return _project_reduce(P, be, BF16)


def _simple_expr64(q, k, v):
    s = 1.0 / (q.norm() * k.norm())
    n = q.shape[0]
    num = s * torch.einsum("nhm,hmd->nhd", q, torch.einsum("lhm,lhd->hmd", k, v)) + v.sum(0)[None]
    den = s * torch.einsum("nhm,hm->nh", q, k.sum(0))[..., None] + n
    return num / den


@case("simple_backward", "dif_simple_bwd_prep_f32", "dif_rowgemm_f32", "dif_simple_reduce_f32")
def _(P, be):
    res = []
    for n, h, m in [(1, 1, 8), (127, 2, 30), (129, 1, 64), (129, 1, 70)]:
        g = _g(n + m)
        q, k, v, go = _rn(g, n, h, m), _rn(g, n, h, m), _rn(g, n, h, m, shift=0.2), _rn(g, n, h, m)
        l64 = [t.double().requires_grad_(True) for t in (q, k, v)]
        out64 = _simple_expr64(*l64)
        out64.backward(go.double())
        qd, kd, vd, gd, od = P(q=q, k=k, v=v, g=go, out=out64.detach().float())
        rec = be.simple_reduce(qd, kd, vd)
        grads = be.simple_backward(qd, kd, vd, rec, od, gd)
        gmax = max(float(t.grad.abs().max()) for t in l64)
        for nm, got, want in zip("qkv", grads, l64):
            res.append((f"d{nm} n={n} m={m}", _d(got) / gmax, _d(want.grad) / gmax, -TOL))
    return res


# ================================================================== a2: sigmoid attention
def _sigmoid_fwd(P, be, dt, shapes):
    res = []
    for n, l, h, m, d in shapes:
        g = _g(n + l + m)
        q, k, v = _rn(g, n, h, m, dt=dt, scale=3.0 / m ** 0.5), _rn(g, l, h, m, dt=dt, scale=0.5), _rn(g, l, h, d, dt=dt)
        qd, kd, vd = P(q=q, k=k, v=v)
        ref = orc.sigmoid_attention(_d(q), _d(k), _d(v))
        res.append((f"out N={n} L={l} m={m} d={d}", be.sigmoid_attention(qd, kd, vd), ref, _tol(dt)))
        if dt == F32:
            out, den = be.sigmoid_attention(qd, kd, vd, want_den=True)
            res.append((f"fwd out N={n} L={l} m={m}", out, ref, TOL))
            res.append((f"fwd den N={n} L={l} m={m}", torch.isfinite(den).all().reshape(1).float(), np.ones(1), TOL))
    return res


@case("sigmoid_attention_f32", "dif_sigmoid_attn_f32", "dif_sigmoid_attn_fwd_f32")
def _(P, be):
    return _sigmoid_fwd(P, be, F32, [(1, 129, 1, 30, 30), (127, 1, 2, 64, 64), (129, 777, 1, 7, 13), (33, 257, 1, 72, 72),
                                     (129, 31, 1, 300, 300), (17, 65, 1, 512, 512), (15, 33, 1, 517, 517)])


@case("sigmoid_attention_bf16", "dif_sigmoid_attn_bf16")
def _(P, be):
    return _sigmoid_fwd(P, be, BF16, [(1, 129, 1, 30, 30), (127, 1, 2, 64, 64), (129, 300, 1, 72, 72)])


@case("sigmoid_backward", "dif_sigmoid_attn_bwd_f32", "dif_sigmoid_attn_fwd_f32")
def _(P, be):
    res = []
    for n, l, m in [(1, 33, 30), (31, 1, 64), (129, 131, 13), (33, 31, 72), (17, 65, 300)]:
        g = _g(n + l + m)
        q, k, v, go = _rn(g, n, 1, m, scale=0.4), _rn(g, l, 1, m, scale=0.4), _rn(g, l, 1, m), _rn(g, n, 1, m)
        qd, kd, vd, gd = P(q=q, k=k, v=v, g=go)
        out, den = be.sigmoid_attention(qd, kd, vd, want_den=True)
        grads = be.sigmoid_backward(qd, kd, vd, out, den, gd)
        refs = orc.sigmoid_attention_grad_blocked(_d(q), _d(k), _d(v), _d(go))
        gmax = max(np.abs(r).max() for r in refs)
        for nm, got, want in zip("qkv", grads, refs):
            res.append((f"d{nm} N={n} L={l} m={m}", _d(got) / gmax, want / gmax, -TOL))
    return res


# ================================================================== f4: batches of graphs
def _layout(n_nodes, P):
    from difformer_amd import ops
    lay = ops.BatchLayout(torch.tensor(n_nodes), "cpu")
    return P(graph_ptr=lay.graph_ptr, ranked_first=lay.ranked_first, pos_count=lay.pos_count)


@case("batched_simple", "dif_batched_simple_attn_f32", "dif_batched_simple_attn_fwd_f32", "dif_batched_simple_raw_f32")
def _(P, be):
    from oracle import difformer_oracle_grad as og
    res = []
    for n_nodes, m, d in [([1, 7, 1, 20, 3], 50, 30), ([20, 1], 97, 35), ([1], 128, 128), ([5, 20, 20], 197, 37)]:
        n = sum(n_nodes)
        g = _g(n + m)
        q, k, v, go = _rn(g, n, 1, m), _rn(g, n, 1, m), _rn(g, n, 1, d), _rn(g, n, 1, d)
        gp, _, _ = _layout(n_nodes, P)
        qd, kd, vd, gd = P(q=q, k=k, v=v, g=go)
        l64 = [t.double().requires_grad_(True) for t in (q, k, v)]
        ref = og.v2_simple_attention(*l64, torch.tensor(n_nodes))
        ref.backward(go.double())
        res.append((f"out {n_nodes} m={m}", be.batched_simple_attention(qd, kd, vd, gp), _d(ref), TOL))
        out, den, sumsq = be.batched_simple_attention(qd, kd, vd, gp, want_den=True)
        res.append((f"fwd out {n_nodes} m={m}", out, _d(ref), TOL))
        grads = be.batched_simple_backward(qd, kd, vd, out, den, sumsq, gd, gp)
        gmax = max(float(t.grad.abs().max()) for t in l64)
        for nm, got, want in zip("qkv", grads, l64):
            res.append((f"d{nm} {n_nodes} m={m}", _d(got) / gmax, _d(want.grad) / gmax, -TOL))
    return res


@case("batched_sigmoid", "dif_batched_sigmoid_attn_f32", "dif_batched_sigmoid_attn_fwd_f32", "dif_batched_sigmoid_attn_bwd_f32")
def _(P, be):
    from oracle import difformer_oracle_grad as og
    res = []
    for n_nodes, m in [([1, 7, 1, 20, 3], 30), ([20, 1], 64), ([1], 13), ([3, 8, 8, 2], 72)]:
        n = sum(n_nodes)
        g = _g(n + m)
        q, k, v, go = _rn(g, n, 1, m, scale=0.4), _rn(g, n, 1, m, scale=0.4), _rn(g, n, 1, m), _rn(g, n, 1, m)
        _, rf, pc = _layout(n_nodes, P)
        qd, kd, vd, gd = P(q=q, k=k, v=v, g=go)
        l64 = [t.double().requires_grad_(True) for t in (q, k, v)]
        ref = og.v2_sigmoid_attention(*l64, torch.tensor(n_nodes))
        ref.backward(go.double())
        res.append((f"out {n_nodes} m={m}", be.batched_sigmoid_attention(qd, kd, vd, rf, pc), _d(ref), TOL))
        if m <= 64:
            out, den = be.batched_sigmoid_attention(qd, kd, vd, rf, pc, want_den=True)
            res.append((f"fwd out {n_nodes} m={m}", out, _d(ref), TOL))
            grads = be.batched_sigmoid_backward(qd, kd, vd, out, den, gd, rf, pc)
            # Per tensor norm-wise at 1e-4, as tests/test_gpu_kernel_coverage.py holds this entry point -- except in a batch
            # of ONE graph.  There every position scores against itself alone, the weight is s / (s + 1e-9) and out = v up
            # to 1e-9: the float64 dq and dk are 1e-9 of dv, while float32 forms them from g.v - g.out, a difference of two
            # sums of m products of size |g||v| whose rounding alone is m * 2^-24 * sum|g_i v_i| ~ 1e-6 of dv.  No float32
            # code (the reference's own float32 run included) resolves such a tensor to 1e-4 of ITSELF, so that batch is
            # held to 1e-4 of the step's largest gradient entry: the norm of the tests of dif_sigmoid_attn_bwd_f32, whose
            # arithmetic this is (test_threshold_widths_of_the_sigmoid_families, tests/test_gpu_parity.py).
            gmax = max(float(t.grad.abs().max()) for t in l64)
            for nm, got, want in zip("qkv", grads, l64):
                scale = gmax if len(n_nodes) == 1 else float(want.grad.abs().max())
                res.append((f"d{nm} {n_nodes} m={m}", _d(got) / scale, _d(want.grad) / scale, -TOL))
    return res


# ================================================================== a3: graph preparation (integer work: exact)
@case("csr_build", "dif_csr_build")
def _(P, be):
    res = []
    for n, deg, weighted, nb, transpose in [(1, 3, False, 1, False), (255, 5, True, 1, False), (257, 5, False, 3, False),
                                            (257, 9, True, 3, True), (1000, 1, True, 1, True)]:
        ei = _graph(n, deg, n + nb)
        w = torch.rand(ei.shape[1], generator=_g(n)) + 0.5 if weighted else None
        eid, wd = P(edge_index=ei, edge_weight=w)
        rp, blk, src, val, longest = be.csr_build(eid, wd, n, nb, transpose)
        r_rp, r_blk, r_src, r_val, e = _csr(ei, w, n, nb, 0, transpose)
        tag = f"n={n} nb={nb} w={weighted} t={transpose}"
        res += [(f"rowptr {tag}", rp, r_rp.numpy(), 0), (f"src {tag}", src[:e], r_src.numpy(), 0),
                (f"val {tag}", val[:e].view(torch.int32), r_val.numpy().view(np.int32), 0),
                (f"longest {tag}", torch.tensor([longest]), np.diff(r_rp.numpy()).max(keepdims=True), 0)]
        if nb > 1:
            res.append((f"blkptr {tag}", blk, r_blk.numpy(), 0))
    return res


@case("subgraph", "dif_subgraph")
def _(P, be):
    res = []
    for n, e, bsz in [(100, 63, 50), (100, 65, 7), (500, 4097, 499), (500, 4095, 1)]:
        g = _g(n + e)
        ei, w, subset = torch.randint(0, n, (2, e), generator=g), torch.rand(e, generator=g), torch.randperm(n, generator=g)[:bsz]
        sd, eid, wd = P(subset=subset, edge_index=ei, edge_weight=w)
        ref, ref_w = orc.subgraph(subset.numpy(), ei.numpy(), w.numpy(), relabel_nodes=True, num_nodes=n)
        out, ow = be.subgraph(sd, eid, wd, n)
        assert tuple(out.shape) == ref.shape
        res += [(f"edges n={n} e={e}", out, ref, 0), (f"weights n={n} e={e}", ow.view(torch.int32), ref_w.view(np.int32), 0)]
        out, ow = be.subgraph(sd, eid, None, n)
        res.append((f"edges, no weights n={n} e={e}", out, ref, 0))
    return res


@case("subgraph_batches", "dif_subgraph_batches_group", "dif_subgraph_batches_emit", "dif_subgraph_batches_csr")
def _(P, be):
    res = []
    for n, e, m, bsz, weighted in [(300, 4000, 300, 64, True), (1000, 5000, 777, 1000, False), (65, 300, 65, 1, True)]:
        g = _g(n + bsz)
        ei = torch.cat([torch.randint(0, n, (2, e), generator=g), torch.arange(n).repeat(2, 1)], dim=1)
        w = torch.rand(ei.shape[1], generator=g) if weighted else None
        perm = torch.randperm(n, generator=g)[:m]
        pd, eid, wd = P(perm=perm, edge_index=ei, edge_weight=w)
        out_ei, out_w, ptr, (rowptr, src, val) = be.subgraph_batches(pd, bsz, eid, wd, n, build_csr=True)
        nb = -(-m // bsz)
        assert len(ptr) == nb + 1
        refs = [orc.subgraph(perm[b * bsz: (b + 1) * bsz].numpy(), ei.numpy(), None if w is None else w.numpy(), relabel_nodes=True,
                             num_nodes=n) for b in range(nb)]
        tag = f"n={n} bsz={bsz}"
        res += [(f"batch_ptr {tag}", torch.tensor(ptr), np.concatenate([[0], np.cumsum([r[0].shape[1] for r in refs])]), 0),
                (f"edges {tag}", out_ei, np.concatenate([r[0] for r in refs], axis=1), 0)]
        if weighted:
            res.append((f"weights {tag}", out_w.view(torch.int32), np.concatenate([r[1] for r in refs]).view(np.int32), 0))
        # the CSR over all batches: batch b's rows are what dif_csr_build makes of batch b's edge list
        r_rp, r_src, r_val = [np.zeros(1, dtype=np.int64)], [], []
        for b, (eb, wb) in enumerate(refs):
            rows = min(bsz, m - b * bsz)
            rp, _, s, v, _ = _csr(torch.from_numpy(eb), None if wb is None else torch.from_numpy(wb), rows)
            r_rp.append(rp.numpy()[1:].astype(np.int64) + r_rp[-1][-1])
            r_src.append(s.numpy()), r_val.append(v.numpy())
        kept = ptr[-1]
        res += [(f"csr rowptr {tag}", rowptr, np.concatenate(r_rp), 0), (f"csr src {tag}", src[:kept], np.concatenate(r_src), 0),
                (f"csr val {tag}", val[:kept].view(torch.int32), np.concatenate(r_val).view(np.int32), 0)]
    return res


@case("graph_prepare", "dif_graph_prepare")
def _(P, be):
    res = []
    for n, e in [(70, 2000), (1, 3), (3000, 100), (257, 4097)]:
        g = _g(n)
        ei = torch.randint(0, n, (2, e), generator=g)
        ei[:, : e // 10] = ei[:, e // 10: 2 * (e // 10)]
        ei[1, : e // 20] = ei[0, : e // 20]
        eid, = P(edge_index=ei)
        a = ei.numpy()
        key = np.unique(np.concatenate([a[0] * n + a[1], a[1] * n + a[0]]))
        und = np.stack([key // n, key % n])
        loops = np.arange(n)[None].repeat(2, 0)
        res += [(f"undirected n={n}", be.graph_prepare(eid, n, undirected=True), und, 0),
                (f"no loops n={n}", be.graph_prepare(eid, n, remove_loops=True), a[:, a[0] != a[1]], 0),
                (f"add loops n={n}", be.graph_prepare(eid, n, add_loops=True), np.concatenate([a, loops], axis=1), 0),
                (f"all three n={n}", be.graph_prepare(eid, n, True, True, True), np.concatenate([und[:, und[0] != und[1]], loops], axis=1), 0)]
    return res


@case("row_order", "dif_row_order")
def _(P, be):
    res = []
    for n, lo, cnt in [(1, 0, 1), (255, 0, 255), (257, 100, 157), (3000, 0, 3000)]:
        rp = _csr(_graph(n, 6, n, hubs=min(n, 4)), None, n)[0]
        rpd, = P(rowptr=rp)
        order, stats = be.row_order(rpd, lo, cnt)
        r_order, r_stats = FAKE.row_order(rp, lo, cnt)
        res += [(f"order n={n} [{lo}, +{cnt})", order, r_order.numpy(), 0), (f"stats n={n}", stats, r_stats.numpy(), 0)]
    return res


@case("edge_weight_grad", "dif_gcn_edge_weight_grad_f32")
def _(P, be):
    res = []
    for n, deg, F in [(1, 2, 4), (63, 5, 64), (65, 5, 7), (257, 3, 300)]:
        ei = _graph(n, deg, n + F)
        g = _g(n)
        w = torch.rand(ei.shape[1], generator=g) + 0.5
        gr, x = _rn(g, n, F), _rn(g, n, F)
        rp = _csr(ei, w, n)[0]
        eid, wd, rpd, gd, xd = P(edge_index=ei, edge_weight=w, rowptr=rp, g=gr, x=x)
        res.append((f"dw n={n} F={F}", be.edge_weight_grad(eid, wd, rpd, n, gd, xd, 1.5), _d(FAKE.edge_weight_grad(ei, w, rp, n, gr, x, 1.5)), TOL))
    return res


# ================================================================== a3: the products
def _spmm_ref(x, ei, a, tail=None):
    ref = 2.0 * orc.gcn_conv(_d(x)[:, None, :], ei.numpy(), None)[:, 0, :] + (0.5 * _d(a) if a is not None else 0.0)
    if tail is not None:
        z = 0.4 * (ref + _d(tail["x0"])) + 0.6 * _d(tail["prev"])
        ref = np.maximum(orc.layer_norm(z, _d(tail["ln_weight"]), _d(tail["ln_bias"])), 0.0)
    return ref


def _spmm_rows(P, be, dt):
    res = []
    for n, deg, F in [(1, 2, 4), (255, 24, 64), (257, 4, 7), (257, 17, 50), (255, 4, 260), (65, 70, 13)]:
        ei = _graph(n, deg, F + deg)
        g = _g(F)
        x, a = _rn(g, n, F, dt=dt), _rn(g, n, F, dt=dt)
        rp, _, src, val, nnz = _csr(ei, None, n)
        rpd, sd, vd, xd, ad = P(rowptr=rp, src=src, val=val, x=x, attn=a)
        out = be.spmm(rpd, None, 1, sd, vd, n, nnz, xd, 0, n, ad, 0.5, 2.0, None, None)
        res.append((f"n={n} deg={deg} F={F}", out, _spmm_ref(x, ei, a), _tol(dt)))
    return res


@case("spmm_row_kernels_f32", "dif_gcn_spmm_f32")
def _(P, be):
    return _spmm_rows(P, be, F32)


@case("spmm_row_kernels_bf16", "dif_gcn_spmm_tail_bf16")
def _(P, be):
    return _spmm_rows(P, be, BF16)


def _spmm_blocked(P, be, dt, widths, tail):
    res = []
    for n, F in [(255, widths[0]), (257, widths[1]), (2049, widths[2])]:
        for ordered in (False, True):
            ei = _graph(n, 12, F, hubs=4)
            g = _g(F + 1)
            x, a = _rn(g, n, F, dt=dt), _rn(g, n, F, dt=dt)
            rp, blk, src, val, nnz = _csr(ei, None, n, 3)
            rpd, bd, sd, vd, xd, ad = P(rowptr=rp, blkptr=blk, src=src, val=val, x=x, attn=a)
            order = None
            if ordered:
                o, stats = FAKE.row_order(rp, 0, n)
                order = (P(order=o)[0], int(stats[0]))
                assert order[1] > 0                                            # hub rows split over a quad of lanes
            t = None
            if tail:
                t = dict(x0=_rn(g, n, F, dt=dt), prev=_rn(g, n, F, dt=dt), alpha=0.4, ln_weight=(torch.rand(F, generator=g) + 0.5).to(dt),
                         ln_bias=_rn(g, F, dt=dt), eps=1e-5, relu=True)
                td = dict(t)
                td["x0"], td["prev"], td["ln_weight"], td["ln_bias"] = P(x0=t["x0"], prev=t["prev"], ln_weight=t["ln_weight"], ln_bias=t["ln_bias"])
            out = be.spmm(rpd, bd, 3, sd, vd, n, nnz, xd, 0, n, ad, 0.5, 2.0, td if tail else None, order)
            res.append((f"n={n} F={F} ordered={ordered} tail={tail}", out, _spmm_ref(x, ei, a, t), (2 if tail else 1) * _tol(dt)))
    return res


@case("spmm_blocked_f32", "dif_gcn_spmm_f32")
def _(P, be):
    return _spmm_blocked(P, be, F32, (64, 128, 256), False)


@case("spmm_blocked_bf16", "dif_gcn_spmm_tail_bf16")
def _(P, be):
    return _spmm_blocked(P, be, BF16, (64, 100, 204), False)


@case("spmm_fused_tail_f32", "dif_gcn_spmm_tail_f32")
def _(P, be):
    return _spmm_blocked(P, be, F32, (64, 128, 256), True)


def _spmm_split(P, be, dt):
    """Both phases of a split product, rank by rank: part 0 is handed a pointer BEFORE its own value rows by design (it
    indexes by global source row); the bands around `own` prove that it touches its own rows only."""
    res = []
    n, F, world, rows = 600, 64, 2, 150
    ei = _graph(n, 12, 3, hubs=6)
    g = _g(9)
    x, a = _rn(g, n, F, dt=dt), _rn(g, n, F, dt=dt)
    rp, blk, src, val, nnz = _csr(ei, None, n, n // rows, rows)
    rpd, bd, sd, vd, xd, ad = P(rowptr=rp, blkptr=blk, src=src, val=val, x=x, attn=a)
    ref = _spmm_ref(x, ei, a)
    for rank in range(world):
        lo, cnt = rank * (n // world), n // world
        own_lo, own_hi = lo // rows, (lo + cnt) // rows
        own, a_own = P(own=x[lo: lo + cnt].clone(), attn_own=a[lo: lo + cnt].clone())
        args = (rpd, bd, n // rows, sd, vd, n, nnz)
        scratch = be.spmm(*args, own, lo, cnt, None, 0.5, 2.0, None, None, (0, own_lo, own_hi, None, lo))
        out = be.spmm(*args, xd, lo, cnt, a_own, 0.5, 2.0, None, None, (1, own_lo, own_hi, scratch, 0))
        res.append((f"rank {rank}", out, ref[lo: lo + cnt], _tol(dt)))
    return res


@case("spmm_split_product_f32", "dif_gcn_spmm_part_f32")
def _(P, be):
    return _spmm_split(P, be, F32)


@case("spmm_split_product_bf16", "dif_gcn_spmm_part_bf16")
def _(P, be):
    return _spmm_split(P, be, BF16)


def _sliced(P, be, quad_cap):
    """The smallest graph that takes the feature-sliced product: 8,192 nodes x 48 entries per row (47 + the self loop)."""
    from difformer_amd import ops
    n, F = 8192, 64
    g = _g(quad_cap)
    ei = torch.stack([torch.cat([torch.randint(0, n, (n * 47,), generator=g), torch.arange(n)]),
                      torch.cat([torch.arange(n).repeat_interleave(47), torch.arange(n)])])
    x, a = _rn(g, n, F), _rn(g, n, F)
    eid, xd, ad = P(edge_index=ei, x=x, attn=a)
    csr = ops.csr_cache.get(eid, None, n, F * 4)                  # dif_csr_build in the format's tiling (outputs: guarded too)
    sl = csr.sliced(0, n, F)
    assert sl is not None and sl.quad_cap == quad_cap
    ys = be.sliced_prescale(xd, csr.rowptr, n, sl.plan)
    out = be.sliced_spmm(sl, ys, csr.rowptr, n, 0, n, F, ad, 0.5, 2.0)
    ops.csr_cache.drop(eid)
    return [(f"quad_cap={quad_cap}", out, _spmm_ref(x, ei, a), TOL)]


@case("sliced_strict", "dif_sliced_measure", "dif_sliced_emit", "dif_sliced_prescale_f32", "dif_sliced_spmm_f32")
def _(P, be):
    return _sliced(P, be, 1)


@case("sliced_packed", "dif_sliced_measure", "dif_sliced_emit", "dif_sliced_prescale_f32", "dif_sliced_spmm_f32")
def _(P, be):
    return _sliced(P, be, 2)


# ================================================================== Gram records and coefficients of the closed form
def _record_ref(x64):
    return np.concatenate([(x64.T @ x64).ravel(), x64.sum(0)])


@case("gram", "dif_gram_f32", "dif_gram_bf16", "dif_gram_coeffs_f32", "dif_simple_coeffs_f32")
def _(P, be):
    res = []
    for n, c, d in [(1, 4, 4), (63, 64, 64), (65, 32, 48), (127, 64, 16), (4097, 64, 64)]:
        g = _g(n + c)
        x = _rn(g, n, c, shift=0.3)
        W = [_rn(g, d, c, scale=c ** -0.5) for _ in range(3)]
        b = [_rn(g, d, scale=0.3) for _ in range(3)]
        xd, xb, *wb = P(x=x, xb=x.to(BF16), Wq=W[0], bq=b[0], Wk=W[1], bk=b[1], Wv=W[2], bv=b[2])
        ref = _record_ref(_d(x))
        rec, _ = be.gram(xd)
        res.append((f"record n={n} c={c}", rec[: ref.size], ref, TOL))
        rec_b, _ = be.gram(xb)
        res.append((f"record bf16 n={n} c={c}", rec_b[: ref.size], _record_ref(_d(x.to(BF16))), BF16_TOL))
        rec_in, = P(record=torch.from_numpy(np.concatenate([ref, [0.0, 0.0]]).astype(np.float32)))
        coef_ref = _d(FAKE.simple_coeffs(rec_in.cpu(), n, c, d, W[0], b[0], W[1], b[1], W[2], b[2], 0.7))
        coef = be.simple_coeffs(rec_in, n, c, d, *wb, 0.7)
        rec2, coef2 = be.gram_coeffs(xd, n, c, d, *wb, 0.7)
        res.append((f"gram_coeffs record n={n} c={c}", rec2[: ref.size], ref, TOL))
        for how, got in (("simple_coeffs", coef), ("gram_coeffs", coef2)):
            for (nm, a), (_, b_) in zip(_coef_parts(got, c, d), _coef_parts(coef_ref, c, d)):
                res.append((f"{how} {nm} n={n} c={c} d={d}", a, b_, TOL))
    return res


@case("gram_sym", "dif_gram_sym_f32", "dif_gram128_f32")
def _(P, be):
    res = []
    for n, c in [(1, 70), (63, 128), (65, 300), (4096, 128), (257, 13)]:
        x = _rn(_g(n + c), n, c, shift=0.3)
        xd, = P(x=x)
        rec = be.gram_sym(xd)
        x64 = _d(x)
        got = _d(rec[: c * c]).reshape(c, c)
        blk = np.arange(c) // 64
        got = np.where(blk[:, None] <= blk[None, :], got, got.T)              # blocks on and above the diagonal are valid
        res += [(f"X^T X n={n} c={c}", got, x64.T @ x64, TOL), (f"sums n={n} c={c}", rec[c * c: c * c + c], x64.sum(0), TOL)]
    return res


@case("input_gram", "dif_input_gram_f32")
def _(P, be):
    res = []
    for n, c, d in [(1, 24, 64), (63, 7, 32), (65, 64, 64), (4097, 30, 48)]:
        g = _g(n + c)
        x, W, b = _rn(g, n, c), _rn(g, d, c, scale=c ** -0.5), _rn(g, d)
        lw, lb = torch.rand(d, generator=g) + 0.5, _rn(g, d)
        xd, Wd, bd, lwd, lbd = P(x=x, weight=W, bias=b, ln_weight=lw, ln_bias=lb)
        h, rec, _ = be.input_gram(xd, Wd, bd, lwd, lbd, 1e-5, True)
        h64 = np.maximum(orc.layer_norm(_d(x) @ _d(W).T + _d(b), _d(lw), _d(lb)), 0.0)
        ref = _record_ref(h64)
        res += [(f"h n={n} c={c} d={d}", h, h64, TOL), (f"record n={n} c={c} d={d}", rec[: ref.size], ref, TOL)]
    return res


def _coef_parts(coef, c, d):
    """[Mn^T | cn | u | cd] of a coefficient record, each held norm-wise on its own (cd ~ N would hide the rest)"""
    return (("MnT", coef[: d * c]), ("cn", coef[d * c: d * c + d]), ("u", coef[d * c + d: d * c + d + c]),
            ("cd", coef[d * c + d + c: d * c + d + c + 1]))


def _coef_params(g, c, d):
    W = [_rn(g, d, c, scale=c ** -0.5) for _ in range(3)]
    b = [_rn(g, d, scale=0.3) for _ in range(3)]
    return [W[0], b[0], W[1], b[1], W[2], b[2]]


@case("simple_coeffs_backward", "dif_simple_coeffs_bwd_f32")
def _(P, be):
    """reference: ops.closed_form_coeffs_backward, the same formulas in float64 tensor ops (tests/test_gpu_closed_form.py)"""
    from difformer_amd import ops
    res = []
    for n, c, d in [(63, 64, 64), (65, 32, 64), (257, 64, 16), (700, 8, 12)]:
        g = _g(n + c)
        x = _rn(g, n, c, shift=0.2)
        wb = _coef_params(g, c, d)
        rec = torch.from_numpy(np.concatenate([_record_ref(_d(x)), [0.0, 0.0]]).astype(np.float32))
        coef = FAKE.simple_coeffs(rec, n, c, d, *wb, 0.7)
        dcoef = _rn(g, d * c + d + c + 2)
        dcoef[: d * c] *= 3.0
        recd, coefd, dcoefd, *wbd = P(record=rec, coef=coef, dcoef=dcoef, Wq=wb[0], bq=wb[1], Wk=wb[2], bk=wb[3], Wv=wb[4], bv=wb[5])
        got = be.simple_coeffs_backward(recd, n, c, d, *wbd, 0.7, coefd, dcoefd)
        ref = ops.closed_form_coeffs_backward(recd, n, c, d, *wbd, 0.7, dcoefd[: d * c].view(d, c), dcoefd[d * c: d * c + d],
                                              dcoefd[d * c + d: d * c + d + c], dcoefd[d * c + d + c])
        for nm, a, b in zip(("S", "t", "dWq", "dbq", "dWk", "dbk", "dWv", "dbv"), got, ref):
            res.append((f"{nm} n={n} c={c} d={d}", a, _d(b), TOL))
    return res


@case("coeffs_bg", "dif_gram_bg_f32", "dif_simple_coeffs_bg_f32")
def _(P, be):
    from difformer_amd import ops
    res = []
    for n, c, d in [(1, 64, 64), (63, 32, 32), (65, 48, 64), (4097, 64, 32)]:
        g = _g(n + c)
        x = _rn(g, n, c, shift=0.2)
        wb = _coef_params(g, c, d)
        rec = torch.from_numpy(np.concatenate([_record_ref(_d(x)), [0.0, 0.0]]).astype(np.float32))
        want = _d(FAKE.simple_coeffs(rec, n, c, d, *wb, 0.7))
        xd, recd, *wbd = P(x=x, record=rec, Wq=wb[0], bq=wb[1], Wk=wb[2], bk=wb[3], Wv=wb[4], bv=wb[5])
        f = ops.NarrowFactors(*wbd)
        for how, got in (("from x", be.coeffs_bg(xd, None, n, f, c, d, 0.7)), ("from the record", be.coeffs_bg(None, recd, n, f, c, d, 0.7))):
            for (nm, a), (_, b) in zip(_coef_parts(got, c, d), _coef_parts(want, c, d)):
                res.append((f"{nm} {how} n={n} c={c} d={d}", a, b, TOL))
    return res


# ================================================================== row GEMM, Linear layers, tails
@case("row_gemm", "dif_rowgemm_f32")
def _(P, be):
    res = []
    for n, K, C in [(1, 64, 64), (127, 64, 128), (129, 70, 130), (129, 512, 64), (127, 13, 7), (4097, 128, 132)]:
        g = _g(n + K)
        A, mat, bias, acc = _rn(g, n, K), _rn(g, K, C, scale=K ** -0.5), _rn(g, C), _rn(g, n, C)
        Ad, md, bd, accd = P(A=A, mat=mat, bias=bias, accumulate=acc)
        res.append((f"n={n} K={K} C={C}", be.row_gemm(Ad, md, bd, accd), _d(A) @ _d(mat) + _d(bias) + _d(acc), TOL))
        res.append((f"n={n} K={K} C={C} plain", be.row_gemm(Ad, md), _d(A) @ _d(mat), TOL))
    return res


def _linear_ref(x, w, b, lw, lb, relu):
    y = _d(x) @ _d(w).T + _d(b)
    if lw is not None:
        y = orc.layer_norm(y, _d(lw), _d(lb))
    return np.maximum(y, 0.0) if relu else y


def _linear(P, be, dt, shapes):
    res = []
    for n, ci, co in shapes:
        g = _g(n + ci)
        x, w, b = _rn(g, n, ci, dt=dt), _rn(g, co, ci, dt=dt, scale=ci ** -0.5), _rn(g, co, dt=dt)
        lw, lb = (torch.rand(co, generator=g) + 0.5).to(dt), _rn(g, co, dt=dt)
        xd, wd, bd, lwd, lbd = P(x=x, weight=w, bias=b, ln_weight=lw, ln_bias=lb)
        res.append((f"n={n} {ci}->{co}", be.linear(xd, wd, bd), _linear_ref(x, w, b, None, None, False), _tol(dt)))
        res.append((f"n={n} {ci}->{co} LN ReLU", be.linear(xd, wd, bd, lwd, lbd, 1e-5, True), _linear_ref(x, w, b, lw, lb, True), _tol(dt)))
    return res


@case("linear_skinny_f32", "dif_linear_f32")
def _(P, be):
    return _linear(P, be, F32, [(1, 16, 112), (63, 30, 112), (65, 128, 64), (65, 65, 7), (16384, 512, 64)])


@case("linear_skinny_bf16", "dif_linear_bf16")
def _(P, be):
    return _linear(P, be, BF16, [(1, 16, 112), (63, 30, 64), (65, 128, 112), (65, 65, 7)])


@case("linear_packed", "dif_linear_pack_f32", "dif_linear_packed_f32", min_align=4)
def _(P, be):
    return _linear(P, be, F32, [(1, 129, 40), (127, 1433, 64), (129, 301, 7), (129, 512, 64)])


@case("linear_xwide", "dif_linear_xwide_f32", "dif_xwide_pack_f32")
def _(P, be):
    return _linear(P, be, F32, [(16384, 512, 400), (16384, 300, 300)])


def _tail_ref(conv, x0, prev, alpha, lw, lb, relu):
    z = _d(conv).mean(axis=1)
    if x0 is not None:
        z = z + _d(x0)
    if prev is not None:
        z = alpha * z + (1.0 - alpha) * _d(prev)
    if lw is not None:
        z = orc.layer_norm(z, _d(lw), _d(lb))
    return np.maximum(z, 0.0) if relu else z


def _layer_tail(P, be, dt):
    res = []
    for n, D, H in [(1, 4, 1), (63, 8, 2), (65, 64, 1), (65, 300, 1), (63, 6, 2), (257, 70, 1), (255, 256, 2)]:
        g = _g(D * 10 + H)
        conv, x0, prev = _rn(g, n, H, D, dt=dt), _rn(g, n, D, dt=dt), _rn(g, n, D, dt=dt)
        lw, lb = (torch.rand(D, generator=g) + 0.5).to(dt), _rn(g, D, dt=dt)
        cd, x0d, pd, lwd, lbd = P(conv=conv, x0=x0, prev=prev, ln_weight=lw, ln_bias=lb)
        for ux, up, ln, relu in ((True, True, True, False), (False, True, False, True), (False, False, True, True)):
            out = be.layer_tail(cd, x0d if ux else None, pd if up else None, 0.4, lwd if ln else None, lbd if ln else None, 1e-5, relu)
            ref = _tail_ref(conv, x0 if ux else None, prev if up else None, 0.4, lw if ln else None, lb if ln else None, relu)
            res.append((f"n={n} D={D} H={H} {ux, up, ln, relu}", out, ref, _tol(dt)))
    return res


@case("layer_tail_f32", "dif_layer_tail_f32")
def _(P, be):
    return _layer_tail(P, be, F32)


@case("layer_tail_bf16", "dif_layer_tail_bf16")
def _(P, be):
    return _layer_tail(P, be, BF16)


@case("layer_tail_mix", "dif_layer_tail_mix_f32")
def _(P, be):
    res = []
    for n, D in [(1, 64), (63, 128), (65, 300), (257, 256)]:
        g = _g(D + n)
        ldz = ((D + 1 + 3) // 4) * 4
        Z = _rn(g, n, ldz)
        Z[:, D] = torch.rand(n, generator=g) + 1.0
        add, rs, bv, x0, prev = _rn(g, n, D), torch.rand(n, generator=g), _rn(g, D), _rn(g, n, D), _rn(g, n, D)
        lw, lb = torch.rand(D, generator=g) + 0.5, _rn(g, D)
        Zd, addd, rsd, bvd, x0d, pd, lwd, lbd = P(Z=Z, add=add, rs=rs, bv=bv, x0=x0, prev=prev, ln_weight=lw, ln_bias=lb)
        out = be.layer_tail_mix(Zd, D, D, 0.7, addd, 1.3, rsd, bvd, x0d, pd, 0.4, lwd, lbd, 1e-5)
        z = 0.7 * _d(Z[:, :D]) / _d(Z[:, D:D + 1]) + 1.3 * (_d(add) + _d(rs)[:, None] * _d(bv)[None, :])
        z = 0.4 * (z + _d(x0)) + 0.6 * _d(prev)
        res.append((f"n={n} D={D}", out, orc.layer_norm(z, _d(lw), _d(lb)), TOL))
        out2 = be.layer_tail_mix(Zd, D, None, 1.0, None, 1.0, None, None, None, None, 0.5, None, None, 1e-5, relu=True)
        res.append((f"n={n} D={D} bare", out2, np.maximum(_d(Z[:, :D]), 0.0), TOL))
    return res


@case("layer_tail_bwd", "dif_layer_tail_bwd_f32")
def _(P, be):
    res = []
    for n, H, D in [(1, 1, 4), (63, 2, 8), (65, 1, 64), (257, 2, 260), (255, 1, 512), (5000, 1, 64)]:
        g = _g(D + n)
        conv, x0, prev = _rn(g, n, H, D), _rn(g, n, D), _rn(g, n, D)
        lw, lb, go = torch.rand(D, generator=g) + 0.5, _rn(g, D), _rn(g, n, D)
        cd, x0d, pd, lwd, lbd, god = P(conv=conv, x0=x0, prev=prev, ln_weight=lw, ln_bias=lb, grad_out=go)
        got = be.layer_tail_bwd(cd, x0d, pd, 0.4, lwd, lbd, 1e-5, False, god, (True, True, True, True))
        assert got is not None
        leaves = [t.double().requires_grad_(True) for t in (conv, x0, prev, lw, lb)]
        z = 0.4 * (leaves[0].mean(dim=1) + leaves[1]) + 0.6 * leaves[2]
        torch.nn.functional.layer_norm(z, (D,), leaves[3], leaves[4], 1e-5).backward(go.double())
        for a, b, nm in zip(got, leaves, ("d_conv", "d_x0", "d_prev", "d_ln_weight", "d_ln_bias")):
            res.append((f"{nm} n={n} H={H} D={D}", a, _d(b.grad), TOL))
    return res


@case("closed_form_attn_backward", "dif_closed_form_attn_bwd_f32")
def _(P, be):
    res = []
    for n, c, d in [(1, 64, 64), (63, 32, 48), (65, 64, 16), (4099, 64, 64)]:
        g = _g(n + c)
        x, dd, dx_in, rs = _rn(g, n, c), _rn(g, n, d), _rn(g, n, c), torch.rand(n, generator=g)
        coef = _rn(g, d * c + d + c + 4, scale=0.2)
        coef[d * c + d + c] = 25.0
        xd, cd_, ddd, dxd, rsd = P(x=x, coef=coef, d=dd, dx_in=dx_in, row_sums=rs)
        got = be.closed_form_attn_backward(xd, cd_, d, ddd, dxd, rsd)
        assert got is not None
        cf, x64, d64 = _d(coef), _d(x), _d(dd)
        MnT, cn, u, cdn = cf[: d * c].reshape(d, c), cf[d * c: d * c + d], cf[d * c + d: d * c + d + c], cf[d * c + d + c]
        den = x64 @ u + cdn
        att = (x64 @ MnT.T + cn) / den[:, None]
        d_num = d64 / den[:, None]
        d_den = -(d64 * att).sum(1) / den
        dx = _d(dx_in) + d_num @ MnT + d_den[:, None] * u[None, :]
        refs = (d_num, d_den, dx, x64.T @ d_den, np.array([d_den.sum()]), _d(rs) @ d64)
        for nm, a, b in zip(("d_num", "d_den", "dx", "d_u", "d_cd", "rs_d"), got, refs):
            res.append((f"{nm} n={n} c={c} d={d}", a.reshape(b.shape), b, TOL))
    return res


# ================================================================== whole models: the layer kernels and what feeds them
def _model(P, be, n, f_in, hidden, classes, layers, kernel, graph, train=False, dt=F32, **flags):
    """DIFFormer forward (and training step) with x, edge_index AND every parameter in guarded blocks, against the float64
    oracle (tests/test_gpu_kernel_coverage.py::_model_forward; gradients: oracle.difformer_oracle_grad as smoke())."""
    from difformer_amd import DIFFormer
    from oracle import difformer_oracle_grad as og
    torch.manual_seed(n + hidden + layers)
    model = DIFFormer(f_in, hidden, classes, num_layers=layers, num_heads=1, kernel=kernel, use_graph=graph is not None,
                      dropout=0.0, **flags).to(dt)
    x = _rn(_g(7), n, f_in, dt=dt)
    cfg = dict(hidden_channels=hidden, num_layers=layers, num_heads=1, kernel=kernel, alpha=0.5, use_bn=True, use_residual=True,
               use_weight=flags.get("use_weight", True), use_graph=graph is not None, graph_weight=flags.get("graph_weight", -1),
               use_source=flags.get("use_source", False))
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    for name, p in list(model.named_parameters()):
        p.data = P(**{name.replace(".", "_"): p.data})[0]
    xd, eid = P(x=x, edge_index=graph)
    tol = _tol(dt) * (2 if dt == BF16 else 1)
    tag = f"{kernel} n={n} hidden={hidden}"
    if not train:
        model.eval()
        with torch.no_grad():
            out = model(xd, eid)
        ref = orc.difformer_forward({k: _d(v) for k, v in sd.items()}, _d(x), None if graph is None else graph.numpy(), None, cfg)
        return [(f"logits {tag}", out, ref, tol)]
    model.train()
    g = _g(3)
    y, idx = torch.randint(0, classes, (n,), generator=g), torch.randperm(n, generator=g)[: max(n // 2, 1)]
    yd, idxd = P(y=y, idx=idx)
    out = model(xd, eid)
    loss = torch.nn.functional.nll_loss(torch.log_softmax(out, dim=1)[idxd], yd[idxd])
    loss.backward()
    pl = og.leaves({k: v.numpy() for k, v in sd.items()})
    lref = og.training_loss(og.difformer_forward(pl, x.double(), graph, None, cfg), y, idx)
    lref.backward()
    gmax = max(float(v.grad.abs().max()) for v in pl.values())
    res = [(f"loss {tag}", loss.detach().reshape(1), _d(lref).reshape(1), tol)]
    for k, prm in model.named_parameters():
        want = _d(pl[k].grad)
        scale = max(float(np.abs(want).max()), 1e-6 * gmax)              # the norm of smoke(): per tensor, floored
        res.append((f"grad {k} {tag}", _d(prm.grad) / scale, want / scale, -tol))
    return res


@case("model_closed_form_64", "dif_gram_coeffs_f32", "dif_simple_layer_f32", "dif_simple_layer_gather_f32", "dif_simple_layer_head_f32")
def _(P, be):
    return (_model(P, be, 65, 24, 64, 10, 2, "simple", None) + _model(P, be, 4097, 24, 32, 10, 2, "simple", _graph(4097, 5, 1)) +
            _model(P, be, 257, 24, 64, 10, 2, "simple", _graph(257, 5, 2), use_weight=False))


@case("model_closed_form_64_bf16", "dif_simple_layer_bf16", "dif_simple_layer_gather_bf16", "dif_simple_layer_head_bf16")
def _(P, be):
    return _model(P, be, 257, 24, 64, 10, 2, "simple", _graph(257, 5, 2), dt=BF16) + _model(P, be, 63, 24, 32, 10, 2, "simple", None, dt=BF16)


@case("model_closed_form_64_dense_graph", "dif_sliced_spmm_f32", "dif_simple_layer_f32")
def _(P, be):
    return _model(P, be, 8192, 24, 64, 10, 2, "simple", _graph(8192, 50, 4))


@case("model_closed_form_wide", "dif_simple_layer_wide_f32", "dif_wide_coeffs_f64")
def _(P, be):
    # the wide closed forms dispatch from n = 4 C rows on (DIFFormerConv._route): exactly that many
    return _model(P, be, 512, 24, 128, 10, 2, "simple", _graph(512, 6, 5)) + _model(P, be, 272, 24, 68, 10, 2, "simple", None)


@case("model_closed_form_xwide", "dif_simple_layer_xwide_f32", "dif_xwide_pack_f32", "dif_wide_coeffs_f64")
def _(P, be):
    return _model(P, be, 1200, 24, 300, 10, 2, "simple", _graph(1200, 6, 6)) + _model(P, be, 528, 24, 132, 10, 2, "simple", None)


@case("model_training_step", "dif_layer_tail_bwd_f32")
def _(P, be):
    return (_model(P, be, 4097, 24, 64, 10, 2, "simple", _graph(4097, 5, 8), train=True) +
            _model(P, be, 129, 24, 32, 10, 2, "sigmoid", _graph(129, 5, 9), train=True))


@case("tiny_model", "dif_tiny_graph_build", "dif_tiny_forward_f32", "dif_tiny_backward_f32")
def _(P, be):
    # whole-model kernels: hidden <= 8, <= 8 classes, <= 64 input channels (tiny.py); 63 / 65 nodes around the 64-node
    # workgroup, 257 / 300 beyond the one-workgroup launches (the grid kernels)
    return (_model(P, be, 63, 16, 8, 5, 2, "simple", _graph(63, 4, 10), train=True) +
            _model(P, be, 1, 16, 4, 5, 2, "sigmoid", _graph(1, 1, 11)) + _model(P, be, 65, 7, 8, 3, 3, "sigmoid", _graph(65, 4, 12), train=True) +
            _model(P, be, 300, 64, 4, 8, 2, "simple", _graph(300, 4, 13), train=True) + _model(P, be, 257, 3, 8, 2, 1, "sigmoid", None))


# ================================================================== the test
class _LibSpy:
    """Forwards to the loaded library and notes which entry points were looked up (= called)."""

    def __init__(self, lib):
        self.__dict__["lib"], self.__dict__["called"] = lib, set()

    def __getattr__(self, name):
        if name.startswith("dif_"):
            self.called.add(name)
        return getattr(self.lib, name)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("placement", ["aligned512", "minimum"])
@pytest.mark.parametrize("name,symbols,run,min_align", CASES, ids=[c[0] for c in CASES])
def test_operands_between_nan_bands(name, symbols, run, min_align, placement, dev, poisoned_allocations, schedule, monkeypatch):
    from difformer_amd import _lib, ops
    be = ops.get_backend()
    spy = _LibSpy(be.lib)
    monkeypatch.setattr(be, "lib", spy)
    monkeypatch.setattr(_lib, "_lib", spy)
    schedule("packed" if name == "sliced_packed" else "strict")
    inputs = GuardedArena()
    results = run(lambda **kw: guarded_inputs(inputs, dev, min_align=min_align if placement == "minimum" else False, **kw), be)
    assert len(inputs.blocks) > 0 and len(poisoned_allocations.blocks) > 0
    inputs.check()                                                  # nothing was written around an operand either
    print(f"{name}[{placement}] launched: {sorted(spy.called)}")
    missing = set(symbols) - spy.called
    assert not missing, f"{name} did not launch {sorted(missing)} (launched: {sorted(spy.called)})"
    failures = []
    for label, got, ref, tol in results:
        got = _d(got) if torch.is_tensor(got) else np.asarray(got, dtype=np.float64)
        ref = np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (label, got.shape, ref.shape)
        finite = bool(np.isfinite(got).all())
        if tol == 0:
            err, ok = float(not np.array_equal(got, ref)), np.array_equal(got, ref)
        elif tol < 0:                                               # pre-scaled by the caller (gradients: largest over the step)
            err = float(np.max(np.abs(got - ref))) if ref.size else 0.0
            ok = err < -tol
        else:
            err = rel_err(got, ref)
            ok = err < tol
        print(f"{name}[{placement}] {label}: err {err:.3e} (tol {abs(tol):.0e}) finite={finite}")
        if not (ok and finite):
            failures.append((label, err, finite))
    assert not failures, failures


# ================================================================== no entry point can skip this file
def _entry_points_with_pointers():
    from difformer_amd import _lib
    code = re.sub(r"^[ \t]*#.*$", "", _lib._code, flags=re.M)
    found = set()
    for m in re.finditer(r"\b(dif_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", code):
        if any("*" in p for p in m.group(2).split(",")):
            found.add(m.group(1))
    return found


def test_every_entry_point_with_a_pointer_is_in_the_table_or_excused():
    """include/difformer_hip.h against CASES + LEFT_OUT: an entry point added later has to come here too."""
    from difformer_amd import _lib
    header = _entry_points_with_pointers()
    assert header <= set(_lib.SIGNATURES) and len(header) > 60
    table = {s for _, symbols, _, _ in CASES for s in symbols}
    assert not (table | set(LEFT_OUT)) - header, f"not in the header: {sorted((table | set(LEFT_OUT)) - header)}"
    assert not table & set(LEFT_OUT)
    assert not header - table - set(LEFT_OUT), f"neither tested nor excused: {sorted(header - table - set(LEFT_OUT))}"
    assert all(len(reason) > 10 for reason in LEFT_OUT.values())
    assert len({c[0] for c in CASES}) == len(CASES)
