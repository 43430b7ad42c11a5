"""Case tables and plain helpers of the backward edge sweep (tests/test_gpu_grad_edges.py, tests/test_grad_edges_host.py).

The backward kernels carry the most row-count-dependent launch arithmetic of the library (split counts, look-ahead fetches,
per-workgroup partial records and their folds).  The tables below hold the SMALLEST shapes that reach each state of that
arithmetic; every op-level case runs with three upstream gradients (`PATTERNS`): a dense one, one that keeps only the last
row, and one that keeps only the first row of the last 16-row tile.  With the two spotlight patterns every gradient that
sums over rows depends on how ONE boundary row was handled: a dropped or doubled row is a 100 % error.

Yardstick: float64 autograd of oracle/difformer_oracle_grad.py (the float64 torch expression for the layer tail, the Linear
and the closed-form stages).  Metric: conftest.grad_err per tensor, gmax = the largest |entry| over the case's gradients;
bar: the project's TOL = 1e-4.  Every case also runs the SAME expression in float32 on the CPU, which must sit within
TOL / 4 of the float64 run (`PRECONDITION`; asserted for every case by tests/test_grad_edges_host.py): a case where float32
arithmetic itself cannot meet the bar is ill-posed and does not belong here.  Tensors that vanish identically take the
absolute floor `ZERO_FLOOR` of test_v2_sigmoid_attention_backward_kernel_vs_oracle (`Problem.floored`); the host test
holds that set to the float64 reference (own maximum below `ZERO_REL` of gmax) in both directions.

Nothing here needs a GPU.
"""
from collections import namedtuple

import numpy as np
import torch
import torch.nn.functional as F

from conftest import grad_err, rel_err
from oracle import difformer_oracle_grad as og

TOL = 1e-4
PRECONDITION = TOL / 4
ZERO_FLOOR = 1e-2            # grad_err floor of the identically vanishing tensors
ZERO_REL = 1e-12             # "vanishes": own largest entry below this fraction of gmax in the float64 reference
PATTERNS = ("dense", "last", "tile")


def spot_row(n, pattern):
    """Row kept by a spotlight pattern: the last row, or the first row of the last 16-row tile (row 0 when n <= 16)."""
    return n - 1 if pattern == "last" else 16 * ((n - 1) // 16)


def cotangent(shape, pattern, seed):
    """Upstream gradient [n, ...]: randn, times the row mask of `pattern`."""
    g = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    if pattern != "dense":
        mask = torch.zeros(shape[0], *([1] * (len(shape) - 1)))
        mask[spot_row(shape[0], pattern)] = 1.0
        g = g * mask
    return g


class Problem:
    """One case: float32 host operands, the oracle expression, and what the GPU side needs to run the same thing.
    leaves   {name: float32 tensor} -- the operands a gradient is taken for, in a fixed order
    consts   {name: anything}       -- integer tensors, flags, shapes (never differentiated)
    expr     (leaves in some dtype, consts) -> output tensor: the oracle
    floored  names of the gradients that vanish identically (ZERO_FLOOR)"""

    def __init__(self, family, name, leaves, consts, expr, floored=()):
        self.family, self.name, self.leaves, self.consts, self.expr = family, name, leaves, consts, expr
        self.floored = frozenset(floored)

    def out_shape(self):
        with torch.no_grad():
            return tuple(self.expr({k: v.double() for k, v in self.leaves.items()}, self.consts).shape)

    def cotangent(self, pattern):
        return cotangent(self.out_shape(), pattern, 1 + PATTERNS.index(pattern))

    def reference(self, cot, dtype=torch.float64):
        """-> (out, {leaf name: gradient}) as float64 ndarrays, the expression evaluated and differentiated in `dtype`."""
        leaves = {k: v.detach().to(dtype, copy=True).requires_grad_(True) for k, v in self.leaves.items()}
        out = self.expr(leaves, self.consts)
        if out.numel():
            out.backward(cot.to(dtype))
        grads = {k: (torch.zeros_like(v) if v.grad is None else v.grad).numpy().astype(np.float64) for k, v in leaves.items()}
        return out.detach().numpy().astype(np.float64), grads

    def __repr__(self):
        return f"{self.family}/{self.name}"


def grad_scale(ref):
    """gmax of a case: the largest finite |entry| over its reference gradients."""
    vals = [float(np.nanmax(np.abs(v))) for v in ref.values() if v.size and not np.isnan(v).all()]
    return max(vals) if vals else 0.0


def errors(got, ref, floored=()):
    """{name: grad_err} of the tensors in `ref`.  NaN entries (the edge-weight gradient of an edge that leaves a node without
    incoming entries, difformer.py:73-74) must sit exactly where the reference's do, as tests/test_gpu_grad.py nan_err asks."""
    gmax = grad_scale(ref)
    out = {}
    for k, r in ref.items():
        g = np.asarray(got[k], dtype=np.float64).reshape(r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), f"{k}: NaN positions differ from the reference's"
        out[k] = grad_err(np.nan_to_num(g), np.nan_to_num(r), gmax, floor=ZERO_FLOOR if k in floored else 2e-6)
    return out


def vanishing(ref):
    """Names of the gradients whose float64 reference vanishes against the case's largest gradient."""
    gmax = grad_scale(ref)
    if gmax == 0.0:
        return frozenset()           # the whole case is zero (a graph without edges): every tensor is compared absolutely
    return frozenset(k for k, v in ref.items() if v.size and float(np.nanmax(np.abs(v))) < ZERO_REL * gmax)


def _gen(*key):
    """A generator seeded from a case's integers (a fixed polynomial mix: the same data on every interpreter)."""
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 1) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---- a / b / c: full_attention_conv ---------------------------------------------------------------------------------
def _attn_expr(kernel):
    return lambda t, c: og.full_attention_conv(t["q"], t["k"], t["v"], kernel)


# (N, L, H, M, D, splits of the dQ sweep, splits of the dK / dV sweep, state reached): sweep_splits(X, Y, H) of
# csrc/sigmoid_attn_bwd.hip at 256 compute units; tests/test_grad_edges_host.py pins the pairs to the library through
# dif_sigmoid_bwd_workspace_bytes, so a change of the heuristic says "pick the shapes again"
SigmoidCase = namedtuple("SigmoidCase", "N L H M D S0 S1 state")
SIGMOID_NARROW = [
    SigmoidCase(1, 1, 1, 64, 64, 1, 1, "single row and key"),
    SigmoidCase(2, 3, 2, 16, 16, 1, 1, "a few rows, two heads"),
    SigmoidCase(15, 17, 2, 32, 32, 1, 1, "one tile, and one tile plus one key"),
    SigmoidCase(32, 128, 1, 64, 64, 1, 1, "exact multiples: every wave has exactly one tile"),
    SigmoidCase(1, 300, 1, 64, 64, 3, 1, "idle waves in the last split"),
    SigmoidCase(300, 1, 1, 64, 64, 1, 3, "the transposed state, one key"),
    SigmoidCase(31, 257, 1, 64, 64, 3, 1, "17 tiles over 3 splits"),
    SigmoidCase(33, 129, 2, 32, 32, 2, 1, "two 32-row groups, the second holds one row"),
    SigmoidCase(129, 400, 3, 20, 20, 4, 2, "both sides split, three heads"),
    SigmoidCase(257, 257, 1, 10, 10, 3, 3, "non-vector path (M % 4 != 0)"),
    SigmoidCase(65, 1025, 1, 30, 30, 9, 1, "non-vector path, many splits"),
    SigmoidCase(17, 2049, 1, 64, 48, 16, 1, "split cap"),
]
# heads of 65 .. 512 columns: the split-bfloat16 plane kernels of csrc/sigmoid_wide.hip (never under set_exact_fp32(True))
SIGMOID_WIDE = [(1, 1, 1, 68, 68), (1, 130, 1, 300, 300), (130, 1, 1, 128, 128), (33, 65, 2, 68, 68), (63, 129, 1, 300, 300),
                (64, 64, 1, 512, 512)]


def sigmoid_workspace_bytes(c):
    """The launcher's workspace formula for the annotated split pair (dif_sigmoid_bwd_workspace_bytes, M, D <= 64)."""
    a16 = lambda b: (b + 15) & ~15
    b = 2 * a16(c.N * c.H * 4)
    if c.S0 > 1:
        b += a16(c.S0 * c.N * c.H * c.M * 4)
    if c.S1 > 1:
        b += a16(c.S1 * c.L * c.H * c.M * 4) + a16(c.S1 * c.L * c.H * c.D * 4)
    return b


def sigmoid_problem(N, L, H, M, D, family="sigmoid"):
    g = _gen(N, L, H, M, D)
    s = M ** -0.25                                          # q.k ~ N(0, 1): sigma does not saturate (tests/test_gpu_attn_topk.py)
    leaves = dict(q=_randn(g, N, H, M) * s, k=_randn(g, L, H, M) * s, v=_randn(g, L, H, D))
    # one key: the weight is sigma / sigma = 1 whatever q and k are, dq = dk = 0, and what float32 leaves of them is the
    # rounding of g.v against the floor -- which grows with sqrt(D) for unit-variance values: the float32 run of the oracle
    # itself sat at 2.8e-5 (TOL / 4 = 2.5e-5) on N = 130, D = 128 with the last-row cotangent.  v is drawn at D^-1/2 there
    # (g.v ~ N(0, 1) at every width; dv, the only gradient that does not vanish, does not depend on v)
    if L == 1:
        leaves["v"] = leaves["v"] * D ** -0.5
    return Problem(family, f"N{N}-L{L}-H{H}-M{M}-D{D}", leaves, dict(kernel="sigmoid"), _attn_expr("sigmoid"),
                   floored=("q", "k") if L == 1 else ())


# `simple` (N == L).  (H, M, D): vector prep + narrow row-GEMM + fused dq|dk|dv buffer; two heads; scalar prep (M % 4 != 0);
# prep_vec<2> + wide row-GEMM; the widest script shape; M != D (separate gradient buffers); and -- read off
# dif_simple_bwd_prep_f32 -- three heads on the VECTOR prep, whose workgroup count is lowered until 16 x count is a multiple
# of H, so that a 16-lane group keeps its head (N = 1: reaches zero and falls back to H; 17: 4 -> 3; 65: 13 -> 12)
SIMPLE = [(1, 1, 64, 64), (1, 3, 10, 10), (1, 1, 300, 300), (1, 3, 12, 12),
          (2, 2, 16, 16), (2, 1, 128, 128),
          (3, 3, 10, 10), (3, 2, 100, 36),
          (15, 1, 64, 64), (15, 2, 100, 36),
          (16, 2, 16, 16), (16, 1, 128, 128),
          (17, 1, 64, 64), (17, 3, 10, 10), (17, 3, 12, 12), (17, 1, 300, 300),
          (63, 2, 16, 16), (63, 1, 128, 128),
          (64, 1, 64, 64), (64, 3, 10, 10),
          (65, 1, 300, 300), (65, 2, 100, 36), (65, 3, 12, 12),
          (257, 1, 64, 64), (257, 1, 128, 128), (257, 2, 16, 16)]


def simple_problem(N, H, M, D):
    # (draw 8: under draw 7 the float32 run of the oracle sat at 4.0e-5 on dk of N = 2, M = D = 128 with the tile cotangent --
    # the normalisation term -(T / |K|^2) k cancels against the main term there -- where the draws 8 .. 14 stay below 7e-6 on
    # every case of the table)
    g = _gen(N, H, M, D, 8)
    leaves = dict(q=_randn(g, N, H, M), k=_randn(g, N, H, M), v=_randn(g, N, H, D))
    # one node: out = v whatever q and k are (difformer.py:25-39 with N = 1)
    return Problem("simple", f"N{N}-H{H}-M{M}-D{D}", leaves, dict(kernel="simple"), _attn_expr("simple"),
                   floored=("q", "k") if N == 1 else ())


# ---- d: layer tail ---------------------------------------------------------------------------------------------------
def tail_group(D):
    """Lanes per row of layer_tail_bwd_kernel<G, V> (csrc/layer_tail_bwd.hip tail_group); a workgroup holds 256 / G rows."""
    q = D // 4
    return next(g for g in (1, 2, 4, 8, 16, 32, 64) if q <= g or g == 64)


def tail_rows(D):
    return 256 // tail_group(D)


TAIL_WIDTHS = (4, 16, 64, 128, 256, 300, 512)
TAIL_ALPHA = 0.3
# (use_x0, use_prev, use_ln, relu): the combinations of test_layer_tail_backward_kernel_matches_float64_autograd
_TAIL_FLAGS = [(True, True, True, False), (False, True, True, False), (True, False, True, True), (False, False, True, True),
               (True, True, False, False), (False, False, False, True)]


def tail_cases():
    """(n, H, D, use_x0, use_prev, use_ln, relu): n in {1, R - 1, R, R + 1, 2 R + 1} per width (R rows per workgroup), the
    flag combinations dealt round-robin; the first case of every width has a LayerNorm (record fold and finalize run)."""
    out, i = [], 0
    for D in TAIL_WIDTHS:
        R = tail_rows(D)
        for j, n in enumerate(sorted({1, R - 1, R, R + 1, 2 * R + 1} - {0})):
            flags = _TAIL_FLAGS[i % len(_TAIL_FLAGS)]
            if j == 0 and not flags[2]:
                flags = _TAIL_FLAGS[0]
            out.append((n, 1 + (i % 2), D) + flags)
            i += 1
    return out


def _tail_expr(t, c):
    z = t["conv"].mean(dim=1)
    if "x0" in t:
        z = z + t["x0"]
    if "prev" in t:
        z = TAIL_ALPHA * z + (1 - TAIL_ALPHA) * t["prev"]
    if "w" in t:
        z = F.layer_norm(z, (z.shape[-1],), t["w"], t["b"], 1e-5)
    return torch.relu(z) if c["relu"] else z


def tail_problem(n, H, D, use_x0, use_prev, use_ln, relu):
    g = _gen(n, H, D, use_x0, use_prev, use_ln, relu)
    leaves = dict(conv=_randn(g, n, H, D))
    if use_x0:
        leaves["x0"] = _randn(g, n, D)
    if use_prev:
        leaves["prev"] = _randn(g, n, D)
    if use_ln:
        leaves["w"] = torch.rand(D, generator=g) + 0.5
        leaves["b"] = _randn(g, D)
    name = f"n{n}-H{H}-D{D}" + "".join(s for s, f in zip(("-x0", "-prev", "-ln", "-relu"), (use_x0, use_prev, use_ln, relu)) if f)
    return Problem("tail", name, leaves, dict(relu=relu), _tail_expr)


# ---- e: Linear --------------------------------------------------------------------------------------------------------
LINEAR = [(n, ci, co) for ci, co in ((64, 192), (8, 64), (100, 40)) for n in (1, 2, 15, 17, 63, 65)]


def linear_problem(n, ci, co):
    g = _gen(n, ci, co)
    leaves = dict(x=_randn(g, n, ci), w=_randn(g, co, ci) / ci ** 0.5, b=_randn(g, co))
    return Problem("linear", f"n{n}-{ci}-{co}", leaves, {}, lambda t, c: F.linear(t["x"], t["w"], t["b"]))


# ---- f: closed form ---------------------------------------------------------------------------------------------------
# (n, C, D, with dx_in): every n with every (C, D), dx_in given in every other case
CLOSED_FORM = [(n, C, D, (i + j) % 2 == 0) for i, n in enumerate((1, 15, 16, 17, 47, 48, 49, 65))
               for j, (C, D) in enumerate(((64, 64), (32, 64), (64, 16)))]
CF_TENSORS = ("d_num", "d_den", "dx", "d_u", "d_cd", "rs_d")
CC_TENSORS = ("S", "t", "dWq", "dbq", "dWk", "dbk", "dWv", "dbv")


def closed_form_operands(n, C, D, with_dx):
    """Operands of test_closed_form_attention_backward_kernel (float32 host tensors): x, coef, dx0 | None, rs."""
    g = _gen(n, C, D, 11)
    x = _randn(g, n, C)
    coef = _randn(g, D * C + D + C + 4) * 0.2
    coef[D * C + D + C] = 25.0                                       # cd: keeps the denominator away from zero
    dx0 = _randn(g, n, C) if with_dx else None
    rs = torch.rand(n, generator=g) + 0.5
    return x, coef, dx0, rs


def closed_form_reference(x, coef, dd, dx0, rs, D, dtype=torch.float64):
    """Backward of att = (x Mn + cn) / (x u + cd) (difformer.py:25-39 in closed form) in `dtype` -> {CF_TENSORS: float64
    ndarray}: d_num, d_den, the gradient of the rows at fixed coefficients (+ dx0), and the three sums over rows the kernel
    leaves as per-workgroup partial records (x^T d_den, sum d_den, rs^T d)."""
    n, C = x.shape
    x_ = x.to(dtype).requires_grad_(True)
    cf, dd_ = coef.to(dtype), dd.to(dtype)
    MnT, cn, u, cd = cf[: D * C].view(D, C), cf[D * C: D * C + D], cf[D * C + D: D * C + D + C], cf[D * C + D + C]
    num, den = x_ @ MnT.t() + cn, x_ @ u + cd
    (gx,) = torch.autograd.grad(num / den[:, None], x_, dd_)
    if dx0 is not None:
        gx = gx + dx0.to(dtype)
    rn = dd_ / den.detach()[:, None]
    rd = -(rn * (num / den[:, None]).detach()).sum(1)
    res = dict(d_num=rn, d_den=rd, dx=gx, d_u=x_.detach().t() @ rd, d_cd=rd.sum().reshape(1), rs_d=dd_.t() @ rs.to(dtype))
    return {k: v.detach().numpy().astype(np.float64) for k, v in res.items()}


def coeff_operands(n, C, D):
    """Operands of test_coefficient_backward_kernel_vs_float64_tensor_ops: x, the projection parameters, the scale of the
    attention term and a gradient in the coefficients' layout [D*C | D | C | 1 | ...]."""
    g = _gen(n, C, D, 13)
    x = _randn(g, n, C) + 0.2
    p = {}
    for nm in ("q", "k", "v"):
        p["W" + nm] = _randn(g, D, C) / C ** 0.5
        p["b" + nm] = _randn(g, D) * 0.1
    dcoef = _randn(g, D * C + D + C + 2)
    dcoef[: D * C] *= 3.0
    return x, p, 0.7, dcoef


def gram_record(x):
    """[G = x^T x : C*C][sx = column sums : C] of float32 rows, formed in float64 (what dif_gram_f32 leaves, rounded once)."""
    x64 = x.double()
    return torch.cat([(x64.t() @ x64).reshape(-1), x64.sum(dim=0)]).float()


def coeffs_autograd(record, n, C, D, p, a, dcoef, dtype):
    """Gradients of <dcoef, coef(G~, W~)> by autograd in `dtype`, coef = [MnT | cn | u | cd] as in the docstring of
    ops.closed_form_coeffs_backward (which states the same derivative in closed form) -> {CC_TENSORS: float64 ndarray}."""
    r = record.to(dtype)
    Gt = torch.empty((C + 1, C + 1), dtype=dtype)
    Gt[:C, :C] = r[: C * C].view(C, C)
    Gt[:C, C] = r[C * C: C * C + C]
    Gt[C, :C] = r[C * C: C * C + C]
    Gt[C, C] = float(n)
    Gt.requires_grad_(True)
    W = {k: torch.cat([p["W" + k], p["b" + k][:, None]], dim=1).to(dtype).requires_grad_(True) for k in "qkv"}
    Ak = W["k"] @ Gt
    ktv, ksum, vsum = Ak @ W["v"].t(), Ak[:, C], (W["v"] @ Gt)[:, C]
    s = (((W["q"] @ Gt) * W["q"]).sum() * (Ak * W["k"]).sum()) ** -0.5
    P, rr = a * s * (W["q"].t() @ ktv), s * (W["q"].t() @ ksum)                  # [C + 1, D], [C + 1]
    coef = torch.cat([P[:C].t().reshape(-1), P[C] + a * vsum, rr[:C], rr[C].reshape(1) + float(n)])
    (coef * dcoef[: coef.numel()].to(dtype)).sum().backward()
    S = Gt.grad + Gt.grad.t()
    res = dict(S=S[:C, :C], t=S[C, :C])
    for k in "qkv":
        res["dW" + k], res["db" + k] = W[k].grad[:, :C], W[k].grad[:, C]
    return {k: v.numpy().astype(np.float64) for k, v in res.items()}


# ---- g: aggregation ---------------------------------------------------------------------------------------------------
def _gcn_expr(t, c):
    return og.gcn_conv(t["x"], c["edge_index"], t.get("w"))


def _gcn_problem(name, n, ei, weighted, H, D, seed):
    g = _gen(n, ei.shape[1], H, D, seed)
    leaves = dict(x=_randn(g, n, H, D))
    if weighted:
        leaves["w"] = torch.rand(ei.shape[1], generator=g) + 0.1
    return Problem("gcn", name, leaves, dict(edge_index=ei), _gcn_expr)


def gcn_problems():
    """One self loop; no edges at all; 15 / 16 / 17 edges (the edge-gradient kernel works in 16-lane groups, 16 edges per
    workgroup) with vector and scalar row loads; 300 weighted edges over 40 nodes of which the last five have no incoming
    entries, so the weight gradient of an edge leaving them is NaN (difformer.py:73-74)."""
    out = [_gcn_problem("N1-loop", 1, torch.zeros(2, 1, dtype=torch.int64), True, 1, 64, 0),
           _gcn_problem("N9-E0", 9, torch.zeros(2, 0, dtype=torch.int64), True, 2, 8, 0)]
    for e, (H, D) in zip((15, 16, 17), ((1, 64), (2, 5), (1, 16))):
        g = _gen(17, e)
        out.append(_gcn_problem(f"N17-E{e}-F{H * D}", 17, torch.randint(0, 17, (2, e), generator=g), True, H, D, 1))
    g = _gen(40, 300)
    ei = torch.stack([torch.randint(0, 40, (300,), generator=g), torch.randint(0, 35, (300,), generator=g)])
    out.append(_gcn_problem("N40-E300-iso5", 40, ei, True, 2, 16, 2))
    return out


# ---- h: batched attention of DIFFormer_v2 ----------------------------------------------------------------------------
BATCHES = ([1], [17], [1] * 33, [1, 40, 1, 16, 17])
BATCH_HEADS = ((1, 64), (2, 16))


def _batched_expr(t, c):
    fn = og.v2_simple_attention if c["kernel"] == "simple" else og.v2_sigmoid_attention
    return fn(t["q"], t["k"], t["v"], c["n_nodes"])


def batched_problem(kernel, n_nodes, H, D):
    n = sum(n_nodes)
    g = _gen(n, len(n_nodes), H, D, 17)
    s = D ** -0.25 if kernel == "sigmoid" else 1.0
    leaves = dict(q=_randn(g, n, H, D) * s, k=_randn(g, n, H, D) * s, v=_randn(g, n, H, D))
    # `simple` with one node in every graph: out = v whatever q and k are (difformer-v2.py:93-109 with n_b = 1)
    floored = ("q", "k") if kernel == "simple" and max(n_nodes) == 1 else ()
    name = f"{kernel}-B{len(n_nodes)}-n{n}-H{H}-D{D}"
    return Problem("batched", name, leaves, dict(kernel=kernel, n_nodes=list(n_nodes)), _batched_expr, floored)


# The batched sigmoid attention scores position b of a graph against position b of EVERY graph (difformer-v2.py:124): a batch
# of ONE graph ([1], [17]) leaves one node per position group, weight s / (s + 1e-9), and dq, dk ~ 1e-9 of dv -- neither zero
# (so the floor rule does not apply) nor resolvable: s + 1e-9 == s in float32, and the float32 run of the oracle misses the
# precondition there (tests/test_grad_edges_host.py test_single_graph_sigmoid_batches_are_ill_posed keeps the figures).  They
# are left out of the sigmoid table; the 33 one-node graphs and the ragged batch are well-posed.
BATCHES_SIGMOID = tuple(b for b in BATCHES if len(b) > 1)


def batched_problems():
    out = []
    for kernel, batches in (("simple", BATCHES), ("sigmoid", BATCHES_SIGMOID)):
        out += [batched_problem(kernel, b, H, D) for b in batches for H, D in BATCH_HEADS]
    return out


# ---- i: whole training step -------------------------------------------------------------------------------------------
STEP_NODES = (3, 17, 33, 65)
STEP_CONFIGS = [(kernel, hidden, heads) for kernel in ("simple", "sigmoid") for hidden, heads in ((64, 1), (32, 2), (128, 1))]
STEP_IN, STEP_CLASSES = 12, 5


# Model seed per `simple` case.  The `simple` kernel's Wq / Wk gradients are 1e-5 .. 1e-7 of the others (conftest.grad_err),
# and at these node counts the float32 run of the oracle lands between 2e-6 and 2e-4 on convs.*.Wk.bias depending on the
# draw of the parameters -- around the precondition of TOL / 4.  Rule: of the seeds 0 .. 9, the one whose float32 oracle run
# is closest to the float64 one (figure beside it); chosen from the oracle's own error alone, and held by
# tests/test_grad_edges_host.py.  `sigmoid` sits at <= 5e-6 with any seed and uses 0.
STEP_SEEDS = {
    ("simple", 64, 1, 3): 6,       # 3.9e-06
    ("simple", 64, 1, 17): 7,      # 4.6e-06
    ("simple", 64, 1, 33): 4,      # 6.5e-06
    ("simple", 64, 1, 65): 7,      # 7.7e-06
    ("simple", 32, 2, 3): 6,       # 5.8e-06
    ("simple", 32, 2, 17): 9,      # 1.2e-05
    ("simple", 32, 2, 33): 5,      # 6.8e-06
    ("simple", 32, 2, 65): 9,      # 9.3e-06
    ("simple", 128, 1, 3): 6,      # 5.2e-06
    ("simple", 128, 1, 17): 2,     # 7.4e-06
    ("simple", 128, 1, 33): 4,     # 7.2e-06
    ("simple", 128, 1, 65): 0,     # 4.0e-06
}


def step_model(kernel, hidden, heads, n):
    """The case's model on the host (train mode, dropout 0), parameters drawn from the case's seed."""
    from difformer_amd import DIFFormer
    torch.manual_seed(STEP_SEEDS.get((kernel, hidden, heads, n), 0))
    return DIFFormer(STEP_IN, hidden, STEP_CLASSES, num_layers=2, num_heads=heads, kernel=kernel, dropout=0.0).train()


def step_cfg(kernel, hidden, heads):
    return dict(hidden_channels=hidden, num_layers=2, num_heads=heads, kernel=kernel, alpha=0.5, use_bn=True,
                use_residual=True, use_weight=True, use_graph=True, graph_weight=-1, use_source=False)


def step_graph(n):
    """-> (x [n, 12], edge_index: 2 n random pairs made undirected + self loops, labels [n]); every node is in the loss."""
    g = _gen(n, 19)
    pairs = torch.randint(0, n, (2, 2 * n), generator=g)
    ei = torch.cat([pairs, pairs.flip(0), torch.arange(n).repeat(2, 1)], dim=1)
    return _randn(g, n, STEP_IN), ei, torch.randint(0, STEP_CLASSES, (n,), generator=g)


def step_reference(state, x, ei, y, cfg, dtype=torch.float64):
    """One training step of the oracle in `dtype` -> {parameter name | 'x': gradient as float64 ndarray}."""
    p = og.leaves({k: v.detach().cpu().numpy() for k, v in state.items()}, dtype)
    xl = x.detach().cpu().to(dtype).requires_grad_(True)
    loss = og.training_loss(og.difformer_forward(p, xl, ei.cpu(), None, cfg), y.cpu(), torch.arange(x.shape[0]))
    loss.backward()
    grads = {k: v.grad.numpy().astype(np.float64) for k, v in p.items() if v.grad is not None}
    grads["x"] = xl.grad.numpy().astype(np.float64)
    return grads


# ---- all op-level problems (the host test walks these) ---------------------------------------------------------------
def op_problems():
    out = [sigmoid_problem(c.N, c.L, c.H, c.M, c.D) for c in SIGMOID_NARROW]
    out += [sigmoid_problem(*c, family="sigmoid-wide") for c in SIGMOID_WIDE]
    out += [simple_problem(*c) for c in SIMPLE]
    out += [tail_problem(*c) for c in tail_cases()]
    out += [linear_problem(*c) for c in LINEAR]
    out += gcn_problems()
    out += batched_problems()
    return out


# ---- recording which entry points of the C ABI ran -------------------------------------------------------------------
class _Recorder:
    """Stands in for backend.lib: every `dif_*` function fetched from it notes its name when called."""

    def __init__(self, lib, seen):
        self.__dict__["_lib"], self.__dict__["_seen"] = lib, seen

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not (name.startswith("dif_") and callable(fn)):
            return fn

        def call(*args):
            self._seen.add(name)
            return fn(*args)
        return call


class entry_points:
    """with entry_points(be) as ran: ... -> `ran.symbols`: the C-ABI symbols called through the backend, `ran.labels`: the
    keys of backend.kernel_events (the label a launch is filed under is usually a family of symbols: the closed-form and
    coefficient backward are filed under their forward's).  Both are complete only after the block."""

    def __init__(self, be):
        self.be, self.symbols, self.labels = be, set(), set()

    def __enter__(self):
        self._lib = self.be.lib
        self.be.lib = _Recorder(self._lib, self.symbols)
        self.be.kernel_events = {}
        return self

    def __exit__(self, *exc):
        self.labels |= set(self.be.kernel_events or ())
        self.be.lib, self.be.kernel_events = self._lib, None
        return False


def report(problem, pattern, hip, f32):
    """One line per tensor for the error record (profiles/r09_backward_edges.txt): measured error of the HIP gradient and of
    the float32 run of the oracle, both against the float64 run."""
    for k in hip:
        print(f"edge | {problem} | {pattern} | {k} | hip {hip[k]:.2e} | f32-oracle {f32.get(k, float('nan')):.2e}")
