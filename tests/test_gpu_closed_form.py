"""Closed-form `simple` layer (csrc/simple_layer.hip) through the C ABI: Gram record, coefficients and the layer kernel
against the float64 oracle (oracle.* <- node classification/difformer.py:18-39, :63-79, :113-145, :200-203).
Tolerance 1e-4 (north_star) on max|y - y64| / max|y64|; measured errors are ~1e-6.
"""
import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import difformer_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


@pytest.mark.parametrize("n,c", [(1, 64), (15, 64), (16, 64), (1000, 64), (132534, 64), (5000, 32), (777, 8), (4099, 48)])
def test_gram_record_vs_numpy(n, c, dev):
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + c)
    x = torch.randn(n, c, generator=g) + 0.3
    rec, ys = ops.get_backend().gram(x.to(dev))
    assert ys is None
    rec = rec.cpu().numpy().astype(np.float64)
    x64 = x.double().numpy()
    G, sx = x64.T @ x64, x64.sum(0)
    assert rel_err(rec[: c * c].reshape(c, c), G) < 1e-5 and rel_err(rec[c * c: c * c + c], sx) < 1e-5


@pytest.mark.parametrize("n,c,d,use_weight", [(2708, 64, 64, True), (1, 64, 64, True), (300, 32, 64, True), (19717, 64, 64, True),
                                              (24576, 64, 64, False), (24577, 64, 64, True), (50000, 64, 64, True), (4000, 48, 20, True),
                                              (777, 8, 8, False)])
def test_gram_and_coefficients_in_one_call(n, c, d, use_weight, dev):
    """dif_gram_coeffs_f32 against dif_gram_f32 + dif_simple_coeffs_f32: up to 48 partial Gram records (24,576 rows) are summed
    inside the coefficient kernel (ascending chunk order; the finalize kernel sums in slices: the two differ in rounding only),
    beyond that the call runs the three launches itself.  Record against float64, coefficients against the two-call path, and
    the same bits on a second call."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + c + d)
    x = (torch.randn(n, c, generator=g) + 0.2).to(dev)
    W = [(torch.randn(d, c, generator=g) / np.sqrt(c)).to(dev) for _ in range(3)]
    b = [(torch.randn(d, generator=g) * 0.1).to(dev) for _ in range(3)]
    Wv, bv = (W[2], b[2]) if use_weight else (None, None)
    be = ops.get_backend()
    rec0, _ = be.gram(x)
    coef0 = be.simple_coeffs(rec0, n, c, d, W[0], b[0], W[1], b[1], Wv, bv, 0.7)
    rec1, coef1 = be.gram_coeffs(x, n, c, d, W[0], b[0], W[1], b[1], Wv, bv, 0.7)
    x64 = x.cpu().double().numpy()
    assert rel_err(rec1[: c * c].cpu().numpy().reshape(c, c), x64.T @ x64) < 1e-5
    assert rel_err(rec1[c * c: c * c + c].cpu().numpy(), x64.sum(0)) < 1e-5
    k = d * c + d + c + 1
    assert rel_err(coef1[:k].cpu().numpy(), coef0[:k].cpu().numpy()) < 1e-5
    rec2, coef2 = be.gram_coeffs(x, n, c, d, W[0], b[0], W[1], b[1], Wv, bv, 0.7)
    assert torch.equal(rec1[: c * c + c], rec2[: c * c + c]) and torch.equal(coef1[:k], coef2[:k])


def test_gram_writes_the_scaled_slice_major_copy(dev):
    from difformer_amd import ops
    n, c = 12000, 64
    g = torch.Generator().manual_seed(2)
    ei = torch.stack([torch.randint(0, n, (n * 64,), generator=g), torch.randint(n // 20, n, (n * 64,), generator=g)]).to(dev)
    x = torch.randn(n, c, generator=g).to(dev)
    csr = ops.csr_cache.get(ei, None, n, c * 4)
    sl = csr.sliced(0, n, c)
    assert sl is not None
    be = ops.get_backend()
    rec, ys = be.gram(x, csr.rowptr, sl.plan)
    ref = be.sliced_prescale(x, csr.rowptr, n, sl.plan)          # the stand-alone pass of gcn_sliced.hip
    assert torch.equal(ys, ref)                                   # same float ops -> same bits, zero padding included
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).float()
    assert (deg[: n // 20] == 0).all() and (ys[:, : n // 20] == 0).all()     # no incoming entries -> contributes nothing


def _params(c, d, g, use_weight=True):
    mk = lambda *s: torch.randn(*s, generator=g) * 0.3
    return dict(Wq=mk(d, c), bq=mk(d), Wk=mk(d, c), bk=mk(d), Wv=mk(d, c) if use_weight else None,
                bv=mk(d) if use_weight else None)


@pytest.mark.parametrize("n,c,d,use_weight", [(500, 64, 64, True), (132534, 64, 64, True), (3000, 32, 64, True),
                                              (2000, 64, 16, True), (1500, 48, 48, False)])
def test_closed_form_attention_matches_the_simple_kernel(n, c, d, use_weight, dev):
    """coefficients + layer kernel with no graph, residual or norm == full_attention_conv(q, k, v, 'simple')[:, 0, :]."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + c + d)
    x = torch.randn(n, c, generator=g)
    p = _params(c, d, g, use_weight)
    be = ops.get_backend()
    td = lambda a: None if a is None else a.to(dev)
    rec, _ = be.gram(x.to(dev))
    coef = be.simple_coeffs(rec, n, c, d, td(p["Wq"]), td(p["bq"]), td(p["Wk"]), td(p["bk"]), td(p["Wv"]), td(p["bv"]), 1.0)
    out = be.simple_layer(x.to(dev), coef, d).cpu().numpy()
    x64 = x.double().numpy()
    lin = lambda W, b: x64 @ W.double().numpy().T + b.double().numpy()
    q, k = lin(p["Wq"], p["bq"]), lin(p["Wk"], p["bk"])
    v = lin(p["Wv"], p["bv"]) if use_weight else x64
    ref = orc.simple_attention(q[:, None, :], k[:, None, :], v[:, None, :])[:, 0, :]
    assert rel_err(out, ref) < TOL
    # the output is ~ mean(v) + O(1/N), which hides the query-dependent part: check the coefficients themselves
    # (num = x Mn + cn, den = x.u + cd) against their float64 definitions
    Wq, bq = p["Wq"].double().numpy(), p["bq"].double().numpy()
    sc = 1.0 / (np.sqrt((q * q).sum()) * np.sqrt((k * k).sum()))
    ktv, ksum, vsum = k.T @ v, k.sum(0), v.sum(0)
    cf = coef.cpu().numpy().astype(np.float64)
    MnT, cn, u, cd = cf[: d * c].reshape(d, c), cf[d * c: d * c + d], cf[d * c + d: d * c + d + c], cf[d * c + d + c]
    assert rel_err(MnT, (sc * Wq.T @ ktv).T) < 1e-4 and rel_err(cn, sc * bq @ ktv + vsum) < 1e-5
    assert rel_err(u, sc * Wq.T @ ksum) < 1e-4 and abs(cd - (sc * bq @ ksum + n)) < 1e-5 * n
    s_, q2, k2 = cf[-3:]
    assert abs(q2 - (q * q).sum()) <= 1e-5 * (q * q).sum() and abs(k2 - (k * k).sum()) <= 1e-5 * (k * k).sum()
    assert abs(s_ - sc) <= 1e-5 * sc


@pytest.mark.parametrize("n,deg,c,use_weight,graph_weight,use_source,ln,residual",
                         [(20000, 60, 64, True, -1, False, True, True),          # sliced SpMM on x
                          (3000, 8, 64, True, 0.3, True, True, True),            # lane-group SpMM, convex mix, + x0
                          (9000, 70, 64, False, -1, False, True, True),          # use_weight = False
                          (4000, 10, 32, True, -1, False, False, False),         # narrow, no tail
                          (2500, 6, 64, True, -1, True, False, True),
                          # the scripts' widths (run.sh: hidden 300 / 400; beyond 128 columns): Gram record + row GEMMs
                          (6000, 8, 192, True, -1, False, True, True),
                          (5000, 5, 300, True, 0.4, True, True, True),
                          (4000, 6, 400, False, -1, False, True, False),
                          (3000, 6, 512, True, -1, False, True, True),          # the widest closed-form layer (ops.CLOSED_FORM_WIDE_MAX; ADVICE r5: raised)
                          (9000, 60, 132, True, -1, False, True, True),         # wide rows on the sliced product
                          # hidden 65..128 (run.sh:42-44 trains Pokec at 128): the one-pass kernel of csrc/simple_layer_wide.hip
                          (9000, 60, 128, True, -1, False, True, True),         # ... behind the sliced product at 128 columns
                          (5000, 7, 128, True, 0.3, True, True, True),          # gather SpMM, convex mix, + x0
                          (4000, 9, 96, False, -1, False, True, True),          # use_weight = False
                          (3000, 5, 68, True, -1, True, False, False),          # no tail, + x0, padding columns
                          (100000, 3, 128, True, -1, False, True, True)])       # a Pokec batch at the script's width
def test_closed_form_layer_vs_oracle(n, deg, c, use_weight, graph_weight, use_source, ln, residual, dev):
    from difformer_amd import DIFFormerConv
    torch.manual_seed(n)
    g = torch.Generator().manual_seed(n + 1)
    conv = DIFFormerConv(c, c, 1, kernel="simple", use_graph=True, use_weight=use_weight, graph_weight=graph_weight,
                         use_source=use_source).to(dev).eval()
    x = torch.randn(n, c, generator=g)
    x0 = torch.randn(n, c, generator=g)
    ei = torch.cat([torch.randint(0, n, (2, n * deg), generator=g), torch.arange(n).repeat(2, 1)], dim=1)
    lw, lb = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
    xd = x.to(dev)
    with torch.no_grad():
        out, _, _ = conv._layer(xd, xd, ei.to(dev), None, x0.to(dev) if use_source else None, xd if residual else None, 0.4,
                                lw.to(dev) if ln else None, lb.to(dev) if ln else None, 1e-5)
    p = {"c." + k: v.detach().cpu().double().numpy() for k, v in conv.state_dict().items()}
    cfg = dict(num_heads=1, kernel="simple", use_graph=True, use_weight=use_weight, graph_weight=graph_weight,
               use_source=use_source, hidden_channels=c)
    x64 = x.double().numpy()
    z = orc.difformer_conv(p, "c.", x64, x64, ei.numpy(), None, x0.double().numpy(), cfg)
    if residual:
        z = 0.4 * z + 0.6 * x64
    if ln:
        z = orc.layer_norm(z, lw.double().numpy(), lb.double().numpy())
    assert rel_err(out.cpu().numpy(), z) < TOL
    if c > 64:      # wide: same numbers as the q / k / v operator path (want_qk forces it)
        with torch.no_grad():
            old, q, _ = conv._layer(xd, xd, ei.to(dev), None, x0.to(dev) if use_source else None, xd if residual else None,
                                    0.4, lw.to(dev) if ln else None, lb.to(dev) if ln else None, 1e-5, want_qk=True)
        assert q is not None and rel_err(out.cpu().numpy(), old.cpu().numpy()) < (2e-5 if c <= 128 else 1e-5)


def test_wide_layer_kernel_without_graph(dev):
    """use_graph = False at hidden 128: the one-pass kernel with the attention term only, against the operator path."""
    from difformer_amd import DIFFormerConv, ops
    if ops.EXACT_FP32:
        pytest.skip("asserts the default kernel choices (split-bfloat16 products); DIFFORMER_EXACT_FP32=1 takes the fp32 paths")
    torch.manual_seed(5)
    conv = DIFFormerConv(128, 128, 1, kernel="simple", use_graph=False).to(dev).eval()
    x = torch.randn(30000, 128, device=dev)
    lw, lb = torch.rand(128, device=dev) + 0.5, torch.randn(128, device=dev)
    be = ops.get_backend()
    be.kernel_events = {}
    with torch.no_grad():
        new, _, _ = conv._layer(x, x, None, None, None, x, 0.5, lw, lb, 1e-5)
    launched, be.kernel_events = set(be.kernel_events), None
    with torch.no_grad():
        old, q, k = conv._layer(x, x, None, None, None, x, 0.5, lw, lb, 1e-5, want_qk=True)
    assert "dif_gram_sym_f32" in launched and "dif_layer_tail_mix_f32" not in launched, launched
    assert q is not None and rel_err(new.cpu().numpy(), old.cpu().numpy()) < 2e-5


def test_closed_form_layer_without_graph_matches_the_operator_path(dev):
    """use_graph = False (BASELINE config C3): closed form vs the q/k/v path of round 1 (want_qk forces it)."""
    from difformer_amd import DIFFormerConv
    torch.manual_seed(3)
    conv = DIFFormerConv(64, 64, 1, kernel="simple", use_graph=False).to(dev).eval()
    x = torch.randn(50000, 64, device=dev)
    lw, lb = torch.rand(64, device=dev) + 0.5, torch.randn(64, device=dev)
    with torch.no_grad():
        new, _, _ = conv._layer(x, x, None, None, None, x, 0.5, lw, lb, 1e-5)
        old, q, k = conv._layer(x, x, None, None, None, x, 0.5, lw, lb, 1e-5, want_qk=True)
    assert q is not None and rel_err(new.cpu().numpy(), old.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("n,deg,c", [(20000, 60, 64), (3000, 8, 32), (12345, 0, 64), (5000, 0, 32)])
def test_layer_kernel_leaves_the_next_layers_copy(n, deg, c, dev):
    """want_next: the slice-major copy of the OUTPUT comes out of the same pass (from the layer kernel's registers) and equals,
    bit for bit, what dif_gram_f32 writes from that output; the next layer's Gram record is computed fresh."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, c, generator=g).to(dev)
    p = {k: (None if v is None else v.to(dev)) for k, v in _params(c, c, g).items()}
    lw, lb = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    be = ops.get_backend()
    csr = sl = None
    if deg:
        ei = torch.cat([torch.randint(0, n, (2, n * deg), generator=g), torch.arange(n).repeat(2, 1)], dim=1).to(dev)
        csr = ops.csr_cache.get(ei, None, n, c * 4)
        sl = csr.sliced(0, n, c)
    carry = ops.LayerChain(want_next=True)
    out = ops.simple_layer_closed_form(x, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], csr, 1.0, 1.0, None, True, 0.5,
                                       lw, lb, 1e-5, carry=carry)
    if sl is not None:
        prod = carry.products
        assert prod is not None and prod["x"] is out and prod["sl"] is sl
        assert prod["record"] is None
        assert torch.equal(prod["ys"], be.gram(out, csr.rowptr, sl.plan)[1])
    else:
        assert carry.products is None              # no sliced product: no copy to leave (and no ys)
    # and the next layer uses them: same result as a fresh call without the carry
    a = ops.simple_layer_closed_form(out, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], csr, 1.0, 1.0, None, True, 0.5,
                                     lw, lb, 1e-5, carry=carry)
    b = ops.simple_layer_closed_form(out, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], csr, 1.0, 1.0, None, True, 0.5,
                                     lw, lb, 1e-5)
    assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-5


class _EmulatedShard:
    """One rank of a row-sharded run, emulated inside one process: the all-reduce hands back the record of the whole
    matrix, the all-gather all source rows (what the collectives of dist.RowShard would deliver)."""

    def __init__(self, x_full, rec_full, counts, rank):
        self.world, self.rank, self.n_global, self.counts = len(counts), rank, x_full.shape[0], counts
        self.offsets = [0] + list(np.cumsum(counts))
        self._x, self._rec = x_full, rec_full
        self.calls = []

    row_begin = property(lambda s: int(s.offsets[s.rank]))
    n_local = property(lambda s: int(s.counts[s.rank]))

    def all_reduce_sum(self, buf):
        self.calls.append("all_reduce")
        buf.copy_(self._rec)
        return buf

    def all_gather_rows_async(self, local):
        assert torch.equal(local, self._x[self.row_begin: self.row_begin + self.n_local])
        self.calls.append("all_gather")
        x = self._x

        class H:
            def wait(self_inner):
                return x
        return H()


@pytest.mark.parametrize("world,n,deg", [(2, 20000, 60), (4, 20000, 60), (3, 3000, 8)])
def test_closed_form_layer_row_sharded_rank_by_rank(world, n, deg, dev):
    """Every rank's closed-form layer (Gram record of its rows -> all-reduce -> coefficients -> all-gather of x -> the
    product over its destination rows -> layer kernel) reproduces its rows of the unsharded layer."""
    from difformer_amd import ops
    from difformer_amd.dist import split_rows
    c = 64
    g = torch.Generator().manual_seed(world)
    x = torch.randn(n, c, generator=g).to(dev)
    p = {k: v.to(dev) for k, v in _params(c, c, g).items()}
    lw, lb = (torch.rand(c, generator=g) + 0.5).to(dev), torch.randn(c, generator=g).to(dev)
    ei = torch.cat([torch.randint(0, n, (2, n * deg), generator=g), torch.arange(n).repeat(2, 1)], dim=1).to(dev)
    csr = ops.csr_cache.get(ei, None, n, c * 4)
    args = (p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], csr, 1.0, 1.0, None, True, 0.5, lw, lb, 1e-5)
    full = ops.simple_layer_closed_form(x, *args)
    rec_full, _ = ops.get_backend().gram(x)
    counts = split_rows(n, world)
    lo = 0
    for r in range(world):
        sh = _EmulatedShard(x, rec_full, counts, r)
        out = ops.simple_layer_closed_form(x[lo: lo + counts[r]].contiguous(), *args, shard=sh)
        assert sh.calls == ["all_gather", "all_reduce"]            # the gather is started first, the reduce follows the Gram pass
        if deg >= 48:
            assert csr.sliced(lo, counts[r], c) is not None        # the shard has its own sliced format
        assert rel_err(out.cpu().numpy(), full[lo: lo + counts[r]].cpu().numpy()) < 1e-5, (world, r)
        lo += counts[r]


@pytest.mark.parametrize("n,deg,c,use_weight,use_source", [(30000, 3, 64, True, False), (5000, 6, 64, False, True),
                                                            (7000, 4, 32, True, True)])
def test_closed_form_layer_bf16_storage(n, deg, c, use_weight, use_source, dev):
    """BASELINE config C5: bfloat16 activations and parameters, float32 arithmetic (dif_gram_bf16, dif_simple_layer_bf16,
    coefficients from exact float32 copies of the parameters) -- against the float64 oracle on the bf16-rounded operands,
    and against the float32 closed form on the same rounded operands (differs only by the rounding of the output and of
    the aggregated rows)."""
    from difformer_amd import DIFFormerConv, ops
    torch.manual_seed(n)
    g = torch.Generator().manual_seed(n + 1)
    conv = DIFFormerConv(c, c, 1, kernel="simple", use_graph=True, use_weight=use_weight, use_source=use_source)
    conv = conv.to(torch.bfloat16).to(dev).eval()
    bf = lambda t: t.to(torch.bfloat16)
    x, x0 = bf(torch.randn(n, c, generator=g)), bf(torch.randn(n, c, generator=g))
    lw, lb = bf(torch.rand(c, generator=g) + 0.5), bf(torch.randn(c, generator=g))
    ei = torch.cat([torch.randint(0, n, (2, n * deg), generator=g), torch.arange(n).repeat(2, 1)], dim=1)
    xd, eid = x.to(dev), ei.to(dev)
    be = ops.get_backend()
    be.kernel_events = {}
    with torch.no_grad():
        out, _, _ = conv._layer(xd, xd, eid, None, x0.to(dev) if use_source else None, xd, 0.4, lw.to(dev), lb.to(dev), 1e-5)
    launched, be.kernel_events = set(be.kernel_events), None
    assert out.dtype == torch.bfloat16 and "dif_simple_layer_f32" in launched and "dif_simple_apply_f32" not in launched
    p = {"c." + k: v.detach().cpu().double().numpy() for k, v in conv.state_dict().items()}
    cfg = dict(num_heads=1, kernel="simple", use_graph=True, use_weight=use_weight, graph_weight=-1,
               use_source=use_source, hidden_channels=c)
    x64 = x.double().numpy()
    z = orc.difformer_conv(p, "c.", x64, x64, ei.numpy(), None, x0.double().numpy(), cfg)
    z = orc.layer_norm(0.4 * z + 0.6 * x64, lw.double().numpy(), lb.double().numpy())
    assert rel_err(out.float().cpu().numpy(), z) < 1e-2
    conv32 = conv.float()
    with torch.no_grad():
        ref32, _, _ = conv32._layer(xd.float(), xd.float(), eid, None, x0.float().to(dev) if use_source else None, xd.float(), 0.4,
                                    lw.float().to(dev), lb.float().to(dev), 1e-5)
    assert rel_err(out.float().cpu().numpy(), ref32.cpu().numpy()) < 1e-2


@pytest.mark.parametrize("n,c,d,use_weight", [(20000, 64, 64, True), (5000, 32, 32, True), (9000, 64, 64, False),
                                              (3000, 48, 64, True), (70, 64, 32, True)])
def test_background_coefficient_chain_matches_the_coefficient_kernel(n, c, d, use_weight, dev):
    """csrc/side_chain.hip (single-wave workgroups without LDS, made to run beside the sliced product): Gram partials
    per wave -> padded augmented Gram matrix -> two tiled 80 x 80 products against the cached weight-only factors give
    the same coefficients as dif_gram_f32 + dif_simple_coeffs_f32 -- from x and from a finished record."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + c)
    x = torch.randn(n, c, generator=g).to(dev)
    p = {k: (None if v is None else v.to(dev)) for k, v in _params(c, d, g, use_weight).items()}
    be = ops.get_backend()
    rec, _ = be.gram(x)
    want = be.simple_coeffs(rec, n, c, d, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], 0.7).cpu().numpy().astype(np.float64)
    f = ops.NarrowFactors(p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"])
    for got in (be.coeffs_bg(x, None, n, f, c, d, 0.7), be.coeffs_bg(None, rec, n, f, c, d, 0.7)):
        got = got.cpu().numpy().astype(np.float64)
        MnT, cn, u, tail = slice(0, d * c), slice(d * c, d * c + d), slice(d * c + d, d * c + d + c), slice(d * c + d + c, None)
        for part in (MnT, cn, u):
            assert rel_err(got[part], want[part]) < 2e-5
        assert np.allclose(got[tail], want[tail], rtol=2e-5, atol=0)
    assert torch.equal(be.coeffs_bg(x, None, n, f, c, d, 0.7), be.coeffs_bg(x, None, n, f, c, d, 0.7))      # deterministic


@pytest.mark.parametrize("n,deg,hidden,classes,f_in", [(20000, 60, 64, 112, 8), (3000, 8, 64, 7, 40), (5000, 0, 32, 10, 64),
                                                        (4000, 6, 64, 128, 16), (2500, 5, 48, 2, 20)])
def test_output_linear_rides_in_the_last_layer_kernel(n, deg, hidden, classes, f_in, dev):
    """dif_simple_layer_head_f32: the model's output Linear (difformer.py:208) applied to the finished rows inside the last
    closed-form layer kernel -- the whole model against the float64 oracle and against the two-kernel path."""
    from difformer_amd import DIFFormer, ops
    torch.manual_seed(n + classes)
    use_graph = deg > 0
    cfg = dict(hidden_channels=hidden, num_layers=2, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
               use_weight=True, use_graph=use_graph, graph_weight=-1, use_source=False)
    model = DIFFormer(f_in, hidden, classes, num_layers=2, num_heads=1, kernel="simple", use_graph=use_graph).to(dev).eval()
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, f_in, generator=g)
    ei = torch.cat([torch.randint(0, n, (2, n * max(deg, 1)), generator=g), torch.arange(n).repeat(2, 1)], dim=1) if use_graph else None
    be = ops.get_backend()
    calls = []
    orig = be.lib.dif_simple_layer_head_f32
    with torch.no_grad():
        out = model(x.to(dev), ei.to(dev) if use_graph else None)
        # the same model with the head un-fused: the last layer leaves its rows, a separate Linear follows
        x1 = model._input_layer(x.to(dev), False)
        layer_ = [x1]
        for i, conv in enumerate(model.convs):
            bn = model.bns[i + 1]
            x1, _, _ = conv._layer(x1, x1, ei.to(dev) if use_graph else None, None, None, layer_[i], model.alpha, bn.weight,
                                   bn.bias, bn.eps)
            layer_.append(x1)
        two = torch.nn.functional.linear(x1, model.fcs[-1].weight, model.fcs[-1].bias)
    p = {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()}
    ref = orc.difformer_forward(p, x.double().numpy(), ei.numpy() if use_graph else None, None, cfg)
    assert out.shape == (n, classes)
    assert rel_err(out.cpu().numpy(), ref) < TOL
    assert rel_err(out.cpu().numpy(), two.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("n,c,dtype,use_weight,graph_weight,use_source,ln,head",
                         [(100003, 64, torch.float32, True, -1, False, True, 0),
                          (100003, 64, torch.bfloat16, True, -1, False, True, 0),
                          (2708, 64, torch.float32, True, -1, False, True, 7),         # Cora-size, output Linear in the pass
                          (5001, 64, torch.bfloat16, True, -1, True, True, 2),
                          (3333, 32, torch.float32, True, 0.3, True, True, 0),
                          (4097, 48, torch.float32, False, -1, False, False, 0),        # use_weight = False: rows are the term
                          (17, 64, torch.float32, True, -1, False, True, 0),
                          (9000, 40, torch.bfloat16, False, 0.6, False, True, 40)])
def test_layer_kernel_aggregates_sparse_graphs_itself(n, c, dtype, use_weight, graph_weight, use_source, ln, head, dev):
    """dif_simple_layer_gather_*: on graphs with a few entries per row the closed-form layer walks the CSR inside its own
    kernel (gcn_conv, difformer.py:59-73, folded into DIFFormerConv.forward :107-130) -- same numbers as SpMM launch +
    layer kernel, and the oracle's.  Ragged rows: Zipf-distributed sources, rows without entries, isolated tail rows."""
    from difformer_amd import DIFFormerConv, ops
    torch.manual_seed(n)
    g = torch.Generator().manual_seed(n + 3)
    conv = DIFFormerConv(c, c, 1, kernel="simple", use_graph=True, use_weight=use_weight, graph_weight=graph_weight,
                         use_source=use_source).to(dtype).to(dev).eval()
    cast = lambda t: t.to(dtype)
    x, x0 = cast(torch.randn(n, c, generator=g)), cast(torch.randn(n, c, generator=g))
    lw, lb = cast(torch.rand(c, generator=g) + 0.5), cast(torch.randn(c, generator=g))
    e = 3 * n
    dst = torch.randint(0, max(n - n // 10, 1), (e,), generator=g)              # the last tenth of the rows has no entries
    src = (torch.rand(e, generator=g) ** 3 * n).long().clamp_(max=n - 1)        # popular sources
    loops = torch.arange(0, n, 2)                                               # every other row carries a self loop
    ei = torch.stack([torch.cat([src, loops]), torch.cat([dst, loops])])
    hw = hb = None
    if head:
        hw, hb = cast(torch.randn(head, c, generator=g) * 0.2).float(), cast(torch.randn(head, generator=g)).float()
    be = ops.get_backend()
    xd, eid = x.to(dev), ei.to(dev)
    run = lambda: conv._layer(xd, xd, eid, None, x0.to(dev) if use_source else None, xd, 0.4, lw.to(dev) if ln else None,
                              lb.to(dev) if ln else None, 1e-5, carry=ops.LayerChain(head=(cast(hw).to(dev), cast(hb).to(dev))) if head else None)[0]
    # (a graph seen for the first time keeps the SpMM launch until its longest row is known: the read is not waited for)
    assert ops.csr_cache.get(eid, None, n, c * xd.element_size(), None, xd.element_size()).max_degree() <= ops.LAYER_GATHER_MAX_ROW
    be.kernel_events = {}
    with torch.no_grad():
        out = run()
    launched, be.kernel_events = set(be.kernel_events), None
    assert "dif_simple_layer_f32" in launched and "dif_gcn_spmm_f32" not in launched
    prev, ops.LAYER_GATHER = ops.LAYER_GATHER, False
    try:
        be.kernel_events = {}
        with torch.no_grad():
            two = run()
        launched, be.kernel_events = set(be.kernel_events), None
    finally:
        ops.LAYER_GATHER = prev
    assert "dif_gcn_spmm_f32" in launched
    assert out.shape == ((n, head) if head else (n, c)) and out.dtype == dtype
    tol2 = 1e-5 if dtype == torch.float32 else 1e-2
    assert rel_err(out.float().cpu().numpy(), two.float().cpu().numpy()) < tol2
    p = {"c." + k: v.detach().cpu().double().numpy() for k, v in conv.state_dict().items()}
    cfg = dict(num_heads=1, kernel="simple", use_graph=True, use_weight=use_weight, graph_weight=graph_weight,
               use_source=use_source, hidden_channels=c)
    x64 = x.double().numpy()
    z = orc.difformer_conv(p, "c.", x64, x64, ei.numpy(), None, x0.double().numpy(), cfg)
    z = 0.4 * z + 0.6 * x64
    if ln:
        z = orc.layer_norm(z, lw.double().numpy(), lb.double().numpy())
    if head:
        z = z @ hw.double().numpy().T + hb.double().numpy()
    assert rel_err(out.float().cpu().numpy(), z) < (TOL if dtype == torch.float32 else 1e-2)


@pytest.mark.parametrize("n,c,d,use_weight", [(5000, 64, 64, True), (3000, 32, 64, True), (2000, 64, 16, True), (1500, 48, 48, False),
                                              (700, 8, 12, True), (132534, 64, 64, True)])
def test_coefficient_backward_kernel_vs_float64_tensor_ops(n, c, d, use_weight, dev):
    """dif_simple_coeffs_bwd_f32 (training through the Gram record) against ops.closed_form_coeffs_backward: the same
    formulas in float64 tensor ops, which tests/test_host_logic.py holds to torch autograd and, through the training step,
    to the reference's gradients."""
    from conftest import grad_err
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + c)
    be = ops.get_backend()
    x = (torch.randn(n, c, generator=g) + 0.2).to(dev)
    p = {k: (None if v is None else v.to(dev)) for k, v in _params(c, d, g, use_weight).items()}
    rec, _ = be.gram(x)
    a_s = 0.7
    coef = be.simple_coeffs(rec, n, c, d, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], a_s)
    dcoef = torch.randn(d * c + d + c + 2, generator=g).to(dev)
    dcoef[: d * c] *= 3.0
    got = be.simple_coeffs_backward(rec, n, c, d, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], a_s, coef, dcoef)
    ref = ops.closed_form_coeffs_backward(rec, n, c, d, p["Wq"], p["bq"], p["Wk"], p["bk"], p["Wv"], p["bv"], a_s,
                                          dcoef[: d * c].view(d, c), dcoef[d * c: d * c + d], dcoef[d * c + d: d * c + d + c],
                                          dcoef[d * c + d + c])
    names = ("S", "t", "dWq", "dbq", "dWk", "dbk", "dWv", "dbv")
    for name, a, b in zip(names, got, ref):
        if b is None:
            assert a is None
            continue
        b = b.cpu().numpy()
        assert grad_err(a.cpu().numpy(), b, float(np.abs(b).max())) < 2e-5, name


@pytest.mark.parametrize("n,c,d,with_dx", [(5000, 64, 64, True), (132534, 64, 64, False), (3001, 32, 64, True), (2000, 64, 16, False),
                                           (17, 48, 48, True), (1, 8, 12, False)])
def test_closed_form_attention_backward_kernel(n, c, d, with_dx, dev):
    """dif_closed_form_attn_bwd_f32 against float64 autograd of att = (x Mn + cn) / (x u + cd) (difformer.py:25-39 in closed
    form): d_num, d_den and the gradient of the rows at fixed coefficients."""
    from conftest import grad_err
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + c + d)
    be = ops.get_backend()
    x = torch.randn(n, c, generator=g)
    coef = torch.randn(d * c + d + c + 4, generator=g) * 0.2
    coef[d * c + d + c] = 25.0                                       # cd: keeps the denominator away from zero
    dd = torch.randn(n, d, generator=g)
    dx0 = torch.randn(n, c, generator=g) if with_dx else None
    rs = torch.rand(n, generator=g) + 0.5
    d_num, d_den, dx, d_u, d_cd, rs_d = be.closed_form_attn_backward(x.to(dev), coef.to(dev), d, dd.to(dev),
                                                                     None if dx0 is None else dx0.to(dev), rs.to(dev))
    x64 = x.double().requires_grad_(True)
    cf = coef.double()
    MnT, cn, u, cd = cf[: d * c].view(d, c), cf[d * c: d * c + d], cf[d * c + d: d * c + d + c], cf[d * c + d + c]
    num, den = x64 @ MnT.t() + cn, x64 @ u + cd
    (gx,) = torch.autograd.grad(num / den[:, None], x64, dd.double())
    if dx0 is not None:
        gx = gx + dx0.double()
    rn = dd.double() / den.detach()[:, None]
    rd = -(rn * (num / den[:, None]).detach()).sum(1)
    sums = (("d_u", d_u, x.double().t() @ rd), ("d_cd", d_cd.reshape(1), rd.sum().reshape(1)), ("rs_d", rs_d, dd.double().t() @ rs.double()))
    for name, a, b in (("d_num", d_num, rn), ("d_den", d_den, rd), ("dx", dx, gx)) + sums:
        b = b.numpy()
        assert grad_err(a.cpu().numpy(), b, float(np.abs(b).max())) < 1e-5, name


def test_closed_form_attention_backward_without_the_partial_sums(dev):
    """dif_closed_form_attn_bwd_f32 with sums = NULL (the lean variant): the same d_num, d_den, dx as with the sums."""
    from difformer_amd import ops
    be = ops.get_backend()
    n, c, d = 4099, 64, 64
    g = torch.Generator().manual_seed(9)
    x = torch.randn(n, c, generator=g).to(dev)
    coef = (torch.randn(d * c + d + c + 4, generator=g) * 0.2).to(dev)
    coef[d * c + d + c] = 25.0
    dd = torch.randn(n, d, generator=g).to(dev)
    d_num, d_den, dx, _, _, _ = be.closed_form_attn_backward(x, coef, d, dd)
    o_num, o_den, o_dx = torch.empty_like(d_num), torch.empty_like(d_den), torch.empty_like(dx)
    rc = be.lib.dif_closed_form_attn_bwd_f32(x.data_ptr(), c, n, c, d, coef.data_ptr(), dd.data_ptr(), d, None, 0, o_num.data_ptr(),
                                             o_den.data_ptr(), o_dx.data_ptr(), c, None, None, torch.cuda.current_stream(dev).cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert torch.equal(o_num, d_num) and torch.equal(o_den, d_den) and torch.equal(o_dx, dx)
    rs = torch.ones(n, device=dev)
    assert be.lib.dif_closed_form_attn_bwd_f32(x.data_ptr(), c, n, c, d, coef.data_ptr(), dd.data_ptr(), d, None, 0, o_num.data_ptr(),
                                               o_den.data_ptr(), o_dx.data_ptr(), c, rs.data_ptr(), None,
                                               torch.cuda.current_stream(dev).cuda_stream) != 0        # row_sums without sums


def test_graphs_with_a_long_row_keep_the_spmm_kernels(dev):
    """The layer kernel's own aggregation walks the rows of a tile in lock step, so a graph with a hub row (a citation
    graph's few-hundred-entry node) stays on the SpMM kernels, which split long rows over lanes: same numbers either way."""
    from difformer_amd import DIFFormerConv, ops
    n, c = 5000, 64
    g = torch.Generator().manual_seed(21)
    ei = torch.cat([torch.randint(0, n, (2, 3 * n), generator=g), torch.arange(n).repeat(2, 1),
                    torch.stack([torch.randint(0, n, (700,), generator=g), torch.full((700,), 11)])], dim=1).to(dev)
    conv = DIFFormerConv(c, c, 1, kernel="simple", use_graph=True).to(dev).eval()
    x = torch.randn(n, c, generator=g).to(dev)
    be = ops.get_backend()
    be.kernel_events = {}
    with torch.no_grad():
        out, _, _ = conv._layer(x, x, ei, None, None, x, 0.5, None, None, 1e-5)
    launched, be.kernel_events = set(be.kernel_events), None
    assert ops.csr_cache.get(ei, None, n, c * 4).max_degree() >= 700 and "dif_gcn_spmm_f32" in launched
    prev, ops.LAYER_GATHER_MAX_ROW = ops.LAYER_GATHER_MAX_ROW, 1 << 30
    try:
        be.kernel_events = {}
        with torch.no_grad():
            forced, _, _ = conv._layer(x, x, ei, None, None, x, 0.5, None, None, 1e-5)
        launched, be.kernel_events = set(be.kernel_events), None
    finally:
        ops.LAYER_GATHER_MAX_ROW = prev
    assert "dif_gcn_spmm_f32" not in launched
    assert rel_err(forced.cpu().numpy(), out.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_model_on_a_sparse_graph_with_zipf_in_degrees(dtype, dev):
    """A citation-like graph: three entries per row on average, Zipf-distributed in-degrees (the longest rows have hundreds
    to thousands of entries).  The closed-form layers keep the SpMM launch there and its kernel hands the long rows to whole
    blocks (csrc/gcn_spmm.hip, spmm_group_row_kernel); the model against the float64 oracle."""
    from difformer_amd import DIFFormer, ops
    n, f_in, hidden, classes = 20000, 24, 64, 5
    g = torch.Generator().manual_seed(31)
    wgt = 1.0 / torch.arange(1, n + 1, dtype=torch.float64) ** 0.9
    dst = torch.multinomial(wgt, 3 * n, replacement=True, generator=g)
    src = torch.randint(0, n, (3 * n,), generator=g)
    ei = torch.cat([torch.stack([src, dst]), torch.arange(n).repeat(2, 1)], dim=1)
    torch.manual_seed(2)
    model = DIFFormer(f_in, hidden, classes, num_layers=2, kernel="simple").to(dev).to(dtype).eval()
    x = torch.randn(n, f_in, generator=g).to(dtype)
    be = ops.get_backend()
    be.kernel_events = {}
    with torch.no_grad():
        out = model(x.to(dev), ei.to(dev))
    launched, be.kernel_events = set(be.kernel_events), None
    csr = ops.csr_cache.get(ei.to(dev), None, n, hidden * x.element_size())
    assert csr.max_degree() > 500 and "dif_gcn_spmm_f32" in launched
    cfg = dict(hidden_channels=hidden, num_layers=2, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
               use_weight=True, use_graph=True, graph_weight=-1, use_source=False)
    p = {k: v.detach().float().cpu().double().numpy() for k, v in model.state_dict().items()}
    ref = orc.difformer_forward(p, x.double().numpy(), ei.numpy(), None, cfg)
    assert rel_err(out.float().cpu().numpy(), ref) < (TOL if dtype == torch.float32 else 2e-2)


@pytest.mark.parametrize("hub", [0, 900])
def test_identical_calls_launch_identical_kernels(hub, dev):
    """kernel selection is a function of the graph alone.  The longest row -- which decides whether the
    closed-form layer kernel aggregates a sparse graph itself or the SpMM kernel is launched -- comes out of the CSR build
    (dif_csr_build status[1]) instead of an un-awaited host read that used to land some calls later: twenty calls on one
    graph give bitwise-equal logits and the same list of entry points, from the FIRST call on."""
    from difformer_amd import DIFFormer, ops
    n = 20000
    g = torch.Generator().manual_seed(9)
    ei = torch.cat([torch.randint(0, n, (2, 3 * n), generator=g), torch.arange(n).repeat(2, 1)], dim=1)
    if hub:
        ei = torch.cat([ei, torch.stack([torch.randint(0, n, (hub,), generator=g), torch.full((hub,), 7)])], dim=1)
    ei, x = ei.to(dev), torch.randn(n, 24, generator=g).to(dev)
    torch.manual_seed(4)
    model = DIFFormer(24, 64, 5, num_layers=3, kernel="simple").to(dev).eval()
    be = ops.get_backend()
    outs, lists = [], []
    with torch.no_grad():
        for _ in range(20):
            be.kernel_events = {}
            outs.append(model(x, ei).clone())
            lists.append(sorted((k, len(v)) for k, v in be.kernel_events.items() if k != "dif_csr_build"))
            be.kernel_events = None
    assert all(torch.equal(o, outs[0]) for o in outs[1:])
    # the first call also builds what is cached per graph (the CSR; with a bias in Wv one extra product for A_hat 1)
    assert all(l == lists[1] for l in lists[2:]), lists[:3]
    assert {k for k, _ in lists[0]} == {k for k, _ in lists[1]}
    names = {k for k, _ in lists[0]}
    assert ("dif_gcn_spmm_f32" in names) == bool(hub)              # no long row: the layer kernel aggregates itself
    csr = ops.csr_cache.get(ei, None, n, 64 * 4)
    assert csr._max_degree == int((csr.rowptr[1:] - csr.rowptr[:-1]).max())


@pytest.mark.parametrize("n,c_in,d,deg", [(9000, 8, 64, 50), (8200, 33, 64, 60), (12000, 64, 48, 50), (8193, 1, 64, 49)])
def test_input_layer_with_gram_and_copy_in_one_pass(n, c_in, d, deg, dev):
    """dif_input_gram_f32 (difformer.py:188-191 in front of a closed-form first layer on a dense graph): the hidden rows, their
    Gram record and the slice-major copy against the three kernels it replaces, and against float64."""
    from difformer_amd import ops
    be = ops.get_backend()
    g = torch.Generator().manual_seed(n + c_in)
    x = torch.randn(n, c_in, generator=g).to(dev)
    W, b = (torch.randn(d, c_in, generator=g) / max(c_in, 1) ** 0.5).to(dev), torch.randn(d, generator=g).to(dev)
    lw, lb = (torch.rand(d, generator=g) + 0.5).to(dev), torch.randn(d, generator=g).to(dev)
    ei = torch.cat([torch.randint(0, n, (2, deg * n), generator=g), torch.arange(n).repeat(2, 1)], dim=1).to(dev)
    csr = ops.csr_cache.get(ei, None, n, d * 4)
    sl = csr.sliced(0, n, d)
    assert sl is not None
    h, record, ys = be.input_gram(x, W, b, lw, lb, 1e-5, True, csr.rowptr, sl.plan)
    h_ref = be.linear(x, W, b, lw, lb, 1e-5, True)
    rec_ref, ys_ref = be.gram(h_ref, csr.rowptr, sl.plan)
    h64 = np.maximum(orc.layer_norm(x.double().cpu().numpy() @ W.double().cpu().numpy().T + b.double().cpu().numpy(),
                                    lw.double().cpu().numpy(), lb.double().cpu().numpy()), 0)
    assert rel_err(h.cpu().numpy(), h64) < 1e-5 and rel_err(h.cpu().numpy(), h_ref.cpu().numpy()) < 1e-6
    g64 = np.concatenate([(h64.T @ h64).ravel(), h64.sum(0)])
    assert rel_err(record[: d * d + d].cpu().numpy(), g64) < 1e-5
    assert rel_err(record[: d * d + d].cpu().numpy(), rec_ref[: d * d + d].cpu().numpy()) < 1e-5
    assert rel_err(ys.cpu().numpy(), ys_ref.cpu().numpy()) < 1e-6
    h2, record2, ys2 = be.input_gram(x, W, b, lw, lb, 1e-5, True, csr.rowptr, sl.plan)
    assert torch.equal(h, h2) and torch.equal(record, record2) and torch.equal(ys, ys2)          # deterministic
    h3, record3, none = be.input_gram(x, W, b, None, None, 1e-5, False)                          # no LayerNorm / ReLU / copy
    assert none is None and rel_err(h3.cpu().numpy(), x.double().cpu().numpy() @ W.double().cpu().numpy().T + b.double().cpu().numpy()) < 1e-5


def test_model_takes_the_fused_input_kernel_on_a_dense_graph(dev):
    from difformer_amd import DIFFormer, ops
    if ops.EXACT_FP32:
        pytest.skip("asserts the default kernel choices (split-bfloat16 products); DIFFORMER_EXACT_FP32=1 takes the fp32 paths")
    n, f_in, c = 9000, 8, 11
    torch.manual_seed(8)
    model = DIFFormer(f_in, 64, c, num_layers=3, kernel="simple").to(dev).eval()
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, f_in, generator=g)
    ei = torch.cat([torch.randint(0, n, (2, 50 * n), generator=g), torch.arange(n).repeat(2, 1)], dim=1)
    be = ops.get_backend()
    be.kernel_events = {}
    with torch.no_grad():
        y = model(x.to(dev), ei.to(dev)).cpu().numpy()
    calls, be.kernel_events = {k: len(v) for k, v in be.kernel_events.items()}, None
    assert calls.get("dif_input_gram_f32") == 1 and "dif_linear_f32" not in calls and "dif_gram_f32" not in calls, calls
    cfg = dict(hidden_channels=64, num_layers=3, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
               use_weight=True, use_graph=True, graph_weight=-1, use_source=False)
    p = {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()}
    assert rel_err(y, orc.difformer_forward(p, x.double().numpy(), ei.numpy(), None, cfg)) < 1e-4


@pytest.mark.parametrize("n,c", [(100000, 128), (5003, 96), (17, 68), (40000, 100), (50000, 300), (4096, 132), (9001, 320), (6000, 400)])
def test_gram_record_at_the_script_widths(n, c, dev):
    """The Gram record of the closed form beyond 64 columns (dif_gram_sym_f32: from 4,096 rows and up to 320 columns the one-read
    slab kernel on split-bfloat16 operands, round 5; else dif_gram128_f32 / the fp32 streaming reduce): X^T X -- the 64 x 64
    blocks on and above the diagonal, which is what the coefficient stage reads -- and the column sums against float64."""
    from difformer_amd import ops
    be = ops.get_backend()
    g = torch.Generator().manual_seed(n + c)
    x = (torch.randn(n, c, generator=g) + 0.3).to(dev)
    rec = be.gram_sym(x)
    x64 = x.double().cpu().numpy()
    got = rec[: c * c].cpu().numpy().reshape(c, c).astype(np.float64)
    blk = np.arange(c) // 64
    upper = blk[:, None] <= blk[None, :]
    got = np.where(upper, got, got.T)                                # the caller mirrors the blocks below the diagonal
    assert rel_err(got, x64.T @ x64) < 1e-5 and rel_err(rec[c * c: c * c + c].cpu().numpy(), x64.sum(0)) < 1e-5
    r2 = be.gram_sym(x)
    assert torch.equal(torch.where(torch.from_numpy(upper).to(dev), rec[: c * c].view(c, c), 0), torch.where(torch.from_numpy(upper).to(dev), r2[: c * c].view(c, c), 0))
    assert torch.equal(rec[c * c: c * c + c], r2[c * c: c * c + c])            # deterministic


@pytest.mark.parametrize("C,D,n", [(300, 300, 5000), (68, 68, 3000), (128, 128, 4000), (400, 400, 6000), (132, 96, 5000),
                                   (512, 512, 4000)])
def test_wide_coefficients_kernel_vs_float64_restatement(C, D, n, dev):
    """dif_wide_coeffs_f64 (round 5: both float64 products of the wide closed form on own kernels) against the same algebra
    in float64 tensor ops, entry by entry -- the model-level parity metric barely sees [Mn | u] (the attention of the `simple`
    kernel is mean(V) + O(1 / N)), so the operands themselves are held to 1e-6 here."""
    from difformer_amd import ops
    be = ops.get_backend()
    g = torch.Generator().manual_seed(C + n)
    x = torch.randn(n, C, generator=g).to(dev)
    Wq, Wk = (torch.randn(D, C, generator=g) / C ** 0.5).to(dev), (torch.randn(D, C, generator=g) / C ** 0.5).to(dev)
    Wv = (torch.randn(D, C, generator=g) / C ** 0.5).to(dev)
    bq, bk, bv = (torch.randn(D, generator=g) * 0.1).to(dev), (torch.randn(D, generator=g) * 0.1).to(dev), (torch.randn(D, generator=g) * 0.1).to(dev)
    co = ops.WideCoefficients(Wq, bq, Wk, bk, Wv, bv)
    rec = be.gram_sym(x)
    B, bias = be.wide_coeffs(rec, C, n, co.S, co.V, co.P)
    # the same algebra from the same record in float64 tensor ops: G~ with the lower 64-blocks mirrored, sum x and N appended
    G = rec[: C * C].view(C, C).double()
    blk = torch.arange(C, device=dev) // 64
    G = torch.where(blk[:, None] <= blk[None, :], G, G.t())
    sx = rec[C * C: C * C + C].double()
    Gt = torch.cat([torch.cat([G, sx[:, None]], dim=1), torch.cat([sx, torch.tensor([float(n)], dtype=torch.float64, device=dev)])[None, :]])
    q2, k2 = (co.S[0].view(C + 1, C + 1) * Gt).sum(), (co.S[1].view(C + 1, C + 1) * Gt).sum()
    s0 = 1.0 / (q2.sqrt() * k2.sqrt())
    T = Gt @ co.V
    R = co.P @ T
    B0, bias0 = (s0 * R[:C]).float(), (s0 * R[C] + T[C]).float()
    assert rel_err(B.cpu().numpy(), B0.cpu().numpy()) < 1e-6 and rel_err(bias.cpu().numpy(), bias0.cpu().numpy()) < 1e-6
    # and against the definition from x itself, in float64
    X = torch.cat([x.double(), torch.ones(n, 1, dtype=torch.float64, device=dev)], dim=1)
    Gd = X.t() @ X
    q2, k2 = (co.S[0].view(C + 1, C + 1) * Gd).sum(), (co.S[1].view(C + 1, C + 1) * Gd).sum()
    s = 1.0 / (q2.sqrt() * k2.sqrt())
    Td = Gd @ co.V
    Rd = co.P @ Td
    assert rel_err(B.cpu().numpy(), (s * Rd[:C]).cpu().numpy()) < 2e-5          # (the Gram record itself is float32 / split-bf16)
    assert rel_err(bias.cpu().numpy(), (s * Rd[C] + Td[C]).cpu().numpy()) < 2e-5
