"""Parity of the HIP path (through the C ABI) against the oracle and the committed golden vectors.

Tolerance (BASELINE.json north_star: 1e-4 rel fp32; metric of SURVEY.md section 8d):
    max|y - y64| / max|y64| <= 1e-4   against the float64 oracle / float64 reference run.
Integer / index work (CSR rowptr, source ids) and the per-entry values are checked BIT-EXACT.
"""
import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, split_model_case
from oracle import difformer_oracle as orc

pytestmark = pytest.mark.gpu

TOL = 1e-4
ATTN = load_golden("attn")
GCN = load_golden("gcn")
MODEL = load_golden("model")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------ a1 / a2 golden
@pytest.mark.parametrize("name", sorted(ATTN))
def test_full_attention_conv_golden(name, dev):
    from difformer_amd import full_attention_conv
    c = ATTN[name]
    out = full_attention_conv(t(c["q"], dev), t(c["k"], dev), t(c["v"], dev), str(c["kernel"]))
    assert out.shape == c["out_f64"].shape and out.dtype == torch.float32
    assert rel_err(out.cpu().numpy(), c["out_f64"]) < TOL


# ------------------------------------------------------------------ a6: dense attention maps (difformer.py:42-43, :58-59, :211-226)
ATTNW = load_golden("attnw")


@pytest.mark.parametrize("name", sorted(ATTNW))
def test_full_attention_conv_output_attn_golden(name, dev):
    """output_attn=True returns (out, [N, L, H] weights); fixtures are outputs of the reference itself."""
    from difformer_amd import full_attention_conv
    c = ATTNW[name]
    out, attn = full_attention_conv(t(c["q"], dev), t(c["k"], dev), t(c["v"], dev), str(c["kernel"]), output_attn=True)
    assert attn.shape == c["attn_f64"].shape and attn.dtype == torch.float32
    assert rel_err(out.cpu().numpy(), c["out_f64"]) < TOL
    assert rel_err(attn.cpu().numpy(), c["attn_f64"]) < TOL


@pytest.mark.parametrize("kernel,n,h,d", [("simple", 300, 1, 64), ("sigmoid", 300, 1, 64), ("sigmoid", 150, 3, 16),
                                          ("simple", 2708, 1, 64)])
def test_output_attn_vs_oracle_weights(kernel, n, h, d, dev):
    from difformer_amd import full_attention_conv
    g = torch.Generator().manual_seed(n + d)
    q, k, v = (torch.randn(n, h, d, generator=g) for _ in range(3))
    out, attn = full_attention_conv(q.to(dev), k.to(dev), v.to(dev), kernel, output_attn=True)
    q64, k64, v64 = (a.double().numpy() for a in (q, k, v))
    if kernel == "simple":
        ref_w = orc.simple_attention_weights(q64, k64)
        ref_o = orc.simple_attention(q64, k64, v64)
    else:
        ref_o, ref_w = orc.sigmoid_attention(q64, k64, v64, return_weights=True)
    assert rel_err(attn.cpu().numpy(), ref_w) < TOL and rel_err(out.cpu().numpy(), ref_o) < TOL
    if kernel == "sigmoid":      # rows of the sigmoid map are a convex combination
        assert torch.allclose(attn.sum(dim=1), torch.ones(n, h, device=dev), atol=1e-5)


def test_simple_output_attn_with_several_heads_fails_like_the_reference(dev):
    """difformer.py:43 divides a [N,L,H] tensor by a [N,H,1] one: only H == 1 broadcasts."""
    from difformer_amd import full_attention_conv
    q, k, v = (torch.randn(40, 2, 8, device=dev) for _ in range(3))
    with pytest.raises(RuntimeError):
        full_attention_conv(q, k, v, "simple", output_attn=True)


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_get_attentions_and_conv_output_attn_on_device(kernel, dev):
    """DIFFormer.get_attentions (:211-226; no graph term) and DIFFormerConv(..., output_attn=True) (:142-143) against
    the oracle's weights of the same projected q, k."""
    from difformer_amd import DIFFormer
    torch.manual_seed(5)
    n, f_in, hidden = 200, 24, 64
    model = DIFFormer(f_in, hidden, 5, num_layers=2, kernel=kernel, use_graph=False).to(dev).eval()
    x = torch.randn(n, f_in, device=dev)
    with torch.no_grad():
        att = model.get_attentions(x)
        assert att.shape == (2, n, n, 1)
        p = {k_: v_.detach().cpu().double().numpy() for k_, v_ in model.state_dict().items()}
        h = orc.linear(x.cpu().double().numpy(), p["fcs.0.weight"], p["fcs.0.bias"])
        h = np.maximum(orc.layer_norm(h, p["bns.0.weight"], p["bns.0.bias"]), 0.0)
        qs = orc.linear(h, p["convs.0.Wq.weight"], p["convs.0.Wq.bias"]).reshape(n, 1, hidden)
        ks = orc.linear(h, p["convs.0.Wk.weight"], p["convs.0.Wk.bias"]).reshape(n, 1, hidden)
        ref = orc.simple_attention_weights(qs, ks) if kernel == "simple" else \
            orc.sigmoid_attention(qs, ks, qs, return_weights=True)[1]
        assert rel_err(att[0].cpu().numpy(), ref) < TOL
        hx = torch.from_numpy(h).float().to(dev)
        out, w = model.convs[0](hx, hx, None, None, hx, output_attn=True)
        assert out.shape == (n, hidden) and rel_err(w.cpu().numpy(), ref) < TOL


# ------------------------------------------------------------------ a1 seeded sizes + properties
@pytest.mark.parametrize("n,h,d", [(1, 1, 64), (15, 1, 64), (17, 2, 32), (2708, 1, 64), (50000, 1, 64),
                                   (4099, 1, 128), (1000, 1, 300), (777, 3, 20), (333, 1, 7), (132534, 1, 64)])
def test_simple_attention_vs_oracle(n, h, d, dev):
    from difformer_amd import full_attention_conv
    g = torch.Generator().manual_seed(n * 7 + d)
    q, k, v = (torch.randn(n, h, d, generator=g) for _ in range(3))
    out = full_attention_conv(q.to(dev), k.to(dev), v.to(dev), "simple").cpu().numpy()
    ref = orc.simple_attention(q.double().numpy(), k.double().numpy(), v.double().numpy())
    assert rel_err(out, ref) < TOL


SIMPLE_SHAPES = [(1, 1, 64), (15, 1, 64), (17, 2, 32), (2708, 1, 64), (50000, 1, 64), (4099, 1, 128), (1000, 1, 300),
                 (777, 3, 20), (333, 1, 7), (132534, 1, 64), (513, 2, 100),
                 # one head of 65..128 columns from 4,096 rows: the one-read slab kernel on split-bf16 operands (round 5)
                 (100000, 1, 128), (20000, 1, 100), (9000, 1, 72), (4096, 1, 68)]


@pytest.mark.parametrize("n,h,d", SIMPLE_SHAPES)
def test_simple_reduce_record_vs_numpy(n, h, d, dev):
    """Stage 1 on its own: KtV, ksum, vsum and both Frobenius sums (the output of the full operator is
    dominated by vsum/N at large N, so the record is checked directly)."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n * 3 + d)
    q, k, v = (torch.randn(n, h, d, generator=g) + 0.25 for _ in range(3))
    rec = ops.get_backend().simple_reduce(q.to(dev), k.to(dev), v.to(dev)).cpu().numpy().astype(np.float64)
    q64, k64, v64 = (x.double().numpy() for x in (q, k, v))
    ktv = np.einsum("lhm,lhd->hmd", k64, v64)
    o = 0
    for name, ref in (("ktv", ktv), ("ksum", k64.sum(0)), ("vsum", v64.sum(0))):
        got = rec[o:o + ref.size].reshape(ref.shape)
        o += ref.size
        assert rel_err(got, ref) < 1e-5, name
    assert abs(rec[o] - (q64 ** 2).sum()) < 1e-5 * (q64 ** 2).sum()
    assert abs(rec[o + 1] - (k64 ** 2).sum()) < 1e-5 * (k64 ** 2).sum()
    assert rec.size == o + 2


@pytest.mark.parametrize("n,h,d", SIMPLE_SHAPES)
def test_simple_apply_with_synthetic_record(n, h, d, dev):
    """Stage 2 on its own with a record whose attention term is O(1) against vsum and N (tiny norms ->
    large s), so a wrong KtV / ksum / scale cannot hide behind the +N."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + 31 * d)
    q = torch.randn(n, h, d, generator=g)
    ktv = torch.randn(h, d, d, generator=g)
    ksum = torch.rand(h, d, generator=g) + 0.5
    vsum = torch.randn(h, d, generator=g)
    qsq, ksq = 4.0 / d, 9.0 / d                     # s = d/6
    n_global = 3 * n + 5
    rec = torch.cat([ktv.reshape(-1), ksum.reshape(-1), vsum.reshape(-1), torch.tensor([qsq, ksq])]).float()
    out = ops.get_backend().simple_apply(q.to(dev), rec.to(dev), n_global, d).cpu().numpy()
    s = 1.0 / (np.sqrt(np.float64(np.float32(qsq))) * np.sqrt(np.float64(np.float32(ksq))))
    q64 = q.double().numpy()
    num = s * np.einsum("nhm,hmd->nhd", q64, ktv.double().numpy()) + vsum.double().numpy()[None]
    den = s * np.einsum("nhm,hm->nh", np.abs(q64), ksum.double().numpy())[..., None] + n_global
    # use |q| in the denominator check only through a second call so den stays positive:
    out_abs = ops.get_backend().simple_apply(q.abs().to(dev), rec.to(dev), n_global, d).cpu().numpy()
    num_abs = s * np.einsum("nhm,hmd->nhd", np.abs(q64), ktv.double().numpy()) + vsum.double().numpy()[None]
    assert rel_err(out_abs, num_abs / den) < 1e-5
    den_signed = s * np.einsum("nhm,hm->nh", q64, ksum.double().numpy())[..., None] + n_global
    ok = np.abs(den_signed) > 0.05 * n_global       # skip rows whose denominator nearly cancels
    assert rel_err(np.where(ok, out, 0), np.where(ok, num / den_signed, 0)) < 1e-5


@pytest.mark.parametrize("n,c,h,d", [(1, 64, 1, 64), (16, 64, 1, 64), (1000, 64, 1, 64), (132534, 64, 1, 64),
                                     (777, 32, 2, 32), (513, 20, 3, 10), (300, 7, 1, 64), (4099, 64, 2, 64)])
def test_project_reduce_vs_numpy(n, c, h, d, dev):
    """Fused projection + reduce: q, v equal x W^T + b, and the record equals the one computed from them."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + c + d)
    x = torch.randn(n, c, generator=g)
    W = [torch.randn(h * d, c, generator=g) / np.sqrt(c) for _ in range(3)]
    b = [torch.randn(h * d, generator=g) * 0.3 for _ in range(3)]
    q, v, rec = ops.get_backend().project_reduce(x.to(dev), W[0].to(dev), b[0].to(dev), W[1].to(dev), b[1].to(dev),
                                                 W[2].to(dev), b[2].to(dev), h, d)
    x64 = x.double().numpy()
    q64, k64, v64 = ((x64 @ W[i].double().numpy().T + b[i].double().numpy()).reshape(n, h, d) for i in range(3))
    assert rel_err(q.cpu().numpy(), q64) < 1e-5 and rel_err(v.cpu().numpy(), v64) < 1e-5
    rec = rec.cpu().numpy().astype(np.float64)
    o = 0
    for name, ref in (("ktv", np.einsum("lhm,lhd->hmd", k64, v64)), ("ksum", k64.sum(0)), ("vsum", v64.sum(0))):
        got = rec[o:o + ref.size].reshape(ref.shape)
        o += ref.size
        assert rel_err(got, ref) < 1e-5, name
    assert abs(rec[o] - (q64 ** 2).sum()) < 1e-5 * (q64 ** 2).sum()
    assert abs(rec[o + 1] - (k64 ** 2).sum()) < 1e-5 * (k64 ** 2).sum()


def test_simple_attention_strided_views(dev):
    """q/k/v as column slices of one fused projection (leading dimension 3*H*D), no copies."""
    from difformer_amd import full_attention_conv
    g = torch.Generator().manual_seed(5)
    n, h, d = 1234, 1, 64
    qkv = torch.randn(n, 3 * h * d, generator=g).to(dev)
    q, k, v = (qkv[:, i * h * d:(i + 1) * h * d].reshape(n, h, d) for i in range(3))
    out = full_attention_conv(q, k, v, "simple").cpu().numpy()
    ref = orc.simple_attention(*(x.cpu().double().numpy() for x in (q, k, v)))
    assert rel_err(out, ref) < TOL


def test_simple_attention_is_invariant_to_row_permutation_of_sources(dev):
    """Size-independent property at full ogbn-proteins size: permuting (k_l, v_l) pairs leaves the
    output unchanged up to summation order."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(11)
    n = 132534
    q, k, v = (torch.randn(n, 1, 64, generator=g).to(dev) for _ in range(3))
    perm = torch.randperm(n, generator=g).to(dev)
    be = ops.get_backend()
    r1 = be.simple_reduce(q, k, v)
    r2 = be.simple_reduce(q, k[perm].contiguous(), v[perm].contiguous())
    assert rel_err(r2.cpu().numpy(), r1.cpu().numpy()) < 1e-5
    o1 = be.simple_apply(q, r1, n, 64)
    o2 = be.simple_apply(q, r2, n, 64)
    assert rel_err(o2.cpu().numpy(), o1.cpu().numpy()) < 1e-5


def test_simple_requires_equal_lengths(dev):
    from difformer_amd import full_attention_conv
    q = torch.randn(8, 1, 16, device=dev); k = torch.randn(9, 1, 16, device=dev)
    with pytest.raises(RuntimeError):
        full_attention_conv(q, k, k, "simple")


# ------------------------------------------------------------------ a2 seeded sizes
@pytest.mark.parametrize("n,l,h,d", [(1, 1, 1, 64), (16, 16, 1, 64), (100, 257, 2, 32), (2708, 2708, 1, 64),
                                     (300, 300, 1, 128), (123, 77, 1, 300), (200, 200, 3, 20), (65, 65, 1, 7)])
def test_sigmoid_attention_vs_oracle(n, l, h, d, dev):
    from difformer_amd import full_attention_conv
    g = torch.Generator().manual_seed(n + l + d)
    q = torch.randn(n, h, d, generator=g) * 0.5
    k = torch.randn(l, h, d, generator=g) * 0.5
    v = torch.randn(l, h, d, generator=g)
    out = full_attention_conv(q.to(dev), k.to(dev), v.to(dev), "sigmoid").cpu().numpy()
    ref = orc.sigmoid_attention(q.double().numpy(), k.double().numpy(), v.double().numpy())
    assert rel_err(out, ref) < TOL


def test_sigmoid_attention_saturated_scores(dev):
    """Large |q.k| drives sigma to 0 / 1; no overflow, rows still normalise."""
    from difformer_amd import full_attention_conv
    g = torch.Generator().manual_seed(3)
    q = torch.randn(64, 1, 64, generator=g) * 4
    k = torch.randn(80, 1, 64, generator=g) * 4
    v = torch.randn(80, 1, 64, generator=g)
    out = full_attention_conv(q.to(dev), k.to(dev), v.to(dev), "sigmoid").cpu().numpy()
    ref = orc.sigmoid_attention(q.double().numpy(), k.double().numpy(), v.double().numpy())
    assert np.isfinite(out).all() and rel_err(out, ref) < TOL


@pytest.mark.parametrize("n,l,h,d", [(70, 17, 1, 64), (300, 1000, 2, 32), (2708, 2708, 1, 64), (5000, 4111, 1, 48)])
def test_sigmoid_attention_split_operands_against_the_fp32_chain(n, l, h, d, dev):
    """Heads of at most 64 channels contract on split-bfloat16 operands (three 32-deep bf16 MFMAs per step, two key tiles per
    wave step); ops.set_exact_fp32 puts the same call back on the fp32 core.  Both are measured against the float64 oracle:
    the split path may cost a few 1e-6 -- far inside the 1e-4 of the contract -- and ragged key counts (odd tile counts, a
    tail tile, several key ranges) are masked the same way in both."""
    from difformer_amd import full_attention_conv, ops
    g = torch.Generator().manual_seed(n + 3 * l + d)
    q = torch.randn(n, h, d, generator=g) * 0.5
    k = torch.randn(l, h, d, generator=g) * 0.5
    v = torch.randn(l, h, d, generator=g)
    ref = orc.sigmoid_attention(q.double().numpy(), k.double().numpy(), v.double().numpy())
    errs = {}
    try:
        for exact in (False, True):
            ops.set_exact_fp32(exact)
            errs[exact] = rel_err(full_attention_conv(q.to(dev), k.to(dev), v.to(dev), "sigmoid").cpu().numpy(), ref)
    finally:
        ops.set_exact_fp32(False)
    assert errs[True] < 5e-6 and errs[False] < 2e-5, errs


def test_sigmoid_training_forward_keeps_the_fp32_chain(dev):
    """Under autograd the forward that leaves the row sums for the backward runs on the fp32 core whatever the switch says
    (gradients that are sums of cancelling rows amplify the split operands' 1e-6: scripts/exp_sigmoid_grad_parity.py): its
    output is bitwise the exact-mode inference output, and differs from the default inference output in the last digits."""
    from difformer_amd import full_attention_conv, ops
    g = torch.Generator().manual_seed(11)
    q, k, v = (torch.randn(300, 1, 64, generator=g).to(dev) * 0.5 for _ in range(3))
    train_out = full_attention_conv(q.clone().requires_grad_(True), k, v, "sigmoid").detach()
    infer_out = full_attention_conv(q, k, v, "sigmoid")
    try:
        ops.set_exact_fp32(True)
        exact_out = full_attention_conv(q, k, v, "sigmoid")
    finally:
        ops.set_exact_fp32(False)
    assert torch.equal(train_out, exact_out)
    assert not torch.equal(infer_out, exact_out) and float((infer_out - exact_out).abs().max() / exact_out.abs().max()) < 2e-5


# ------------------------------------------------------------------ a3
def _csr_reference(edge_index, n, edge_weight, n_blocks=1):
    """numpy statement of the CSR layout: entries sorted (stably) by destination, then source block."""
    row, col, val = orc.gcn_edge_values(edge_index, n, edge_weight, dtype=np.float32)
    block_rows = -(-n // n_blocks)
    key = col * n_blocks + row // block_rows
    order = np.argsort(key, kind="stable")
    kptr = np.concatenate([[0], np.cumsum(np.bincount(key, minlength=n * n_blocks))]).astype(np.int32)
    rowptr = kptr[::n_blocks].copy()
    blkptr = np.concatenate([kptr[:-1].reshape(n, n_blocks).T, kptr[n_blocks::n_blocks][None]], axis=0)
    return rowptr, row[order].astype(np.int32), val[order], blkptr.astype(np.int32)


def _check_csr(csr, edge_index, n, w, n_blocks):
    rp, src, val, blk = _csr_reference(edge_index, n, w, n_blocks)
    assert np.array_equal(csr.rowptr.cpu().numpy(), rp)                                   # integer work: exact
    assert np.array_equal(csr.src.cpu().numpy()[: csr.nnz], src)
    assert np.array_equal(csr.val.cpu().numpy()[: csr.nnz].view(np.uint32), val.view(np.uint32))  # bit-exact
    if n_blocks > 1:
        assert np.array_equal(csr.blkptr.cpu().numpy().reshape(n_blocks + 1, n), blk)


@pytest.mark.parametrize("name", sorted(GCN))
def test_gcn_conv_golden(name, dev):
    from difformer_amd import gcn_conv, ops
    c = GCN[name]
    w = c.get("edge_weight")
    ei = t(c["edge_index"], dev)
    wt = None if w is None else t(w, dev)
    n = c["x"].shape[0]
    x = t(c["x"], dev)
    for n_blocks in (1, 3):
        if ei.shape[1]:
            csr = ops.GraphCSR.build(ei, wt, n, n_blocks)
            _check_csr(csr, c["edge_index"], n, w, n_blocks)
            out = ops.gcn_aggregate(csr, x)                  # n_blocks > 1 exercises the blocked sweep
            assert rel_err(out.cpu().numpy(), c["out_f64"]) < 1e-5
    out = gcn_conv(x, ei, wt)
    assert rel_err(out.cpu().numpy(), c["out_f64"]) < 1e-5


@pytest.mark.parametrize("n,e,h,d,weighted", [(2708, 13264, 1, 64, False), (5000, 400000, 1, 64, True),
                                              (3000, 50000, 2, 32, False), (1000, 20000, 1, 300, True),
                                              (4000, 30000, 1, 10, False), (100000, 330000, 1, 64, False),
                                              (20000, 3000000, 1, 64, False), (200, 3000, 1, 8, False)])
def test_gcn_conv_vs_oracle(n, e, h, d, weighted, dev):
    from difformer_amd import gcn_conv, ops
    g = torch.Generator().manual_seed(e + n)
    x = torch.randn(n, h, d, generator=g)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[1, : e // 3] = torch.randint(0, max(n // 50, 1), (e // 3,), generator=g)   # skewed in-degree
    w = (torch.rand(e, generator=g) + 0.1) if weighted else None
    eid, wd = ei.to(dev), None if w is None else w.to(dev)
    ref = orc.gcn_conv(x.double().numpy(), ei.numpy(), None if w is None else w.double().numpy())
    for n_blocks in (1, 5):
        csr = ops.GraphCSR.build(eid, wd, n, n_blocks)
        _check_csr(csr, ei.numpy(), n, None if w is None else w.numpy(), n_blocks)
        out = ops.gcn_aggregate(csr, x.to(dev)).cpu().numpy()
        assert rel_err(out, ref) < 1e-5, n_blocks
    out = gcn_conv(x.to(dev), eid, wd).cpu().numpy()
    assert rel_err(out, ref) < 1e-5


def test_gcn_conv_linearity_and_determinism(dev):
    """Size-independent properties: A(ax + by) = a Ax + b Ay, and bitwise run-to-run reproducibility."""
    from difformer_amd import gcn_conv
    g = torch.Generator().manual_seed(21)
    n, e = 30000, 2000000
    ei = torch.randint(0, n, (2, e), generator=g).to(dev)
    x, y = torch.randn(n, 1, 64, generator=g).to(dev), torch.randn(n, 1, 64, generator=g).to(dev)
    ax, ay, axy = gcn_conv(x, ei, None), gcn_conv(y, ei, None), gcn_conv(2.0 * x - 0.5 * y, ei, None)
    assert rel_err(axy.cpu().numpy(), (2.0 * ax - 0.5 * ay).cpu().numpy()) < 1e-5
    assert torch.equal(gcn_conv(x, ei, None), ax)


def test_gcn_conv_rejects_bad_indices(dev):
    from difformer_amd import gcn_conv
    x = torch.randn(10, 1, 8, device=dev)
    ei = torch.tensor([[0, 1, 11], [1, 2, 3]], device=dev)
    with pytest.raises(IndexError):
        gcn_conv(x, ei, None)


def test_csr_cache_tracks_identity_and_version(dev):
    from difformer_amd import ops
    ops.csr_cache.clear()
    ei = torch.randint(0, 50, (2, 300), device=dev)
    a = ops.csr_cache.get(ei, None, 50)
    assert ops.csr_cache.get(ei, None, 50) is a
    ei[0, 0] = (ei[0, 0] + 1) % 50            # in-place edit bumps _version -> rebuild
    assert ops.csr_cache.get(ei, None, 50) is not a
    assert ops.csr_cache.get(ei.clone(), None, 50) is not ops.csr_cache.get(ei, None, 50)


# ------------------------------------------------------------------ a4 / a5
def test_layer_tail_vs_oracle(dev):
    from difformer_amd import ops
    g = torch.Generator().manual_seed(9)
    for n, h, d in [(1000, 1, 64), (333, 2, 32), (200, 1, 300), (129, 3, 10), (50, 1, 256)]:
        conv = torch.randn(n, h, d, generator=g)
        x0, prev = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
        w, b = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
        for use_x0, use_prev, use_ln in [(True, True, True), (False, True, True), (False, False, False), (True, False, True)]:
            out = ops.layer_tail(conv.to(dev), x0.to(dev) if use_x0 else None, prev.to(dev) if use_prev else None,
                                 0.3, w.to(dev) if use_ln else None, b.to(dev) if use_ln else None, 1e-5).cpu().numpy()
            z = conv.double().numpy().mean(axis=1)
            if use_x0:
                z = z + x0.double().numpy()
            if use_prev:
                z = 0.3 * z + 0.7 * prev.double().numpy()
            if use_ln:
                z = orc.layer_norm(z, w.double().numpy(), b.double().numpy())
            assert rel_err(out, z) < 1e-5, (n, h, d, use_x0, use_prev, use_ln)


@pytest.mark.parametrize("n,e,d,n_blocks", [(3000, 30000, 64, 1),      # lane-group-per-row kernel
                                            (3000, 300000, 64, 1),     # wave-per-row kernel
                                            (20000, 3000000, 64, 4),   # blocked sweep
                                            (2000, 100000, 128, 3), (1500, 60000, 10, 1), (900, 40000, 256, 2)])
def test_spmm_with_fused_tail_matches_unfused(n, e, d, n_blocks, dev):
    """dif_gcn_spmm_tail_f32 == dif_gcn_spmm_f32 followed by dif_layer_tail_f32, and both match the oracle."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + d)
    x = torch.randn(n, 1, d, generator=g).to(dev)
    attn = torch.randn(n, 1, d, generator=g).to(dev)
    x0, prev = torch.randn(n, d, generator=g).to(dev), torch.randn(n, d, generator=g).to(dev)
    w, b = (torch.rand(d, generator=g) + 0.5).to(dev), torch.randn(d, generator=g).to(dev)
    ei = torch.randint(0, n, (2, e), generator=g)
    csr = ops.GraphCSR.build(ei.to(dev), None, n, n_blocks)
    ref_conv = 0.7 * orc.gcn_conv(x.cpu().double().numpy(), ei.numpy(), None) + 0.3 * attn.cpu().double().numpy()
    for use_x0, use_prev, use_ln in [(True, True, True), (False, True, True), (False, False, False), (True, False, True)]:
        tail = dict(x0=x0 if use_x0 else None, prev=prev if use_prev else None, alpha=0.3,
                    ln_weight=w if use_ln else None, ln_bias=b if use_ln else None, eps=1e-5)
        fused = ops.gcn_aggregate(csr, x, attn, 0.3, 0.7, None, tail)[:, 0, :]
        conv = ops.gcn_aggregate(csr, x, attn, 0.3, 0.7)
        unfused = ops.layer_tail(conv, tail["x0"], tail["prev"], 0.3, tail["ln_weight"], tail["ln_bias"], 1e-5)
        z = ref_conv[:, 0, :]
        if use_x0:
            z = z + x0.cpu().double().numpy()
        if use_prev:
            z = 0.3 * z + 0.7 * prev.cpu().double().numpy()
        if use_ln:
            z = orc.layer_norm(z, w.cpu().double().numpy(), b.cpu().double().numpy())
        assert rel_err(fused.cpu().numpy(), z) < 2e-5
        assert rel_err(unfused.cpu().numpy(), z) < 2e-5


@pytest.mark.parametrize("n,ci,co,ln,relu", [(132534, 8, 64, True, True), (5000, 64, 112, False, False),
                                              (777, 33, 7, False, False), (1000, 64, 64, True, False),
                                              (100, 10, 10, True, True), (17, 1, 200, False, True),
                                              (3000, 64, 256, False, False), (3000, 64, 700, False, True),
                                              (100000, 65, 64, True, True), (2000, 100, 130, False, False),
                                              (2000, 128, 64, True, False), (333, 127, 300, False, True)])
def test_skinny_linear_vs_numpy(n, ci, co, ln, relu, dev):
    from difformer_amd import ops
    g = torch.Generator().manual_seed(ci * 100 + co)
    x = torch.randn(n, ci, generator=g)
    W, b = torch.randn(co, ci, generator=g) / np.sqrt(ci), torch.randn(co, generator=g)
    lw, lb = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g)
    out = ops.linear(x.to(dev), W.to(dev), b.to(dev), lw.to(dev) if ln else None, lb.to(dev) if ln else None, 1e-5,
                     relu).cpu().numpy()
    ref = x.double().numpy() @ W.double().numpy().T + b.double().numpy()
    if ln:
        ref = orc.layer_norm(ref, lw.double().numpy(), lb.double().numpy())
    if relu:
        ref = np.maximum(ref, 0)
    assert rel_err(out, ref) < 1e-5


@pytest.mark.parametrize("n,ci,co,dtype", [(100000, 65, 64, torch.float32), (100000, 65, 64, torch.bfloat16), (16, 5, 9, torch.float32),
                                           (4099, 127, 64, torch.bfloat16), (1000, 3, 64, torch.bfloat16), (2049, 17, 130, torch.float32)])
def test_skinny_linear_odd_widths_and_views(n, ci, co, dtype, dev):
    """Rows whose width is not a multiple of four elements (Pokec: 65 features, main-batch.py), float32 and bfloat16, stored
    back to back, with padded rows, and as a view that starts one row into the buffer: the same numbers every way."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(ci * 100 + co)
    x = torch.randn(n + 1, ci, generator=g).to(dtype)
    W, b = (torch.randn(co, ci, generator=g) / np.sqrt(ci)).to(dtype), torch.randn(co, generator=g).to(dtype)
    xd = x.to(dev)
    staged = ops.linear(xd[:n], W.to(dev), b.to(dev), None, None, 1e-5, False)
    ref = x[:n].double().numpy() @ W.double().numpy().T + b.double().numpy()
    tol = 1e-5 if dtype == torch.float32 else 1e-2
    assert staged.dtype == dtype and rel_err(staged.float().cpu().numpy(), ref) < tol
    padded = torch.zeros(n, ci + 3, dtype=dtype, device=dev)
    padded[:, :ci] = xd[:n]
    scalar = ops.linear(padded[:, :ci], W.to(dev), b.to(dev), None, None, 1e-5, False)          # ldx != C_in
    assert torch.equal(staged, scalar)
    ref1 = x[1:].double().numpy() @ W.double().numpy().T + b.double().numpy()
    off = ops.linear(xd[1:], W.to(dev), b.to(dev), None, None, 1e-5, False)                     # starts one row in
    assert rel_err(off.float().cpu().numpy(), ref1) < tol


@pytest.mark.parametrize("n,ci,co,ln,relu", [(50000, 512, 64, True, True), (20000, 1432, 64, True, True), (3001, 132, 10, False, False),
                                              (17, 516, 33, True, False), (40000, 300, 64, False, True), (5000, 2048, 7, True, True),
                                              (2708, 1433, 64, True, True),        # Cora (BASELINE C1 / C2): rows 4-byte aligned only
                                              (19717, 500, 64, True, True),        # Pubmed
                                              (30000, 1433, 64, True, True), (1, 129, 1, False, False), (33, 131, 64, True, False),
                                              (2708, 8191, 64, False, True)])
def test_long_linear_vs_numpy(n, ci, co, ln, relu, dev):
    """Long rows into a narrow layer (the input MLP on image / text embeddings, difformer.py:188-191): K in 64-channel chunks
    through double-buffered LDS weights; row counts that leave waves without a tile, widths that are not multiples of 64 --
    and of 4: few rows or rows that are not 16-byte aligned take the kernel that splits K over a workgroup's waves."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(ci * 100 + co)
    x = torch.randn(n, ci, generator=g)
    W, b = torch.randn(co, ci, generator=g) / np.sqrt(ci), torch.randn(co, generator=g)
    lw, lb = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g)
    be = ops.get_backend()
    out = be.linear(x.to(dev), W.to(dev), b.to(dev), lw.to(dev) if ln else None, lb.to(dev) if ln else None, 1e-5, relu)
    ref = x.double().numpy() @ W.double().numpy().T + b.double().numpy()
    if ln:
        ref = orc.layer_norm(ref, lw.double().numpy(), lb.double().numpy())
    if relu:
        ref = np.maximum(ref, 0)
    assert rel_err(out.cpu().numpy(), ref) < 1e-5
    assert torch.equal(out, be.linear(x.to(dev), W.to(dev), b.to(dev), lw.to(dev) if ln else None, lb.to(dev) if ln else None, 1e-5, relu))
    if n >= 16384 and ci % 4 == 0:      # bfloat16 storage of the same layer (rows aligned to 4 elements)
        bf = lambda t: t.to(torch.bfloat16)
        ob = be.linear(bf(x).to(dev), bf(W).to(dev), bf(b).to(dev), bf(lw).to(dev) if ln else None, bf(lb).to(dev) if ln else None,
                       1e-5, relu)
        refb = bf(x).double().numpy() @ bf(W).double().numpy().T + bf(b).double().numpy()
        if ln:
            refb = orc.layer_norm(refb, bf(lw).double().numpy(), bf(lb).double().numpy())
        if relu:
            refb = np.maximum(refb, 0)
        assert ob.dtype == torch.bfloat16 and rel_err(ob.float().cpu().numpy(), refb) < 1e-2


@pytest.mark.parametrize("n,ci,co,ln,relu", [(50000, 512, 300, True, True),          # image and text/run.sh:27 (CIFAR embeddings)
                                              (17000, 256, 128, True, False), (16384, 832, 416, True, True),
                                              (16385, 300, 68, False, True), (20001, 136, 100, True, True),
                                              (20000, 384, 400, False, False)])
def test_wide_linear_vs_numpy(n, ci, co, ln, relu, dev):
    """Wide rows into a wide layer (the input MLP at hidden 300 / 400, difformer.py:188-191): dif_linear_xwide_f32 -- one product
    up to 416 input channels, the two halves of the channels as two accumulating products beyond; split-bf16 terms (~4e-6 of the
    float64 result), LayerNorm / ReLU in the same pass.  The model path (autograd_ops.linear, no gradient) takes it too."""
    from difformer_amd import autograd_ops as ag, ops
    g = torch.Generator().manual_seed(ci * 100 + co)
    x = torch.randn(n, ci, generator=g)
    W, b = torch.randn(co, ci, generator=g) / np.sqrt(ci), torch.randn(co, generator=g)
    lw, lb = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g)
    be = ops.get_backend()
    xd, Wd, bd = x.to(dev), W.to(dev), b.to(dev)
    lwd, lbd = (lw.to(dev), lb.to(dev)) if ln else (None, None)
    assert ops.linear_xwide_covers(xd, Wd)
    be.kernel_events = {}
    try:
        out = be.linear(xd, Wd, bd, lwd, lbd, 1e-5, relu)
        with torch.no_grad():
            out_model = ag.linear(xd, Wd, bd, lwd, lbd, 1e-5, relu)
        launched = set(be.kernel_events)
    finally:
        be.kernel_events = None
    assert "dif_xwide_pack_f32" in launched, launched
    ref = x.double().numpy() @ W.double().numpy().T + b.double().numpy()
    if ln:
        ref = orc.layer_norm(ref, lw.double().numpy(), lb.double().numpy())
    if relu:
        ref = np.maximum(ref, 0)
    assert rel_err(out.cpu().numpy(), ref) < 2e-5
    assert torch.equal(out, out_model)
    # a parameter update (version bump) re-packs the weights
    with torch.no_grad():
        Wd.mul_(2.0)
    out2 = be.linear(xd, Wd, bd, None, None, 1e-5, False)
    assert rel_err(out2.cpu().numpy(), 2 * (x.double().numpy() @ W.double().numpy().T) + b.double().numpy()) < 2e-5
    # a column slice of a wider tensor as x (leading dimension != C_in)
    wide = torch.randn(n, ci + 8, generator=g).to(dev)
    out3 = be.linear(wide[:, 4:4 + ci], Wd, bd, None, None, 1e-5, False)
    assert rel_err(out3.cpu().numpy(), wide[:, 4:4 + ci].cpu().double().numpy() @ (2 * W.double().numpy()).T + b.double().numpy()) < 2e-5


def test_layer_tail_relu(dev):
    from difformer_amd import ops
    g = torch.Generator().manual_seed(2)
    for d in (64, 10, 300):
        x = torch.randn(500, 1, d, generator=g)
        w, b = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
        out = ops.layer_tail(x.to(dev), None, None, 0.5, w.to(dev), b.to(dev), 1e-5, relu=True).cpu().numpy()
        ref = np.maximum(orc.layer_norm(x[:, 0].double().numpy(), w.double().numpy(), b.double().numpy()), 0)
        assert rel_err(out, ref) < 1e-5 and (out >= 0).all()


@pytest.mark.parametrize("name", sorted(MODEL))
def test_model_forward_golden(name, dev):
    """DIFFormer.forward and DIFFormerConv.forward with the reference's own state_dict."""
    from difformer_amd import DIFFormer
    c = MODEL[name]
    cfg, sd = split_model_case(c)
    kw = {k: cfg[k] for k in ("num_layers", "num_heads", "kernel", "alpha", "use_bn", "use_residual", "use_weight",
                              "use_graph", "graph_weight", "use_source")}
    kw["kernel"] = str(kw["kernel"])
    model = DIFFormer(int(cfg["in_channels"]), int(cfg["hidden_channels"]), int(cfg["out_channels"]), **kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.to(dev).eval()
    ei = t(c["edge_index"], dev) if cfg["use_graph"] else None
    w = c.get("edge_weight")
    wt = None if w is None else t(w, dev)
    from difformer_amd import ops
    be = ops.get_backend()
    be.kernel_events = {}
    try:
        with torch.no_grad():
            out = model(t(c["x"], dev), ei, wt)
            launched = set(be.kernel_events)
            h0 = model._input_layer(t(c["x"], dev), False)
            conv0 = model.convs[0](h0, h0, ei, wt, h0)
    finally:
        be.kernel_events = None
    assert rel_err(out.cpu().numpy(), c["out_f64"]) < TOL
    assert rel_err(conv0.cpu().numpy(), c["conv0_f64"]) < TOL
    if int(cfg["hidden_channels"]) > 64:       # the scripts' widths: the wide closed form (Gram record of 65+ columns, one-pass
        # layer kernels of csrc/simple_layer_wide.hip / simple_layer_xwide.hip), not the operator path
        assert "dif_gram_sym_f32" in launched and "dif_simple_apply_f32" not in launched, launched


@pytest.mark.parametrize("kernel,n,f_in,layers,use_graph", [("simple", 2708, 1433, 2, True),     # C1
                                                            ("sigmoid", 2708, 1433, 2, True),    # C2
                                                            ("simple", 50000, 512, 4, False)])   # C3
def test_model_forward_baseline_configs(kernel, n, f_in, layers, use_graph, dev):
    from difformer_amd import DIFFormer
    torch.manual_seed(123)
    model = DIFFormer(f_in, 64, 7, num_layers=layers, kernel=kernel, use_graph=use_graph).eval()
    g = torch.Generator().manual_seed(0)
    x = torch.rand(n, f_in, generator=g)
    x = x / x.sum(dim=1, keepdim=True) if use_graph else torch.randn(n, f_in, generator=g)
    ei = None
    if use_graph:
        pairs = torch.randint(0, n, (2, 5278), generator=g)
        ei = torch.cat([pairs, pairs.flip(0), torch.arange(n).repeat(2, 1)], dim=1)
    cfg = dict(hidden_channels=64, num_layers=layers, num_heads=1, kernel=kernel, alpha=0.5, use_bn=True,
               use_residual=True, use_weight=True, use_graph=use_graph, graph_weight=-1, use_source=False)
    p = {k: v.double().numpy() for k, v in model.state_dict().items()}
    ref = orc.difformer_forward(p, x.double().numpy(), None if ei is None else ei.numpy(), None, cfg)
    model = model.to(dev)
    with torch.no_grad():
        out = model(x.to(dev), None if ei is None else ei.to(dev))
    assert rel_err(out.cpu().numpy(), ref) < TOL


def test_cpu_tensors_never_compute_on_the_host(dev):
    """No CPU arithmetic anywhere: host operands of the public functions are staged onto the GPU (the HIP entry points are
    what runs; the result returns to the host -- difformer_amd/staging.py), and the backend itself refuses a host tensor."""
    from difformer_amd import full_attention_conv, ops
    q = torch.randn(8, 1, 16)
    be = ops.get_backend()
    be.kernel_events = {}
    out = full_attention_conv(q, q, q, "simple")
    launched, be.kernel_events = set(be.kernel_events), None
    assert out.device.type == "cpu" and {"dif_simple_reduce_f32", "dif_simple_apply_f32"} <= launched
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        be.simple_reduce(q, q, q)


def _reference_forward_f64(p, x, ei, layers, alpha=0.5):
    """float64 torch restatement of DIFFormer.forward with the `simple` kernel, H = 1 (difformer.py:18-39, :63-79,
    :113-140, :184-209), differentiable: the yardstick for the gradients (the reference relies on autograd too)."""
    lin = lambda h, k: h @ p[k + ".weight"].T + p[k + ".bias"]
    ln = lambda h, k: torch.nn.functional.layer_norm(h, (h.shape[-1],), p[k + ".weight"], p[k + ".bias"], 1e-5)
    n = x.shape[0]
    row, col = ei[0], ei[1]
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, col, torch.ones(ei.shape[1], dtype=torch.float64))
    val = torch.nan_to_num((1.0 / deg[col]).sqrt() * (1.0 / deg[row]).sqrt(), nan=0.0, posinf=0.0, neginf=0.0)
    h = torch.relu(ln(lin(x, "fcs.0"), "bns.0"))
    for i in range(layers):
        q, k, v = (lin(h, f"convs.{i}.W{c}") for c in "qkv")
        s = 1.0 / (q.norm() * k.norm())
        num = s * q @ (k.T @ v) + v.sum(0)
        den = s * q @ k.sum(0) + n
        att = num / den[:, None]
        gcn = torch.zeros_like(v).index_add_(0, col, val[:, None] * v[row])
        h = ln(alpha * (att + gcn) + (1 - alpha) * h, f"bns.{i + 1}")
    return lin(h, "fcs.1")


def test_training_step_gradients_match_float64_autograd(dev):
    """loss.backward() through the HIP forward / backward kernels (reference main.py:119-131): EVERY parameter gradient
    against float64 autograd of the restated forward, 1e-4 norm-wise per tensor."""
    from difformer_amd import DIFFormer
    torch.manual_seed(1)
    n, layers = 300, 2
    model = DIFFormer(16, 32, 4, num_layers=layers, kernel="simple").to(dev).train()
    model.dropout = 0.0
    x = torch.randn(n, 16, device=dev)
    ei = torch.cat([torch.randint(0, n, (2, 2000), device=dev), torch.arange(n, device=dev).repeat(2, 1)], dim=1)
    out = model(x, ei)
    out.square().mean().backward()
    p64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.named_parameters()}
    ref = _reference_forward_f64(p64, x.cpu().double(), ei.cpu(), layers)
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) < TOL
    ref.square().mean().backward()
    for k, prm in model.named_parameters():
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), k
        assert rel_err(prm.grad.cpu().numpy(), p64[k].grad.numpy()) < 1e-4, k


@pytest.mark.parametrize("hidden", [64, 300])
def test_graphed_forward_replays_match_eager(hidden, dev):
    """hipGraph capture of the whole forward: replays equal the eager result, also after the input changes (hidden 300:
    the closed form at the scripts' widths, whose coefficient algebra runs as library GEMMs inside the capture)."""
    from difformer_amd import DIFFormer, GraphedForward
    torch.manual_seed(3)
    n = 3000
    model = DIFFormer(40, hidden, 6, num_layers=3, kernel="simple").to(dev).eval()
    g = torch.Generator().manual_seed(1)
    x1, x2 = torch.randn(n, 40, generator=g).to(dev), torch.randn(n, 40, generator=g).to(dev)
    ei = torch.cat([torch.randint(0, n, (2, 20000), generator=g), torch.arange(n).repeat(2, 1)], dim=1).to(dev)
    from difformer_amd import ops
    with torch.no_grad():
        e1, e2 = model(x1, ei).clone(), model(x2, ei).clone()
    fwd = GraphedForward(model, x1, ei)
    assert torch.equal(fwd(x1), e1)
    assert torch.equal(fwd(x2), e2)
    assert torch.equal(fwd(x1), e1)
    with pytest.raises(ValueError):
        fwd(x1[:10])


def test_graphed_forward_with_the_background_coefficient_chain(dev):
    """A dense graph takes the sliced product, and with it the coefficient chain on a second stream (csrc/side_chain.hip):
    the fork / join is captured into the hipGraph; replays equal the eager result and the single-stream result."""
    from difformer_amd import DIFFormer, GraphedForward, ops
    torch.manual_seed(5)
    n = 9000
    model = DIFFormer(24, 64, 5, num_layers=3, kernel="simple").to(dev).eval()
    g = torch.Generator().manual_seed(2)
    x1, x2 = torch.randn(n, 24, generator=g).to(dev), torch.randn(n, 24, generator=g).to(dev)
    ei = torch.cat([torch.randint(0, n, (2, 60 * n), generator=g), torch.arange(n).repeat(2, 1)], dim=1).to(dev)
    be = ops.get_backend()
    be.kernel_events = {}
    with torch.no_grad():
        e1, e2 = model(x1, ei).clone(), model(x2, ei).clone()
    launched, be.kernel_events = set(be.kernel_events), None
    assert {"dif_sliced_spmm_f32", "dif_simple_coeffs_bg_f32", "dif_gram_bg_f32"} <= launched
    fwd = GraphedForward(model, x1, ei)
    assert torch.equal(fwd(x1), e1) and torch.equal(fwd(x2), e2) and torch.equal(fwd(x1), e1)
    old, ops.SIDE_CHAIN = ops.SIDE_CHAIN, False
    try:
        with torch.no_grad():
            single = model(x1, ei)
    finally:
        ops.SIDE_CHAIN = old
    assert rel_err(e1.cpu().numpy(), single.cpu().numpy()) < 1e-5


def test_rccl_single_rank_collectives(dev):
    """The collectives the sharded path uses work on this box (RCCL, one rank; multi-rank logic is covered by the
    gloo tests)."""
    import torch.distributed as dist
    if dist.is_initialized():
        pytest.skip("process group already initialised")
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1, device_id=dev)
    try:
        t = torch.arange(8, dtype=torch.float32, device=dev)
        dist.all_reduce(t)
        out = torch.empty(8, device=dev)
        dist.all_gather_into_tensor(out, t)
        dist.barrier()
        assert torch.equal(out.cpu(), torch.arange(8, dtype=torch.float32))
    finally:
        dist.destroy_process_group()


def _full_config_parity(dev, n, pairs, f_in, classes, layers, tol=TOL, zipf=False, blocks=0, hidden=64):
    from difformer_amd import DIFFormer
    from bench import make_graph
    torch.manual_seed(123)
    model = DIFFormer(f_in, hidden, classes, num_layers=layers, kernel="simple", use_graph=True).eval()
    gx = torch.Generator().manual_seed(1)
    x = torch.randn(n, f_in, generator=gx)
    ei = make_graph(n, pairs, dev, zipf=zipf, blocks=blocks)
    cfg = dict(hidden_channels=hidden, num_layers=layers, num_heads=1, kernel="simple", alpha=0.5, use_bn=True,
               use_residual=True, use_weight=True, use_graph=True, graph_weight=-1, use_source=False)
    p = {k: v.double().numpy() for k, v in model.state_dict().items()}
    model = model.to(dev)
    with torch.no_grad():
        out = model(x.to(dev), ei).cpu().numpy()
    ref = orc.difformer_forward(p, x.double().numpy(), ei.cpu().numpy(), None, cfg)
    assert np.isfinite(out).all()
    assert rel_err(out, ref) < tol


def test_model_forward_c5_pokec_batch_shape(dev):
    """BASELINE config C5 shape (one Pokec mini-batch: 100k nodes, ~230k random edge pairs + self loops, F_in=65,
    C=2, 3 layers) in fp32 against the float64 oracle."""
    _full_config_parity(dev, 100000, 115000, 65, 2, 3)


def test_model_forward_c4_ogbn_proteins_full_size(dev):
    """BASELINE config C4 at FULL size -- the exact bench.py workload (132,534 nodes, 79,255,038 CSR entries,
    4 layers) -- against the float64 oracle (OpenMP C gcn_conv + numpy)."""
    _full_config_parity(dev, 132534, 39561252, 8, 112, 4)


def test_model_forward_c4_zipf_degree_profile_full_size(dev):
    """SURVEY section 8d's second degree profile for C4: the same sizes with a Zipf-like endpoint distribution (max / mean
    degree ~13, as the real ogbn-proteins) -- the blocked SpMM walks the rows in degree order with split hub rows here;
    2 layers keep the oracle time bounded."""
    _full_config_parity(dev, 132534, 39561252, 8, 112, 2, zipf=True)


def test_model_forward_c4_zipf_degrees_inside_communities_full_size(dev):
    """The two properties of the real ogbn-proteins TOGETHER at C4 size: 8 contiguous communities (95 % of the pairs
    inside) with Zipf degrees inside each -- the model runs in the mixed node order AND the hub rows are split."""
    from difformer_amd import ops
    _full_config_parity(dev, 132534, 39561252, 8, 112, 2, zipf=True, blocks=8)
    mixed = [m for m in ops.mix_cache.values() if m is not None]
    assert mixed, "the community structure should have switched the model to the mixed node order"


@pytest.mark.parametrize("hidden,layers", [(64, 3), (128, 2)])
def test_model_forward_pokec_full_graph(hidden, layers, dev):
    """The evaluation pass of the mini-batch scripts (node classification/eval.py:40-43, main-batch.py:144-145): ONE forward
    over the whole Pokec-sized graph -- 1,632,803 nodes, 32.4 M entries (mean degree ~19: gather kernels), F_in = 65,
    hidden 64 (closed-form layers) and 128 (the script's width, run.sh:42-44: operator path) -- against the float64 oracle."""
    _full_config_parity(dev, 1632803, 15400000, 65, 2, layers, hidden=hidden)


# ------------------------------------------------------------------ bfloat16 storage variants (config C5)
BF16_TOL = 1e-2      # bf16 storage / fp32 accumulate against the fp32-or-better oracle


def _bf(t):
    """Round to bfloat16 and return (bf16 tensor, its exact float64 numpy value)."""
    b = t.to(torch.bfloat16)
    return b, b.to(torch.float64).numpy()


def test_bf16_operators_vs_oracle(dev):
    from difformer_amd import ops
    be = ops.get_backend()
    g = torch.Generator().manual_seed(77)
    n, c, h, d = 3000, 64, 1, 64
    x, x64 = _bf(torch.randn(n, c, generator=g))
    W = [_bf(torch.randn(h * d, c, generator=g) / 8) for _ in range(3)]
    b = [_bf(torch.randn(h * d, generator=g) * 0.3) for _ in range(3)]
    lw, lw64 = _bf(torch.rand(d, generator=g) + 0.5)
    lb, lb64 = _bf(torch.randn(d, generator=g))
    # Linear + LayerNorm + ReLU
    out = ops.linear(x.to(dev), W[0][0].to(dev), b[0][0].to(dev), lw.to(dev), lb.to(dev), 1e-5, True)
    assert out.dtype == torch.bfloat16
    ref = np.maximum(orc.layer_norm(x64 @ W[0][1].T + b[0][1], lw64, lb64), 0)
    assert rel_err(out.float().cpu().numpy(), ref) < BF16_TOL
    # projection + reduce, apply
    q, v, rec = be.project_reduce(x.to(dev), W[0][0].to(dev), b[0][0].to(dev), W[1][0].to(dev), b[1][0].to(dev),
                                  W[2][0].to(dev), b[2][0].to(dev), h, d)
    q64, k64, v64 = ((x64 @ W[i][1].T + b[i][1]).reshape(n, h, d) for i in range(3))
    assert q.dtype == torch.bfloat16 and rec.dtype == torch.float32
    assert rel_err(q.float().cpu().numpy(), q64) < BF16_TOL and rel_err(v.float().cpu().numpy(), v64) < BF16_TOL
    assert rel_err(rec[: d * d].cpu().numpy(), np.einsum("lhm,lhd->hmd", k64, v64).ravel()) < 1e-4
    attn = be.simple_apply(q, rec, n, d)
    q_r, v_r = q.double().cpu().numpy(), v64
    ref_attn = orc.simple_attention(q_r, k64, v_r)
    assert rel_err(attn.float().cpu().numpy(), ref_attn) < BF16_TOL
    # stand-alone reduce on bf16 q, k, v
    k_b, _ = _bf(torch.from_numpy(k64))
    rec2 = be.simple_reduce(q, k_b.to(dev), v)
    assert rel_err(rec2[: d * d].cpu().numpy(), np.einsum("lhm,lhd->hmd", k_b.double().numpy(), v.double().cpu().numpy()).ravel()) < 1e-4
    # SpMM (+ combine, + fused tail) with bf16 rows, blocked and plain
    ei = torch.randint(0, n, (2, 200000), generator=g)
    prev, prev64 = _bf(torch.randn(n, d, generator=g))
    gref = orc.gcn_conv(v.double().cpu().numpy(), ei.numpy(), None)
    for n_blocks in (1, 3):
        csr = ops.GraphCSR.build(ei.to(dev), None, n, n_blocks)
        plain = ops.gcn_aggregate(csr, v, attn, 1.0, 1.0)
        assert plain.dtype == torch.bfloat16
        assert rel_err(plain.float().cpu().numpy(), gref + attn.double().cpu().numpy()) < BF16_TOL
        tail = dict(x0=None, prev=prev.to(dev), alpha=0.5, ln_weight=lw.to(dev), ln_bias=lb.to(dev), eps=1e-5)
        fused = ops.gcn_aggregate(csr, v, attn, 1.0, 1.0, None, tail)[:, 0, :]
        z = 0.5 * (gref + attn.double().cpu().numpy())[:, 0, :] + 0.5 * prev64
        assert rel_err(fused.float().cpu().numpy(), orc.layer_norm(z, lw64, lb64)) < BF16_TOL
    # stand-alone tail
    t = ops.layer_tail(plain, None, prev.to(dev), 0.5, lw.to(dev), lb.to(dev), 1e-5)
    z = 0.5 * plain.double().cpu().numpy()[:, 0, :] + 0.5 * prev64
    assert rel_err(t.float().cpu().numpy(), orc.layer_norm(z, lw64, lb64)) < BF16_TOL


@pytest.mark.parametrize("n,l,h,d", [(300, 300, 1, 64), (100, 257, 2, 32), (2708, 2708, 1, 64), (123, 77, 1, 300), (65, 65, 1, 7)])
def test_bf16_sigmoid_attention_vs_oracle(n, l, h, d, dev):
    """dif_sigmoid_attn_bf16: bfloat16 q, k, v, out; scores, sigma and both sums in fp32 -- against the float64 oracle on
    the bf16-rounded operands (difformer.py:45-56), including the key-split path (n = 2708) and odd widths."""
    from difformer_amd import full_attention_conv
    g = torch.Generator().manual_seed(n + l + d)
    q, q64 = _bf(torch.randn(n, h, d, generator=g) * 0.5)
    k, k64 = _bf(torch.randn(l, h, d, generator=g) * 0.5)
    v, v64 = _bf(torch.randn(l, h, d, generator=g))
    out = full_attention_conv(q.to(dev), k.to(dev), v.to(dev), "sigmoid")
    assert out.dtype == torch.bfloat16
    assert rel_err(out.float().cpu().numpy(), orc.sigmoid_attention(q64, k64, v64)) < BF16_TOL


def test_bf16_model_forward_c5_shape(dev):
    """BASELINE config C5: one Pokec-shaped mini-batch in bfloat16 storage (model.to(bfloat16), x bfloat16) against the
    float64 oracle evaluated with the bf16-rounded parameters and inputs."""
    from difformer_amd import DIFFormer
    from bench import make_graph
    n, f_in, classes, layers = 100000, 65, 2, 3
    torch.manual_seed(123)
    model = DIFFormer(f_in, 64, classes, num_layers=layers, kernel="simple", use_graph=True).eval()
    gx = torch.Generator().manual_seed(1)
    x = torch.randn(n, f_in, generator=gx).to(torch.bfloat16)
    ei = make_graph(n, 115000, dev)
    model = model.to(torch.bfloat16)
    cfg = dict(hidden_channels=64, num_layers=layers, num_heads=1, kernel="simple", alpha=0.5, use_bn=True,
               use_residual=True, use_weight=True, use_graph=True, graph_weight=-1, use_source=False)
    p = {k: v.double().numpy() for k, v in model.state_dict().items()}
    ref = orc.difformer_forward(p, x.double().numpy(), ei.cpu().numpy(), None, cfg)
    model = model.to(dev)
    with torch.no_grad():
        out = model(x.to(dev), ei)
    assert out.dtype == torch.bfloat16
    assert rel_err(out.float().cpu().numpy(), ref) < 2 * BF16_TOL     # 4 LayerNorm-separated bf16 round trips


@pytest.mark.parametrize("n,e,weighted,n_blocks", [(500, 6000, True, 1), (20000, 3000000, False, 4)])
def test_gcn_conv_adjoint_and_backward(n, e, weighted, n_blocks, dev):
    """The transposed CSR (entries filed under their source) gives A_hat^T g, and x.grad of gcn_conv is exactly that."""
    from difformer_amd import ops, autograd_ops as ag
    g = torch.Generator().manual_seed(n)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[1, : e // 4] = torch.randint(0, max(n // 20, 1), (e // 4,), generator=g)      # asymmetric, skewed
    w = (torch.rand(e, generator=g) + 0.1) if weighted else None
    go = torch.randn(n, 1, 64, generator=g)
    row, col, val = orc.gcn_edge_values(ei.numpy(), n, None if w is None else w.numpy(), dtype=np.float64)
    ref = np.zeros((n, 64))
    np.add.at(ref, row, val[:, None] * go.double().numpy()[col, 0])                    # A^T g
    eid, wd = ei.to(dev), None if w is None else w.to(dev)
    csr = ops.GraphCSR.build(eid, wd, n, n_blocks)
    adj = csr.adjoint()
    out = ops.gcn_aggregate(adj, go.to(dev)).cpu().numpy()[:, 0]
    assert rel_err(out, ref) < 1e-5
    x = torch.randn(n, 1, 64, generator=g).to(dev).requires_grad_(True)
    y = ag.gcn_aggregate(csr, x, None, 1.0, 0.7)
    y.backward(go.to(dev))
    assert rel_err(x.grad.cpu().numpy()[:, 0], 0.7 * ref) < 1e-5


@pytest.mark.parametrize("world", [2, 3, 8])
def test_row_sharded_kernels_match_unsharded(world, dev):
    """What each of `world` ranks would run -- its rows of the fused projection+reduce, the summed record (the
    all-reduce), apply with the GLOBAL N, the SpMM over its destination rows of the full CSR with the gathered V --
    done rank after rank in one process on the GPU, must reproduce the unsharded layer."""
    from difformer_amd import ops
    from difformer_amd.dist import split_rows
    be = ops.get_backend()
    g = torch.Generator().manual_seed(world)
    n, d = 20011, 64
    x = torch.randn(n, d, generator=g).to(dev)
    W = [(torch.randn(d, d, generator=g) / 8).to(dev) for _ in range(3)]
    b = [(torch.randn(d, generator=g) * 0.2).to(dev) for _ in range(3)]
    prev = torch.randn(n, d, generator=g).to(dev)
    lw, lb = (torch.rand(d, generator=g) + 0.5).to(dev), torch.randn(d, generator=g).to(dev)
    ei = torch.randint(0, n, (2, 2500000), generator=g).to(dev)
    csr = ops.GraphCSR.build(ei, None, n, 3)
    tail = lambda lo, hi: dict(x0=None, prev=prev[lo:hi], alpha=0.5, ln_weight=lw, ln_bias=lb, eps=1e-5)
    # unsharded
    q, v, rec = be.project_reduce(x, W[0], b[0], W[1], b[1], W[2], b[2], 1, d)
    attn = be.simple_apply(q, rec, n, d)
    full = be.spmm(csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, n, csr.nnz, v.reshape(n, d), 0, n,
                   attn.reshape(n, d), 1.0, 1.0, tail(0, n))
    # sharded, rank by rank
    counts = split_rows(n, world)
    offs = np.concatenate([[0], np.cumsum(counts)])
    parts = [be.project_reduce(x[offs[r]:offs[r + 1]].contiguous(), W[0], b[0], W[1], b[1], W[2], b[2], 1, d)
             for r in range(world)]
    rec_sum = torch.stack([p[2] for p in parts]).sum(dim=0)                 # the all-reduce
    v_all = torch.cat([p[1] for p in parts]).reshape(n, d)                  # the all-gather
    assert rel_err(rec_sum.cpu().numpy(), rec.cpu().numpy()) < 1e-5
    for r in range(world):
        lo, hi = int(offs[r]), int(offs[r + 1])
        attn_r = be.simple_apply(parts[r][0], rec_sum, n, d)                # n_global = N, not the shard size
        out_r = be.spmm(csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, n, csr.nnz, v_all, lo, hi - lo,
                        attn_r.reshape(hi - lo, d), 1.0, 1.0, tail(lo, hi), csr.row_order(lo, hi - lo))
        assert rel_err(out_r.cpu().numpy(), full[lo:hi].cpu().numpy()) < 1e-5, (world, r)


@pytest.mark.parametrize("n,h,d", [(300, 1, 64), (1000, 2, 32), (257, 3, 20), (50000, 1, 64), (3000, 1, 128), (40000, 1, 128),
                                   (700, 2, 100), (900, 1, 300), (333, 1, 130), (64, 1, 512)])
def test_simple_attention_backward_kernels(n, h, d, dev):
    """dq, dk, dv from the HIP backward (bwd_prep + reduce + row-GEMMs) against float64 autograd of the closed form
    of difformer.py:18-39 (the reference itself relies on autograd).  Heads wider than 64 (hidden 128 / 300 of the
    reference's scripts): the 128-column prep kernel or the generic one, and the wide row-GEMM with the [K x 64] slab in LDS."""
    from difformer_amd import autograd_ops as ag, ops
    g = torch.Generator().manual_seed(n + d)
    q, k, v = (torch.randn(n, h, d, generator=g) for _ in range(3))
    go = torch.randn(n, h, d, generator=g)
    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    be = ops.get_backend()
    be.kernel_events = {}
    try:
        out = ag.simple_attention(qd, kd, vd)
        out.backward(go.to(dev))
        launched = set(be.kernel_events)
    finally:
        be.kernel_events = None
    assert {"dif_simple_bwd_prep_f32", "dif_rowgemm_f32"} <= launched, launched
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    ag._simple_expr(q64, k64, v64).backward(go.double())
    for got, ref, name in ((qd.grad, q64.grad, "dq"), (kd.grad, k64.grad, "dk"), (vd.grad, v64.grad, "dv")):
        assert rel_err(got.cpu().numpy(), ref.numpy()) < 1e-4, name


@pytest.mark.parametrize("n,K,C,acc", [(5000, 128, 128, True), (777, 300, 300, False), (3000, 64, 192, True), (1000, 130, 7, True),
                                       (20, 512, 64, False), (4000, 40, 40, True)])
def test_row_gemm_wide(n, K, C, acc, dev):
    """dif_rowgemm_f32 beyond 64 columns (the [K x 64] slab of the matrix resident in LDS, K <= 512): A mat + bias
    (+ accumulate) against float64, odd widths included (scalar loads / stores)."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(K + C)
    A, mat, bias, prev = torch.randn(n, K, generator=g), torch.randn(K, C, generator=g), torch.randn(C, generator=g), torch.randn(n, C, generator=g)
    got = ops.get_backend().row_gemm(A.to(dev), mat.to(dev), bias.to(dev), prev.to(dev) if acc else None)
    ref = A.double() @ mat.double() + bias.double() + (prev.double() if acc else 0)
    assert rel_err(got.cpu().numpy(), ref.numpy()) < 1e-5
    # a column slice of a wider tensor as A (leading dimension != K)
    wide = torch.randn(n, K + 8, generator=g).to(dev)
    got = ops.get_backend().row_gemm(wide[:, 4:4 + K], mat.to(dev))
    assert rel_err(got.cpu().numpy(), (wide[:, 4:4 + K].cpu().double() @ mat.double()).numpy()) < 1e-5


@pytest.mark.parametrize("n,l,h,m,d", [(300, 300, 1, 64, 64), (100, 257, 2, 32, 32), (2708, 2708, 1, 64, 64), (65, 65, 1, 7, 7),
                                       (500, 123, 3, 20, 20), (200, 150, 1, 48, 64), (1, 1, 1, 64, 64), (4000, 37, 1, 64, 16)])
def test_sigmoid_attention_backward_kernel(n, l, h, m, d, dev):
    """dq, dk, dv of difformer.py:45-56 from csrc/sigmoid_attn_bwd.hip (sigma recomputed tile by tile from the saved row
    sums) against float64 autograd of the same expression -- the reference itself relies on autograd (main.py:130).
    Covers N != L, several heads, odd widths (scalar loads), M != D and the swept-side splits of small problems."""
    from difformer_amd import autograd_ops as ag, ops
    g = torch.Generator().manual_seed(n + l + d)
    q = torch.randn(n, h, m, generator=g) * 0.5
    k = torch.randn(l, h, m, generator=g) * 0.5
    v = torch.randn(l, h, d, generator=g)
    go = torch.randn(n, h, d, generator=g)
    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    be = ops.get_backend()
    be.kernel_events = {}
    out = ag.sigmoid_attention(qd, kd, vd)
    out.backward(go.to(dev))
    launched, be.kernel_events = set(be.kernel_events), None
    assert "dif_sigmoid_attn_bwd_f32" in launched and "dif_sigmoid_attn_fwd_f32" in launched
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    ref = ag._sigmoid_expr(q64, k64, v64)
    ref.backward(go.double())
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) < TOL
    for got, want, name in ((qd.grad, q64.grad, "dq"), (kd.grad, k64.grad, "dk"), (vd.grad, v64.grad, "dv")):
        assert rel_err(got.cpu().numpy(), want.numpy()) < 1e-4, name
    # bitwise reproducible (fixed fold / combine order)
    qd2, kd2, vd2 = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    ag.sigmoid_attention(qd2, kd2, vd2).backward(go.to(dev))
    assert torch.equal(qd2.grad, qd.grad) and torch.equal(kd2.grad, kd.grad) and torch.equal(vd2.grad, vd.grad)


def test_sigmoid_attention_backward_split_operands_against_the_fp32_chain(dev):
    """DIFFORMER_SIGMOID_BWD_SPLIT=1 (opt-in, read once per process: a child): the backward sweeps take TWO 16-row tiles of the
    swept side per step on split-bfloat16 operands; without it (and under ops.set_exact_fp32) one tile on the fp32 core.  Both
    against float64 autograd, the split path within a few 1e-6 of the fp32 chain -- odd tile counts, a masked tail tile,
    swept-side splits and scalar-load widths included.  (Why it is opt-in: model/a_nobn_src in test_gpu_grad.py -- a bias
    gradient that is a sum of cancelling rows lands ON the 1e-4 bar with it, 4e-6 without.)"""
    import os, subprocess, sys, json
    code = r'''
import json, sys, numpy as np, torch
sys.path.insert(0, ".")
from difformer_amd import ops, autograd_ops as ag
dev = torch.device("cuda:0")
be = ops.get_backend()
res = []
for n, l, h, m, d in [(70, 17, 1, 64, 64), (300, 1000, 2, 32, 32), (2708, 2708, 1, 64, 64), (333, 95, 1, 20, 12)]:
    g = torch.Generator().manual_seed(n + l + d)
    q = torch.randn(n, h, m, generator=g) * 0.5
    k = torch.randn(l, h, m, generator=g) * 0.5
    v = torch.randn(l, h, d, generator=g)
    go = torch.randn(n, h, d, generator=g)
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    ag._sigmoid_expr(q64, k64, v64).backward(go.double())
    want = [t.grad.numpy() for t in (q64, k64, v64)]
    qd, kd, vd, gd = (t.to(dev) for t in (q, k, v, go))
    errs = {}
    for exact in (False, True):
        ops.set_exact_fp32(exact)
        be.kernel_events = {}
        out, den = be.sigmoid_attention(qd, kd, vd, want_den=True)
        got = be.sigmoid_backward(qd, kd, vd, out, den, gd)
        errs["exact" if exact else "split"] = max(float(np.max(np.abs(a.cpu().numpy() - b)) / np.max(np.abs(b))) for a, b in zip(got, want))
    ops.set_exact_fp32(False)
    res.append(errs)
print(json.dumps(res))
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, DIFFORMER_SIGMOID_BWD_SPLIT="1"),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for errs in res:
        assert errs["exact"] < 1e-5 and 0 < errs["split"] < 3e-5 and errs["split"] != errs["exact"], res


def test_sigmoid_attention_backward_beyond_512_columns_falls_back_to_tensor_ops(dev):
    """Heads wider than 512 columns are beyond both backward kernels (csrc/sigmoid_attn_bwd.hip: 64, csrc/sigmoid_wide.hip: 512):
    the gradient is re-derived with device tensor ops -- checked against the ORACLE's float64 autograd of difformer.py:45-56
    (oracle/difformer_oracle_grad.py), not against the package's own expression; 65..512 columns: tests/test_gpu_sigmoid_wide.py."""
    from difformer_amd import autograd_ops as ag, ops
    from oracle import difformer_oracle_grad as og
    g = torch.Generator().manual_seed(5)
    q, k, v, go = (torch.randn(150, 1, 520, generator=g) * 0.15 for _ in range(4))
    qd, kd, vd = (t.to(dev).requires_grad_(True) for t in (q, k, v))
    be = ops.get_backend()
    be.kernel_events = {}
    try:
        ag.sigmoid_attention(qd, kd, vd).backward(go.to(dev))
    finally:
        names, be.kernel_events = set(be.kernel_events), None
    assert "dif_sigmoid_attn_bwd_f32" not in names
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    og.sigmoid_attention(q64, k64, v64).backward(go.double())
    for got, want in ((qd.grad, q64.grad), (kd.grad, k64.grad), (vd.grad, v64.grad)):
        assert rel_err(got.cpu().numpy(), want.numpy()) < 1e-4


def test_subgraph_relabel_matches_numpy(dev):
    """dif_subgraph (main-batch.py:131 semantics): kept edges in original order, relabelled; integer work -> exact."""
    from difformer_amd import graph_utils as gu
    g = torch.Generator().manual_seed(4)
    n, e, bsz = 50000, 1200000, 10000
    ei = torch.randint(0, n, (2, e), generator=g)
    w = torch.rand(e, generator=g)
    subset = torch.randperm(n, generator=g)[:bsz]
    ref, ref_w = orc.subgraph(subset.numpy(), ei.numpy(), w.numpy(), relabel_nodes=True, num_nodes=n)
    out, ow = gu.subgraph(subset.to(dev), ei.to(dev), w.to(dev), relabel_nodes=True, num_nodes=n)
    assert np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(ow.cpu().numpy(), ref_w)
    out2, _ = gu.subgraph(subset.to(dev), ei.to(dev), None, relabel_nodes=False, num_nodes=n)
    assert np.array_equal(out2.cpu().numpy(), orc.subgraph(subset.numpy(), ei.numpy(), None, False, n)[0])
    empty, _ = gu.subgraph(torch.zeros(0, dtype=torch.long, device=dev), ei.to(dev), None, True, n)
    assert empty.shape == (2, 0)
    with pytest.raises(IndexError):
        gu.subgraph(torch.tensor([n + 5], device=dev), ei.to(dev), None, True, n)
    # the small helpers
    a, _ = gu.remove_self_loops(torch.tensor([[0, 1, 2], [0, 2, 2]], device=dev))
    assert a.tolist() == [[1], [2]]
    b, _ = gu.add_self_loops(a, num_nodes=3)
    assert b.tolist() == [[1, 0, 1, 2], [2, 0, 1, 2]]
    u = gu.to_undirected(torch.tensor([[0, 1, 1], [1, 0, 2]], device=dev), num_nodes=3)
    assert u.tolist() == [[0, 1, 1, 2], [1, 0, 2, 1]]


@pytest.mark.parametrize("n,e,bsz", [(100, 1, 100), (100, 63, 50), (100, 64, 100), (100, 65, 7), (500, 4095, 500), (500, 4096, 250),
                                     (500, 4097, 499), (3000, 300001, 3000), (3000, 300001, 1), (20000, 2000003, 6000), (50, 0, 10)])
def test_subgraph_edge_counts_around_the_mask_words_and_chunks(n, e, bsz, dev):
    """dif_subgraph keeps one BIT per edge (a wave's ballot = a 64-edge mask word) and scans per-chunk counts (4,096 edges): edge
    counts on both sides of a word / chunk boundary, every edge kept (the subset is all nodes), a single node, no edges -- bit-exact
    against the numpy restatement of main-batch.py:131."""
    from difformer_amd import graph_utils as gu
    g = torch.Generator().manual_seed(n + e)
    ei = torch.randint(0, n, (2, e), generator=g)
    w = torch.rand(e, generator=g)
    subset = torch.randperm(n, generator=g)[:bsz]
    ref, ref_w = orc.subgraph(subset.numpy(), ei.numpy(), w.numpy(), relabel_nodes=True, num_nodes=n)
    out, ow = gu.subgraph(subset.to(dev), ei.to(dev), w.to(dev), relabel_nodes=True, num_nodes=n)
    assert out.shape == ref.shape and np.array_equal(out.cpu().numpy(), ref)
    assert np.array_equal(ow.cpu().numpy(), ref_w)


@pytest.mark.parametrize("n,e,m,bsz,weighted", [(50000, 1200000, 50000, 10000, True), (50000, 1200000, 31234, 7000, False),
                                                 (3000, 40000, 3000, 10, False), (1000, 5000, 1000, 1000, True),
                                                 (600, 3000, 508, 2, False), (600, 3000, 510, 2, True),
                                                 (300, 2000, 200, 64, False), (70000, 5000, 66000, 33000, True)])
def test_subgraph_batches_equal_the_per_batch_calls(n, e, m, bsz, weighted, dev):
    """All mini-batch subgraphs of an epoch from ONE pass over the edge list (main-batch.py:121-131): every batch must be
    exactly what subgraph(idx_i, edge_index, relabel_nodes=True) returns for it -- integer work, compared exactly
    against the oracle's restatement of torch_geometric.utils.subgraph (the last batch is ragged, 300 batches need two
    radix passes, one batch = the whole permutation)."""
    from difformer_amd import graph_utils as gu
    g = torch.Generator().manual_seed(n + bsz)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei = torch.cat([ei, torch.arange(n).repeat(2, 1)], dim=1)           # self loops survive in their node's batch
    w = torch.rand(ei.shape[1], generator=g) if weighted else None
    perm = torch.randperm(n, generator=g)[:m]
    batches = gu.subgraph_batches(perm.to(dev), bsz, ei.to(dev), None if w is None else w.to(dev), num_nodes=n)
    assert len(batches) == -(-m // bsz)
    for b, (eb, wb) in enumerate(batches):
        idx = perm[b * bsz: (b + 1) * bsz]
        ref, ref_w = orc.subgraph(idx.numpy(), ei.numpy(), None if w is None else w.numpy(), relabel_nodes=True, num_nodes=n)
        assert np.array_equal(eb.cpu().numpy(), ref), b
        if weighted:
            assert np.array_equal(wb.cpu().numpy(), ref_w), b
        else:
            assert wb is None
    # direct CSR emission: every batch's registered CSR is, bit for bit, what dif_csr_build makes of its edge list
    from difformer_amd import ops
    for b, (eb, wb) in enumerate(batches):
        nb_rows = min(bsz, m - b * bsz)
        got = ops.csr_cache.get(eb, wb, nb_rows, 256)
        assert got.n_blocks == 1 and got.nnz == eb.shape[1]
        want = ops.GraphCSR.build(eb.contiguous(), wb, nb_rows, 1)
        assert torch.equal(got.rowptr, want.rowptr), b
        assert torch.equal(got.src[: got.nnz], want.src[: got.nnz]) and torch.equal(got.val[: got.nnz], want.val[: got.nnz]), b
        if b >= 3:
            break
    with pytest.raises(ValueError):
        gu.subgraph_batches(torch.tensor([1, 2, 1], device=dev), 2, ei.to(dev), None, num_nodes=n)
    with pytest.raises(IndexError):
        gu.subgraph_batches(torch.tensor([1, n + 3], device=dev), 2, ei.to(dev), None, num_nodes=n)


@pytest.mark.parametrize("n,e", [(5000, 40000), (132534, 3000000), (70, 2000), (300000, 100)])
def test_graph_prepare_matches_numpy(n, e, dev):
    """dif_graph_prepare: to_undirected / remove_self_loops / add_self_loops of main.py:72-76 (torch_geometric semantics:
    coalesced and sorted by (row, col); loops dropped; N loops appended) -- integer work, exact."""
    from difformer_amd import graph_utils as gu
    g = torch.Generator().manual_seed(n)
    ei = torch.randint(0, n, (2, e), generator=g)
    ei[:, : e // 10] = ei[:, e // 10: 2 * (e // 10)]               # duplicates
    ei[1, : e // 20] = ei[0, : e // 20]                             # self loops
    a = ei.numpy()
    key = np.unique(np.concatenate([a[0] * n + a[1], a[1] * n + a[0]]))
    und = np.stack([key // n, key % n])
    assert np.array_equal(gu.to_undirected(ei.to(dev), num_nodes=n).cpu().numpy(), und)
    nol = a[:, a[0] != a[1]]
    out, _ = gu.remove_self_loops(ei.to(dev))
    assert np.array_equal(out.cpu().numpy(), nol)
    out, _ = gu.add_self_loops(ei.to(dev), num_nodes=n)
    assert np.array_equal(out.cpu().numpy(), np.concatenate([a, np.arange(n)[None].repeat(2, 0)], axis=1))
    full = np.concatenate([und[:, und[0] != und[1]], np.arange(n)[None].repeat(2, 0)], axis=1)
    assert np.array_equal(gu.prepare_graph(ei.to(dev), num_nodes=n).cpu().numpy(), full)
    w = torch.rand(e, generator=g).to(dev)
    o2, w2 = gu.remove_self_loops(ei.to(dev), w)
    assert np.array_equal(o2.cpu().numpy(), nol) and w2.shape[0] == nol.shape[1]
    with pytest.raises(IndexError):
        gu.to_undirected(torch.tensor([[0, n + 1], [1, 2]], device=dev), num_nodes=n)


def _random_cfgs(count, seed):
    rng = np.random.default_rng(seed)
    cfgs = []
    while len(cfgs) < count:
        c = dict(hidden_channels=int(rng.choice([8, 16, 20, 64, 96])), num_layers=int(rng.integers(1, 4)),
                 num_heads=int(rng.choice([1, 1, 2, 3])), kernel=str(rng.choice(["simple", "simple", "sigmoid"])),
                 alpha=float(rng.choice([0.5, 0.2])), use_bn=bool(rng.integers(0, 2)), use_residual=bool(rng.integers(0, 2)),
                 use_weight=bool(rng.integers(0, 4) > 0), use_graph=bool(rng.integers(0, 4) > 0),
                 graph_weight=float(rng.choice([-1, -1, 0.3])), use_source=bool(rng.integers(0, 2)))
        c["weighted"] = bool(rng.integers(0, 2)) and c["use_graph"]
        c["n"] = int(rng.integers(50, 600))
        c["f_in"] = int(rng.choice([5, 32, 64, 130]))
        cfgs.append(c)
    return cfgs


@pytest.mark.parametrize("idx,cfg", list(enumerate(_random_cfgs(28, 2024))))
def test_model_forward_random_flag_combinations(idx, cfg, dev):
    """Every constructor switch of difformer.py:154-155 in random combinations (incl. the CLI defaults of parse.py:48-52,
    several heads, odd widths, use_weight=False, graph_weight > 0, edge weights) against the float64 oracle."""
    from difformer_amd import DIFFormer
    cfg = dict(cfg)
    n, f_in, weighted = cfg.pop("n"), cfg.pop("f_in"), cfg.pop("weighted")
    torch.manual_seed(1000 + idx)
    model = DIFFormer(f_in, cfg["hidden_channels"], 6, **{k: v for k, v in cfg.items() if k != "hidden_channels"}).eval()
    g = torch.Generator().manual_seed(idx)
    x = torch.randn(n, f_in, generator=g)
    ei = torch.cat([torch.randint(0, n, (2, 5 * n), generator=g), torch.arange(n).repeat(2, 1)], dim=1)
    w = (torch.rand(ei.shape[1], generator=g) + 0.05) if weighted else None
    p = {k: v.double().numpy() for k, v in model.state_dict().items()}
    ref = orc.difformer_forward(p, x.double().numpy(), ei.numpy() if cfg["use_graph"] else None,
                                None if w is None else w.double().numpy(), cfg)
    model = model.to(dev)
    with torch.no_grad():
        out = model(x.to(dev), ei.to(dev) if cfg["use_graph"] else None, None if w is None else w.to(dev))
    assert rel_err(out.cpu().numpy(), ref) < TOL, cfg


_SCRIPT_SHAPES = [
    # (name, n, f_in, classes, cfg): widths the reference's run.sh files actually pass
    ("cifar-script hidden 300 no graph", 3000, 512, 10,
     dict(hidden_channels=300, num_layers=2, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
          use_weight=True, use_graph=False, graph_weight=-1, use_source=False)),
    ("pokec-script hidden 128", 4000, 65, 2,
     dict(hidden_channels=128, num_layers=3, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
          use_weight=True, use_graph=True, graph_weight=-1, use_source=False)),
    ("hidden 256 sigmoid, 2 heads", 1500, 100, 5,
     dict(hidden_channels=256, num_layers=2, num_heads=2, kernel="sigmoid", alpha=0.5, use_bn=True, use_residual=True,
          use_weight=True, use_graph=True, graph_weight=-1, use_source=True)),
    ("hidden 32, 4 heads, graph_weight", 2500, 40, 7,
     dict(hidden_channels=32, num_layers=2, num_heads=4, kernel="simple", alpha=0.3, use_bn=False, use_residual=True,
          use_weight=True, use_graph=True, graph_weight=0.7, use_source=False)),
]


@pytest.mark.parametrize("name,n,f_in,classes,cfg", _SCRIPT_SHAPES, ids=[s[0] for s in _SCRIPT_SHAPES])
def test_model_forward_script_widths(name, n, f_in, classes, cfg, dev):
    """Hidden widths of the shipped scripts (image and text/run.sh:27 hidden 300; node classification/run.sh:42-44
    hidden 128) and wide multi-head cases, against the float64 oracle."""
    from difformer_amd import DIFFormer
    torch.manual_seed(7)
    model = DIFFormer(f_in, cfg["hidden_channels"], classes,
                      **{k: v for k, v in cfg.items() if k != "hidden_channels"}).eval()
    g = torch.Generator().manual_seed(11)
    x = torch.randn(n, f_in, generator=g)
    ei = torch.cat([torch.randint(0, n, (2, 6 * n), generator=g), torch.arange(n).repeat(2, 1)], dim=1)
    p = {k: v.double().numpy() for k, v in model.state_dict().items()}
    ref = orc.difformer_forward(p, x.double().numpy(), ei.numpy() if cfg["use_graph"] else None, None, cfg)
    model = model.to(dev)
    with torch.no_grad():
        out = model(x.to(dev), ei.to(dev) if cfg["use_graph"] else None)
    assert rel_err(out.cpu().numpy(), ref) < TOL, name


# ------------------------------------------------------------------ f4: DIFFormer_v2 (batches of graphs)
V2 = load_golden("v2")


def _v2_attention(q, k, v, n_nodes, kernel, dev):
    from difformer_amd import TransConv
    conv = TransConv(q.shape[2], q.shape[2], num_heads=q.shape[1], kernel=kernel)
    return conv.full_attention(t(q, dev), t(k, dev), t(v, dev), kernel, torch.as_tensor(n_nodes).to(dev))


@pytest.mark.parametrize("name", sorted(n for n in V2 if n.startswith("attn/")))
def test_v2_full_attention_golden(name, dev):
    c = V2[name]
    out = _v2_attention(c["q"], c["k"], c["v"], c["n_nodes"], str(c["kernel"]), dev)
    assert out.shape == c["out_f64"].shape and out.dtype == torch.float32
    assert rel_err(out.cpu().numpy(), c["out_f64"]) < TOL


@pytest.mark.parametrize("name", sorted(n for n in V2 if n.startswith("model/")))
def test_v2_model_forward_golden(name, dev):
    from difformer_amd import DIFFormer_v2
    c = V2[name]
    cfg, sd = split_model_case(c)
    kw = {k: cfg[k] for k in ("num_layers", "kernel", "alpha", "use_bn", "use_residual", "use_weight", "use_graph",
                              "graph_weight")}
    kw["kernel"] = str(kw["kernel"])
    h = int(cfg["hidden_channels"])
    model = DIFFormer_v2(int(cfg["in_channels"]), h, h, **kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.to(dev).eval()
    with torch.no_grad():
        out = model(t(c["x"], dev), t(c["edge_index"], dev) if cfg["use_graph"] else None, t(c["n_nodes"], dev))
    assert rel_err(out.cpu().numpy(), c["out_f64"]) < TOL


_V2_RANDOM = [  # (B, max graph size, H, D, kernel)
    (300, 60, 1, 64, "simple"), (300, 60, 2, 16, "simple"), (64, 200, 1, 10, "simple"), (100, 40, 1, 128, "simple"),
    (50, 30, 2, 200, "simple"), (40, 25, 1, 256, "simple"), (7, 1500, 1, 64, "simple"),
    (300, 30, 1, 64, "sigmoid"), (200, 20, 2, 16, "sigmoid"), (150, 12, 1, 10, "sigmoid"), (90, 9, 1, 96, "sigmoid"),
]


@pytest.mark.parametrize("B,mx,H,D,kernel", _V2_RANDOM)
def test_v2_attention_random_batches(B, mx, H, D, kernel, dev):
    """Ragged batches incl. empty and single-node graphs, several heads, odd / wide widths, vs the float64 oracle."""
    rng = np.random.default_rng(B * 1000 + D)
    n_nodes = rng.integers(1, mx + 1, size=B)
    n_nodes[rng.integers(0, B, size=max(B // 20, 1))] = 0            # empty graphs
    n_nodes[rng.integers(0, B, size=max(B // 20, 1))] = 1
    n = int(n_nodes.sum())
    q, k, v = (rng.standard_normal((n, H, D)).astype(np.float32) for _ in range(3))
    out = _v2_attention(q, k, v, n_nodes, kernel, dev)
    fn = orc.v2_simple_attention if kernel == "simple" else orc.v2_sigmoid_attention
    ref = fn(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), n_nodes)
    assert rel_err(out.cpu().numpy(), ref) < TOL


@pytest.mark.parametrize("B,mx,H,M,D", [(40, 12, 1, 64, 64), (300, 30, 2, 16, 24), (9, 700, 1, 64, 64), (64, 20, 1, 100, 36),
                                        (2000, 6, 4, 8, 8)])
def test_v2_simple_attention_backward_kernels(B, mx, H, M, D, dev):
    """dq, dk, dv of the batched simple attention (three raw launches of the forward kernel + row arithmetic) against
    float64 autograd of the graph-by-graph expression (difformer-v2.py:80-111), on ragged batches with empty graphs."""
    from difformer_amd import autograd_ops as ag, ops
    rng = np.random.default_rng(B + M)
    n_nodes = rng.integers(1, mx + 1, size=B)
    n_nodes[rng.integers(0, B, size=max(B // 20, 1))] = 0
    n = int(n_nodes.sum())
    offs = np.concatenate([[0], np.cumsum(n_nodes)])
    mk = lambda w: torch.from_numpy(rng.standard_normal((n, H, w)).astype(np.float32))
    q, k, v, g = mk(M), mk(M), mk(D), mk(D)
    layout = ops.BatchLayout(torch.from_numpy(n_nodes), dev)
    leaves = [t.to(dev).requires_grad_(True) for t in (q, k, v)]
    out = ag.batched_attention(*leaves, layout, "simple")
    out.backward(g.to(dev))
    q64, k64, v64 = (t.double().requires_grad_(True) for t in (q, k, v))
    qn, kn = q64 / q64.norm(), k64 / k64.norm()
    ref = torch.zeros(n, H, D, dtype=torch.float64)
    pieces = []
    for b in range(B):
        sl = slice(int(offs[b]), int(offs[b + 1]))
        if offs[b + 1] == offs[b]:
            continue
        num = torch.einsum("nhm,hmd->nhd", qn[sl], torch.einsum("lhm,lhd->hmd", kn[sl], v64[sl])) + v64[sl].sum(0)
        den = torch.einsum("nhm,hm->nh", qn[sl], kn[sl].sum(0)) + float(n_nodes[b])
        pieces.append((sl, num / den[..., None]))
    ref = torch.cat([p for _, p in pieces], dim=0)
    assert rel_err(out.detach().cpu().numpy(), ref.detach().numpy()) < TOL
    ref.backward(g.double())
    for got, want, nm in zip(leaves, (q64, k64, v64), "qkv"):
        assert rel_err(got.grad.cpu().numpy(), want.grad.numpy()) < 2e-5, nm


def test_v2_single_graph_equals_a1(dev):
    """B = 1: difformer-v2.py:80-111 is difformer.py:18-39."""
    from difformer_amd import full_attention_conv
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(5000, 1, 64, generator=g).to(dev) for _ in range(3))
    from difformer_amd import ops
    ptr = torch.tensor([0, 5000], dtype=torch.int32, device=dev)
    a = ops.get_backend().batched_simple_attention(q, k, v, ptr)           # the batched kernel itself
    b = full_attention_conv(q, k, v, "simple")
    c = _v2_attention(q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy(), [5000], "simple", dev)   # routed to a1
    assert torch.equal(b, c)
    assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-5


def test_v2_particle_scale_batch(dev):
    """Shape of the shipped scripts (physical particle/run.sh: batch_size 8192, hidden 64, 2 layers): 8192 graphs of
    ~20 nodes, whole model against the float64 oracle; the same batch under a permutation of its graphs gives
    the same rows (graphs are independent in the simple kernel)."""
    from difformer_amd import DIFFormer_v2
    rng = np.random.default_rng(42)
    B = 8192
    n_nodes = rng.integers(8, 33, size=B)
    offs = np.concatenate([[0], np.cumsum(n_nodes)])
    n = int(offs[-1])
    src, dst = [], []
    for b in range(B):                                        # ~3 random edges per node inside each graph + self loops
        e = 3 * n_nodes[b]
        src.append(rng.integers(0, n_nodes[b], size=e) + offs[b]); dst.append(rng.integers(0, n_nodes[b], size=e) + offs[b])
    loops = np.arange(n)
    ei = np.stack([np.concatenate(src + [loops]), np.concatenate(dst + [loops])]).astype(np.int64)
    x = rng.standard_normal((n, 7)).astype(np.float32)
    cfg = dict(hidden_channels=64, num_layers=2, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
               use_weight=True, use_graph=True, graph_weight=-1)
    torch.manual_seed(9)
    model = DIFFormer_v2(7, 64, 64, **{k: v for k, v in cfg.items() if k != "hidden_channels"}).eval()
    p = {k: v.double().numpy() for k, v in model.state_dict().items()}
    ref = orc.difformer_v2_forward(p, x.astype(np.float64), ei, n_nodes, cfg)
    model = model.to(dev)
    with torch.no_grad():
        out = model(t(x, dev), t(ei, dev), t(n_nodes, dev))
    assert rel_err(out.cpu().numpy(), ref) < TOL


# ------------------------------------------------------------------ skewed degrees: row order of the blocked SpMM
def _zipf_graph(n, e, seed, dev):
    g = torch.Generator().manual_seed(seed)
    w = (torch.arange(n, dtype=torch.float64) + max(n // 120, 1)) ** -0.75
    cdf = torch.cumsum(w, 0) / w.sum()
    perm = torch.randperm(n, generator=g)
    a, b = (perm[torch.searchsorted(cdf, torch.rand(e, generator=g, dtype=torch.float64)).clamp_(max=n - 1)]
            for _ in range(2))
    return torch.stack([torch.cat([a, b]), torch.cat([b, a])]).to(dev)


@pytest.mark.parametrize("n,e,lo,cnt", [(5000, 200000, 0, 5000), (5000, 200000, 1234, 2001), (70000, 3000000, 0, 70000),
                                        (70000, 3000000, 61250, 8750), (700, 9000, 13, 513), (700, 9000, 100, 300)])
def test_row_order_is_the_stable_degree_sort(n, e, lo, cnt, dev):
    """dif_row_order: bit-exact against a stable argsort of the shard's degrees (descending, ties by row)."""
    from difformer_amd import ops
    ei = _zipf_graph(n, e, n + lo, dev)
    csr = ops.GraphCSR.build(ei, None, n, 4)
    order, stats = ops.get_backend().row_order(csr.rowptr, lo, cnt)
    deg = np.diff(csr.rowptr.cpu().numpy().astype(np.int64))[lo: lo + cnt]
    assert np.array_equal(order.cpu().numpy(), np.argsort(-deg, kind="stable").astype(np.int32))
    assert stats.tolist() == [int((deg * cnt > 4 * deg.sum()).sum()), int(deg.max())]
    o2, n_split = csr.row_order(lo, cnt)                      # skewed graph: the host keeps the order
    assert n_split == stats[0].item() and n_split > 0 and torch.equal(o2, order)


@pytest.mark.parametrize("n,e,d,nb", [(30000, 3000000, 64, 5), (30000, 3000000, 128, 3), (9000, 400000, 32, 2)])
def test_blocked_spmm_with_row_order_equals_natural_order(n, e, d, nb, dev):
    """The row order only regroups rows into waves: rows that are not split are summed in the same order -> bitwise
    equal; the split hub rows (degree > 4x mean) add four partial sums -> equal to rounding; everything matches the
    oracle on a Zipf-profile graph (hub rows ~13x the mean degree)."""
    from difformer_amd import ops
    be = ops.get_backend()
    ei = _zipf_graph(n, e, d, dev)
    csr = ops.GraphCSR.build(ei, None, n, nb)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(n, d, generator=g).to(dev)
    a = torch.randn(n, d, generator=g).to(dev)
    args = (csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, n, csr.nnz, x)
    full_nat = be.spmm(*args, 0, n, a, 0.5, 2.0, None, None)
    order, n_split = csr.row_order(0, n)
    assert n_split > 0
    full_ord = be.spmm(*args, 0, n, a, 0.5, 2.0, None, (order, n_split))
    whole = order[n_split:].long()
    assert torch.equal(full_nat[whole], full_ord[whole])
    assert rel_err(full_ord.cpu().numpy(), full_nat.cpu().numpy()) < 2e-6
    assert torch.equal(full_nat, be.spmm(*args, 0, n, a, 0.5, 2.0, None, (order, 0)))   # ordered, nothing split
    lo, cnt = n // 3, n // 2 + 7
    part = be.spmm(*args, lo, cnt, a[lo: lo + cnt], 0.5, 2.0, None, csr.row_order(lo, cnt))
    assert rel_err(part.cpu().numpy(), full_nat[lo: lo + cnt].cpu().numpy()) < 2e-6
    ref = 2.0 * orc.gcn_conv(x.cpu().numpy().astype(np.float64)[:, None, :], ei.cpu().numpy(), None)[:, 0, :] \
        + 0.5 * a.cpu().numpy().astype(np.float64)
    assert rel_err(full_ord.cpu().numpy(), ref) < TOL


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_v2_training_step_gradients(kernel, dev):
    """loss.backward() through DIFFormer_v2 (physical particle/main.py:85-93): every parameter gradient against float64
    autograd of a graph-by-graph restatement of difformer-v2.py written with dense per-graph tensors."""
    from difformer_amd import DIFFormer_v2
    torch.manual_seed(2)
    n_nodes = torch.tensor([5, 1, 9, 3])
    offs = [0, 5, 6, 15, 18]
    n = 18
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, 6, generator=g)
    pieces = [torch.randint(offs[b], offs[b + 1], (2, 3 * int(n_nodes[b])), generator=g) for b in range(4)]
    ei = torch.cat(pieces + [torch.arange(n).repeat(2, 1)], dim=1)
    model = DIFFormer_v2(6, 16, 16, num_layers=2, kernel=kernel, dropout=0.0).train()
    ref = {k: v.detach().double().requires_grad_(True) for k, v in model.named_parameters()}

    def ref_forward(p, x):
        lin = torch.nn.functional.linear
        ln = lambda t, i: torch.nn.functional.layer_norm(t, (16,), p[f"bns.{i}.weight"], p[f"bns.{i}.bias"])
        deg = torch.zeros(n, dtype=torch.float64).index_add_(0, ei[1], torch.ones(ei.shape[1], dtype=torch.float64))
        val = (1.0 / deg[ei[1]]).sqrt() * (1.0 / deg[ei[0]]).sqrt()
        adj = torch.zeros(n, n, dtype=torch.float64).index_put_((ei[1], ei[0]), val, accumulate=True)
        h = torch.relu(ln(lin(x, p["fcs.0.weight"], p["fcs.0.bias"]), 0))
        hs = [h]
        B = len(n_nodes)
        for i in range(2):
            q = lin(h, p[f"convs.{i}.Wq.weight"], p[f"convs.{i}.Wq.bias"])
            k = lin(h, p[f"convs.{i}.Wk.weight"], p[f"convs.{i}.Wk.bias"])
            v = lin(h, p[f"convs.{i}.Wv.weight"], p[f"convs.{i}.Wv.bias"])
            att = torch.zeros_like(v)
            if kernel == "simple":
                qn, kn = q / q.norm(), k / k.norm()
                for b in range(B):
                    sl = slice(offs[b], offs[b + 1])
                    num = qn[sl] @ (kn[sl].T @ v[sl]) + v[sl].sum(0)
                    den = qn[sl] @ kn[sl].sum(0) + float(n_nodes[b])
                    att[sl] = num / den[:, None]
            else:
                for pos in range(int(n_nodes.max())):
                    idx = torch.tensor([offs[b] + pos for b in range(B) if n_nodes[b] > pos])
                    s = torch.sigmoid(q[idx] @ k[idx].T)
                    den = s.sum(1) + 0.5 * (B - len(idx)) + 1e-9
                    att = att.index_put((idx,), (s / den[:, None]) @ v[idx])
            z = 0.5 * (att + adj @ v) + 0.5 * hs[i]
            h = torch.relu(ln(z, i + 1))
            hs.append(h)
        return lin(h, p["fcs.1.weight"], p["fcs.1.bias"])

    w = torch.randn(n, 16, generator=g)
    (ref_forward(ref, x.double()) * w.double()).sum().backward()
    model = model.to(dev)
    out = model(x.to(dev), ei.to(dev), n_nodes.to(dev))
    (out * w.to(dev)).sum().backward()
    for name, p in model.named_parameters():
        assert rel_err(p.grad.cpu().numpy(), ref[name].grad.numpy()) < 2e-4, name


# ------------------------------------------------------------------ edge cases
@pytest.mark.parametrize("n", [1, 2, 3, 15, 17, 63, 65])
@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_attention_tiny_inputs(n, kernel, dev):
    """Fewer rows than one MFMA tile / one wave step, down to a single node."""
    from difformer_amd import full_attention_conv
    rng = np.random.default_rng(n)
    q, k, v = (rng.standard_normal((n, 2, 24)).astype(np.float32) for _ in range(3))
    out = full_attention_conv(t(q, dev), t(k, dev), t(v, dev), kernel)
    ref = orc.full_attention_conv(q.astype(np.float64), k.astype(np.float64), v.astype(np.float64), kernel)
    assert rel_err(out.cpu().numpy(), ref) < TOL


def test_simple_attention_zero_norm_is_non_finite_like_the_reference(dev):
    """difformer.py:20-21 divides by the Frobenius norms: all-zero queries give 0/0 there, and here."""
    from difformer_amd import full_attention_conv
    q = torch.zeros(40, 1, 16, device=dev)
    k, v = torch.randn(40, 1, 16, device=dev), torch.randn(40, 1, 16, device=dev)
    ref = orc.simple_attention(q.cpu().numpy(), k.cpu().numpy(), v.cpu().numpy())
    out = full_attention_conv(q, k, v, "simple")
    assert not np.isfinite(ref).any() and not torch.isfinite(out).any()


def test_gcn_conv_edge_free_and_single_node_graphs(dev):
    """E = 0 (every degree 0 -> every value dropped, difformer.py:73-74) and N = 1 with a self loop."""
    from difformer_amd import DIFFormer, gcn_conv
    x = torch.randn(9, 1, 8, device=dev)
    out = gcn_conv(x, torch.zeros(2, 0, dtype=torch.long, device=dev), None)
    assert out.shape == x.shape and not out.any()
    one = gcn_conv(x[:1], torch.zeros(2, 1, dtype=torch.long, device=dev), None)
    assert rel_err(one.cpu().numpy(), x[:1].cpu().numpy()) < 1e-6
    torch.manual_seed(0)
    model = DIFFormer(5, 8, 3).eval()
    xs = torch.randn(1, 5)
    p = {k: v.double().numpy() for k, v in model.state_dict().items()}
    cfg = dict(hidden_channels=8, num_layers=2, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
               use_weight=True, use_graph=True, graph_weight=-1, use_source=False)
    ei = torch.zeros(2, 1, dtype=torch.long)
    ref = orc.difformer_forward(p, xs.double().numpy(), ei.numpy(), None, cfg)
    with torch.no_grad():
        out = model.to(dev)(xs.to(dev), ei.to(dev))
    assert rel_err(out.cpu().numpy(), ref) < TOL


def test_empty_inputs_raise(dev):
    """Zero nodes: the C ABI refuses (DIF_E_BADARG) and the host raises; nothing is launched."""
    from difformer_amd import full_attention_conv
    from difformer_amd._lib import DifformerHipError
    q = torch.zeros(0, 1, 8, device=dev)
    with pytest.raises(DifformerHipError):
        full_attention_conv(q, q, q, "simple")


@pytest.mark.parametrize("d,nb", [(64, 4), (128, 3), (256, 2), (72, 3)])
def test_bf16_blocked_spmm_wide_lanes_and_row_order(d, nb, dev):
    """bfloat16 rows in the blocked kernel (8 elements = 16 bytes per lane when the width allows; d = 72 keeps the 4-wide
    mapping), natural and degree-ordered walks with split hub rows, against the oracle on the bf16-rounded operands."""
    from difformer_amd import ops
    be = ops.get_backend()
    n, e = 20000, 1500000
    ei = _zipf_graph(n, e, d, dev)
    csr = ops.GraphCSR.build(ei, None, n, nb)
    g = torch.Generator().manual_seed(d)
    x, x64 = _bf(torch.randn(n, d, generator=g))
    a, a64 = _bf(torch.randn(n, d, generator=g))
    args = (csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, n, csr.nnz, x.to(dev))
    ref = 2.0 * orc.gcn_conv(x64[:, None, :], ei.cpu().numpy(), None)[:, 0, :] + 0.5 * a64
    order = csr.row_order(0, n)
    assert order is not None and order[1] > 0
    for o in (None, order):
        out = be.spmm(*args, 0, n, a.to(dev), 0.5, 2.0, None, o)
        assert out.dtype == torch.bfloat16
        assert rel_err(out.float().cpu().numpy(), ref) < BF16_TOL


@pytest.mark.parametrize("world,zipf,dt", [(2, False, torch.float32), (4, True, torch.float32), (8, False, torch.float32),
                                           (8, True, torch.float32), (4, False, torch.bfloat16)])
def test_split_product_own_blocks_then_the_rest(world, zipf, dt, dev):
    """Row-sharded SpMM as gcn_aggregate runs it: source blocks aligned with the rank boundaries, part 0 over a tensor
    that holds ONLY the rank's own value rows (what exists before the all-gather lands), part 1 over the gathered rows
    on top of the parked accumulators, with combine and fused tail -- rank after rank against the unsharded launch."""
    from difformer_amd import ops
    from difformer_amd.dist import RowShard
    be = ops.get_backend()
    n, e, d = (24000 if dt == torch.float32 else 40000), 1600000, 64      # bf16 rows: x must still exceed the L2
    g = torch.Generator().manual_seed(world)
    ei = _zipf_graph(n, e, world, dev) if zipf else torch.randint(0, n, (2, 2 * e), generator=g).to(dev)
    shards = [RowShard(n, rank=r, world=world) for r in range(world)]
    nb, rows = ops.choose_shard_blocks(n, d * (2 if dt == torch.bfloat16 else 4), ei.shape[1], shards[0])
    assert shards[0].counts[0] % rows == 0
    csr = ops.GraphCSR.build(ei, None, n, nb, block_rows=rows)
    v = torch.randn(n, d, generator=g).to(dev).to(dt)
    a = torch.randn(n, d, generator=g).to(dev).to(dt)
    prev = torch.randn(n, d, generator=g).to(dev).to(dt)
    lw, lb = (torch.rand(d, generator=g) + 0.5).to(dev).to(dt), torch.randn(d, generator=g).to(dev).to(dt)
    tail = lambda lo, hi: dict(x0=None, prev=prev[lo:hi], alpha=0.5, ln_weight=lw, ln_bias=lb, eps=1e-5)
    args = (csr.rowptr, csr.blkptr, csr.n_blocks, csr.src, csr.val, n, csr.nnz)
    full = be.spmm(*args, v, 0, n, a, 1.0, 1.0, tail(0, n), csr.row_order(0, n)).float()
    tol = 2e-2 if dt == torch.bfloat16 else 1e-5
    for s in shards:
        lo, cnt = s.row_begin, s.n_local
        own_lo, own_hi = lo // rows, -(-(lo + cnt) // rows)
        order = csr.row_order(lo, cnt)
        assert zipf == (order is not None)
        own = v[lo: lo + cnt].clone()                                        # nothing but this rank's rows
        scratch = be.spmm(*args, own, lo, cnt, None, 1.0, 1.0, None, order, (0, own_lo, own_hi, None, lo))
        out = be.spmm(*args, v, lo, cnt, a[lo: lo + cnt], 1.0, 1.0, tail(lo, lo + cnt), order,
                      (1, own_lo, own_hi, scratch, 0))
        assert rel_err(out.float().cpu().numpy(), full[lo: lo + cnt].cpu().numpy()) < tol, (world, s.rank)


@pytest.mark.parametrize("n,H,D,use_x0,use_prev,use_ln,relu", [
    (5000, 1, 64, True, True, True, False), (3001, 2, 64, False, True, True, False), (4097, 1, 128, True, False, True, True),
    (2500, 1, 32, False, False, True, True), (2000, 3, 16, True, True, False, False), (1000, 1, 64, False, False, False, True),
    (70000, 1, 64, True, True, True, False), (300, 1, 256, False, True, True, False), (15000, 1, 300, False, True, True, False),
    (1300, 2, 400, True, True, True, True), (777, 1, 512, True, False, False, True)])
def test_layer_tail_backward_kernel_matches_float64_autograd(n, H, D, use_x0, use_prev, use_ln, relu):
    """dif_layer_tail_bwd_f32 against torch autograd of difformer.py:137-140, :200-203 in float64."""
    from difformer_amd import autograd_ops as ag
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(n + D)
    conv = torch.randn(n, H, D, generator=g)
    x0 = torch.randn(n, D, generator=g) if use_x0 else None
    prev = torch.randn(n, D, generator=g) if use_prev else None
    w = (torch.rand(D, generator=g) + 0.5) if use_ln else None
    b = torch.randn(D, generator=g) if use_ln else None
    gout = torch.randn(n, D, generator=g)
    leaves64 = [None if t is None else t.double().requires_grad_(True) for t in (conv, x0, prev, w, b)]
    z = leaves64[0].mean(dim=1)
    if x0 is not None:
        z = z + leaves64[1]
    if prev is not None:
        z = 0.3 * z + 0.7 * leaves64[2]
    if use_ln:
        z = torch.nn.functional.layer_norm(z, (D,), leaves64[3], leaves64[4], 1e-5)
    if relu:
        z = torch.relu(z)
    z.backward(gout.double())
    leaves = [None if t is None else t.to(dev).requires_grad_(True) for t in (conv, x0, prev, w, b)]
    out = ag.layer_tail(leaves[0], leaves[1], leaves[2], 0.3, leaves[3], leaves[4], 1e-5, relu)
    assert rel_err(out.detach().cpu().numpy(), z.detach().numpy()) < 1e-5
    from difformer_amd import ops
    be = ops.get_backend()
    be.kernel_events = {}
    out.backward(gout.to(dev))
    torch.cuda.synchronize()
    launched, be.kernel_events = set(be.kernel_events), None
    assert "dif_layer_tail_bwd_f32" in launched            # the HIP backward ran, not the tensor-op fallback
    for got, want in zip(leaves, leaves64):
        if got is not None:
            assert rel_err(got.grad.cpu().numpy(), want.grad.numpy()) < 2e-5, (got.shape,)


@pytest.mark.parametrize("n,ci,co", [(20000, 64, 192), (132534, 8, 64), (9000, 64, 112), (5000, 100, 40)])
def test_linear_weight_gradient_through_the_reduce_kernel(n, ci, co):
    """d_W = g^T x and d_b = colsum(g) from stage 1 of the simple kernel (K = g, V = x) vs float64."""
    from difformer_amd import autograd_ops as ag
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(ci * co)
    x, w, b, gout = (torch.randn(n, ci, generator=g), torch.randn(co, ci, generator=g) / ci ** 0.5,
                     torch.randn(co, generator=g), torch.randn(n, co, generator=g))
    xd, wd, bd = (t.to(dev).requires_grad_(True) for t in (x, w, b))
    y = ag.linear(xd, wd, bd)
    y.backward(gout.to(dev))
    x64, w64, b64 = (t.double().requires_grad_(True) for t in (x, w, b))
    y64 = torch.nn.functional.linear(x64, w64, b64)
    y64.backward(gout.double())
    assert rel_err(y.detach().cpu().numpy(), y64.detach().numpy()) < 1e-5
    for got, want in ((xd, x64), (wd, w64), (bd, b64)):
        assert rel_err(got.grad.cpu().numpy(), want.grad.numpy()) < 2e-5


@pytest.mark.parametrize("n,h,m,d,bf16", [(20000, 1, 400, 400, False), (3000, 2, 128, 128, False), (5000, 1, 512, 64, False),
                                          (4000, 1, 96, 200, False), (2500, 1, 300, 300, True), (9000, 3, 68, 132, False),
                                          (700, 1, 130, 70, False)])
def test_simple_apply_wide_heads(n, h, m, d, bf16, dev):
    """Stage 2 (difformer.py:29-39) for the widths the scripts train with (run.sh: 128 / 300 / 400): the workgroup keeps
    s * KtV^T for 64 output columns in LDS.  M != D and ragged widths included; checked against the float64 oracle fed
    with the stage-1 record it implies (so only stage 2 is under test)."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + m + d)
    q, k = (torch.randn(n, h, m, generator=g) for _ in range(2))
    v = torch.randn(n, h, d, generator=g)
    if bf16:
        q, k, v = (t.to(torch.bfloat16) for t in (q, k, v))
    be = ops.get_backend()
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    rec = be.simple_reduce(qd, kd, vd)
    out = be.simple_apply(qd, rec, n, d).float().cpu().numpy()
    q64, k64, v64 = (t.double().numpy() for t in (q.float(), k.float(), v.float()))
    s = 1.0 / (np.linalg.norm(q64) * np.linalg.norm(k64))
    num = s * np.einsum("nhm,hmd->nhd", q64, np.einsum("lhm,lhd->hmd", k64, v64)) + v64.sum(0)
    den = s * np.einsum("nhm,hm->nh", q64, k64.sum(0)) + n
    assert rel_err(out, num / den[..., None]) < (2e-2 if bf16 else TOL)


@pytest.mark.parametrize("n,m,d", [(6000, 128, 128), (4100, 96, 72), (5003, 68, 128), (4096, 128, 100), (20000, 72, 68)])
def test_simple_apply_on_the_split_row_gemm_kernel(n, m, d, dev):
    """Stage 2 at ONE head of 65..128 columns on >= 4,096 rows (run.sh's hidden 128): rowgemm_split_kernel in its apply mode --
    K^T V and sum k scaled on the device by the record's norms, sum v as the bias, the division by q . sum k + N per row -- on
    split-bfloat16 operands; ops.set_exact_fp32 puts the call back on simple_apply_wide_kernel.  Both against float64; ragged
    row counts and M != D included."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + m + d)
    q, k = (torch.randn(n, 1, m, generator=g) for _ in range(2))
    v = torch.randn(n, 1, d, generator=g)
    be = ops.get_backend()
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
    rec = be.simple_reduce(qd, kd, vd)
    q64, k64, v64 = (t.double().numpy() for t in (q, k, v))
    s = 1.0 / (np.linalg.norm(q64) * np.linalg.norm(k64))
    num = s * np.einsum("nhm,hmd->nhd", q64, np.einsum("lhm,lhd->hmd", k64, v64)) + v64.sum(0)
    den = s * np.einsum("nhm,hm->nh", q64, k64.sum(0)) + n
    want = num / den[..., None]
    errs, outs = {}, {}
    try:
        for exact in (False, True):
            ops.set_exact_fp32(exact)
            outs[exact] = be.simple_apply(qd, rec, n, d)
            errs[exact] = rel_err(outs[exact].cpu().numpy(), want)
    finally:
        ops.set_exact_fp32(False)
    assert errs[True] < 5e-6 and errs[False] < 2e-5 and not torch.equal(outs[True], outs[False]), errs


# ------------------------------------------------------------------ repeated inference forwards replay as one hipGraph
def test_repeated_inference_forwards_are_captured_and_stay_correct(dev):
    """DIFFormer.forward: the third consecutive eval / no_grad call with the same operands captures the forward as a hipGraph;
    replays are bitwise equal to the eager result, see new VALUES written into x in place, never alias one another, and any
    change of operands or parameters falls back to the eager path."""
    from difformer_amd import DIFFormer
    torch.manual_seed(11)
    n = 3000
    model = DIFFormer(40, 64, 6, num_layers=2, kernel="simple").to(dev).eval()
    g = torch.Generator().manual_seed(4)
    x = torch.randn(n, 40, generator=g).to(dev)
    x2 = torch.randn(n, 40, generator=g).to(dev)
    ei = torch.cat([torch.randint(0, n, (2, 12000), generator=g), torch.arange(n).repeat(2, 1)], dim=1).to(dev)
    from difformer_amd import ops
    model.auto_graph = False                               # (it picks the aggregation kernel: otherwise eager #1 and the capture differ by rounding)
    with torch.no_grad():
        ref, ref2 = model(x, ei).clone(), model(x2, ei).clone()
    model.auto_graph = True
    with torch.no_grad():
        outs = [model(x, ei) for _ in range(6)]
    assert model._ag_state is not None and model._ag_state[2] is not None, "the forward should have been captured"
    assert all(torch.equal(o, ref) for o in outs)
    assert len({o.data_ptr() for o in outs[3:]}) == 3                  # replays return fresh tensors
    with torch.no_grad():
        x.copy_(x2)                                                    # new values at the same address: the replay reads them
        assert torch.equal(model(x, ei), ref2)
        other = x2.clone()
        assert torch.equal(model(other, ei), ref2)                     # another tensor: eager (and the capture is dropped)
        assert model._ag_state[2] is None
        for _ in range(3):
            model(x, ei)
        assert model._ag_state[2] is not None
        model.fcs[1].bias.add_(1.0)                                    # a parameter changed (in place: version bump)
        shifted = model(x, ei)
        assert model._ag_state[2] is None and torch.allclose(shifted, ref2 + 1.0, atol=1e-5)
    model.train()
    out_t = model(x, ei)                                               # training: never captured
    assert out_t.requires_grad and model._ag_state[2] is None


def test_exact_fp32_switch_keeps_every_product_on_the_fp32_core(dev):
    """DIFFORMER_EXACT_FP32=1 (read once per process, so this runs in a child): the long-row input Linear takes the fp32
    MFMA and the output Linear is its own launch instead of the split-bfloat16 product inside the last layer kernel; the
    logits agree with the default build of the same forward to the few 1e-6 the split operands move them, and with the
    float64 oracle to 1e-4."""
    import os, subprocess, sys, json
    code = r'''
import json, sys, numpy as np, torch
sys.path.insert(0, ".")
from difformer_amd import DIFFormer, ops
from oracle import difformer_oracle as orc
dev = torch.device("cuda:0")
torch.manual_seed(5)
n, f_in, c = 9000, 260, 12
model = DIFFormer(f_in, 64, c, num_layers=2, kernel="simple").to(dev).eval()
g = torch.Generator().manual_seed(6)
x = torch.randn(n, f_in, generator=g)
ei = torch.cat([torch.randint(0, n, (2, 50 * n), generator=g), torch.arange(n).repeat(2, 1)], dim=1)
be = ops.get_backend()
be.kernel_events = {}
with torch.no_grad():
    y = model(x.to(dev), ei.to(dev)).cpu().numpy()
calls = {k: len(v) for k, v in be.kernel_events.items()}
cfg = dict(hidden_channels=64, num_layers=2, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
           use_weight=True, use_graph=True, graph_weight=-1, use_source=False)
p = {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()}
ref = orc.difformer_forward(p, x.double().numpy(), ei.numpy(), None, cfg)
np.save(sys.argv[1], y)
print(json.dumps({"calls": calls, "err": float(np.max(np.abs(y - ref)) / np.max(np.abs(ref)))}))
'''
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    outs = {}
    with tempfile.TemporaryDirectory() as td:
        for flag in ("0", "1"):
            env = dict(os.environ, DIFFORMER_EXACT_FP32=flag)
            r = subprocess.run([sys.executable, "-c", code, os.path.join(td, f"y{flag}.npy")], cwd=root, env=env,
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr[-2000:]
            outs[flag] = (json.loads(r.stdout.strip().splitlines()[-1]), np.load(os.path.join(td, f"y{flag}.npy")))
    (d0, y0), (d1, y1) = outs["0"], outs["1"]
    assert d0["err"] < TOL and d1["err"] < TOL
    assert d0["calls"].get("dif_linear_f32", 0) == 1 and d1["calls"].get("dif_linear_f32", 0) == 2     # input (+ output) Linear
    assert rel_err(y1, y0) < 5e-5 and d1["err"] <= d0["err"] * 1.5 + 1e-7


def test_packed_weight_cache_does_not_confuse_tensors_at_a_recycled_address(dev):
    """The long-row Linear packs W once per tensor; a NEW weight that the allocator places at a freed weight's address (same
    shape, version 0) must be packed afresh."""
    from difformer_amd import ops
    be = ops.get_backend()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(300, 1433, generator=g).to(dev)
    b = torch.zeros(64, device=dev)
    for trial in range(6):
        W = (torch.randn(64, 1433, generator=g) / 38.0).to(dev)
        out = be.linear(x, W, b)
        assert rel_err(out.cpu().numpy(), x.double().cpu().numpy() @ W.double().cpu().numpy().T) < 1e-5, trial
        del W


@pytest.mark.parametrize("n,ci,co", [(100000, 65, 128), (3000, 128, 96), (5001, 8, 68), (700, 40, 128)])
def test_narrow_linear_with_layernorm_over_up_to_128_features(n, ci, co, dev):
    """The input layer at the scripts' hidden 128 (run.sh:42-44: Pokec, 65 -> 128, LayerNorm, ReLU) in one launch: both
    64-feature blocks of a row tile are normalised together."""
    from difformer_amd import ops
    g = torch.Generator().manual_seed(n + co)
    x = torch.randn(n, ci, generator=g)
    W, b = torch.randn(co, ci, generator=g) / np.sqrt(ci), torch.randn(co, generator=g)
    lw, lb = torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g)
    be = ops.get_backend()
    for relu in (True, False):
        out = be.linear(x.to(dev), W.to(dev), b.to(dev), lw.to(dev), lb.to(dev), 1e-5, relu)
        ref = orc.layer_norm(x.double().numpy() @ W.double().numpy().T + b.double().numpy(), lw.double().numpy(), lb.double().numpy())
        if relu:
            ref = np.maximum(ref, 0)
        assert rel_err(out.cpu().numpy(), ref) < 1e-5


@pytest.mark.parametrize("n,deg,hubs,F", [(120000, 20, (15000, 1025, 1024), 64), (90000, 24, (130000, 3000), 64), (70000, 18, (5000,) * 20, 32)])
def test_gcn_conv_hub_rows_of_a_mid_degree_graph(n, deg, hubs, F, dev):
    """spmm_wave_row_kernel (graphs of ~20 entries per row: the full Pokec graph, eval.py:40-43) gives a row to ONE wave; a social
    graph's hubs (Pokec: 14,854 entries) are noted and taken by the block's four waves together at the end (round 5; before: a
    120,000-entry row held one wave for 4 ms of a 1.3-ms launch).  Rows just below / above the threshold, more hubs than a block
    can note, one giant row: against the float64 oracle, bitwise equal from call to call."""
    from difformer_amd import gcn_conv
    g = torch.Generator().manual_seed(n + deg)
    ei = torch.randint(0, n, (2, n * deg), generator=g)
    at = 0
    for k, h in enumerate(hubs):                       # hub k: the first entries of the list point at node 7 k + 3
        ei[1, at: at + h] = 7 * k + 3
        at += h
    x = torch.randn(n, 1, F, generator=g)
    ref = orc.gcn_conv(x.double().numpy(), ei.numpy(), None)
    eid, xd = ei.to(dev), x.to(dev)
    out = gcn_conv(xd, eid, None)
    assert rel_err(out.cpu().numpy(), ref) < 1e-5
    assert torch.equal(gcn_conv(xd, eid, None), out)
    w = torch.rand(ei.shape[1], generator=g) + 0.1
    refw = orc.gcn_conv(x.double().numpy(), ei.numpy(), w.double().numpy())
    assert rel_err(gcn_conv(xd, eid, w.to(dev)).cpu().numpy(), refw) < 1e-5


@pytest.mark.parametrize("n,m,d", [(100000, 384, 128), (6000, 256, 100), (5000, 128, 64), (4100, 72, 128), (9000, 512, 68)])
def test_reduce_slab_kernel_with_wide_k(n, m, d, dev):
    """g^T x for the fused q | k | v projection at hidden 128 (k = g [n, 384], v = x [n, 128]) and other k / v widths through
    dif_simple_reduce_f32's one-read slab kernel (round 5): K^T V, both column sums and both sums of squares against float64."""
    import ctypes
    from difformer_amd import _lib, ops
    from difformer_amd.backend_hip import _stream
    lib = _lib.load()
    g = torch.Generator().manual_seed(n + m + d)
    q = (torch.randn(n, m, generator=g) + 0.1).to(dev)
    k = (torch.randn(n, m, generator=g) - 0.2).to(dev)
    v = (torch.randn(n, d, generator=g) + 0.3).to(dev)
    rec = torch.empty(lib.dif_simple_reduced_len(1, m, d), dtype=torch.float32, device=dev)
    ws_bytes = lib.dif_simple_workspace_bytes(n, 1, m, d)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    rc = lib.dif_simple_reduce_f32(q.data_ptr(), m, k.data_ptr(), m, v.data_ptr(), d, n, 1, m, d, rec.data_ptr(), ws.data_ptr(), ws_bytes,
                                   _stream(dev))
    assert rc == 0
    r = rec.cpu().numpy().astype(np.float64)
    q64, k64, v64 = (t.double().cpu().numpy() for t in (q, k, v))
    assert rel_err(r[: m * d].reshape(m, d), k64.T @ v64) < 1e-5
    assert rel_err(r[m * d: m * d + m], k64.sum(0)) < 1e-5 and rel_err(r[m * d + m: m * d + m + d], v64.sum(0)) < 1e-5
    assert abs(r[m * d + m + d] - (q64 ** 2).sum()) < 1e-5 * (q64 ** 2).sum()
    assert abs(r[m * d + m + d + 1] - (k64 ** 2).sum()) < 1e-5 * (k64 ** 2).sum()


@pytest.mark.parametrize("n,K,C", [(15000, 300, 300), (13000, 400, 400), (2000, 512, 64), (5000, 68, 300), (1024, 132, 196),
                                   (18846, 300, 304), (3000, 64, 192)])
def test_rowgemm_wide_split_kernel_vs_float64(n, K, C, dev):
    """dif_rowgemm_f32 beyond 128 columns from 1,024 rows (hidden 300 / 400 of image and text/run.sh in training): a workgroup per 64
    output columns with its slab of the matrix as split-bfloat16 fragments in LDS (round 6; the fp32 kernel below that size and under
    DIFFORMER_EXACT_FP32=1) -- A Mat + bias + accumulate against float64, a column slice as A, bitwise repeatable."""
    from difformer_amd import ops
    be = ops.get_backend()
    g = torch.Generator().manual_seed(n + K + C)
    wide = torch.randn(n, K + 8, generator=g).to(dev)
    A = wide[:, 4:4 + K]
    mat = (torch.randn(K, C, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    acc = torch.randn(n, C, generator=g).to(dev)
    be.kernel_events = {}
    out = be.row_gemm(A, mat, bias, acc)
    launched, be.kernel_events = set(be.kernel_events), None
    assert "dif_rowgemm_f32" in launched
    ref = A.double() @ mat.double() + bias.double() + acc.double()
    assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 2e-5
    assert torch.equal(be.row_gemm(A, mat, bias, acc), out)


@pytest.mark.parametrize("n,K,C", [(100000, 128, 128), (5000, 100, 128), (4096, 128, 72), (6000, 68, 96)])
def test_rowgemm_split_kernel_vs_float64(n, K, C, dev):
    """dif_rowgemm_f32 at one head of 65..128 x 65..128 from 4,096 rows: all output columns per workgroup, split-bfloat16 operands
    (round 5; the fp32 kernel below that size and under DIFFORMER_EXACT_FP32=1) -- A Mat + bias + accumulate against float64."""
    from difformer_amd import ops
    be = ops.get_backend()
    g = torch.Generator().manual_seed(n + K + C)
    A = torch.randn(n, K, generator=g).to(dev)
    mat = (torch.randn(K, C, generator=g) / K ** 0.5).to(dev)
    bias = torch.randn(C, generator=g).to(dev)
    acc = torch.randn(n, C, generator=g).to(dev)
    out = be.row_gemm(A, mat, bias, acc)
    ref = A.double() @ mat.double() + bias.double() + acc.double()
    assert rel_err(out.cpu().numpy(), ref.cpu().numpy()) < 2e-5
    assert torch.equal(be.row_gemm(A, mat, bias, acc), out)
