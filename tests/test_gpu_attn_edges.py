"""Attention on graph edges on the MI355X (csrc/attn_edges.hip behind include/difformer_edges.h): parity through the C ABI for
every kernel instantiation between guard bands, exact sums, permutation, ids out of range, the functional API, the model method
against the dense map, and peak memory.  The bar is rel_err <= 1e-4 against tests/edges_ref.py (float64)."""
import functools
import gc

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, split_model_case
from guarded import GuardedArena
import edges_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = {"simple": 0, "sigmoid": 1}
PAD = 8             # columns around the operands inside their wider tensors: ld = H M + 8, the slice starts at element 4

# (n_q, n_k, E): one edge; fewer, as many and more edges than a wave has lanes; several workgroups; n_q != n_k with more than
# one workgroup of every lane-group width (the widest takes 16 edges per workgroup, the narrowest 256).
GRAPHS = [(1, 1, 1), (17, 33, 63), (17, 33, 64), (17, 33, 65), (100, 100, 257), (300, 1000, 4099)]
# (H, M) -> lanes per dot product: 4 (M <= 16), 16 (<= 64), 32 (<= 128: 68 leaves lanes idle, 128 fills them), 64 (300: second
# piece partly masked; 512: both pieces full).  Both modes on every case: all 16 kernels run.
WIDTHS = [(1, 4), (2, 64), (1, 68), (2, 128), (1, 300), (1, 512)]


@pytest.fixture(scope="module")
def edges():
    from difformer_amd import _lib
    return _lib.load_edges()


def _csr(ei, n_q):
    """Target-row CSR of an edge list on the host, entries of a row in list order: (rowptr int32 [n_q + 1], src int32 [E])."""
    order = np.argsort(ei[1], kind="stable")
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(ei[1], minlength=n_q))]).astype(np.int32)
    return torch.from_numpy(rowptr), torch.from_numpy(ei[0][order].astype(np.int32))


@functools.lru_cache(maxsize=None)
def _case(n_q, n_k, E, h, m, mode, hubs=()):
    """Operands (host) and the float64 results, made once per case: qw / kw the WIDE tensors, q / k their column slices."""
    g = torch.Generator().manual_seed(n_q + n_k + E + h + m)
    std = m ** -0.25 if mode == 1 else 1.0                      # scores of unit variance: sigma does not saturate
    qw, kw = torch.randn(n_q, h * m + PAD, generator=g) * std, torch.randn(n_k, h * m + PAD, generator=g) * std
    qw[:, :4] = qw[:, 4 + h * m:] = kw[:, :4] = kw[:, 4 + h * m:] = float("nan")        # what lies around the operands
    q, k = qw[:, 4:4 + h * m].view(n_q, h, m), kw[:, 4:4 + h * m].view(n_k, h, m)
    scale = torch.rand(n_q, h, generator=g) + 0.5
    ei = edges_ref.random_graph(n_q, n_k, E, seed=E + m, hubs=hubs)
    return dict(qw=qw, kw=kw, q=q, k=k, scale=scale, ei=ei, values=edges_ref.raw_values(q, k, scale, mode, ei),
                mass=edges_ref.raw_mass(q, k, scale, mode, ei))


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _run_edges(edges, qw, kw, scale, n_q, n_k, h, m, mode, ei, arena=None):
    """dif_edge_attn_f32 on device copies of the wide tensors; out and status between guard bands, poisoned."""
    from difformer_amd import _lib
    arena = arena or GuardedArena()
    qd, kd = qw.to(DEV), kw.to(DEV)
    eid = torch.from_numpy(ei).to(DEV) if isinstance(ei, np.ndarray) else ei
    E = eid.shape[1]
    out = arena.alloc((E, h), torch.float32, DEV)
    status = arena.alloc((3,), torch.int32, DEV)
    sd = None if scale is None else scale.to(DEV)
    rc = edges.dif_edge_attn_f32(qd[:, 4:].data_ptr(), qd.stride(0), kd[:, 4:].data_ptr(), kd.stride(0),
                                 None if sd is None else sd.data_ptr(), n_q, n_k, h, m, mode, eid.data_ptr(), E, out.data_ptr(),
                                 status.data_ptr(), _stream())
    _lib.check_edges(rc, "dif_edge_attn_f32")
    arena.check()
    return out.cpu(), status.cpu()


def _run_mass(edges, qw, kw, scale, n_q, n_k, h, m, mode, rowptr, src, arena=None):
    from difformer_amd import _lib
    arena = arena or GuardedArena()
    qd, kd = qw.to(DEV), kw.to(DEV)
    rp, sr = rowptr.to(DEV), src.to(DEV)
    mass = arena.alloc((n_q, h), torch.float32, DEV)
    sd = None if scale is None else scale.to(DEV)
    rc = edges.dif_edge_attn_mass_f32(qd[:, 4:].data_ptr(), qd.stride(0), kd[:, 4:].data_ptr(), kd.stride(0),
                                      None if sd is None else sd.data_ptr(), n_q, n_k, h, m, mode, rp.data_ptr(), sr.data_ptr(),
                                      sr.numel(), mass.data_ptr(), _stream())
    _lib.check_edges(rc, "dif_edge_attn_mass_f32")
    arena.check()
    return mass.cpu()


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
@pytest.mark.parametrize("h,m", WIDTHS)
@pytest.mark.parametrize("n_q,n_k,E", GRAPHS)
def test_parity_through_the_c_abi(edges, kernel, n_q, n_k, E, h, m):
    mode = MODES[kernel]
    c = _case(n_q, n_k, E, h, m, mode)
    out, status = _run_edges(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, c["ei"])
    mass = _run_mass(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, *_csr(c["ei"], n_q))
    e1, e2 = rel_err(out.numpy(), c["values"]), rel_err(mass.numpy(), c["mass"])
    print(f"edges {kernel} n_q={n_q} n_k={n_k} E={E} H={h} M={m}: values {e1:.2e}, mass {e2:.2e}")
    assert status.tolist() == [0, 0, 0]
    assert e1 <= edges_ref.TOL and e2 <= edges_ref.TOL
    if n_q >= 3:
        assert (mass[n_q // 2] == 0).all()                     # the target without in-edges


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
@pytest.mark.parametrize("h,m", [(1, 4), (2, 64), (1, 128), (1, 300)])
def test_hub_rows_of_300_and_4099_entries(edges, kernel, h, m):
    """Rows longer than one 64-entry chunk of the mass kernel: 4 full chunks + 44 entries, and 64 chunks + 3."""
    mode, (n_q, n_k, E) = MODES[kernel], (300, 1000, 4999)
    c = _case(n_q, n_k, E, h, m, mode, hubs=(4099, 300))
    rowptr, src = _csr(c["ei"], n_q)
    deg = np.diff(rowptr.numpy())
    assert deg.max() >= 4099 and np.sort(deg)[-2] >= 300
    mass = _run_mass(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, rowptr, src)
    again = _run_mass(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, rowptr, src)
    e2 = rel_err(mass.numpy(), c["mass"])
    hub = int(deg.argmax())
    e_hub = rel_err(mass[hub].numpy(), c["mass"][hub])
    print(f"hubs {kernel} H={h} M={m}: mass {e2:.2e}, the 4099-entry row {e_hub:.2e}")
    assert e2 <= edges_ref.TOL and e_hub <= edges_ref.TOL
    assert torch.equal(mass.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("h,m", WIDTHS)
def test_ones_give_exact_counts(edges, h, m):
    """q = k = 1, mode 0, no scale: every edge value is M and every mass M x degree, exactly -- a skipped or doubled entry
    cannot hide in a tolerance."""
    n_q, n_k, E = 300, 1000, 4999
    ei = edges_ref.random_graph(n_q, n_k, E, seed=m, hubs=(4099, 300))
    qw, kw = torch.ones(n_q, h * m + PAD), torch.ones(n_k, h * m + PAD)
    qw[:, :4] = qw[:, 4 + h * m:] = kw[:, :4] = kw[:, 4 + h * m:] = float("nan")          # what lies around the operands
    out, status = _run_edges(edges, qw, kw, None, n_q, n_k, h, m, 0, ei)
    rowptr, src = _csr(ei, n_q)
    mass = _run_mass(edges, qw, kw, None, n_q, n_k, h, m, 0, rowptr, src)
    assert status.tolist() == [0, 0, 0]
    assert torch.equal(out, torch.full((E, h), float(m)))
    want = torch.from_numpy(np.diff(rowptr.numpy()).astype(np.float32) * m)[:, None].expand(n_q, h)
    assert torch.equal(mass, want) and int(want.max()) >= 4099 * m and int(want.min()) == 0


def test_complete_bipartite_sigmoid_mass_is_one():
    """All 17 x 33 pairs as the edge list: the mass is the sum of a whole row of the map, 1 -- `den` end to end."""
    from difformer_amd import attention_on_edges
    c = _case(17, 33, 63, 2, 64, 1)
    col, row = np.meshgrid(np.arange(17), np.arange(33), indexing="ij")
    ei = torch.from_numpy(np.stack([row.ravel(), col.ravel()]).astype(np.int64)).to(DEV)
    assert ei.shape == (2, 561)
    values, mass = attention_on_edges(c["q"].to(DEV), c["k"].to(DEV), "sigmoid", ei, mass=True)
    dev = float((mass - 1).abs().max())
    e1 = rel_err(values.cpu().numpy(), edges_ref.edge_values(c["q"], c["k"], "sigmoid", ei.cpu().numpy()))
    print(f"complete bipartite sigmoid: |mass - 1| {dev:.2e}, values {e1:.2e}")
    assert mass.shape == (17, 2) and dev <= 1e-5 and e1 <= edges_ref.TOL


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
@pytest.mark.parametrize("h,m", [(2, 64), (1, 300)])
def test_a_shuffled_edge_list_gives_the_shuffled_output_bit_for_bit(edges, kernel, h, m):
    mode, (n_q, n_k, E) = MODES[kernel], (300, 1000, 4099)
    c = _case(n_q, n_k, E, h, m, mode)
    perm = np.random.default_rng(5).permutation(E)
    out, _ = _run_edges(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, c["ei"])
    shuffled, _ = _run_edges(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, np.ascontiguousarray(c["ei"][:, perm]))
    assert torch.equal(shuffled.view(torch.int32), out[torch.from_numpy(perm)].view(torch.int32))
    rowptr, src = _csr(c["ei"], n_q)
    one = _run_mass(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, rowptr, src)
    two = _run_mass(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, rowptr, src)
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
@pytest.mark.parametrize("h,m", [(2, 64), (1, 300)])
def test_ids_out_of_range_are_nan_and_reported_and_never_dereferenced(edges, kernel, h, m):
    """One source id equal to n_k and one target id of -1: only those edges are NaN, the status names both sides, the guard
    bands around the outputs hold.  The mass kernel turns a source id out of range into a NaN of its row alone."""
    from difformer_amd import attention_on_edges
    mode, (n_q, n_k, E) = MODES[kernel], (100, 100, 257)
    c = _case(n_q, n_k, E, h, m, mode)
    ei = c["ei"].copy()
    ei[0, 70], ei[1, 200] = n_k, -1
    out, status = _run_edges(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, ei)
    nan_rows = torch.isnan(out).any(dim=1).nonzero().flatten().tolist()
    assert nan_rows == [70, 200] and torch.isnan(out[[70, 200]]).all() and all(status.tolist())
    keep = np.delete(np.arange(E), [70, 200])
    assert rel_err(out[keep].numpy(), c["values"][keep]) <= edges_ref.TOL
    for bad_col, want in ((0, [1, 1, 0]), (1, [1, 0, 1])):
        one = c["ei"].copy()
        one[bad_col, 5] = 1 << 40
        assert _run_edges(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, one)[1].tolist() == want
    rowptr, src = _csr(c["ei"], n_q)
    hit = int(np.diff(rowptr.numpy()).argmax())
    src[rowptr[hit]], src[rowptr[hit + 1] - 1] = n_k, -1
    mass = _run_mass(edges, c["qw"], c["kw"], c["scale"], n_q, n_k, h, m, mode, rowptr, src)
    assert torch.isnan(mass).any(dim=1).nonzero().flatten().tolist() == [hit]
    others = np.delete(np.arange(n_q), hit)
    assert rel_err(mass[others].numpy(), c["mass"][others]) <= edges_ref.TOL
    with pytest.raises(IndexError, match=r"source \(key\) ids outside \[0, 100\) and target \(query\) ids outside \[0, 100\)"):
        attention_on_edges(c["q"].to(DEV), c["k"].to(DEV), kernel, torch.from_numpy(ei).to(DEV), mass=True)


# ---- the functional API and the model method ----------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,n,l,h,m,E", [("simple", 100, 1000, 2, 30, 700), ("sigmoid", 257, 300, 1, 64, 3000),
                                              ("sigmoid", 120, 90, 1, 300, 500)])
def test_attention_on_edges_against_the_reference_definition(kernel, n, l, h, m, E):
    from difformer_amd import attention_on_edges, ops
    c = _case(n, l, E, h, m, MODES[kernel])
    q, k, ei = c["q"], c["k"], torch.from_numpy(c["ei"])
    be = ops.get_backend()
    be.kernel_events = events = {}
    try:
        values, mass = attention_on_edges(q.to(DEV), k.to(DEV), kernel, ei.to(DEV), mass=True)
    finally:
        be.kernel_events = None
    assert {"dif_edge_attn_f32", "dif_edge_attn_mass_f32", "dif_csr_build"} <= set(events)
    assert ("dif_sigmoid_attn_fwd_f32" in events) == (kernel == "sigmoid")
    assert values.device.type == "cuda" and values.shape == (E, h) and mass.shape == (n, h) and not values.requires_grad
    e1 = rel_err(values.cpu().numpy(), edges_ref.edge_values(q, k, kernel, c["ei"]))
    e2 = rel_err(mass.cpu().numpy(), edges_ref.edge_mass(q, k, kernel, c["ei"]))
    print(f"attention_on_edges {kernel} N={n} L={l} H={h} M={m}: values {e1:.2e}, mass {e2:.2e}")
    assert e1 <= edges_ref.TOL and e2 <= edges_ref.TOL
    host_v, host_m = attention_on_edges(q, k, kernel, ei, mass=True)       # host operands are staged and come back on the host
    assert host_v.device.type == "cpu" and torch.equal(host_v, values.cpu()) and torch.equal(host_m, mass.cpu())
    half = attention_on_edges(q.to(DEV).bfloat16(), k.to(DEV).bfloat16(), kernel, ei.to(DEV))     # storage only
    assert half.dtype == torch.float32
    assert rel_err(half.cpu().numpy(), edges_ref.edge_values(q.bfloat16().float(), k.bfloat16().float(), kernel, c["ei"])) <= edges_ref.TOL


@pytest.mark.parametrize("placement", ["offset", "odd_stride", "permuted"])
@pytest.mark.parametrize("h,m", [(2, 64), (1, 300)])
def test_backend_methods_take_views_that_are_not_aligned_rows(placement, h, m):
    """HipBackend.edge_attention / edge_attention_mass on q / k views the launchers reject -- rows that start one element off
    the 16-byte boundary, a leading dimension that is no multiple of 4, a permuted [H, N, M] storage: copied by the backend,
    the result bit for bit that of dense operands."""
    from difformer_amd import ops
    n_q, n_k, E = 100, 100, 257
    c = _case(n_q, n_k, E, h, m, 1)
    be = ops.get_backend()
    q, k, scale, ei = c["q"].contiguous().to(DEV), c["k"].contiguous().to(DEV), c["scale"].to(DEV), torch.from_numpy(c["ei"]).to(DEV)
    rowptr, src = (t.to(DEV) for t in _csr(c["ei"], n_q))

    def place(t):
        rows, width = t.shape[0], h * m
        if placement == "permuted":
            return t.permute(1, 0, 2).contiguous().permute(1, 0, 2)
        wide = torch.full((rows, width + (5 if placement == "offset" else 3)), float("nan"), device=DEV)
        first = 1 if placement == "offset" else 0
        wide[:, first: first + width] = t.reshape(rows, width)
        return wide[:, first: first + width].view(rows, h, m)

    qv, kv = place(q), place(k)
    assert torch.equal(qv, q) and (not qv.is_contiguous() or (placement == "permuted" and h == 1))    # (one head: nothing to permute)
    want_v, want_s = be.edge_attention(q, k, scale, ei, 1)
    want_m = be.edge_attention_mass(q, k, scale, rowptr, src, 1)
    got_v, got_s = be.edge_attention(qv, kv, scale, ei, 1)
    got_m = be.edge_attention_mass(qv, kv, scale, rowptr, src, 1)
    assert got_s.tolist() == want_s.tolist() == [0, 0, 0]
    assert torch.equal(got_v.view(torch.int32), want_v.view(torch.int32)) and torch.equal(got_m.view(torch.int32), want_m.view(torch.int32))
    assert rel_err(got_v.cpu().numpy(), c["values"]) <= edges_ref.TOL and rel_err(got_m.cpu().numpy(), c["mass"]) <= edges_ref.TOL


@pytest.mark.parametrize("name", ["s_default", "s_h132_nograph", "a_default", "a_h2_weighted"])
def test_edge_attentions_is_get_attentions_at_the_edges_of_the_golden_models(name):
    from difformer_amd import DIFFormer
    c = load_golden("model")[name]
    cfg, sd = split_model_case(c)
    model = DIFFormer(int(cfg.pop("in_channels")), int(cfg.pop("hidden_channels")), int(cfg.pop("out_channels")), **cfg).eval()
    model.load_state_dict({key: torch.from_numpy(v) for key, v in sd.items()})
    x, ei = torch.from_numpy(c["x"]), torch.from_numpy(c["edge_index"]).long()
    n, E = x.shape[0], ei.shape[1]
    host_v, host_m = model.edge_attentions(x, ei, mass=True)       # model and operands on the host: staged through the twin
    assert host_v.device.type == "cpu" and "_staged" in model.__dict__
    model = model.to(DEV)
    values, mass = model.edge_attentions(x.to(DEV), ei.to(DEV), mass=True)
    only = model.edge_attentions(x.to(DEV), ei.to(DEV))
    assert values.shape == (len(model.convs), E, model.convs[0].num_heads) and mass.shape == (len(model.convs), n, values.shape[2])
    assert torch.equal(values.cpu(), host_v) and torch.equal(mass.cpu(), host_m) and torch.equal(only, values)
    with torch.no_grad():
        dense = model.get_attentions(x.to(DEV)).double().cpu().numpy()              # [layers, N, N, H]
    for layer in range(dense.shape[0]):
        want = dense[layer][ei[1].numpy(), ei[0].numpy()]
        e1 = rel_err(values[layer].cpu().numpy(), want)
        e2 = rel_err(mass[layer].cpu().numpy(), edges_ref.sum_per_target(want, ei.numpy(), n))
        print(f"golden model {name} layer {layer}: values {e1:.2e}, mass {e2:.2e}")
        assert e1 <= edges_ref.TOL and e2 <= edges_ref.TOL


def test_peak_memory_stays_below_one_dense_map():
    """N = 15,000, E = 75,000, hidden 64, 2 layers: operands and outputs are a few MB; one [N, N] float32 map is 900 MB."""
    from difformer_amd import DIFFormer, ops
    torch.manual_seed(5)
    n, E = 15000, 75000
    model = DIFFormer(16, 64, 4, num_layers=2, num_heads=1, kernel="sigmoid", use_graph=False).to(DEV).eval()
    x = torch.randn(n, 16, device=DEV)
    ei = torch.randint(0, n, (2, E), device=DEV)
    ops.csr_cache.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    values, mass = model.edge_attentions(x, ei, mass=True)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"peak memory over edge_attentions at N = {n}, E = {E}: {peak / 1e6:.1f} MB ({(peak - base) / 1e6:.1f} MB above the start)")
    assert values.shape == (2, E, 1) and mass.shape == (2, n, 1)
    assert bool(torch.isfinite(values).all()) and bool((values > 0).all()) and bool(torch.isfinite(mass).all())
    assert peak < n * n * 4, f"{peak / 1e6:.1f} MB"
