"""Single-copy mode of the narrow closed-form route (ops.simple_layer_closed_form on dense unweighted float32 graphs, one GPU,
inference): every layer's rows exist once in HBM, as the slice-major pre-scaled copy ys = deg^-1/2 x that the sliced product
reads; the layer kernels and the background Gram pass read their input from that copy times rscale = deg^1/2 and the
row-major copy is neither written nor read (csrc/simple_layer.hip: load_slices, input_gram_kernel<KQ, false>,
simple_layer_kernel<..., SC = true>; csrc/side_chain.hip: gram_bg_kernel<true>).

Shapes: 8,205 nodes (no multiple of 16 or 64; the sliced product dispatches from 8,192 nodes and 48 entries per row), 48..60
entries per row plus self-loops, 8 input features, hidden 64 (the split-bf16 kernels) and 32 (the general kernels).  The entry
points are also called directly at 1 / 63 / 65 / 127 / 129 / 4,097 rows -- around the 64 rows of a layer workgroup and the 128
of a HEAD workgroup -- between NaN bands (tests/guarded.py), as tests/test_gpu_guarded_inputs.py does for the two-copy path.
Tolerance: 1e-4 norm-wise against float64, the bar of the closed-form parity tests.  Single copy against two
copies: the recovered row ys * rscale is within 2 ulp (1.2e-7) of the stored one, every layer ends in a LayerNorm (rows of
O(1)) and is the next layer's input, so the difference grows by a small factor per layer and stays below 1e-5 of the logits'
scale -- the bound test_gpu_closed_form.py holds two fusions of the same arithmetic to (measured: 2.8e-6 / 3.0e-6 at 2 / 3
layers)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import rel_err
from fake_backend import OracleBackend
from guarded import GuardedArena, guarded_inputs, poisoned_allocations  # noqa: F401
from oracle import difformer_oracle as orc

TOL = 1e-4
N, F_IN, CLASSES = 8205, 8, 10
FAKE = OracleBackend()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _d(t):
    return t.detach().to(torch.float64).cpu().numpy()


def _dense_graph(seed, loops=True, orphan=None):
    """48..60 incoming entries per node (edge_index[1] is the destination, difformer.py:62-66) plus self-loops; `orphan`: a
    node that keeps no incoming entry at all."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(48, 61, (N,), generator=g)
    dst = torch.repeat_interleave(torch.arange(N), deg)
    src = torch.randint(0, N, (dst.numel(),), generator=g)
    if not loops:
        src = torch.where(src == dst, (src + 1) % N, src)
    ei = torch.stack([src, dst])
    if loops:
        ei = torch.cat([ei, torch.arange(N).repeat(2, 1)], dim=1)
    if orphan is not None:
        ei = ei[:, ei[1] != orphan]
    return ei


def _model(hidden, layers, dev, seed):
    from difformer_amd import DIFFormer
    torch.manual_seed(seed)
    model = DIFFormer(F_IN, hidden, CLASSES, num_layers=layers, num_heads=1, kernel="simple").to(dev).eval()
    cfg = dict(hidden_channels=hidden, num_layers=layers, num_heads=1, kernel="simple", alpha=0.5, use_bn=True, use_residual=True,
               use_weight=True, use_graph=True, graph_weight=-1, use_source=False)
    return model, cfg


def _oracle(model, cfg, x, ei):
    p = {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()}
    return orc.difformer_forward(p, x.double().numpy(), ei.numpy(), None, cfg)


def _forward(model, x, ei, single, monkeypatch, events=True):
    """One forward in the given mode -> (logits, layer kernels that read the slice-major copy, labels launched).  events: collect
    the launched labels (the forward then runs kernel by kernel: a forward with event collection is never captured)."""
    from difformer_amd import ops
    monkeypatch.setattr(ops, "SINGLE_COPY", single)
    be = ops.get_backend()
    be.kernel_events = {} if events else None
    try:
        with torch.no_grad():
            y = model(x, ei)
    finally:
        launched, be.kernel_events = set(be.kernel_events or ()), None
    return y, model.last_single_copy, launched


@pytest.fixture(scope="module")
def graph():
    return _dense_graph(11)


@pytest.fixture(scope="module")
def features():
    return torch.randn(N, F_IN, generator=torch.Generator().manual_seed(12))


# ================================================================== the model
@pytest.mark.gpu
@pytest.mark.parametrize("layers", [2, 3])
def test_single_copy_forward_matches_the_oracle_and_the_two_copy_path(layers, graph, features, dev, monkeypatch):
    model, cfg = _model(64, layers, dev, 20 + layers)
    ref = _oracle(model, cfg, features, graph)
    x, ei = features.to(dev), graph.to(dev)
    one, n_single, launched = _forward(model, x, ei, True, monkeypatch)
    two, n_two, _ = _forward(model, x, ei, False, monkeypatch)
    e1, e2, e12 = rel_err(one.cpu().numpy(), ref), rel_err(two.cpu().numpy(), ref), rel_err(one.cpu().numpy(), two.cpu().numpy())
    print(f"layers={layers}: single copy vs float64 {e1:.3e}, two copies vs float64 {e2:.3e}, single vs two {e12:.3e}")
    assert n_single == layers and n_two == 0                   # every layer kernel read the copy / none did
    assert {"dif_input_gram_f32", "dif_sliced_spmm_f32", "dif_gram_bg_f32", "dif_simple_layer_f32"} <= launched
    assert one.shape == (N, CLASSES) and bool(torch.isfinite(one).all())
    assert e1 < TOL and e2 < TOL
    assert e12 < 1e-5


@pytest.mark.gpu
def test_graph_with_a_node_without_incoming_entries_keeps_two_copies(features, dev, monkeypatch):
    """deg = 0 gives dinv = 0: the row cannot be recovered from the copy, so the whole forward stays on the two-copy path."""
    from difformer_amd import ops
    ei_cpu = _dense_graph(11, loops=False, orphan=4711)
    assert int((ei_cpu[1] == 4711).sum()) == 0 and int((ei_cpu[0] == ei_cpu[1]).sum()) == 0
    model, cfg = _model(64, 2, dev, 31)
    ref = _oracle(model, cfg, features, ei_cpu)
    x, ei = features.to(dev), ei_cpu.to(dev)
    y, n_single, launched = _forward(model, x, ei, True, monkeypatch)
    csr = ops.csr_cache.get(ei, None, N, 64 * 4)
    assert csr.sliced(0, N, 64) is not None and csr.row_scale() is None
    assert n_single == 0 and {"dif_input_gram_f32", "dif_sliced_spmm_f32", "dif_simple_layer_f32"} <= launched
    err = rel_err(y.cpu().numpy(), ref)
    print(f"no self-loops, one node without incoming entries: two-copy path vs float64 {err:.3e}")
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("hidden", [32, 64])
def test_awkward_inputs_zero_rows_and_strided_features(hidden, graph, dev, monkeypatch):
    """Hidden rows that are exactly zero after the ReLU (zero input rows, no Linear bias, negative LayerNorm bias: the
    LayerNorm of a zero row is its bias), features handed over as a column block of a wider tensor (ldx 12 > 8), and the
    general kernels at hidden 32."""
    model, cfg = _model(hidden, 2, dev, 40 + hidden)
    g = torch.Generator().manual_seed(41)
    with torch.no_grad():
        model.fcs[0].bias.zero_()
        model.bns[0].bias.copy_(-(torch.rand(hidden, generator=g) * 0.4 + 0.1))
    wide = torch.randn(N, 12, generator=g)
    zero_rows = torch.randperm(N, generator=g)[:300]
    wide[zero_rows] = 0.0
    x_cpu = wide[:, 2:2 + F_IN]
    h0 = np.maximum(orc.layer_norm(_d(x_cpu) @ _d(model.fcs[0].weight).T, _d(model.bns[0].weight), _d(model.bns[0].bias)), 0)
    assert not h0[zero_rows.numpy()].any() and h0.any(axis=1).sum() > N - 400
    ref = _oracle(model, cfg, x_cpu.contiguous(), graph)
    x = wide.to(dev)[:, 2:2 + F_IN]
    assert not x.is_contiguous() and x.stride(0) == 12
    y, n_single, _ = _forward(model, x, graph.to(dev), True, monkeypatch)
    err = rel_err(y.cpu().numpy(), ref)
    print(f"hidden={hidden}: zero rows + strided features, single copy vs float64 {err:.3e}")
    assert n_single == 2 and bool(torch.isfinite(y).all()) and err < TOL


@pytest.mark.gpu
def test_two_single_copy_forwards_are_bit_identical(graph, features, dev, monkeypatch):
    model, _ = _model(64, 3, dev, 50)
    model.auto_graph = False                                   # both calls launch kernel by kernel
    x, ei = features.to(dev), graph.to(dev)
    a, n_a, _ = _forward(model, x, ei, True, monkeypatch)
    b, n_b, _ = _forward(model, x, ei, True, monkeypatch)
    assert n_a == n_b == 3 and torch.equal(a, b)


@pytest.mark.gpu
def test_replayed_graph_returns_the_eager_result(graph, features, dev, monkeypatch):
    """The third identical call captures the forward into a hipGraph (DIFFormer._forward_graphed); the replay reads the same
    slice-major buffers."""
    model, _ = _model(64, 2, dev, 51)
    x, ei = features.to(dev), graph.to(dev)
    outs = [_forward(model, x, ei, True, monkeypatch, events=False)[0] for _ in range(4)]
    assert model._ag_state is not None and model._ag_state[2] is not None          # captured, and replayed by the last call
    assert model.last_single_copy == 2 and all(torch.equal(outs[0], o) for o in outs[1:])


# ================================================================== the entry points between NaN bands
def _slice_major(rows64, dinv64, npad, pad=0.0):
    """[n, C] float64 rows -> the float32 slice-major copy [C/4, npad, 4] of dinv * rows; rows n .. npad-1 hold `pad`."""
    n, C = rows64.shape
    ys = np.full((C // 4, npad, 4), pad, dtype=np.float32)
    ys[:, :n, :] = (rows64 * dinv64[:, None]).astype(np.float32).reshape(n, C // 4, 4).transpose(1, 0, 2)
    return ys


def _rowptr(n, g):
    deg = torch.randint(1, 70, (n,), generator=g)
    rowptr = torch.zeros(n + 1, dtype=torch.int32)
    rowptr[1:] = torch.cumsum(deg, 0).to(torch.int32)
    return rowptr, deg.double().numpy()


def _coef_params(g, c, d):
    W = [torch.randn(d, c, generator=g) * c ** -0.5 for _ in range(3)]
    b = [torch.randn(d, generator=g) * 0.3 for _ in range(3)]
    return [W[0], b[0], W[1], b[1], W[2], b[2]]


def _record(x64):
    return np.concatenate([(x64.T @ x64).ravel(), x64.sum(0)])


class _ArgSpy:
    """Forwards to the loaded library and keeps the arguments of every call by entry point."""

    def __init__(self, lib):
        self.__dict__["lib"], self.__dict__["calls"] = lib, {}

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if not name.startswith("dif_"):
            return fn

        def call(*args):
            self.calls.setdefault(name, []).append(args)
            return fn(*args)
        return call


@pytest.fixture
def spied_backend(monkeypatch):
    from difformer_amd import _lib, ops
    be = ops.get_backend()
    spy = _ArgSpy(be.lib)
    monkeypatch.setattr(be, "lib", spy)
    monkeypatch.setattr(_lib, "_lib", spy)
    return be, spy


def _hold(results):
    failures = []
    for label, got, ref, tol in results:
        got, ref = _d(got), np.asarray(ref, dtype=np.float64)
        assert got.shape == ref.shape, (label, got.shape, ref.shape)
        err, finite = rel_err(got, ref), bool(np.isfinite(got).all())
        print(f"{label}: err {err:.3e} (tol {tol:.0e}) finite={finite}")
        if not (err < tol and finite):
            failures.append((label, err, finite))
    assert not failures, failures


PLACEMENTS = pytest.mark.parametrize("placement", ["aligned512", "minimum"])


@pytest.mark.gpu
@PLACEMENTS
def test_input_pass_without_row_major_output_between_nan_bands(placement, dev, poisoned_allocations, spied_backend):
    """dif_input_gram_f32 with out = NULL (input_gram_kernel<1..4, false>): record and slice-major copy against float64; the
    rows of the copy past n_rows are zero (the product's last tile reads them)."""
    be, spy = spied_backend
    inputs = GuardedArena()
    P = lambda **kw: guarded_inputs(inputs, dev, min_align=placement == "minimum", **kw)
    res = []
    for n, c, d in [(1, 24, 64), (63, 7, 32), (65, 64, 64), (4097, 40, 48)]:
        g = torch.Generator().manual_seed(n + c)
        x, W, b = torch.randn(n, c, generator=g), torch.randn(d, c, generator=g) * c ** -0.5, torch.randn(d, generator=g)
        lw, lb = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
        rowptr, deg = _rowptr(n, g)
        plan = be.sliced_plan(n, n, d)
        npad = int(plan[6]) * int(plan[7])
        xd, Wd, bd, lwd, lbd, rpd = P(x=x, weight=W, bias=b, ln_weight=lw, ln_bias=lb, rowptr=rowptr)
        h, rec, ys = be.input_gram(xd, Wd, bd, lwd, lbd, 1e-5, True, rpd, plan, rows=False)
        assert h is None
        h64 = np.maximum(orc.layer_norm(_d(x) @ _d(W).T + _d(b), _d(lw), _d(lb)), 0.0)
        ref = _record(h64)
        res += [(f"record n={n} c={c} d={d}", rec[: ref.size], ref, TOL),
                (f"copy n={n} c={c} d={d}", ys, _slice_major(h64, deg ** -0.5, npad), TOL)]
        assert not bool(ys[:, n:, :].any())
    assert len(inputs.blocks) > 0 and len(poisoned_allocations.blocks) > 0
    inputs.check()
    calls = spy.calls["dif_input_gram_f32"]
    assert len(calls) == 4 and all(a[11] is None for a in calls)          # `out`: no address to write through
    _hold(res)


@pytest.mark.gpu
@PLACEMENTS
@pytest.mark.parametrize("head", [False, True], ids=["rows", "head"])
def test_layer_kernel_on_the_slice_major_copy_between_nan_bands(head, placement, dev, poisoned_allocations, spied_backend):
    """dif_simple_layer_f32 / dif_simple_layer_head_f32 with rscale (simple_layer_kernel<..., SC = true>: split-bf16 at 64 x 64,
    the general kernel below; with and without the graph term): the input comes from the copy -- whose rows past n_rows are NaN
    here and must not be read -- and, between two layers, nothing is written row-major (out = NULL)."""
    be, spy = spied_backend
    inputs = GuardedArena()
    P = lambda **kw: guarded_inputs(inputs, dev, min_align=placement == "minimum", **kw)
    res = []
    shapes = [(1, 64), (127, 64), (129, 32), (4097, 48)] if head else [(1, 64), (63, 64), (65, 32), (4097, 48)]
    for n, c in shapes:
        for graph_term in (True, False):
            g = torch.Generator().manual_seed(n + c + graph_term)
            x = torch.randn(n, c, generator=g) + 0.2
            wb = _coef_params(g, c, c)
            rec = torch.from_numpy(np.concatenate([_record(_d(x)), [0.0, 0.0]]).astype(np.float32))
            coef = FAKE.simple_coeffs(rec, n, c, c, *wb, 0.7)
            ax = torch.randn(n, c, generator=g) if graph_term else None
            rs = torch.rand(n, generator=g) + 0.5 if graph_term else None
            Wv, bv = (wb[4], wb[5]) if graph_term else (None, None)
            lw, lb = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g)
            rowptr, deg = _rowptr(n, g)
            plan = be.sliced_plan(n, n, c)
            npad = int(plan[6]) * int(plan[7])
            xs = torch.from_numpy(_slice_major(_d(x), deg ** -0.5, npad, pad=np.nan))
            rscale = torch.from_numpy(np.sqrt(deg).astype(np.float32))
            Wo, bo = torch.randn(11, c, generator=g) * c ** -0.5, torch.randn(11, generator=g)
            xsd, rsc, coefd, axd, Wvd, bvd, rsd, lwd, lbd, rpd, Wod, bod = P(xs=xs, rscale=rscale, coef=coef, ax=ax, Wv=Wv, bv=bv,
                                                                            row_sums=rs, ln_weight=lw, ln_bias=lb, rowptr=rowptr,
                                                                            Wo=Wo, bo=bo)
            args = (coefd, c, axd, Wvd, bvd, rsd, 0.9, None, True, 0.5, lwd, lbd, 1e-5, True)
            want = FAKE.simple_layer(x, coef, c, ax, Wv, bv, rs, 0.9, None, True, 0.5, lw, lb, 1e-5, True,
                                     head=(Wo, bo) if head else None)
            tag = f"n={n} c={c} graph_term={graph_term}"
            if head:
                res.append((f"logits {tag}", be.simple_layer(xsd, *args, head=(Wod, bod), rscale=rsc), _d(want), TOL))
            else:
                out, ys2 = be.simple_layer(xsd, *args, next_rowptr=rpd, next_plan=plan, rscale=rsc, rows=False)
                assert out is None
                res.append((f"next copy {tag}", ys2, _slice_major(_d(want), deg ** -0.5, npad), TOL))
                assert not bool(ys2[:, n:, :].any())
                rows, _ = be.simple_layer(xsd, *args, next_rowptr=rpd, next_plan=plan, rscale=rsc)     # last layer without a head
                res.append((f"rows {tag}", rows, _d(want), TOL))
    assert len(inputs.blocks) > 0 and len(poisoned_allocations.blocks) > 0
    inputs.check()
    if head:
        calls = spy.calls["dif_simple_layer_head_f32"]
        assert len(calls) == 8 and all(a[20] is None and a[27] is not None for a in calls)       # out, rscale
    else:
        calls = spy.calls["dif_simple_layer_f32"]
        assert len(calls) == 16 and all(a[25] is not None for a in calls)                         # rscale
        assert sum(a[20] is None for a in calls) == 8                                             # out of the rows=False calls
    _hold(res)


@pytest.mark.gpu
@PLACEMENTS
def test_background_gram_pass_on_the_slice_major_copy_between_nan_bands(placement, dev, poisoned_allocations, spied_backend):
    """dif_gram_bg_f32 with rscale (gram_bg_kernel<true>) -> coefficients against the float64 restatement; the copy's rows past
    n_rows are NaN and must not be read."""
    from difformer_amd import ops
    be, spy = spied_backend
    inputs = GuardedArena()
    P = lambda **kw: guarded_inputs(inputs, dev, min_align=placement == "minimum", **kw)
    res = []
    for n, c, d in [(1, 64, 64), (63, 32, 32), (65, 48, 64), (4097, 64, 32)]:
        g = torch.Generator().manual_seed(n + c)
        x = torch.randn(n, c, generator=g) + 0.2
        wb = _coef_params(g, c, d)
        rec = torch.from_numpy(np.concatenate([_record(_d(x)), [0.0, 0.0]]).astype(np.float32))
        want = _d(FAKE.simple_coeffs(rec, n, c, d, *wb, 0.7))
        _, deg = _rowptr(n, g)
        plan = be.sliced_plan(n, n, c)
        xs = torch.from_numpy(_slice_major(_d(x), deg ** -0.5, int(plan[6]) * int(plan[7]), pad=np.nan))
        xsd, rsc, *wbd = P(xs=xs, rscale=torch.from_numpy(np.sqrt(deg).astype(np.float32)), Wq=wb[0], bq=wb[1], Wk=wb[2], bk=wb[3],
                           Wv=wb[4], bv=wb[5])
        got = be.coeffs_bg(xsd, None, n, ops.NarrowFactors(*wbd), c, d, 0.7, rscale=rsc)
        parts = lambda co: (("MnT", co[: d * c]), ("cn", co[d * c: d * c + d]), ("u", co[d * c + d: d * c + d + c]),
                            ("cd", co[d * c + d + c: d * c + d + c + 1]))
        for (nm, a), (_, b) in zip(parts(got), parts(want)):
            res.append((f"{nm} n={n} c={c} d={d}", a, b, TOL))
    assert len(inputs.blocks) > 0 and len(poisoned_allocations.blocks) > 0
    inputs.check()
    assert all(a[9] is not None for a in spy.calls["dif_gram_bg_f32"])
    _hold(res)


# ================================================================== the bindings (no GPU)
def test_bindings_of_the_single_copy_arguments_match_the_header():
    """The four entry points the mode goes through, transcribed by hand from include/difformer_hip.h: rscale sits in front of
    the stream of dif_simple_layer_f32, dif_simple_layer_head_f32 and dif_gram_bg_f32; dif_input_gram_f32 is unchanged (its
    `out` may be NULL)."""
    from ctypes import c_float as f32, c_int, c_int64 as i64, c_size_t, c_void_p as vp
    from difformer_amd import _lib
    sig = _lib.SIGNATURES
    layer = [vp, i64, i64, c_int, c_int, vp, vp, i64, vp, vp, vp, f32, vp, i64, c_int, f32, vp, vp, f32, c_int, vp, i64]
    assert sig["dif_simple_layer_f32"] == (c_int, layer + [vp, vp, vp, vp, vp])
    assert sig["dif_simple_layer_head_f32"] == (c_int, layer + [vp, vp, c_int, vp, i64, vp, vp])
    assert sig["dif_simple_layer_head_bf16"] == (c_int, layer + [vp, vp, c_int, vp, i64, vp])
    assert sig["dif_gram_bg_f32"] == (c_int, [vp, i64, i64, c_int, i64, vp, vp, vp, c_size_t, vp, vp])
    assert sig["dif_input_gram_f32"] == (c_int, [vp, i64, i64, c_int, vp, vp, c_int, vp, vp, f32, c_int, vp, i64, vp, vp, vp, vp, vp,
                                                c_size_t, vp])


def test_single_copy_argument_checks_reject_before_touching_the_device():
    """Host-side checks only: the addresses are never dereferenced."""
    from difformer_amd import _lib
    lib = _lib.load()
    p = 4096                                                       # any 16-byte aligned non-null address
    plan = (ctypes.c_int32 * 8)()
    assert lib.dif_sliced_plan(5000, 5000, 64, plan) == 0
    # neither a row-major output nor a slice-major copy: nothing to write
    rc = lib.dif_input_gram_f32(p, 8, 5000, 8, p, p, 64, p, p, 1e-5, 1, None, 0, None, None, None, p, p, 1 << 30, None)
    assert rc == -1 and b"null pointer" in lib.dif_last_error()
    # out = NULL without rscale, and without a next-layer copy
    layer = lambda x, ldx, out, next_ys, rscale: lib.dif_simple_layer_f32(x, ldx, 5000, 64, 64, p, None, 0, None, None, None, 1.0,
                                                                         None, 0, 1, 0.5, p, p, 1e-5, 1, out, 64, p, plan, next_ys,
                                                                         rscale, None)
    assert layer(p, 64, None, p, None) == -1 and b"null pointer" in lib.dif_last_error()
    assert layer(p, 5008, None, None, p) == -1 and b"null pointer" in lib.dif_last_error()
    # rscale: ldx counts the rows of a slice
    assert layer(p, 64, None, p, p) == -1 and b"rows per slice" in lib.dif_last_error()
    rc = lib.dif_gram_bg_f32(None, 0, 5000, 64, 5000, p, p, p, 1 << 30, p, None)
    assert rc == -1 and b"rscale" in lib.dif_last_error()
    rc = lib.dif_gram_bg_f32(p, 64, 5000, 64, 5000, p, p, p, 1 << 30, p, None)
    assert rc == -1 and b"rows per slice" in lib.dif_last_error()


def test_row_scale_is_kept_with_the_csr_and_refuses_empty_rows():
    """GraphCSR.row_scale on CPU tensors: deg^1/2 once per graph; None as soon as one node has no incoming entry, for weighted
    graphs and for an adjoint CSR."""
    from difformer_amd import ops
    rowptr = torch.tensor([0, 2, 3, 7], dtype=torch.int32)
    mk = lambda rp: ops.GraphCSR(rp, None, 1, torch.zeros(int(rp[-1]), dtype=torch.int32), torch.ones(int(rp[-1])), rp.numel() - 1,
                                 int(rp[-1]))
    csr = mk(rowptr)
    rs = csr.row_scale()
    assert rs.dtype == torch.float32 and torch.equal(rs, torch.tensor([2.0, 1.0, 4.0]).sqrt()) and csr.row_scale() is rs
    assert mk(torch.tensor([0, 2, 2, 7], dtype=torch.int32)).row_scale() is None
    weighted = mk(rowptr)
    weighted.weighted = True
    assert weighted.row_scale() is None
    adjoint = mk(rowptr)
    adjoint.transposed = True
    assert adjoint.row_scale() is None
