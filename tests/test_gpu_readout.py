"""Graph read-out on the MI355X (csrc/graph_readout.hip behind include/difformer_readout.h) against the long-double oracle of
tests/readout_ref.py, through the C ABI and through global_add_pool / global_mean_pool / global_max_pool / GraphGNN.

Tolerances follow from the arithmetic (float64 sums in a fixed order, one rounding to the storage type); none is measured:
    add / mean forward      |out - ref| <= 1/2 ulp_storage(ref) + length * 2^-53 * sum |x|       (for mean, over length)
    max forward             bitwise
    add backward            bitwise (the row of grad_out)
    mean / max backward     |g - ref| <= 1/2 ulp_storage(ref) + 2^-53 |ref|                      (so +0 exactly where ref is 0)
Measured worst cases, as multiples of the bound (test_zz_report_the_worst_cases prints them; profiles/r16_readout.md):
    float32    add 1.000, mean 1.000 forward; mean 0.999, max 0.667 backward
    bfloat16   add 1.000, mean 1.000 forward; mean 0.996, max 0.667 backward
(1.000, printed to three places and not above 1, is a result half an ulp from the reference: the one rounding, which the bound
allows in full -- sums of bfloat16-exact values often land on a tie; 0.667 is a gradient split among three tied rows.)

Every call through the C ABI here runs on row-offset views with odd leading dimensions (x: H + 3, out / pooled: H + 1,
grad_out: H + 2, grad_x: H + 5), one element past a 512-byte boundary, the operands between NaN rows and NaN row tails, the
outputs pre-filled with 0xFF between checked guard bands (tests/guarded.py); after the call every element of out and of
grad_x[0:n_rows] has been written and no byte around them has.

Which case reaches which mechanism (tests/readout_ref.py builds the inputs, tests/test_readout_host.py shows them well-posed):
  columns in flight   H in {1, 63, 64, 65, 255, 256, 257, 300, 1024}: 256 .. 1 row phases; H > 256 loops with a ragged last block
  graphs              B in {1, 3, 257}: one workgroup, three, more than a wave of them; lengths 0 .. 1,025 around the phase counts
  empty graphs        first, last, in the middle, adjacent
  ties                2 and 3 equal maxima inside one row phase and across two
"""
import copy
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import grad_err, rel_err
from guarded import GuardedArena, guarded_inputs, install
import readout_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {}                 # (mode, pass, dtype) -> worst error / bound, printed by the last test
POOLS = {"add": "global_add_pool", "mean": "global_mean_pool", "max": "global_max_pool"}


@pytest.fixture(scope="module", autouse=True)
def leave_the_allocator_as_found():
    """torch keeps one BLAS workspace per stream that ever ran one of its GEMMs, for the life of the process: the training
    steps below run them on the default stream and on the capture's side stream.  Modules that run after this one count
    allocated bytes, so the workspaces are handed back when this module is done (as tests/test_gpu_adam.py does)."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    getattr(torch._C, "_cuda_clearCublasWorkspaces", lambda: None)()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def lib():
    from difformer_amd import _lib
    return _lib.load_readout()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _storage(bf16):
    return (torch.bfloat16, 2, torch.int16) if bf16 else (torch.float32, 4, torch.int32)


def _bits(t, bf16):
    return t.detach().cpu().contiguous().view(_storage(bf16)[2]).numpy().copy()


def _between_nan_rows(t):
    nan = torch.full((1, t.shape[1]), float("nan"), dtype=t.dtype)
    return torch.cat([nan, t, nan])


def _payload_bits(t, ld, bf16):
    """All rows of the block `t` was cut from, tails included, as integers: 0xFF.. reads -1."""
    return t.as_strided((t.shape[0], ld), (ld, 1)).cpu().view(_storage(bf16)[2]).numpy()


def _run(lib, case, mode, bf16=False, x=None):
    """Forward and backward of a case through the C ABI -> dict(out, gx as float64 ndarrays; out_bits, gx_bits)."""
    from difformer_amd import _lib
    dtype, item, _ = _storage(bf16)
    sfx = "bf16" if bf16 else "f32"
    H, ptr = case["H"], case["ptr"]
    B, N = len(ptr) - 1, int(ptr[-1])
    xs = torch.from_numpy(case["xb" if bf16 else "x32"] if x is None else x).to(dtype)
    if bf16:                                       # torch's vectorised conversion writes a NaN as 0xFFFF, the fill pattern
        xs.view(torch.int16)[torch.isnan(xs)] = 0x7FC0
    gs = torch.from_numpy(case["gb" if bf16 else "g32"]).to(dtype)
    arena = GuardedArena()
    xd, gd = guarded_inputs(arena, DEV, item, x=(_between_nan_rows(xs), H + 3), g=(_between_nan_rows(gs), H + 2))
    pd, = guarded_inputs(arena, DEV, 4, graph_ptr=torch.from_numpy(ptr))
    out = arena.alloc((B + 2, H), dtype, DEV, ld=H + 1, offset_bytes=item)
    gx = arena.alloc((N + 2, H), dtype, DEV, ld=H + 5, offset_bytes=item)
    code = _lib.READOUT_CONSTANTS["DIF_READOUT_" + mode.upper()]
    rc = getattr(lib, "dif_readout_fwd_" + sfx)(xd[1:].data_ptr(), H + 3, pd.data_ptr(), B, N, H, code, out[1:].data_ptr(), H + 1, _stream())
    _lib.check_readout(rc, "dif_readout_fwd_" + sfx)
    fwd_operands = (xd[1:].data_ptr(), H + 3, out[1:].data_ptr(), H + 1) if mode == "max" else (None, 0, None, 0)
    rc = getattr(lib, "dif_readout_bwd_" + sfx)(*fwd_operands, gd[1:].data_ptr(), H + 2, pd.data_ptr(), B, N, H, code, gx[1:].data_ptr(),
                                                H + 5, _stream())
    _lib.check_readout(rc, "dif_readout_bwd_" + sfx)
    arena.check()
    for t, ld, rows in ((out, H + 1, B), (gx, H + 5, N)):
        full = _payload_bits(t, ld, bf16)
        assert (full[0] == -1).all() and (full[rows + 1] == -1).all() and (full[:, H:] == -1).all(), "written outside the rows"
        assert not (full[1:rows + 1, :H] == -1).any(), "an element was not written"
    return dict(out=out[1:B + 1].double().cpu().numpy(), gx=gx[1:N + 1].double().cpu().numpy(), out_bits=_bits(out[1:B + 1], bf16),
                gx_bits=_bits(gx[1:N + 1], bf16))


def _worst(key, err, bound):
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0, 0.0, np.asarray(err / bound, dtype=np.float64))
    w = float(ratio.max()) if ratio.size else 0.0
    WORST[key] = max(WORST.get(key, 0.0), w)
    return w


def _hold(got, name, mode, bf16):
    """The bounds of the module docstring for one case, mode and storage type."""
    case = rr.cases()[name]
    ref_out, ref_gx = rr.evaluate(name, bf16)[mode]
    dtype = _storage(bf16)[0]
    tag = "bf16" if bf16 else "f32"
    if mode == "max":
        want = _bits(torch.from_numpy(ref_out.astype(np.float32)).to(dtype), bf16)
        assert np.array_equal(got["out_bits"], want), (name, mode, tag)
    else:
        err = np.abs(got["out"].astype(np.longdouble) - ref_out)
        assert _worst((mode, "forward", tag), err, rr.forward_bound(ref_out, case, mode, bf16)) <= 1, (name, mode, tag)
    if mode == "add":
        g_bits = _bits(torch.from_numpy(case["gb" if bf16 else "g32"]).to(dtype), bf16)
        want = np.repeat(g_bits, case["lengths"], axis=0)
        assert np.array_equal(got["gx_bits"], want), (name, mode, tag)
    else:
        err = np.abs(got["gx"].astype(np.longdouble) - ref_gx)
        assert _worst((mode, "backward", tag), err, rr.backward_bound(ref_gx, bf16)) <= 1, (name, mode, tag)
        assert not got["gx_bits"][np.asarray(ref_gx == 0)].any()                     # +0, not -0
    empty = np.flatnonzero(np.asarray(case["lengths"]) == 0)
    assert not got["out_bits"][empty].any()                                          # +0 for a graph without rows


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(rr.cases()))
def test_every_case_mode_and_storage_type_holds_the_bounds(lib, name):
    for mode in rr.MODES:
        for bf16 in (False, True):
            _hold(_run(lib, rr.cases()[name], mode, bf16), name, mode, bf16)


def test_more_than_1024_columns_are_rejected_and_nothing_is_touched(lib):
    from difformer_amd import _lib
    arena = GuardedArena()
    H = 1025
    x = arena.alloc((4, H), torch.float32, DEV)
    out = arena.alloc((2, H), torch.float32, DEV)
    gx = arena.alloc((4, H), torch.float32, DEV)
    pd, = guarded_inputs(arena, DEV, 4, graph_ptr=torch.tensor([0, 1, 4], dtype=torch.int32))
    for sfx in ("f32", "bf16"):
        for mode in range(3):
            rc = getattr(lib, "dif_readout_fwd_" + sfx)(x.data_ptr(), H, pd.data_ptr(), 2, 4, H, mode, out.data_ptr(), H, _stream())
            assert rc == _lib.ERROR_CODES["DIF_E_SHAPE"] and b"1 <= H <= 1024" in lib.dif_readout_last_error()
            rc = getattr(lib, "dif_readout_bwd_" + sfx)(x.data_ptr(), H, out.data_ptr(), H, out.data_ptr(), H, pd.data_ptr(), 2, 4, H, mode,
                                                        gx.data_ptr(), H, _stream())
            assert rc == _lib.ERROR_CODES["DIF_E_SHAPE"]
    with pytest.raises(_lib.DifformerHipError, match="1 <= H <= 1024"):
        _lib.check_readout(rc, "dif_readout_bwd_bf16")
    arena.check()
    for t in (out, gx):
        assert (t.cpu().view(torch.int32) == -1).all()


def test_a_nan_stays_in_its_column_and_its_graph(lib):
    """triple/H65: graphs of 4, 257 and 1 rows; a NaN at row 100 of the second graph, column 33."""
    name = "triple/H65"
    case = rr.cases()[name]
    assert case["lengths"] == [4, 257, 1]
    row, col = 4 + 100, 33
    for bf16 in (False, True):
        x = case["xb" if bf16 else "x32"].copy()
        x[row, col] = np.nan
        for mode in rr.MODES:
            clean, got = _run(lib, case, mode, bf16), _run(lib, case, mode, bf16, x=x)
            assert np.isnan(got["out"][1, col])
            same = np.ones_like(got["out_bits"], dtype=bool)
            same[1, col] = False
            assert np.array_equal(got["out_bits"][same], clean["out_bits"][same])
            if mode == "max":                                                    # a NaN column compares equal nowhere: no gradient
                assert not got["gx_bits"][4:261, col].any()
                got["gx_bits"][4:261, col] = clean["gx_bits"][4:261, col]
            assert np.array_equal(got["gx_bits"], clean["gx_bits"])


def test_the_same_call_twice_is_bitwise_equal(lib):
    for name in ("many/H64", "long/H65"):
        for mode in rr.MODES:
            for bf16 in (False, True):
                a, b = _run(lib, rr.cases()[name], mode, bf16), _run(lib, rr.cases()[name], mode, bf16)
                assert np.array_equal(a["out_bits"], b["out_bits"]) and np.array_equal(a["gx_bits"], b["gx_bits"])


# ---- the public functions ----------------------------------------------------------------------------------------------------------------
def _public(case, mode, bf16, form, view):
    """global_*_pool on device tensors -> (dict as _run's, events)."""
    import difformer_amd
    from difformer_amd import ops
    dtype = _storage(bf16)[0]
    H, lengths = case["H"], case["lengths"]
    x = torch.from_numpy(case["xb" if bf16 else "x32"]).to(dtype)
    g = torch.from_numpy(case["gb" if bf16 else "g32"]).to(dtype).to(DEV)
    if view:                                                                     # a column slice: rows H + 7 apart, not copied
        wide = torch.full((x.shape[0], H + 7), float("nan"), dtype=dtype)
        wide[:, 3:3 + H] = x
        leaf = wide.to(DEV).requires_grad_()
        xv = leaf[:, 3:3 + H]
    else:
        leaf = xv = x.to(DEV).requires_grad_()
    pool = getattr(difformer_amd, POOLS[mode])
    be = ops.get_backend()
    be.kernel_events = events = {}
    try:
        if form == "batch":
            batch = torch.repeat_interleave(torch.arange(len(lengths)), torch.tensor(lengths)).to(DEV)
            out = pool(xv, batch, len(lengths))
            again = pool(xv.detach(), batch, len(lengths))                       # the table of this `batch` is remembered
            assert torch.equal(out.detach().view(_storage(bf16)[2]), again.view(_storage(bf16)[2]))
            assert len([k for k in difformer_amd.readout.batch_cache.entries if k[0][0] == id(batch)]) == 1
        else:
            out = pool(xv, n_nodes=torch.tensor(lengths))
        out.backward(g)
    finally:
        be.kernel_events = None
    gx = leaf.grad[:, 3:3 + H] if view else leaf.grad
    assert out.dtype == dtype and gx.dtype == dtype and out.shape == (len(lengths), H)
    return dict(out=out.detach().double().cpu().numpy(), gx=gx.double().cpu().numpy(), out_bits=_bits(out, bf16), gx_bits=_bits(gx, bf16)), events


@pytest.mark.parametrize("name", ["triple/H1", "triple/H65", "triple/H300", "single/H256", "many/H64", "ties/H64", "ties/H1"])
def test_public_functions_hold_the_bounds_between_guard_bands(name, monkeypatch):
    """Both call forms, a column-slice view and bfloat16; the outputs the backend allocates come poisoned and guarded."""
    arena = install(monkeypatch)
    case = rr.cases()[name]
    for mode in rr.MODES:
        for bf16, form, view in ((False, "n_nodes", False), (False, "batch", True), (True, "batch", False)):
            got, events = _public(case, mode, bf16, form, view)
            sfx = "bf16" if bf16 else "f32"
            assert {"dif_readout_fwd_" + sfx, "dif_readout_bwd_" + sfx} <= set(events)
            _hold(got, name, mode, bf16)
    arena.check()


def test_an_unsorted_batch_and_float64_take_the_tensor_expression():
    import difformer_amd
    from difformer_amd import ops
    case = rr.cases()["triple/H65"]
    perm = torch.from_numpy(np.random.default_rng(3).permutation(case["x32"].shape[0]))
    batch = torch.repeat_interleave(torch.arange(3), torch.tensor(case["lengths"]))[perm].to(DEV)
    be = ops.get_backend()
    for mode in rr.MODES:
        ref = rr.evaluate("triple/H65")[mode][0].astype(np.float64)
        pool = getattr(difformer_amd, POOLS[mode])
        be.kernel_events = events = {}
        try:
            out = pool(torch.from_numpy(case["x32"])[perm].to(DEV), batch, 3)
            out64 = pool(torch.from_numpy(case["x32"]).double().to(DEV), n_nodes=case["lengths"])
        finally:
            be.kernel_events = None
        assert not events
        # float32 sums in any order: length * 2^-24 * sum |x| and one rounding
        slack = np.asarray(case["lengths"])[:, None] * 2.0 ** -24 * rr.sum_abs(case["x32"], case["ptr"]) + 2.0 ** -23 * np.abs(ref)
        assert (np.abs(out.double().cpu().numpy() - ref) <= slack).all()
        assert out64.dtype == torch.float64 and (np.abs(out64.cpu().numpy() - ref) <= 2.0 ** -40 * (1 + np.abs(ref))).all()


# ---- GraphGNN ----------------------------------------------------------------------------------------------------------------------------
LENGTHS = [1, 40, 17, 8, 23]
CFG = dict(hidden_channels=64, num_layers=2, kernel="simple", alpha=0.5, use_bn=True, use_residual=True, use_weight=True,
           use_graph=True, graph_weight=-1)


def _particle_batch(seed):
    """Five graphs of 1 .. 40 nodes back to back: x [89, 7], symmetric edges inside the graphs plus self loops, labels [5, 1]."""
    g = torch.Generator().manual_seed(seed)
    n = sum(LENGTHS)
    x = torch.randn(n, 7, generator=g)
    edges, first = [], 0
    for m in LENGTHS:
        pairs = torch.randint(0, m, (2, 3 * m), generator=g) + first
        edges += [pairs, pairs.flip(0)]
        first += m
    ei = torch.cat(edges + [torch.arange(n).repeat(2, 1)], dim=1)
    y = (torch.rand(len(LENGTHS), 1, generator=g) > 0.5).float()
    return x, ei, y


def _graph_model(seed, pooling):
    import difformer_amd
    torch.manual_seed(seed)
    gnn = difformer_amd.DIFFormer_v2(7, 64, 64, num_layers=2, kernel="simple", dropout=0.0)
    return difformer_amd.GraphGNN(64, 1, gnn, pooling).to(DEV).train()


@pytest.mark.parametrize("pooling", ["sum", "mean", "max"])
def test_graphgnn_over_difformer_v2_against_float64_autograd(pooling):
    """Logits and every parameter gradient of one BCE step against float64 autograd of the differentiable oracle, the float64
    pool and `lin`; 1e-4 norm-wise per tensor, the bar of the v2 tests in tests/test_gpu_grad.py."""
    import difformer_amd
    from difformer_amd import ops
    from oracle import difformer_oracle_grad as og
    x, ei, y = _particle_batch(41)
    model = _graph_model(42, pooling)
    be = ops.get_backend()
    be.kernel_events = events = {}
    try:
        logits = model(x.to(DEV), ei.to(DEV), torch.tensor(LENGTHS))
        loss = difformer_amd.bce_with_logits(logits, y.to(DEV))
        loss.backward()
    finally:
        be.kernel_events = None
    assert {"dif_readout_fwd_f32", "dif_readout_bwd_f32"} <= set(events)
    p = og.leaves({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
    h = og.difformer_v2_forward({k[len("gnn_node."):]: v for k, v in p.items() if k.startswith("gnn_node.")}, x.double(), ei, LENGTHS, CFG)
    parts = torch.split(h, LENGTHS)
    pooled = torch.stack([t.sum(0) if pooling == "sum" else t.mean(0) if pooling == "mean" else t.amax(0) for t in parts])
    ref = F.linear(pooled, p["lin.weight"], p["lin.bias"])
    ref_loss = F.binary_cross_entropy_with_logits(ref, y.double())
    ref_loss.backward()
    assert rel_err(logits.detach().cpu().numpy(), ref.detach().numpy()) < 1e-4
    assert abs(float(loss.detach()) - float(ref_loss.detach())) < 1e-4 * abs(float(ref_loss.detach()))
    gmax = max(float(v.grad.abs().max()) for v in p.values())
    worst = {k: grad_err(prm.grad.cpu().numpy(), p[k].grad.numpy(), gmax) for k, prm in model.named_parameters()}
    print(f"{pooling}: worst parameter grad_err {max(worst.values()):.2e}")
    assert max(worst.values()) < 1e-4, worst
    # the batched_data form takes the same path: the same bits
    import types
    again = model(types.SimpleNamespace(x=x.to(DEV), edge_index=ei.to(DEV), n_nodes=torch.tensor(LENGTHS)))
    assert torch.equal(again.detach(), logits.detach())


@pytest.mark.parametrize("pooling", ["sum", "mean", "max"])
def test_a_whole_step_of_graphgnn_is_captured_as_one_chain(pooling, monkeypatch):
    """GraphedTrainStep(GraphGNN, difformer_amd.Adam, bce_with_logits): three replays are bitwise equal to the eager loop (three
    warm-up steps run before the capture), and every kernel of the capture -- the read-out's two among them -- is enqueued on
    the capturing stream: the read-out introduces no side stream, the captured graph is a single chain."""
    import difformer_amd
    from difformer_amd import backend_hip, ops
    x, ei, y = _particle_batch(43)
    x, ei, y = x.to(DEV), ei.to(DEV), y.to(DEV)
    n_nodes = torch.tensor(LENGTHS, device=DEV)
    eager = _graph_model(44, pooling)
    twin = copy.deepcopy(eager)
    loss_fn = lambda out: difformer_amd.bce_with_logits(out, y)
    opt_e = difformer_amd.Adam(eager.parameters(), lr=1e-3, weight_decay=1e-3)
    opt_g = difformer_amd.Adam(twin.parameters(), lr=1e-3, weight_decay=1e-3)
    captured, side = [], []
    real_call, real_side = backend_hip.HipBackend._call, ops.side_stream

    def call(self, label, symbol, dev, *args, **kw):
        if torch.cuda.is_current_stream_capturing():
            captured.append((symbol, torch.cuda.current_stream(dev).cuda_stream))
        return real_call(self, label, symbol, dev, *args, **kw)

    def side_stream(dev):
        side.append(torch.cuda.is_current_stream_capturing())
        return real_side(dev)

    monkeypatch.setattr(backend_hip.HipBackend, "_call", call)
    monkeypatch.setattr(ops, "side_stream", side_stream)
    step = difformer_amd.GraphedTrainStep(twin, opt_g, loss_fn, x, ei, n_nodes, warmup=3)
    monkeypatch.undo()
    assert {"dif_readout_fwd_f32", "dif_readout_bwd_f32", "dif_bce_with_logits_fwd_f32", "dif_adam_step_f32"} <= {s for s, _ in captured}
    assert len({st for _, st in captured}) == 1 and not any(side)
    losses_g = [step().detach().clone() for _ in range(3)]
    losses_e = []
    for _ in range(3 + 3):
        opt_e.zero_grad(set_to_none=True)
        loss = loss_fn(eager(x, ei, n_nodes))
        loss.backward()
        opt_e.step()
        losses_e.append(loss.detach().clone())
    print("graphed", [float(v) for v in losses_g], "eager", [float(v) for v in losses_e[-3:]])
    assert float(losses_g[0]) != float(losses_g[2])                              # the replays do train
    for a, b in zip(losses_g, losses_e[-3:]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), (losses_g, losses_e)
    for (k, a), (_, b) in zip(twin.named_parameters(), eager.named_parameters()):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32)), k


def test_zz_report_the_worst_cases():
    """Prints what the tests above measured (profiles/r16_readout.md quotes it); run last in this module."""
    for key, w in sorted(WORST.items()):
        print(f"worst case {key}: {w:.3f} x bound")
    assert WORST and all(w <= 1 for w in WORST.values())
