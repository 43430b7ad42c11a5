"""Self-tests of tests/guarded.py on CPU arenas: deliberately wrong stand-in operations (written here, never run on a GPU)
must each be flagged, their correct versions must pass, and the package's host logic must compute the same bits when its
allocations come out of an arena.  This is what shows that the guarded GPU tests would fail for a subtly wrong kernel."""
import numpy as np
import pytest
import torch

import guarded
from conftest import load_golden, split_model_case
from fake_backend import OracleBackend
from guarded import GuardedArena, guarded_inputs

GRAD = load_golden("grad")


def _flat_neighbourhood(t, before, after):
    """The elements of t's storage from `before` elements ahead of t to `after` elements past it: what a kernel that is
    handed t's address can reach with an index outside [0, n)."""
    n = t.numel()
    return torch.empty(0, dtype=t.dtype).set_(t.untyped_storage(), t.storage_offset() - before, (before + n + after,), (1,))


# ---- stand-in "kernels": y = 2 x over n elements, given raw neighbourhoods as a kernel is given raw addresses ----------
def _scale_ok(x, y):
    y.copy_(2 * x)


def _scale_writes_one_past(x, y):
    _flat_neighbourhood(y, 0, 1).copy_(torch.cat([2 * x.flatten(), torch.ones(1)]))


def _scale_writes_one_before(x, y):
    _flat_neighbourhood(y, 1, 0).copy_(torch.cat([torch.ones(1), 2 * x.flatten()]))


def _sum_reads_index_n(x, y):
    y.copy_(_flat_neighbourhood(x, 0, 1)[1:].sum().expand_as(y))           # x[1 .. n] instead of x[0 .. n-1]


def _scale_skips_last_row(x, y):
    y[:-1].copy_(2 * x[:-1])


def _run(op, shape=(5, 8)):
    arena = GuardedArena()
    x, = guarded_inputs(arena, "cpu", x=torch.arange(1.0, 1 + shape[0] * shape[1]).reshape(shape))
    y = arena.alloc(shape, torch.float32)
    op(x, y)
    return arena, x, y


def test_correct_stand_in_passes():
    arena, x, y = _run(_scale_ok)
    arena.check()
    assert torch.equal(y, 2 * x) and np.isfinite(y.numpy()).all()


def test_write_one_element_past_the_payload_is_flagged():
    arena, x, y = _run(_scale_writes_one_past)
    assert torch.equal(y, 2 * x)                      # the values inside are right: only the guard can tell
    with pytest.raises(AssertionError, match=r"trailing guard .*test_guarded_harness\.py:\d+ \(shape \(5, 8\), torch\.float32.*payload end \+0"):
        arena.check()


def test_write_one_element_before_the_payload_is_flagged():
    arena, x, y = _run(_scale_writes_one_before)
    assert torch.equal(y, 2 * x)
    with pytest.raises(AssertionError, match=r"leading guard .*payload start -4, 4 bytes"):
        arena.check()


def test_read_at_index_n_turns_the_result_into_nan():
    arena, x, y = _run(_sum_reads_index_n)
    arena.check()                                     # nothing was written outside ...
    assert not np.isfinite(y.numpy()).any()           # ... but the result is NaN, which no tolerance lets through


def test_unwritten_last_row_stays_nan():
    arena, x, y = _run(_scale_skips_last_row)
    arena.check()
    assert torch.equal(y[:-1], 2 * x[:-1]) and torch.isnan(y[-1]).all() and not np.isfinite(y.numpy()).all()


def test_status_word_that_is_never_set_reads_minus_one():
    arena = GuardedArena()
    status = arena.alloc((2,), torch.int32)
    assert status.tolist() == [-1, -1]                # a caller that tests `status != 0` raises; zeros would pass silently
    assert arena.alloc((1,), torch.int64).item() == -1
    arena.check()


def test_minus_one_as_a_row_index_lands_in_the_leading_guard():
    arena = GuardedArena()
    x, = guarded_inputs(arena, "cpu", x=torch.ones(3, 2000))             # rows of 8,000 bytes: wider than the 4,096 minimum
    row = _flat_neighbourhood(x, 2000, 0)[:2000]                          # x[-1]
    assert torch.isnan(row).all()
    arena.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64])
def test_poison_reads_as_nan_in_every_float_type(dtype):
    arena = GuardedArena()
    assert torch.isnan(arena.alloc((7, 3), dtype)).all()
    assert torch.isnan(_flat_neighbourhood(arena.alloc((4,), dtype), 5, 5)).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16, torch.float64, torch.int32, torch.int64, torch.uint8])
@pytest.mark.parametrize("offset", [0, 4, 16, 256])
def test_payload_alignment_is_the_requested_one(dtype, offset):
    item = torch.empty(0, dtype=dtype).element_size()
    arena = GuardedArena()
    if offset % item:
        with pytest.raises(ValueError):
            arena.alloc((3, 5), dtype, offset_bytes=offset)
        return
    t = arena.alloc((3, 5), dtype, offset_bytes=offset)
    assert t.data_ptr() % guarded.ALIGN == offset and t.is_contiguous() and t._base is None
    b = arena.blocks[-1]
    assert b.start >= guarded.MIN_GUARD and b.buf.numel() - b.start - b.nbytes >= guarded.MIN_GUARD
    x, = guarded_inputs(arena, "cpu", min_align=True, x=torch.zeros(3, 5, dtype=dtype))
    assert x.data_ptr() % guarded.ALIGN == 16
    arena.check()


def test_row_strided_operand_keeps_nan_row_tails():
    arena = GuardedArena()
    src = torch.randn(6, 5)
    x, = guarded_inputs(arena, "cpu", x=(src, 8))
    assert x.shape == (6, 5) and x.stride() == (8, 1) and torch.equal(x, src)
    full = torch.empty(0).set_(x.untyped_storage(), x.storage_offset(), (6, 8), (8, 1))
    assert torch.isnan(full[:, 5:]).all()                                 # a read past `width` inside a row is NaN too
    assert arena.blocks[-1].nbytes == 6 * 8 * 4
    arena.check()


def test_zeros_are_zero_inside_and_guarded_outside():
    arena = GuardedArena()
    proxy = guarded.TorchProxy(arena, cpu_too=True)
    z = proxy.zeros(3, 4, dtype=torch.float64)
    assert z.dtype == torch.float64 and not z.any() and torch.isnan(_flat_neighbourhood(z, 1, 1)[[0, -1]]).all()
    e = proxy.empty((2, 3), dtype=torch.int32, device="cpu")
    assert e.tolist() == [[-1] * 3] * 2
    assert torch.isnan(proxy.empty_like(torch.zeros(4))).all()
    assert len(arena.blocks) == 3 and all("test_guarded_harness.py" in b.site for b in arena.blocks)
    # what the proxy leaves alone: CPU tensors by default, pinned memory, everything else of torch
    plain = guarded.TorchProxy(arena)
    assert plain.empty(3).untyped_storage().nbytes() == 12 and plain.float32 is torch.float32 and plain.nn is torch.nn
    assert len(arena.blocks) == 3
    arena.check()


def test_releasing_arena_checks_the_oldest_blocks_when_it_holds_too_much(monkeypatch):
    monkeypatch.setattr(guarded, "KEEP_BYTES", 64 << 10)
    arena = guarded._ReleasingArena()
    first = arena.alloc((4,), torch.float32)
    _flat_neighbourhood(first, 0, 1)[-1] = 0.0                            # a guard hit in the oldest block ...
    with pytest.raises(AssertionError, match="trailing guard"):           # ... is reported when that block is released
        for _ in range(20):
            arena.alloc((1024,), torch.float32)


# ---- the package's host logic under the proxy: same bits -----------------------------------------------------------------
def _model_case(kernel):
    for name in sorted(GRAD):
        if name.startswith("model/") and str(split_model_case(GRAD[name])[0]["kernel"]) == kernel:
            return GRAD[name]
    raise AssertionError(f"no golden grad model case with kernel {kernel}")


def _forward_and_step(c):
    import torch.nn.functional as F
    from difformer_amd import DIFFormer
    cfg, sd = split_model_case(c)
    kw = {k: cfg[k] for k in ("num_layers", "num_heads", "kernel", "alpha", "use_bn", "use_residual", "use_weight",
                              "use_graph", "graph_weight", "use_source")}
    kw["kernel"] = str(kw["kernel"])
    model = DIFFormer(int(cfg["in_channels"]), int(cfg["hidden_channels"]), int(cfg["out_channels"]), dropout=0.0, **kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    ei = torch.from_numpy(c["edge_index"]) if cfg["use_graph"] else None
    w = torch.from_numpy(c["edge_weight"]).requires_grad_(True) if "edge_weight" in c else None
    model.eval()
    with torch.no_grad():
        results = [model(torch.from_numpy(c["x"]), ei, None if w is None else w.detach())]
    model.train()
    x = torch.from_numpy(c["x"]).requires_grad_(True)
    out = model(x, ei, w)
    idx, y = torch.from_numpy(c["train_idx"]), torch.from_numpy(c["y"])
    if str(c["loss_kind"]) == "bce":
        loss = F.binary_cross_entropy_with_logits(out[idx], y[idx])
    else:
        loss = F.nll_loss(F.log_softmax(out, dim=1)[idx], y[idx])
    loss.backward()
    results += [out.detach(), loss.detach(), x.grad] + ([] if w is None else [w.grad])
    results += [p.grad for _, p in model.named_parameters() if p.grad is not None]
    return results


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_host_logic_computes_the_same_bits_under_the_proxy(kernel, monkeypatch):
    """A forward and a training step of a golden model on tests/fake_backend.py, plain and with every torch.empty /
    empty_like / zeros of the package's modules coming out of an arena (CPU included here): the host logic tolerates
    outputs that sit inside larger storages at a non-zero offset (autograd_ops._adjacent_columns, TensorCache identity
    keys, the `_difformer_fused_grad` tag), and reads nothing it did not write -- a single NaN would change the bits."""
    from difformer_amd import ops
    c = _model_case(kernel)
    monkeypatch.setattr(ops, "_BACKEND", OracleBackend())
    ops.csr_cache.clear()
    plain = _forward_and_step(c)
    ops.csr_cache.clear()
    arena = guarded.install(monkeypatch, cpu_too=True)
    proxied = _forward_and_step(c)
    ops.csr_cache.clear()
    arena.check()
    assert len(plain) == len(proxied)
    for a, b in zip(plain, proxied):
        assert a.dtype == b.dtype and np.array_equal(a.numpy(), b.numpy(), equal_nan=True)
        assert np.isfinite(a.numpy()).all() == np.isfinite(b.numpy()).all()


def test_fused_gradient_buffer_from_an_arena_is_found_adjacent():
    """backend.simple_backward's dq | dk | dv buffer, allocated from an arena: its column views have the BUFFER as `_base`
    (an arena tensor is no autograd view), so autograd_ops._adjacent_columns takes the same in-place route as on a plain
    allocation."""
    from difformer_amd import autograd_ops as ag
    arena = GuardedArena()
    n, w = 6, 4
    fused = arena.alloc((n, 3 * w), torch.float32)
    fused._difformer_fused_grad = True
    dq, dk, dv = (fused[:, i * w: (i + 1) * w] for i in range(3))
    for i, t in enumerate((dq, dk, dv)):
        t.fill_(float(i))
    other = torch.full((n, w), 7.0)                   # dv accumulated with another consumer's gradient: a new tensor
    got = ag._adjacent_columns([dq, dk, other], n, [w, w, w])
    assert got is fused and torch.equal(fused[:, 2 * w:], other) and torch.equal(fused[:, :w], torch.zeros(n, w))
    arena.check()
