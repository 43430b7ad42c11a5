"""Snapshot batches without a GPU: the layout of SnapshotBatch, its rejections, the eleventh library's header and the argument
errors of its entry points, and the fallback loop of DIFFormer.forward_snapshots on CPU tensors."""
import ctypes
import os
import re

import pytest
import torch

from fake_backend import OracleBackend

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_snapshots.h")
NAMES = ["dif_snap_backward_f32", "dif_snap_forward_f32", "dif_snap_last_error", "dif_snap_scratch_floats", "dif_snap_tape_floats",
         "dif_snap_version"]
FWD_ARGS = ("cfg", "T", "records", "x", "ldx", "params", "rnd", "tape", "y", "stream")
BWD_ARGS = ("cfg", "T", "records", "x", "ldx", "params", "rnd", "tape", "grad_y", "grads", "slabs", "slab_stride", "grad_out", "dx",
            "scratch", "stream")


def _graph(n, e, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.cat([torch.randint(0, n, (2, e), generator=g), torch.arange(n).repeat(2, 1)], 1)


# ---- SnapshotBatch ------------------------------------------------------------------------------------------------------------
def test_layout_of_a_mixed_batch_with_per_snapshot_graphs():
    from difformer_amd import SnapshotBatch
    sizes = [3, 1, 7, 20]
    xs = [torch.randn(n, 5) for n in sizes]
    eis = [_graph(n, 2 * n, n) for n in sizes]
    ews = [torch.rand(ei.shape[1]) for ei in eis]
    batch = SnapshotBatch(xs, eis, ews)
    assert len(batch) == 4 and batch.node_ptr == [0, 3, 4, 11, 31] and batch.max_n == 20
    assert batch.node_ptr_dev.dtype == torch.int64 and batch.node_ptr_dev.tolist() == batch.node_ptr
    assert batch.x.shape == (31, 5) and batch.x.is_contiguous() and torch.equal(batch.x, torch.cat(xs))
    assert all(a is b for a, b in zip(batch.edge_index, eis)) and all(a is b for a, b in zip(batch.edge_weight, ews))
    Y = torch.randn(31, 2)
    parts = batch.split(Y)
    assert [p.shape[0] for p in parts] == sizes and all(p._base is Y for p in parts) and torch.equal(torch.cat(parts), Y)
    assert batch.graphs is None                                             # host memory: no tiny CSR is built
    xs[0].zero_()
    assert batch.x[:3].abs().sum() > 0                                      # a copy, not a view of the caller's tensors


def test_shared_graph_and_the_stacked_form():
    from difformer_amd import SnapshotBatch
    xs = torch.randn(6, 9, 4)
    ei = _graph(9, 20, 0)
    batch = SnapshotBatch(xs, ei)
    assert len(batch) == 6 and batch.node_ptr == [0, 9, 18, 27, 36, 45, 54] and batch.sizes == [9] * 6
    assert torch.equal(batch.x, xs.reshape(54, 4)) and batch.x.data_ptr() != xs.data_ptr()
    assert all(e is ei for e in batch.edge_index) and batch.edge_weight == [None] * 6
    one = SnapshotBatch([xs[0]], ei)
    assert len(one) == 1 and one.x.data_ptr() != xs[0].data_ptr()
    none = SnapshotBatch([xs[0], xs[1]])
    assert none.edge_index == [None, None]
    batch.x.requires_grad_()
    assert batch.x.is_leaf and batch.x.requires_grad


def test_rejections():
    from difformer_amd import SnapshotBatch
    xs = [torch.randn(4, 3), torch.randn(5, 3)]
    ei = [_graph(4, 6, 0), _graph(5, 6, 1)]
    with pytest.raises(TypeError, match="float32"):
        SnapshotBatch([xs[0], xs[1].double()], ei)
    with pytest.raises(TypeError, match="float32"):
        SnapshotBatch(torch.zeros(2, 4, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="1 entries for 2 snapshots"):
        SnapshotBatch(xs, ei[:1])
    with pytest.raises(ValueError, match="3 entries for 2 snapshots"):
        SnapshotBatch(xs, ei, [None, None, None])
    with pytest.raises(ValueError, match="one entry per edge"):
        SnapshotBatch(xs, ei, [torch.rand(ei[0].shape[1]), torch.rand(ei[1].shape[1] - 1)])
    with pytest.raises(ValueError, match="one entry per edge"):
        SnapshotBatch(torch.randn(2, 4, 3), ei[0], torch.rand(3))
    with pytest.raises(ValueError, match="same F"):
        SnapshotBatch([xs[0], torch.randn(5, 2)], ei)
    with pytest.raises(TypeError, match="int64"):
        SnapshotBatch(xs, [ei[0].int(), ei[1]])
    with pytest.raises(ValueError, match=r"\[T, n, F\]"):
        SnapshotBatch(torch.randn(4, 3))
    with pytest.raises(ValueError, match="at least one"):
        SnapshotBatch([])


# ---- the fallback loop --------------------------------------------------------------------------------------------------------
@pytest.fixture()
def fake_backend(monkeypatch):
    from difformer_amd import ops
    be = OracleBackend()
    monkeypatch.setattr(ops, "_BACKEND", be)
    ops.csr_cache.clear()
    yield be
    ops.csr_cache.clear()


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_cpu_tensors_take_the_loop_and_equal_it_bitwise(kernel, fake_backend):
    from difformer_amd import DIFFormer, SnapshotBatch, snapshots
    torch.manual_seed(0)
    model = DIFFormer(5, 4, 2, num_layers=2, num_heads=1, kernel=kernel, use_graph=True, use_weight=False).eval()
    sizes = [6, 11, 3]
    xs = [torch.randn(n, 5) for n in sizes]
    eis = [_graph(n, 3 * n, n) for n in sizes]
    ews = [torch.rand(ei.shape[1]) + 0.1 for ei in eis]
    batch = SnapshotBatch(xs, eis, ews)
    try:
        # the loop over the batch's own rows: the host BLAS rounds a product by the alignment of its operand, so rows at another
        # address are no bitwise yardstick
        with torch.no_grad():
            loop = torch.cat([model(x, ei, ew) for x, ei, ew in zip(batch.split(batch.x), eis, ews)])
            again = torch.cat([model(x, ei, ew) for x, ei, ew in zip(batch.split(batch.x), eis, ews)])
            fresh = torch.cat([model(x, ei, ew) for x, ei, ew in zip(xs, eis, ews)])
    except Exception as e:                                                  # the test-only backend cannot run this model
        pytest.skip(f"fake backend cannot run the model: {type(e).__name__}")
    assert torch.allclose(loop, fresh, rtol=1e-5, atol=1e-6)
    if not torch.equal(loop, again):
        pytest.skip("the host backend does not repeat its own bits: no bitwise yardstick")
    before = dict(snapshots.stats)
    with torch.no_grad():
        Y = model.forward_snapshots(batch)
    assert snapshots.stats["fallback"] == before["fallback"] + 1 and snapshots.stats["forward"] == before["forward"]
    assert Y.shape == (sum(sizes), 2) and torch.equal(Y, loop)
    assert all(torch.equal(a, b) for a, b in zip(batch.split(Y), loop.split(sizes)))

# ---- header and library -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def snap():
    from difformer_amd import _lib
    if not os.path.exists(_lib.SNAPSHOTS_LIB_PATH):
        pytest.skip("libdifformer_snapshots.so not built")
    return _lib.load_snapshots()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(snap):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.SNAPSHOTS_SIGNATURES) == NAMES
    for name in declared:
        assert getattr(snap, name) is not None
    others = (set(_lib.SIGNATURES) | set(_lib.MAPS_SIGNATURES) | set(_lib.EDGES_SIGNATURES) | set(_lib.KNN_SIGNATURES)
              | set(_lib.SLOTS_SIGNATURES) | set(_lib.METRICS_SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAM_SIGNATURES)
              | set(_lib.READOUT_SIGNATURES) | set(_lib.NBR_SIGNATURES))
    assert not set(_lib.SNAPSHOTS_SIGNATURES) & others
    fwd, bwd = _lib.SNAPSHOTS_SIGNATURES["dif_snap_forward_f32"], _lib.SNAPSHOTS_SIGNATURES["dif_snap_backward_f32"]
    assert len(fwd[1]) == len(FWD_ARGS) and len(bwd[1]) == len(BWD_ARGS)
    assert fwd[1][0] is bwd[1][0] and fwd[1][0]._type_ is _lib.TinyCfg            # dif_tiny_cfg comes from difformer_hip.h
    assert fwd[1][FWD_ARGS.index("ldx")] is ctypes.c_int64 and bwd[1][BWD_ARGS.index("slab_stride")] is ctypes.c_int64
    assert _lib.SNAPSHOTS_SIGNATURES["dif_snap_tape_floats"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert _lib.SNAPSHOTS_SIGNATURES["dif_snap_last_error"][0] is ctypes.c_char_p
    assert snap.dif_snap_version() == _lib.SNAPSHOTS_VERSION == 1
    assert _lib.SNAPSHOTS_CONSTANTS == {"DIF_SNAP_RECORD_FIELDS": 12}


def test_buffer_sizes_are_host_arithmetic_without_the_grid_regions(snap):
    from difformer_amd import _lib
    lib = _lib.load()
    for n, d, L in ((1, 1, 1), (20, 4, 2), (129, 4, 2), (129, 5, 3), (1068, 4, 2), (1067, 8, 8), (4096, 8, 8)):
        DP = 4 if d <= 4 else 8
        tape = n * DP * (2 * (L + 1) + L + 3) + L * n + L * 96              # H, Z, ATT, Q K V rows; DEN; SUM
        scratch = 14 * n * DP + 3 * n
        assert snap.dif_snap_tape_floats(n, d, L) == -(-tape // 4) * 4
        assert snap.dif_snap_scratch_floats(n, d, L) == -(-scratch // 4) * 4
        assert snap.dif_snap_tape_floats(n, d, L) <= lib.dif_tiny_tape_floats(n, d, L)
        assert snap.dif_snap_scratch_floats(n, d, L) <= lib.dif_tiny_scratch_floats(n, d, L) + 3
    # wikimath: 146 snapshots of 1,068 nodes stay far below what the grid plans' partial sums would take
    assert 146 * snap.dif_snap_tape_floats(1068, 4, 2) * 4 < 32 << 20
    for bad in ((0, 4, 2), (5, 0, 2), (5, 9, 2), (5, 4, 0), (5, 4, 9)):
        assert snap.dif_snap_tape_floats(*bad) == 0 and snap.dif_snap_scratch_floats(*bad) == 0


# made-up (never dereferenced) addresses: every rejection happens before any HIP call
def _cfg(**over):
    from difformer_amd import _lib
    f = dict(n=20, in_channels=4, hidden=4, out_channels=1, num_layers=2, kernel=0, use_bn=1, use_residual=1, use_weight=0, use_graph=1,
             use_source=0, training=1, alpha=0.5, attn_scale=1.0, gcn_scale=1.0, dropout=0.0, eps=1e-5, launch_plan=1, nnz=0)
    f.update(over)
    return _lib.TinyCfg(**f)


def _params(L=2, base=0x100000):
    return (ctypes.c_void_p * (6 + 8 * L))(*[base + 256 * k for k in range(6 + 8 * L)])


def _grads(L=2, base=0x200000, stride=16):
    return (ctypes.c_void_p * (6 + 8 * L))(*[base + 4 * stride * k for k in range(6 + 8 * L)])


def _backward(snap, cfg=None, **over):
    a = dict(T=3, records=0x50000, x=0x10000, ldx=4, params=_params(), rnd=None, tape=0x300000, grad_y=0x20000, grads=_grads(),
             slabs=0x200000, slab_stride=16 * 22, grad_out=0x400000, dx=None, scratch=0x500000, stream=None)
    a.update(over)
    return snap.dif_snap_backward_f32(ctypes.byref(cfg or _cfg()), *[a[k] for k in BWD_ARGS[1:]])


def test_rejections_of_the_entry_points(snap):
    from difformer_amd import _lib
    E = _lib.ERROR_CODES

    def fwd(cfg=None, **over):
        a = dict(T=3, records=0x50000, x=0x10000, ldx=4, params=_params(), rnd=None, tape=0x300000, y=0x20000, stream=None)
        a.update(over)
        return snap.dif_snap_forward_f32(ctypes.byref(cfg or _cfg()), *[a[k] for k in FWD_ARGS[1:]])

    assert fwd(T=0) == E["DIF_E_SHAPE"] and b"snapshots" in snap.dif_snap_last_error()
    assert fwd(T=65536) == E["DIF_E_SHAPE"]
    assert fwd(records=None) == E["DIF_E_BADARG"] and fwd(records=0x50008) == E["DIF_E_BADARG"]
    assert fwd(cfg=_cfg(hidden=9)) == E["DIF_E_SHAPE"] and fwd(cfg=_cfg(n=4097)) == E["DIF_E_SHAPE"]
    assert fwd(tape=0x300004) == E["DIF_E_BADARG"] and fwd(y=None) == E["DIF_E_BADARG"] and fwd(ldx=3) == E["DIF_E_BADARG"]
    assert _backward(snap, slab_stride=18) == E["DIF_E_BADARG"] and _backward(snap, slabs=None) == E["DIF_E_BADARG"]
    assert _backward(snap, grad_out=None) == E["DIF_E_BADARG"] and _backward(snap, scratch=0x500008) == E["DIF_E_BADARG"]
    # a gradient pointer outside slab 0, or a parameter that does not fit before the slab ends
    assert _backward(snap, slab_stride=16 * 21) == E["DIF_E_BADARG"] and b"slab 0" in snap.dif_snap_last_error()
    assert _backward(snap, slabs=0x200040) == E["DIF_E_BADARG"]
