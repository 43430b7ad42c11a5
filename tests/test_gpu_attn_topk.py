"""Streaming top-k attention maps on the MI355X (csrc/attn_topk.hip behind include/difformer_maps.h): parity through the C
ABI for every kernel instantiation, the tie rule, guard bands, the model method against the dense map, and peak memory.
The criterion is tests/topk_ref.py's: values and values-at-indices to 1e-4 of the float64 restatement, indices distinct and
in range."""
import functools
import gc

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, split_model_case
from guarded import GuardedArena, guarded_inputs
import topk_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = {"simple": 0, "sigmoid": 1}

# (N, L, H, M, k): (N, L) in {(1, 1), (17, 33), (100, 1000), (257, 4099)}, H in {1, 2}, M in {4, 64, 68, 128, 300},
# k in {1, 8, 9, 32} and k = L.  Per mode every sweep instantiation <KMAX in {8, 16, 32}, M <= 64 or wider> and every merge
# instantiation <KMAX> runs; (17, 33) sweeps the keys in one range, (100, 1000) and (257, 4099) in several.
SHAPES = [
    (1, 1, 1, 4, 1),             # k = L
    (1, 1, 2, 128, 1),
    (17, 33, 2, 64, 8),          # KMAX 8,  registers
    (17, 33, 1, 68, 9),          # KMAX 16, wide
    (17, 33, 2, 4, 32),          # KMAX 32, registers
    (17, 33, 1, 300, 32),        # KMAX 32, wide, one range
    (100, 1000, 1, 64, 9),       # KMAX 16, registers
    (100, 1000, 2, 128, 8),      # KMAX 8,  wide
    (100, 1000, 1, 300, 32),     # KMAX 32, wide
    (257, 4099, 2, 64, 32),
    (257, 4099, 1, 300, 9),
    (257, 4099, 1, 4, 1),
    (257, 4099, 2, 68, 8),
]


@pytest.fixture(scope="module")
def maps():
    from difformer_amd import _lib
    return _lib.load_maps()


def _operands(kernel, n, l, h, m, seed=0, pad=8):
    """q [n,h,m], k [l,h,m] as column slices of wider tensors (ld = h m + pad > h m, rows 16-byte aligned)."""
    g = torch.Generator().manual_seed(1000 * seed + n + l + h + m)
    scale = m ** -0.25 if kernel == "sigmoid" else 1.0          # scores of unit variance: sigma does not saturate
    qw, kw = torch.randn(n, h * m + pad, generator=g) * scale, torch.randn(l, h * m + pad, generator=g) * scale
    return qw[:, 4:4 + h * m].view(n, h, m), kw[:, 4:4 + h * m].view(l, h, m), qw, kw


def _raw_attention(q, k, mode):
    """float64 [N,L,H] of what the ENTRY POINT ranks and reports: mode 0 the score itself, mode 1 sigma(s) / sum sigma(s)."""
    s = np.einsum("nhm,lhm->nlh", q.numpy().astype(np.float64), k.numpy().astype(np.float64))
    if mode == 0:
        return s
    sig = 1.0 / (1.0 + np.exp(-s))
    return sig / sig.sum(axis=1, keepdims=True)


def _launch(maps, q, ldq, k, ldk, n, l, h, m, mode, topk, values, indices, ws):
    from difformer_amd import _lib
    rc = maps.dif_attn_topk_f32(q.data_ptr(), ldq, k.data_ptr(), ldk, n, l, h, m, mode, topk, values.data_ptr(), indices.data_ptr(),
                                ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    _lib.check_maps(rc, "dif_attn_topk_f32")


def _topk(maps, qv, kv, qw, kw, mode, topk):
    """The entry point on device copies of the wide tensors; q / k are the column slices at element 4."""
    (n, h, m), l = qv.shape, kv.shape[0]
    qd, kd = qw.to(DEV), kw.to(DEV)
    values = torch.full((n, h, topk), float("nan"), device=DEV)
    indices = torch.full((n, h, topk), -1, dtype=torch.int32, device=DEV)
    ws = torch.empty(maps.dif_attn_topk_workspace_bytes(n, l, h, m, topk), dtype=torch.uint8, device=DEV)
    _launch(maps, qd[:, 4:], qd.stride(0), kd[:, 4:], kd.stride(0), n, l, h, m, mode, topk, values, indices, ws)
    torch.cuda.synchronize()
    return values.cpu(), indices.cpu()


@functools.lru_cache(maxsize=None)
def _case(kernel, n, l, h, m):
    qv, kv, qw, kw = _operands(kernel, n, l, h, m)
    return qv, kv, qw, kw, _raw_attention(qv, kv, MODES[kernel])


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
@pytest.mark.parametrize("n,l,h,m,k", SHAPES)
def test_parity_through_the_c_abi(maps, kernel, n, l, h, m, k):
    qv, kv, qw, kw, attn = _case(kernel, n, l, h, m)
    values, indices = _topk(maps, qv, kv, qw, kw, MODES[kernel], k)
    topk_ref.check_topk(values.numpy(), indices.numpy(), attn, k, f"{kernel} N={n} L={l} H={h} M={m} k={k}")


def test_the_grid_has_split_and_unsplit_sweeps(maps):
    assert maps.dif_attn_topk_splits(17, 33, 2, 64, 8) == 1 and maps.dif_attn_topk_splits(1, 1, 1, 4, 1) == 1
    assert maps.dif_attn_topk_splits(100, 1000, 1, 64, 9) > 1 and maps.dif_attn_topk_splits(257, 4099, 2, 64, 32) > 1


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
@pytest.mark.parametrize("n,l,h,m,k", [(100, 1000, 2, 64, 8), (17, 34, 1, 68, 32)])
def test_ties_go_to_the_lower_index_and_calls_repeat_bitwise(maps, kernel, n, l, h, m, k):
    """The second half of K is a copy of the first: every score occurs twice, bit for bit, at another place of another tile
    (and, in the split shape, in another key range).  The top-k is then pairs (i, i + L/2), lower index first."""
    qv, kv, qw, kw = _operands(kernel, n, l, h, m, seed=5)
    kw[l // 2:] = kw[: l // 2]
    assert (maps.dif_attn_topk_splits(n, l, h, m, k) > 1) == (l == 1000)
    values, indices = _topk(maps, qv, kv, qw, kw, MODES[kernel], k)
    again = _topk(maps, qv, kv, qw, kw, MODES[kernel], k)
    assert torch.equal(values.view(torch.int32), again[0].view(torch.int32)) and torch.equal(indices, again[1])
    assert torch.equal(values[:, :, 0::2].view(torch.int32), values[:, :, 1::2].view(torch.int32))
    assert torch.equal(indices[:, :, 0::2] + l // 2, indices[:, :, 1::2])
    topk_ref.check_topk(values.numpy(), indices.numpy(), _raw_attention(qv, kv, MODES[kernel]), k, f"ties {kernel} L={l}")


def test_a_nan_score_ranks_last(maps):
    qv, kv, qw, kw = _operands("simple", 5, 20, 1, 8, seed=7)
    kw[7] = float("nan")
    values, indices = _topk(maps, qv, kv, qw, kw, 0, 20)
    assert (indices[:, :, -1] == 7).all() and torch.isnan(values[:, :, -1]).all() and not torch.isnan(values[:, :, :-1]).any()
    assert (torch.sort(indices, dim=2).values == torch.arange(20, dtype=torch.int32)).all()


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
@pytest.mark.parametrize("n,l,h,m,k", [(100, 1000, 1, 64, 9), (17, 33, 2, 68, 32)])
def test_between_guard_bands(maps, kernel, n, l, h, m, k):
    """Operands between NaN bands at 16-byte alignment (rows padded: the tail of every row is NaN too), outputs and workspace
    poisoned between checked guard bands."""
    qv, kv, _, _ = _operands(kernel, n, l, h, m, seed=9)
    arena = GuardedArena()
    ld = h * m + 4
    qd, kd = guarded_inputs(arena, DEV, True, q=(qv.reshape(n, h * m).contiguous(), ld), k=(kv.reshape(l, h * m).contiguous(), ld))
    values = arena.alloc((n, h, k), torch.float32, DEV)
    indices = arena.alloc((n, h, k), torch.int32, DEV)
    ws = arena.alloc((maps.dif_attn_topk_workspace_bytes(n, l, h, m, k),), torch.uint8, DEV, offset_bytes=16)
    _launch(maps, qd, ld, kd, ld, n, l, h, m, MODES[kernel], k, values, indices, ws)
    arena.check()
    topk_ref.check_topk(values.cpu().numpy(), indices.cpu().numpy(), _raw_attention(qv, kv, MODES[kernel]), k, f"guarded {kernel} L={l}")


# ---- the functional API and the model method ----------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,n,l,h,m,k", [("simple", 100, 1000, 2, 30, 8), ("sigmoid", 257, 300, 1, 64, 16)])
def test_attention_topk_against_the_reference_definition(kernel, n, l, h, m, k):
    from difformer_amd import attention_topk
    qv, kv, _, _ = _operands(kernel, n, l, h, m, seed=11)
    be_events = {}
    from difformer_amd import ops
    be = ops.get_backend()
    be.kernel_events = be_events
    try:
        values, indices = attention_topk(qv.to(DEV), kv.to(DEV), kernel, k)
    finally:
        be.kernel_events = None
    assert "dif_attn_topk_f32" in be_events and indices.dtype == torch.int64 and values.device.type == "cuda"
    topk_ref.check_topk(values.cpu().numpy(), indices.cpu().numpy(), topk_ref.dense_attention(qv.numpy(), kv.numpy(), kernel), k, kernel)
    host_v, host_i = attention_topk(qv, kv, kernel, k)                      # host operands are staged and come back on the host
    assert host_v.device.type == "cpu" and torch.equal(host_v, values.cpu()) and torch.equal(host_i, indices.cpu())


def _dense_per_head(model, x):
    """get_attentions for the one combination at which it (like the reference, difformer.py:43) cannot divide: `simple`
    with several heads.  The same layer sequence, the dense map from tests/topk_ref.py per layer."""
    from difformer_amd import autograd_ops as ag
    from difformer_amd.difformer import _ln_args, full_attention_conv
    maps_, layer_ = [], []
    with torch.no_grad():
        x = model._input_layer(x, False)
        layer_.append(x)
        for i, conv in enumerate(model.convs):
            q, k, v = conv._project(x, x)
            maps_.append(topk_ref.dense_attention(q.cpu().numpy(), k.cpu().numpy(), conv.kernel))
            c = full_attention_conv(q, k, v, conv.kernel)
            bn = model.bns[i + 1] if model.use_bn else None
            x = ag.layer_tail(c, None, layer_[i] if model.residual else None, model.alpha, *_ln_args(bn))
            layer_.append(x)
    return np.stack(maps_)


@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
@pytest.mark.parametrize("heads", [1, 2])
def test_top_attentions_against_the_dense_map_on_the_same_gpu(kernel, heads):
    from difformer_amd import DIFFormer
    torch.manual_seed(3)
    n, k = 300, 8
    model = DIFFormer(12, 32, 4, num_layers=2, num_heads=heads, kernel=kernel, use_graph=False).to(DEV).eval()
    x = torch.randn(n, 12, generator=torch.Generator().manual_seed(4)).to(DEV)
    values, indices = model.top_attentions(x, k)
    assert values.shape == indices.shape == (2, n, heads, k) and indices.dtype == torch.int64
    if kernel == "simple" and heads > 1:
        dense = _dense_per_head(model, x)
    else:
        with torch.no_grad():
            att = model.get_attentions(x)                                   # [layers, N, N, H]
        tv, _ = torch.topk(att.permute(0, 1, 3, 2), k)
        assert rel_err(values.cpu().numpy(), tv.cpu().numpy()) <= topk_ref.TOL
        dense = att.double().cpu().numpy()
    for layer in range(2):
        topk_ref.check_topk(values[layer].cpu().numpy(), indices[layer].cpu().numpy(), dense[layer], k, f"{kernel} H={heads} layer {layer}")


def test_top_attentions_golden_model_and_host_resident_model():
    from difformer_amd import DIFFormer
    c = load_golden("topk")["model/a_h2_nograph"]
    cfg, sd = split_model_case(c)
    model = DIFFormer(int(cfg.pop("in_channels")), int(cfg.pop("hidden_channels")), int(cfg.pop("out_channels")), **cfg).eval()
    model.load_state_dict({name: torch.from_numpy(v) for name, v in sd.items()})
    k = c["values"].shape[-1]
    x = torch.from_numpy(c["x"])
    host_v, host_i = model.top_attentions(x, k)                 # model and x on the host: staged through the device twin
    assert host_v.device.type == "cpu" and "_staged" in model.__dict__
    model = model.to(DEV)
    values, indices = model.top_attentions(x.to(DEV), k)
    assert torch.equal(values.cpu(), host_v) and torch.equal(indices.cpu(), host_i)
    e1 = rel_err(values.cpu().numpy(), c["values"])
    print(f"golden model: values {e1:.2e}")
    assert e1 <= topk_ref.TOL
    with torch.no_grad():
        dense = model.get_attentions(x.to(DEV)).double().cpu().numpy()
    for layer in range(dense.shape[0]):
        topk_ref.check_topk(values[layer].cpu().numpy(), indices[layer].cpu().numpy(), dense[layer], k, f"golden layer {layer}")


def test_peak_memory_stays_far_below_one_dense_map():
    """N = 40,000, hidden 64, 2 layers, k = 16: operands, outputs and workspace are tens of MB; one [N, N] float32 tensor is
    6.4 GB.  The bound is a tenth of that."""
    from difformer_amd import DIFFormer, ops
    torch.manual_seed(5)
    n = 40000
    model = DIFFormer(16, 64, 4, num_layers=2, num_heads=1, kernel="simple", use_graph=False).to(DEV).eval()
    x = torch.randn(n, 16, device=DEV)
    ops.csr_cache.clear()
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    values, indices = model.top_attentions(x, 16)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    print(f"peak memory over top_attentions at N = {n}: {peak / 1e6:.1f} MB")
    assert values.shape == (2, n, 1, 16) and bool(torch.isfinite(values).all())
    assert int(indices.min()) >= 0 and int(indices.max()) < n
    assert peak < 640e6, f"{peak / 1e6:.1f} MB"
