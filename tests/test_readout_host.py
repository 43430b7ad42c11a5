"""The graph read-out without a GPU: the ninth library's header, the long-double oracle of tests/readout_ref.py against torch's
scatter expressions in float64, the well-posedness of the case table the GPU tests share, the CPU-tensor path of the three
pools in both call forms, and GraphGNN."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

import readout_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_readout.h")
FWD = ("x", "ldx", "graph_ptr", "n_graphs", "n_rows", "H", "mode", "out", "ldo", "stream")
BWD = ("x", "ldx", "pooled", "ldp", "grad_out", "ldgo", "graph_ptr", "n_graphs", "n_rows", "H", "mode", "grad_x", "ldgx", "stream")
NAMES = ["dif_readout_bwd_bf16", "dif_readout_bwd_f32", "dif_readout_fwd_bf16", "dif_readout_fwd_f32", "dif_readout_last_error",
         "dif_readout_version"]
POOLS = {"add": "global_add_pool", "mean": "global_mean_pool", "max": "global_max_pool"}


def _pool(mode):
    import difformer_amd
    return getattr(difformer_amd, POOLS[mode])


def _batch_of(case):
    return torch.repeat_interleave(torch.arange(len(case["lengths"])), torch.tensor(case["lengths"]))


# ---- header and library -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from difformer_amd import _lib
    return _lib.load_readout()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(lib):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.READOUT_SIGNATURES) == NAMES
    for name in declared:
        assert getattr(lib, name) is not None
    others = (set(_lib.SIGNATURES) | set(_lib.MAPS_SIGNATURES) | set(_lib.EDGES_SIGNATURES) | set(_lib.KNN_SIGNATURES)
              | set(_lib.SLOTS_SIGNATURES) | set(_lib.METRICS_SIGNATURES) | set(_lib.LOSS_SIGNATURES) | set(_lib.ADAM_SIGNATURES))
    assert not set(_lib.READOUT_SIGNATURES) & others
    for sfx in ("f32", "bf16"):
        assert len(_lib.READOUT_SIGNATURES["dif_readout_fwd_" + sfx][1]) == len(FWD)
        assert len(_lib.READOUT_SIGNATURES["dif_readout_bwd_" + sfx][1]) == len(BWD)
    assert _lib.READOUT_SIGNATURES["dif_readout_last_error"][0] is ctypes.c_char_p
    assert lib.dif_readout_version() == _lib.READOUT_VERSION == 1
    assert _lib.READOUT_CONSTANTS == dict(DIF_READOUT_ADD=0, DIF_READOUT_MEAN=1, DIF_READOUT_MAX=2, DIF_READOUT_MAX_COLUMNS=1024)
    assert '#include "difformer_hip.h"' in open(HEADER).read()


def test_rejected_shapes_and_empty_batches_return_before_any_launch(lib):
    """The argument checks are host arithmetic: they run here, with null operands."""
    from difformer_amd import _lib
    shape, badarg = _lib.ERROR_CODES["DIF_E_SHAPE"], _lib.ERROR_CODES["DIF_E_BADARG"]
    for sfx in ("f32", "bf16"):
        fwd, bwd = getattr(lib, "dif_readout_fwd_" + sfx), getattr(lib, "dif_readout_bwd_" + sfx)
        for H in (0, 1025, -3):
            assert fwd(None, H, None, 3, 7, H, 0, None, H, None) == shape
            assert bwd(None, H, None, H, None, H, None, 3, 7, H, 0, None, H, None) == shape
        assert b"H" in lib.dif_readout_last_error()
        assert fwd(None, 4, None, -1, 7, 4, 0, None, 4, None) == badarg
        assert fwd(None, 4, None, 3, 2 ** 31, 4, 0, None, 4, None) == badarg
        assert fwd(None, 4, None, 3, 7, 4, 3, None, 4, None) == badarg               # no such mode
        assert fwd(None, 4, None, 3, 7, 4, 0, None, 4, None) == badarg               # null operands
        assert fwd(None, 4, None, 0, 0, 4, 1, None, 4, None) == 0                    # no graphs: nothing to write
        assert bwd(None, 0, None, 0, None, 4, None, 0, 0, 4, 2, None, 4, None) == 0
        assert bwd(None, 0, None, 0, None, 4, None, 5, 0, 4, 2, None, 4, None) == 0  # graphs without rows: no gradient rows


def test_nothing_is_loaded_at_import():
    import subprocess
    import sys
    code = ("import difformer_amd, difformer_amd._lib as l; "
            "assert l._readout is None and l._lib is None; print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def _scatter_float64(x, batch, B, mode, g):
    """torch's scatter expression of the pool in float64 and its autograd gradient."""
    x = torch.from_numpy(np.asarray(x, dtype=np.float64)).requires_grad_()
    H = x.shape[1]
    zeros = torch.zeros((B, H), dtype=torch.float64)
    if mode == "max":
        out = zeros.scatter_reduce(0, batch[:, None].expand(-1, H), x, "amax", include_self=False)
    else:
        out = zeros.index_add(0, batch, x)
        if mode == "mean":
            out = out / torch.bincount(batch, minlength=B).clamp(min=1)[:, None]
    out.backward(torch.from_numpy(np.asarray(g, dtype=np.float64)))
    return out.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("name", [n for n in rr.cases() if not n.startswith(("many/H300", "long/H1024"))])
def test_oracle_equals_torch_autograd_of_the_scatter_expression_in_float64(name):
    """Forward within length * 2^-53 * sum |x| (over length for mean) + 2^-52 |ref|, gradient within 2^-52 |ref|; `max` exactly,
    planted ties included: torch's amax splits the gradient evenly among them."""
    case = rr.cases()[name]
    batch, B = _batch_of(case), len(case["lengths"])
    for bf16 in (False, True):
        x, g = (case["xb"], case["gb"]) if bf16 else (case["x32"], case["g32"])
        for mode in rr.MODES:
            ref_out, ref_gx = rr.evaluate(name, bf16)[mode]
            out, gx = _scatter_float64(x, batch, B, mode, g)
            if mode == "max":
                assert np.array_equal(out, ref_out.astype(np.float64))
            else:
                n = np.asarray(case["lengths"], dtype=np.float64)[:, None]
                slack = n * 2.0 ** -53 * rr.sum_abs(x, case["ptr"]) / (np.maximum(n, 1) if mode == "mean" else 1)
                assert (np.abs(out - ref_out) <= slack + 2.0 ** -52 * np.abs(ref_out)).all(), (name, mode)
            assert (np.abs(gx - ref_gx) <= 2.0 ** -52 * np.abs(ref_gx)).all(), (name, mode)
            empty = np.flatnonzero(np.asarray(case["lengths"]) == 0)
            assert not out[empty].any() and not np.signbit(out[empty]).any()          # +0 for empty graphs


def test_oracle_nan_and_tie_rules():
    x = np.array([[1.0, np.nan, 5.0], [3.0, 2.0, 5.0], [3.0, 0.0, -1.0], [7.0, 7.0, 7.0]])
    ptr = np.array([0, 3, 3, 4], dtype=np.int32)
    out = rr.forward(x, ptr, "max")
    assert out[0, 0] == 3 and np.isnan(out[0, 1]) and out[0, 2] == 5 and not out[1].any() and (out[2] == 7).all()
    g = np.array([[6.0, 6.0, 6.0], [9.0, 9.0, 9.0], [1.0, 2.0, 3.0]])
    gx = rr.backward(x, ptr, "max", g)
    assert np.array_equal(gx, [[0, 0, 3], [3, 0, 3], [3, 0, 0], [1, 2, 3]])          # two ties each; the NaN column gets nothing
    assert np.array_equal(rr.backward(x, ptr, "mean", g)[:3], np.full((3, 3), 2.0))
    assert np.array_equal(rr.forward(x[:, [0, 2]], ptr, "mean"), [[7 / np.longdouble(3), 3], [0, 0], [7, 7]])
    assert rr.ulp(1.0) == 2.0 ** -23 and rr.ulp(1.999, True) == 2.0 ** -7 and rr.ulp(0.0) == 2.0 ** -149 and rr.ulp(0.0, True) == 2.0 ** -133


# ---- the case table -------------------------------------------------------------------------------------------------------------------
def test_the_case_table_is_well_posed():
    """What tests/test_gpu_readout.py relies on, shown on the CPU:
      * the layout's boundaries are all there (column counts, lengths, empty graphs first / last / adjacent, > 256 graphs);
      * add / mean: the float64-summation allowance length * 2^-53 * sum |x| is below 2^-8 of HALF a float32 ulp of the column's
        largest element, so the bound is one rounding of the result and little else -- a float32 accumulation misses it;
      * max: every column of every graph has exactly one maximal row, or exactly the planted number."""
    table = rr.cases()
    assert {c["H"] for c in table.values()} == set(rr.COLUMNS)
    seen = set()
    for c in table.values():
        seen |= set(c["lengths"])
    assert seen == set(rr.LENGTHS)
    assert max(len(c["lengths"]) for c in table.values()) == 257 and {1, 3} <= {len(c["lengths"]) for c in table.values()}
    firsts = [c["lengths"] for c in table.values() if len(c["lengths"]) > 1]
    assert any(l[0] == 0 for l in firsts) and any(l[-1] == 0 for l in firsts)
    assert any(a == 0 and b == 0 for l in firsts for a, b in zip(l, l[1:]))
    assert table["long/H1024"]["x32"].shape == (1025, 1024)
    assert max(c["x32"].size for n, c in table.items() if n != "long/H1024") < 257 * 65 * 300
    for name, c in table.items():
        ptr = c["ptr"]
        planted = {(b, col): len(rows) for b, col, rows in c["plant"]}
        for key in ("x32", "xb"):
            x = c[key].astype(np.float64)
            if key == "xb":
                assert np.array_equal(rr._to_bf16(c[key]), c[key]), name                       # bfloat16-exact
            for b, n in enumerate(c["lengths"]):
                if not n:
                    continue
                rows = x[ptr[b]:ptr[b + 1]]
                slack = n * 2.0 ** -53 * np.abs(rows).sum(axis=0)
                assert (slack <= 2.0 ** -8 * 0.5 * rr.ulp(np.abs(rows).max(axis=0))).all(), (name, b)
                ties = (rows == rows.max(axis=0)).sum(axis=0)
                want = np.ones(c["H"], dtype=np.int64)
                for (pb, col), k in planted.items():
                    if pb == b:
                        want[col] = k
                assert np.array_equal(ties, want), (name, key, b)
    # planted ties reach 2 and 3 rows, within a row phase and across two
    c = table["ties/H64"]
    assert rr.phases(64) == (64, 4) and rr.phases(300) == (256, 1) and rr.phases(1) == (1, 256) and rr.phases(1024) == (256, 1)
    assert {len(rows) for _, _, rows in c["plant"]} == {2, 3}
    assert any(len({r % 4 for r in rows}) == 1 for _, _, rows in c["plant"]) and any(len({r % 4 for r in rows}) > 1 for _, _, rows in c["plant"])
    # a float32 accumulation of the long case does miss the bound: the bound constrains the arithmetic
    c = table["long/H65"]
    acc = np.zeros(65, dtype=np.float32)
    for row in c["x32"][:1025]:
        acc = acc + row
    ref = rr.evaluate("long/H65")["add"][0][0]
    assert (np.abs(acc - ref) > rr.forward_bound(ref, c, "add")[0]).any()


# ---- the CPU-tensor path ----------------------------------------------------------------------------------------------------------------
HOST_CASES = ["triple/H1", "triple/H63", "triple/H65", "triple/H257", "single/H64", "many/H64", "ties/H64", "ties/H300", "ties/H1"]


@pytest.mark.parametrize("name", HOST_CASES)
@pytest.mark.parametrize("mode", rr.MODES)
def test_cpu_tensors_equal_the_oracle_in_both_call_forms(name, mode):
    """float64 CPU tensors take the tensor expression: forward within length * 2^-53 * sum |x| + 2^-52 |ref|, gradient within
    2^-52 |ref|; `batch` and `n_nodes` give the same bits; empty graphs are +0."""
    case = rr.cases()[name]
    ref_out, ref_gx = rr.evaluate(name)[mode]
    pool = _pool(mode)
    B = len(case["lengths"])
    results = []
    for form in ("batch", "n_nodes", "n_nodes list"):
        x = torch.from_numpy(case["x32"]).double().requires_grad_()
        if form == "batch":
            out = pool(x, _batch_of(case), B)                      # (size: trailing empty graphs are not in `batch`)
        elif form == "n_nodes":
            out = pool(x, n_nodes=torch.tensor(case["lengths"]))
        else:
            out = pool(x, n_nodes=case["lengths"])
        out.backward(torch.from_numpy(case["g32"]).double())
        results.append((out.detach().numpy(), x.grad.numpy()))
    out, gx = results[0]
    for other in results[1:]:
        assert np.array_equal(out, other[0], equal_nan=True) and np.array_equal(gx, other[1])
    assert out.shape == (B, case["H"])
    n = np.asarray(case["lengths"], dtype=np.float64)[:, None]
    slack = n * 2.0 ** -53 * rr.sum_abs(case["x32"], case["ptr"]) / (np.maximum(n, 1) if mode == "mean" else 1)
    assert (np.abs(out - ref_out) <= (0 if mode == "max" else slack + 2.0 ** -52 * np.abs(ref_out))).all()
    assert (np.abs(gx - ref_gx) <= 2.0 ** -52 * np.abs(ref_gx)).all()
    empty = np.flatnonzero(np.asarray(case["lengths"]) == 0)
    assert not out[empty].any() and not np.signbit(out[empty]).any()


@pytest.mark.parametrize("mode", rr.MODES)
def test_an_unsorted_batch_is_still_correct(mode):
    case = rr.cases()["triple/H65"]
    ref_out, ref_gx = rr.evaluate("triple/H65")[mode]
    perm = torch.from_numpy(np.random.default_rng(3).permutation(case["x32"].shape[0]))
    batch = _batch_of(case)[perm]
    assert (batch[1:] < batch[:-1]).any()
    x = torch.from_numpy(case["x32"]).double()[perm].requires_grad_()
    out = _pool(mode)(x, batch, len(case["lengths"]))
    out.backward(torch.from_numpy(case["g32"]).double())
    assert (np.abs(out.detach().numpy() - ref_out) <= 2.0 ** -40 * (1 + np.abs(ref_out))).all()
    assert (np.abs(x.grad.numpy() - ref_gx[perm.numpy()]) <= 2.0 ** -52 * np.abs(ref_gx[perm.numpy()])).all()


def test_size_is_inferred_and_float32_and_half_run_too():
    import difformer_amd
    x = torch.arange(12.0).reshape(6, 2)
    batch = torch.tensor([0, 0, 2, 2, 2, 3])
    out = difformer_amd.global_add_pool(x, batch)
    assert out.shape == (4, 2) and out.tolist() == [[2, 4], [0, 0], [18, 21], [10, 11]]
    assert difformer_amd.global_mean_pool(x, batch, 6).shape == (6, 2)
    assert difformer_amd.global_max_pool(x.half(), batch).tolist() == [[2, 3], [0, 0], [8, 9], [10, 11]]
    assert difformer_amd.global_mean_pool(x[:0], batch[:0]).shape == (0, 2)
    assert difformer_amd.global_mean_pool(x[:0], n_nodes=[0, 0]).tolist() == [[0, 0], [0, 0]]


def test_argument_errors():
    import difformer_amd
    x = torch.zeros(5, 3)
    batch = torch.tensor([0, 0, 1, 1, 1])
    with pytest.raises(ValueError, match="exactly one"):
        difformer_amd.global_add_pool(x)
    with pytest.raises(ValueError, match="exactly one"):
        difformer_amd.global_add_pool(x, batch, n_nodes=[2, 3])
    with pytest.raises(ValueError, match="x has 5 rows"):
        difformer_amd.global_mean_pool(x, n_nodes=[2, 2])
    with pytest.raises(ValueError, match="int64"):
        difformer_amd.global_max_pool(x, batch.int())
    with pytest.raises(ValueError, match="int64"):
        difformer_amd.global_max_pool(x, batch[:4])
    with pytest.raises(ValueError, match="size = 1"):
        difformer_amd.global_max_pool(x, batch, 1)
    with pytest.raises(ValueError, match=r"\[N, H\]"):
        difformer_amd.global_add_pool(x[0], batch)


# ---- GraphGNN -------------------------------------------------------------------------------------------------------------------------------
class _NodeModel(torch.nn.Module):
    """Stands in for DIFFormer_v2 on the CPU: the same call, one Linear."""

    def __init__(self, f_in, hidden):
        super().__init__()
        self.fc = torch.nn.Linear(f_in, hidden)
        self.calls = []

    def reset_parameters(self):
        self.fc.reset_parameters()

    def forward(self, x, edge_index, n_nodes):
        self.calls.append((edge_index, n_nodes))
        return torch.tanh(self.fc(x))


def test_graphgnn_state_dict_keys_are_the_references():
    import difformer_amd
    gnn = difformer_amd.DIFFormer_v2(7, 16, 16, num_layers=2)
    model = difformer_amd.GraphGNN(16, 3, gnn, "max")
    assert set(model.state_dict()) == {"gnn_node." + k for k in gnn.state_dict()} | {"lin.weight", "lin.bias"}
    assert model.gnn_node is gnn and isinstance(model.lin, torch.nn.Linear) and tuple(model.lin.weight.shape) == (3, 16)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    torch.manual_seed(5)
    model.reset_parameters()                                        # models.py:34-36: lin and the node model
    after = model.state_dict()
    assert not torch.equal(before["lin.weight"], after["lin.weight"]) and not torch.equal(before["gnn_node.fcs.0.weight"], after["gnn_node.fcs.0.weight"])
    assert {"GraphGNN", "global_add_pool", "global_mean_pool", "global_max_pool"} <= set(difformer_amd.__all__)
    assert set(difformer_amd.readout.__all__) == {"GraphGNN", "global_add_pool", "global_mean_pool", "global_max_pool"}


@pytest.mark.parametrize("pooling,mode", [("sum", "add"), ("mean", "mean"), ("max", "max")])
def test_graphgnn_both_call_forms(pooling, mode):
    import difformer_amd
    torch.manual_seed(1)
    lengths = [3, 0, 5, 1]
    x = torch.randn(9, 4, dtype=torch.float64)
    ei = torch.tensor([[0, 1], [1, 0]])
    n_nodes = torch.tensor(lengths)
    model = difformer_amd.GraphGNN(6, 2, _NodeModel(4, 6), pooling).double()
    want = model.lin(_pool(mode)(torch.tanh(model.gnn_node.fc(x)), n_nodes=n_nodes))
    a = model(x, ei, n_nodes)                                                        # main.py:85
    b = model(types.SimpleNamespace(x=x, edge_index=ei, n_nodes=n_nodes))            # models.py:28
    batch = torch.repeat_interleave(torch.arange(4), n_nodes)
    c = model(types.SimpleNamespace(x=x, edge_index=ei, batch=batch))                # ... with torch_geometric's batch vector
    assert a.shape == (4, 2) and torch.equal(a, want) and torch.equal(b, want)
    assert torch.equal(c[[0, 2, 3]], want[[0, 2, 3]]) and torch.equal(c[1], want[1])
    assert all(e is ei for e, _ in model.gnn_node.calls[-3:])
    assert model.gnn_node.calls[-1][1].tolist() == lengths
    a.sum().backward()
    assert model.gnn_node.fc.weight.grad is not None and model.lin.weight.grad is not None
    with pytest.raises(ValueError, match="sorted"):
        model(types.SimpleNamespace(x=x, edge_index=ei, batch=batch.flip(0)))
    with pytest.raises(ValueError, match="n_nodes"):
        model(x, ei)


def test_graphgnn_rejects_an_unknown_pooling():
    import difformer_amd
    for bad in ("avg", "add", None, ""):
        with pytest.raises(ValueError, match="graph_pooling"):
            difformer_amd.GraphGNN(4, 1, _NodeModel(4, 4), bad)
