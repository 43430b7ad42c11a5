"""Attention on graph edges without a GPU: the third library's header and argument checks, the float64 restatement pinned to
the reference's own tensors, the host logic on a numpy backend, and the generated code's resources."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import rel_err
from fake_backend import OracleBackend
import edges_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_edges.h")
SOURCE = os.path.join(ROOT, "difformer_amd", "csrc", "attn_edges.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
EDGE_ARGS = ("q", "ldq", "k", "ldk", "scale", "n_q", "n_k", "H", "M", "mode", "edge_index", "E", "out", "status", "stream")
MASS_ARGS = ("q", "ldq", "k", "ldk", "scale", "n_q", "n_k", "H", "M", "mode", "rowptr", "src", "nnz", "mass", "stream")


# ---- header and library ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edges():
    from difformer_amd import _lib
    return _lib.load_edges()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(edges):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.EDGES_SIGNATURES) == ["dif_edge_attn_f32", "dif_edge_attn_mass_f32", "dif_edges_last_error",
                                                         "dif_edges_version"]
    for name in declared:
        assert getattr(edges, name) is not None
    assert not set(_lib.EDGES_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.MAPS_SIGNATURES))
    assert len(_lib.EDGES_SIGNATURES["dif_edge_attn_f32"][1]) == len(EDGE_ARGS)
    assert len(_lib.EDGES_SIGNATURES["dif_edge_attn_mass_f32"][1]) == len(MASS_ARGS)
    assert _lib.EDGES_SIGNATURES["dif_edges_last_error"][0] is ctypes.c_char_p
    assert os.path.basename(_lib.EDGES_LIB_PATH) == "libdifformer_edges.so"


def test_version_matches(edges):
    from difformer_amd import _lib
    assert edges.dif_edges_version() == _lib.EDGES_VERSION == 1


def test_a_missing_library_is_an_import_error_with_build_instructions(monkeypatch, tmp_path):
    from difformer_amd import _lib
    monkeypatch.setattr(_lib, "_edges", None)
    monkeypatch.setattr(_lib, "EDGES_LIB_PATH", str(tmp_path / "libdifformer_edges.so"))
    with pytest.raises(ImportError, match="HIP extension not built.*no CPU / eager fallback"):
        _lib.load_edges()


def _edge_call(edges, **over):
    """dif_edge_attn_f32 with made-up (never dereferenced) addresses: every rejection happens before any HIP call."""
    a = dict(q=0x10000, ldq=64, k=0x20000, ldk=64, scale=0x30000, n_q=100, n_k=1000, H=1, M=64, mode=0, edge_index=0x40000, E=500,
             out=0x50000, status=0x60000, stream=None)
    a.update(over)
    return edges.dif_edge_attn_f32(*[a[n] for n in EDGE_ARGS])


def _mass_call(edges, **over):
    a = dict(q=0x10000, ldq=64, k=0x20000, ldk=64, scale=0x30000, n_q=100, n_k=1000, H=1, M=64, mode=0, rowptr=0x40000, src=0x50000,
             nnz=500, mass=0x60000, stream=None)
    a.update(over)
    return edges.dif_edge_attn_mass_f32(*[a[n] for n in MASS_ARGS])


SHARED_CHECKS = [
    (dict(q=None), "DIF_E_BADARG"), (dict(k=None), "DIF_E_BADARG"), (dict(q=0x10004), "DIF_E_BADARG"), (dict(k=0x20008), "DIF_E_BADARG"),
    (dict(scale=0x30002), "DIF_E_BADARG"), (dict(ldq=66), "DIF_E_BADARG"), (dict(ldk=32), "DIF_E_BADARG"),
    (dict(n_q=0), "DIF_E_BADARG"), (dict(H=0), "DIF_E_BADARG"),
    (dict(M=6, ldq=64, ldk=64), "DIF_E_SHAPE"), (dict(M=516, ldq=516, ldk=516), "DIF_E_SHAPE"), (dict(mode=2), "DIF_E_SHAPE"),
    (dict(mode=-1), "DIF_E_SHAPE"), (dict(H=65536, ldq=1 << 23, ldk=1 << 23), "DIF_E_RANGE"),
]


@pytest.mark.parametrize("over,code", SHARED_CHECKS + [
    (dict(edge_index=None), "DIF_E_BADARG"), (dict(out=None), "DIF_E_BADARG"), (dict(status=None), "DIF_E_BADARG"),
    (dict(edge_index=0x40004), "DIF_E_BADARG"), (dict(out=0x50002), "DIF_E_BADARG"),
    (dict(E=0), "DIF_E_RANGE"), (dict(E=-1), "DIF_E_RANGE"), (dict(E=1 << 31), "DIF_E_RANGE"),
])
def test_every_argument_check_of_the_edge_entry_returns_its_code_without_a_gpu(edges, over, code):
    from difformer_amd import _lib
    rc = _edge_call(edges, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, edges.dif_edges_last_error())
    assert b"dif_edge_attn_f32" in edges.dif_edges_last_error()


@pytest.mark.parametrize("over,code", SHARED_CHECKS + [
    (dict(rowptr=None), "DIF_E_BADARG"), (dict(src=None), "DIF_E_BADARG"), (dict(mass=None), "DIF_E_BADARG"),
    (dict(src=0x50002), "DIF_E_BADARG"), (dict(nnz=-1), "DIF_E_RANGE"), (dict(nnz=1 << 31), "DIF_E_RANGE"),
])
def test_every_argument_check_of_the_mass_entry_returns_its_code_without_a_gpu(edges, over, code):
    from difformer_amd import _lib
    rc = _mass_call(edges, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, edges.dif_edges_last_error())
    assert b"dif_edge_attn_mass_f32" in edges.dif_edges_last_error()


def test_the_package_exports_attention_on_edges():
    import difformer_amd
    from difformer_amd import difformer
    assert "attention_on_edges" in difformer_amd.__all__ and callable(difformer_amd.attention_on_edges)
    assert hasattr(difformer_amd.DIFFormer, "edge_attentions") and "edge_attentions" not in difformer.__all__


# ---- the float64 restatement is the reference's attention ---------------------------------------------------------------
def _n20_graph():
    """20 nodes: random edges, the pair (3 -> 7) three times, the self-loop (5, 5), node 11 without any edge."""
    rng = np.random.default_rng(4)
    nodes = np.delete(np.arange(20), 11)
    ei = np.stack([rng.choice(nodes, 60), rng.choice(nodes, 60)])
    ei[:, 10] = ei[:, 20] = ei[:, 30] = (3, 7)
    ei[:, 40] = (5, 5)
    return ei.astype(np.int64)


@pytest.mark.parametrize("name", ["simple_n20", "sigmoid_n20"])
def test_helper_equals_the_reference_dense_attention_at_the_edges(golden, name):
    c = golden["attnw"][name]
    kernel, attn, ei = str(c["kernel"]), c["attn_f64"], _n20_graph()
    assert attn.shape[0] == 20 and 11 not in ei and (ei[0] == ei[1]).any()
    assert len({tuple(e) for e in ei.T}) < ei.shape[1]
    values = edges_ref.edge_values(c["q"], c["k"], kernel, ei)
    assert values.dtype == np.float64 and values.shape == (60, attn.shape[2])
    assert rel_err(values, attn[ei[1], ei[0]]) < 1e-12
    want = np.zeros((20, attn.shape[2]))
    for e in range(60):
        want[ei[1, e]] += attn[ei[1, e], ei[0, e]]
    mass = edges_ref.edge_mass(c["q"], c["k"], kernel, ei)
    assert rel_err(mass, want) < 1e-12 and (mass[11] == 0).all()
    # the entry points' own arithmetic restates the same numbers from (scale, mode)
    q, k = c["q"].astype(np.float64), c["k"].astype(np.float64)
    if kernel == "simple":
        inv = 1.0 / np.sqrt((q * q).sum() * (k * k).sum())
        scale, mode = inv / (np.einsum("nhm,hm->nh", q, k.sum(axis=0)) * inv + q.shape[0]), 0
    else:
        scale, mode = 1.0 / (1.0 / (1.0 + np.exp(-np.einsum("nhm,lhm->nlh", q, k)))).sum(axis=1), 1
    assert rel_err(edges_ref.raw_values(q, k, scale, mode, ei), values) < 1e-12
    assert rel_err(edges_ref.raw_mass(q, k, scale, mode, ei), mass) < 1e-12


def test_random_graph_has_what_the_gpu_tests_rely_on():
    for n_q, n_k, E in [(17, 33, 63), (100, 100, 257), (300, 1000, 4099)]:
        ei = edges_ref.random_graph(n_q, n_k, E, seed=1)
        assert ei.shape == (2, E) and ei.dtype == np.int64 and ei[0].max() < n_k and ei[1].max() < n_q and ei.min() >= 0
        assert len({tuple(e) for e in ei.T}) < E and (ei[0] == ei[1]).any() and n_q // 2 not in ei[1]
    ei = edges_ref.random_graph(300, 1000, 4999, seed=2, hubs=(4099, 300))
    assert sorted(np.bincount(ei[1], minlength=300))[-2:] >= [300, 4099]
    assert edges_ref.random_graph(1, 1, 1).tolist() == [[0], [0]]


# ---- host logic on a numpy backend --------------------------------------------------------------------------------------
class EdgesBackend(OracleBackend):
    """OracleBackend with the contract of HipBackend.edge_attention / edge_attention_mass / sigmoid_attention(want_den)."""

    def __init__(self):
        self.edge_calls, self.mass_calls, self.den_calls, self.csr_builds = [], [], 0, 0

    def sigmoid_attention(self, q, k, v, want_den=False):
        out = super().sigmoid_attention(q, k, v)
        if not want_den:
            return out
        self.den_calls += 1
        s = np.einsum("nhm,lhm->nlh", q.numpy().astype(np.float64), k.numpy().astype(np.float64))
        return out, torch.from_numpy((1.0 / (1.0 + np.exp(-s))).sum(axis=1).astype(np.float32))

    def csr_build(self, edge_index, edge_weight, num_nodes, *args, **kw):
        self.csr_builds += 1
        return super().csr_build(edge_index, edge_weight, num_nodes, *args, **kw)

    def _check(self, q, k, scale, mode):
        assert q.dtype == torch.float32 and k.dtype == torch.float32, "the backend takes float32 operands"
        assert q.shape[2] % 4 == 0 and q.shape[2] <= 512 and mode in (0, 1) and q.shape[1:] == k.shape[1:]
        assert scale is None or (scale.dtype == torch.float32 and tuple(scale.shape) == tuple(q.shape[:2]) and scale.is_contiguous())

    def edge_attention(self, q, k, scale, edge_index, mode):
        self._check(q, k, scale, mode)
        assert edge_index.dtype == torch.int64 and edge_index.shape[0] == 2 and edge_index.shape[1] >= 1
        self.edge_calls.append((tuple(q.shape), tuple(k.shape), mode))
        ei = edge_index.numpy()
        bad_key, bad_query = (ei[0] < 0) | (ei[0] >= k.shape[0]), (ei[1] < 0) | (ei[1] >= q.shape[0])
        safe = np.where(bad_key | bad_query, 0, ei)
        out = edges_ref.raw_values(q.numpy(), k.numpy(), None if scale is None else scale.numpy(), mode, safe)
        out[bad_key | bad_query] = np.nan
        status = [int((bad_key | bad_query).any()), int(bad_key.any()), int(bad_query.any())]
        return torch.from_numpy(out.astype(np.float32)), torch.tensor(status, dtype=torch.int32)

    def edge_attention_mass(self, q, k, scale, rowptr, src, mode):
        self._check(q, k, scale, mode)
        assert rowptr.dtype == torch.int32 and src.dtype == torch.int32 and rowptr.numel() >= q.shape[0] + 1
        self.mass_calls.append((tuple(q.shape), tuple(k.shape), mode))
        n = q.shape[0]
        rp = rowptr.numpy().astype(np.int64)[: n + 1]
        ei = np.stack([src.numpy().astype(np.int64)[: rp[-1]], np.repeat(np.arange(n), np.diff(rp))])
        mass = edges_ref.raw_mass(q.numpy(), k.numpy(), None if scale is None else scale.numpy(), mode, ei)
        return torch.from_numpy(mass.astype(np.float32))


@pytest.fixture()
def edges_backend(monkeypatch):
    from difformer_amd import ops
    be = EdgesBackend()
    monkeypatch.setattr(ops, "_BACKEND", be)
    ops.csr_cache.clear()
    yield be
    ops.csr_cache.clear()


def _operands(kernel, n, l, h, m, seed=0):
    g = torch.Generator().manual_seed(seed)
    scale = m ** -0.25 if kernel == "sigmoid" else 1.0
    return torch.randn(n, h, m, generator=g) * scale, torch.randn(l, h, m, generator=g) * scale


@pytest.mark.parametrize("kernel,n,l,h,m,E", [("simple", 37, 37, 2, 16, 150), ("simple", 30, 45, 1, 10, 77), ("simple", 9, 5, 3, 7, 20),
                                              ("sigmoid", 30, 45, 2, 16, 90), ("sigmoid", 20, 33, 1, 6, 41)])
def test_attention_on_edges_scale_operand_and_padding(edges_backend, kernel, n, l, h, m, E):
    from difformer_amd import attention_on_edges
    q, kk = _operands(kernel, n, l, h, m)
    ei = torch.from_numpy(edges_ref.random_graph(n, l, E, seed=3))
    values = attention_on_edges(q, kk, kernel, ei)
    assert torch.is_tensor(values) and values.dtype == torch.float32 and values.shape == (E, h) and not values.requires_grad
    values2, mass = attention_on_edges(q.requires_grad_(), kk, kernel, ei, mass=True)
    assert torch.equal(values, values2) and mass.shape == (n, h) and mass.dtype == torch.float32 and not mass.requires_grad
    pm = -(-m // 4) * 4
    assert edges_backend.edge_calls == [((n, h, pm), (l, h, pm), int(kernel == "sigmoid"))] * 2
    assert edges_backend.mass_calls == edges_backend.edge_calls[:1] and edges_backend.csr_builds == 1
    assert edges_backend.den_calls == (2 if kernel == "sigmoid" else 0)
    e1 = rel_err(values.numpy(), edges_ref.edge_values(q.detach().numpy(), kk.numpy(), kernel, ei.numpy()))
    e2 = rel_err(mass.numpy(), edges_ref.edge_mass(q.detach().numpy(), kk.numpy(), kernel, ei.numpy()))
    print(f"{kernel}: values {e1:.2e}, mass {e2:.2e}")
    assert e1 <= edges_ref.TOL and e2 <= edges_ref.TOL


def test_attention_on_edges_equals_the_dense_output_of_full_attention_conv(edges_backend):
    from difformer_amd import attention_on_edges
    from difformer_amd.difformer import _dense_attention
    for kernel, heads in (("simple", 1), ("sigmoid", 2)):           # (`simple` with several heads: the dense map cannot divide, :43)
        q, kk = _operands(kernel, 25, 31, heads, 8, seed=5)
        ei = torch.from_numpy(edges_ref.random_graph(25, 31, 64, seed=6))
        dense = _dense_attention(q, kk, kernel)                        # what output_attn=True returns next to the output
        assert rel_err(attention_on_edges(q, kk, kernel, ei).numpy(), dense[ei[1], ei[0], :].numpy()) <= edges_ref.TOL


def test_attention_on_edges_upcasts_bfloat16_storage(edges_backend):
    from difformer_amd import attention_on_edges
    for kernel in ("simple", "sigmoid"):
        q, kk = (t.bfloat16() for t in _operands(kernel, 25, 40, 2, 12, seed=3))
        ei = torch.from_numpy(edges_ref.random_graph(25, 40, 90, seed=7))
        values, mass = attention_on_edges(q, kk, kernel, ei, mass=True)          # (EdgesBackend asserts float32 operands)
        assert values.dtype == mass.dtype == torch.float32
        assert rel_err(values.numpy(), edges_ref.edge_values(q.float().numpy(), kk.float().numpy(), kernel, ei.numpy())) <= edges_ref.TOL
        assert rel_err(mass.numpy(), edges_ref.edge_mass(q.float().numpy(), kk.float().numpy(), kernel, ei.numpy())) <= edges_ref.TOL


def test_attention_on_edges_without_edges(edges_backend):
    from difformer_amd import attention_on_edges
    q, kk = _operands("simple", 10, 12, 2, 8)
    values, mass = attention_on_edges(q, kk, "simple", torch.zeros((2, 0), dtype=torch.int64), mass=True)
    assert values.shape == (0, 2) and mass.shape == (10, 2) and not mass.any() and not edges_backend.edge_calls


def test_attention_on_edges_argument_errors(edges_backend):
    from difformer_amd import attention_on_edges
    q, kk = _operands("simple", 10, 40, 1, 8)
    ei = torch.from_numpy(edges_ref.random_graph(10, 40, 30))
    with pytest.raises(ValueError, match="unknown attention kernel"):
        attention_on_edges(q, kk, "softmax", ei)
    with pytest.raises(ValueError, match=r"\(40, 1, 12\)"):
        attention_on_edges(q, torch.zeros(40, 1, 12), "simple", ei)
    with pytest.raises(ValueError, match=r"\[N,H,M\]"):
        attention_on_edges(q[:, 0], kk[:, 0], "simple", ei)
    with pytest.raises(ValueError, match="512"):
        attention_on_edges(torch.zeros(4, 1, 516), torch.zeros(4, 1, 516), "simple", ei)
    with pytest.raises(TypeError, match="int64"):
        attention_on_edges(q, kk, "simple", ei.int())
    with pytest.raises(TypeError, match=r"\[2, E\]"):
        attention_on_edges(q, kk, "simple", ei.t().contiguous())
    assert not edges_backend.edge_calls and not edges_backend.csr_builds


@pytest.mark.parametrize("mass", [False, True])
def test_a_bad_id_raises_index_error_naming_its_side(edges_backend, mass):
    from difformer_amd import attention_on_edges
    q, kk = _operands("sigmoid", 10, 40, 1, 8)
    ei = torch.from_numpy(edges_ref.random_graph(10, 40, 30))
    bad = ei.clone()
    bad[0, 4] = 40
    with pytest.raises(IndexError, match=r"source \(key\) ids outside \[0, 40\)$"):
        attention_on_edges(q, kk, "sigmoid", bad, mass)
    bad = ei.clone()
    bad[1, 9] = -1
    with pytest.raises(IndexError, match=r"edge_index holds target \(query\) ids outside \[0, 10\)$"):
        attention_on_edges(q, kk, "sigmoid", bad, mass)
    bad[0, 2] = 12345
    with pytest.raises(IndexError, match="source.*and target"):
        attention_on_edges(q, kk, "sigmoid", bad, mass)
    bad = ei.clone()
    bad[1, 0] = 25                                  # a key id that is no query id (L > N)
    with pytest.raises(IndexError, match="target"):
        attention_on_edges(q, kk, "sigmoid", bad, mass)
    assert not edges_backend.csr_builds


def _model(kernel, heads, hidden=16, f_in=6, layers=2, **kw):
    from difformer_amd import DIFFormer
    torch.manual_seed(0)
    return DIFFormer(f_in, hidden, 3, num_layers=layers, num_heads=heads, kernel=kernel, use_graph=False, **kw).eval()


@pytest.mark.parametrize("kernel,heads", [("simple", 1), ("sigmoid", 1), ("sigmoid", 2)])
def test_edge_attentions_is_get_attentions_at_the_edges(edges_backend, kernel, heads):
    model = _model(kernel, heads)
    x = torch.randn(23, 6, generator=torch.Generator().manual_seed(1))
    ei = torch.from_numpy(edges_ref.random_graph(23, 23, 70, seed=8))
    with torch.no_grad():
        dense = model.get_attentions(x).numpy().astype(np.float64)        # [layers, N, N, H]
    values = model.edge_attentions(x, ei)
    assert torch.is_tensor(values) and values.shape == (2, 70, heads) and values.dtype == torch.float32 and not values.requires_grad
    assert not edges_backend.csr_builds and not edges_backend.mass_calls
    values2, mass = model.edge_attentions(x, ei, mass=True)
    assert torch.equal(values, values2) and mass.shape == (2, 23, heads)
    assert edges_backend.csr_builds == 1 and len(edges_backend.mass_calls) == 2               # one CSR for both layers
    assert edges_backend.den_calls == (4 if kernel == "sigmoid" else 0)                       # one forward per sigmoid layer and call
    for layer in range(2):
        want = dense[layer][ei[1].numpy(), ei[0].numpy()]
        e1 = rel_err(values[layer].numpy(), want)
        e2 = rel_err(mass[layer].numpy(), edges_ref.sum_per_target(want, ei.numpy(), 23))
        print(f"{kernel} H={heads} layer {layer}: values {e1:.2e}, mass {e2:.2e}")
        assert e1 <= edges_ref.TOL and e2 <= edges_ref.TOL


def test_edge_attentions_refuses_a_row_sharded_model(edges_backend):
    model = _model("simple", 1)
    model.set_row_shard(object())
    with pytest.raises(NotImplementedError, match="row-sharded"):
        model.edge_attentions(torch.randn(8, 6), torch.zeros((2, 3), dtype=torch.int64))


def test_edge_attentions_of_a_host_model_goes_through_its_device_twin(edges_backend, monkeypatch):
    """The staged path with the "device" forced to the host for the model's own call (the twin then computes unstaged)."""
    from difformer_amd import staging
    model = _model("sigmoid", 2)
    x = torch.randn(19, 6, generator=torch.Generator().manual_seed(2))
    ei = torch.from_numpy(edges_ref.random_graph(19, 19, 50, seed=9))
    plain_v, plain_m = model.edge_attentions(x, ei, mass=True)
    assert "_staged" not in model.__dict__
    real = staging.staging_device
    monkeypatch.setattr(staging, "staging_device",
                        lambda module, tensors: torch.device("cpu") if module is model else real(module, tensors))
    staging.operands.clear()
    values, mass = model.edge_attentions(x, ei, mass=True)
    only_values = model.edge_attentions(x, ei)
    staging.operands.clear()
    assert "_staged" in model.__dict__ and model.__dict__["_staged"][0].module is not model
    assert torch.equal(values, plain_v) and torch.equal(mass, plain_m) and torch.equal(only_values, plain_v)


# ---- generated code -----------------------------------------------------------------------------------------------------
def test_no_spills_and_no_scratch_in_any_kernel(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", SOURCE, "-o", str(tmp_path / "attn_edges.s")],
                       stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    usage, name = {}, None
    for line in p.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
        m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
        if m and name:
            usage[name][m.group(1)] = int(m.group(2))
    kernels = {n: u for n, u in usage.items() if "edge_attn_kernel" in n or "edge_mass_kernel" in n}
    assert len(kernels) == len(usage) == 16, sorted(usage)           # 2 kernels x 4 lane-group widths x 2 modes, nothing else
    for n, u in kernels.items():
        assert u == {"VGPRs Spill": 0, "SGPRs Spill": 0, "ScratchSize [bytes/lane]": 0}, (n, u)


# ---- coverage -----------------------------------------------------------------------------------------------------------
def test_every_kernel_of_the_edges_library_is_launched_by_the_gpu_tests():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_symbols as ks
    from difformer_amd import _lib
    launched, unlaunched, section = {}, [], "launched"
    for line in open(os.path.join(ROOT, "profiles", "r10_edges_kernel_coverage.txt")):
        line = line.rstrip("\n")
        if not line or line.startswith("#"):
            continue
        if line.strip() == "UNLAUNCHED":
            section = "unlaunched"
            continue
        count, name = line.split(None, 1)
        (unlaunched.append(name.strip()) if section == "unlaunched" else launched.__setitem__(name.strip(), int(count)))
    assert not unlaunched, unlaunched
    have = set(ks.kernels(_lib.EDGES_LIB_PATH))
    assert len(have) == 16 and have == set(launched) and all(v > 0 for v in launched.values()), sorted(have ^ set(launched))
