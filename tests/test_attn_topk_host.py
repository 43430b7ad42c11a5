"""Top-k attention maps without a GPU: the second library's header and argument checks, the float64 restatement pinned to the
reference's own tensors, the host logic on a numpy backend, and the generated code's resources."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err, split_model_case
from fake_backend import OracleBackend
import topk_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_maps.h")
SOURCE = os.path.join(ROOT, "difformer_amd", "csrc", "attn_topk.hip")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TOPK = load_golden("topk")


# ---- header and library ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def maps():
    from difformer_amd import _lib
    return _lib.load_maps()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(maps):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.MAPS_SIGNATURES) == ["dif_attn_topk_f32", "dif_attn_topk_splits", "dif_attn_topk_workspace_bytes",
                                                        "dif_maps_last_error", "dif_maps_version"]
    for name in declared:
        assert getattr(maps, name) is not None
    assert not set(_lib.MAPS_SIGNATURES) & set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 101
    assert _lib.MAPS_SIGNATURES["dif_attn_topk_workspace_bytes"][0] is ctypes.c_int64
    assert len(_lib.MAPS_SIGNATURES["dif_attn_topk_f32"][1]) == 15


def test_version_matches(maps):
    from difformer_amd import _lib
    assert maps.dif_maps_version() == _lib.MAPS_VERSION == 1


def _call(maps, **over):
    """dif_attn_topk_f32 with made-up (never dereferenced) addresses: every rejection happens before any HIP call."""
    a = dict(q=0x10000, ldq=64, k=0x20000, ldk=64, n_q=100, n_k=1000, H=1, M=64, mode=0, topk=8, values=0x30000, indices=0x40000,
             workspace=0x50000, workspace_bytes=1 << 40, stream=None)
    a.update(over)
    return maps.dif_attn_topk_f32(*[a[n] for n in ("q", "ldq", "k", "ldk", "n_q", "n_k", "H", "M", "mode", "topk", "values", "indices",
                                                    "workspace", "workspace_bytes", "stream")])


@pytest.mark.parametrize("over,code", [
    (dict(q=None), "DIF_E_BADARG"), (dict(k=None), "DIF_E_BADARG"), (dict(values=None), "DIF_E_BADARG"),
    (dict(indices=None), "DIF_E_BADARG"), (dict(workspace=None), "DIF_E_BADARG"),
    (dict(q=0x10004), "DIF_E_BADARG"), (dict(k=0x20008), "DIF_E_BADARG"), (dict(workspace=0x50004), "DIF_E_BADARG"),
    (dict(values=0x30002), "DIF_E_BADARG"), (dict(ldq=66), "DIF_E_BADARG"), (dict(ldk=32), "DIF_E_BADARG"),
    (dict(topk=0), "DIF_E_SHAPE"), (dict(topk=33), "DIF_E_SHAPE"), (dict(topk=9, n_k=8), "DIF_E_SHAPE"),
    (dict(M=62, ldq=64, ldk=64), "DIF_E_SHAPE"), (dict(M=516, ldq=516, ldk=516), "DIF_E_SHAPE"), (dict(mode=2), "DIF_E_SHAPE"),
    (dict(mode=-1), "DIF_E_SHAPE"),
    (dict(workspace_bytes=15), "DIF_E_WORKSPACE"),
    (dict(n_k=1 << 31), "DIF_E_RANGE"),
])
def test_every_argument_check_returns_its_code_without_a_gpu(maps, over, code):
    from difformer_amd import _lib
    rc = _call(maps, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, maps.dif_maps_last_error())
    assert b"dif_attn_topk_f32" in maps.dif_maps_last_error()


def test_short_workspace_is_one_byte_short(maps):
    from difformer_amd import _lib
    need = maps.dif_attn_topk_workspace_bytes(100, 1000, 1, 64, 8)
    assert _call(maps, workspace_bytes=need - 1) == _lib.ERROR_CODES["DIF_E_WORKSPACE"]


def test_workspace_and_splits_over_random_shapes(maps):
    rng = np.random.default_rng(0)
    seen = set()
    for _ in range(400):
        n_q, n_k = int(10 ** rng.uniform(0, 6)), int(10 ** rng.uniform(0, 6))
        H, M = int(rng.integers(1, 5)), 4 * int(rng.integers(1, 129))
        topk = int(rng.integers(1, min(n_k, 32) + 1))
        S = maps.dif_attn_topk_splits(n_q, n_k, H, M, topk)
        ws = maps.dif_attn_topk_workspace_bytes(n_q, n_k, H, M, topk)
        kmax = 8 if topk <= 8 else (16 if topk <= 16 else 32)
        assert 1 <= S <= 32 and S <= max(1, (n_k + 15) // 16)
        assert ws == S * n_q * H * (8 * kmax + 4) > 0
        seen.add(S > 1)
    assert seen == {True, False}
    assert maps.dif_attn_topk_splits(132534, 132534, 1, 64, 16) == 1


def test_the_package_exports_attention_topk():
    import difformer_amd
    from difformer_amd import difformer
    assert "attention_topk" in difformer_amd.__all__ and callable(difformer_amd.attention_topk)
    assert hasattr(difformer_amd.DIFFormer, "top_attentions") and "top_attentions" not in difformer.__all__


# ---- the float64 restatement is the reference's attention ---------------------------------------------------------------
@pytest.mark.parametrize("name", ["simple_n20", "sigmoid_n20"])
def test_helper_equals_topk_of_the_reference_dense_attention(golden, name):
    c = golden["attnw"][name]
    kernel = str(c["kernel"])
    for k in (1, 5, 20):
        want_v, want_i = topk_ref.topk_rows(c["attn_f64"], k)
        got_v, got_i = topk_ref.reference_topk(c["q"], c["k"], kernel, k)
        assert np.array_equal(got_i, want_i)
        assert rel_err(got_v, want_v) < 1e-12


@pytest.mark.parametrize("name", sorted(n for n in TOPK if n.startswith("attn/")))
def test_helper_equals_the_golden_topk(name):
    c = TOPK[name]
    k = c["values"].shape[-1]
    got_v, got_i = topk_ref.reference_topk(c["q"], c["k"], str(c["kernel"]), k)
    assert c["q"].shape[0] <= 300 and c["values"].dtype == np.float64
    assert np.array_equal(got_i, c["indices"])
    assert rel_err(got_v, c["values"]) < 1e-12


def test_criterion_discriminates():
    """A result that misses the last three keys of every row fails criterion 1; a float32 restatement passes."""
    rng = np.random.default_rng(1)
    q, k = rng.standard_normal((40, 1, 16)), rng.standard_normal((200, 1, 16))
    attn = topk_ref.dense_attention(q, k, "simple")
    v, i = topk_ref.topk_rows(attn, 11)
    topk_ref.check_topk(v[:, :, :8].astype(np.float32), i[:, :, :8], attn, 8)
    bad_v, bad_i = np.concatenate([v[:, :, :5], v[:, :, 8:]], axis=2), np.concatenate([i[:, :, :5], i[:, :, 8:]], axis=2)
    with pytest.raises(AssertionError):
        topk_ref.check_topk(bad_v, bad_i, attn, 8)
    dup = i[:, :, :8].copy()
    dup[:, :, 7] = dup[:, :, 6]
    with pytest.raises(AssertionError):
        topk_ref.check_topk(v[:, :, :8], dup, attn, 8)


# ---- host logic on a numpy backend --------------------------------------------------------------------------------------
class TopkBackend(OracleBackend):
    """OracleBackend with the contract of HipBackend.attn_topk: float32 operands, M % 4 == 0, mode 0 / 1."""

    def attn_topk(self, q, k, mode, topk):
        assert q.dtype == torch.float32 and k.dtype == torch.float32, "the backend takes float32 operands"
        assert q.shape[2] % 4 == 0 and q.shape[2] <= 512 and 1 <= topk <= min(32, k.shape[0]) and mode in (0, 1)
        self.topk_calls = getattr(self, "topk_calls", []) + [(tuple(q.shape), tuple(k.shape), mode, topk)]
        s = np.einsum("nhm,lhm->nlh", q.numpy().astype(np.float64), k.numpy().astype(np.float64))
        if mode == 0:
            v, i = topk_ref.topk_rows(s, topk)
        else:
            sig = 1.0 / (1.0 + np.exp(-s))
            v, i = topk_ref.topk_rows(sig / sig.sum(axis=1, keepdims=True), topk, rank=s)
        return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(i.astype(np.int32))


@pytest.fixture()
def topk_backend(monkeypatch):
    from difformer_amd import ops
    be = TopkBackend()
    monkeypatch.setattr(ops, "_BACKEND", be)
    ops.csr_cache.clear()
    yield be
    ops.csr_cache.clear()


def _operands(kernel, n, l, h, m, seed=0):
    g = torch.Generator().manual_seed(seed)
    scale = m ** -0.25 if kernel == "sigmoid" else 1.0
    return torch.randn(n, h, m, generator=g) * scale, torch.randn(l, h, m, generator=g) * scale


@pytest.mark.parametrize("kernel,n,l,h,m,k", [("simple", 37, 37, 2, 16, 8), ("simple", 30, 45, 1, 10, 32), ("simple", 9, 5, 3, 7, 5),
                                              ("sigmoid", 30, 45, 2, 16, 9), ("sigmoid", 20, 33, 1, 6, 1)])
def test_attention_topk_prescaling_and_padding(topk_backend, kernel, n, l, h, m, k):
    from difformer_amd import attention_topk
    q, kk = _operands(kernel, n, l, h, m)
    values, indices = attention_topk(q, kk, kernel, k)
    assert values.dtype == torch.float32 and indices.dtype == torch.int64 and values.shape == indices.shape == (n, h, k)
    assert not values.requires_grad
    (qs, ks, mode, topk), = topk_backend.topk_calls
    assert qs == (n, h, -(-m // 4) * 4) and ks == (l, h, -(-m // 4) * 4) and mode == (kernel == "sigmoid") and topk == k
    topk_ref.check_topk(values.numpy(), indices.numpy(), topk_ref.dense_attention(q.numpy(), kk.numpy(), kernel), k, kernel)


def test_attention_topk_golden_cases(topk_backend):
    from difformer_amd import attention_topk
    for name, c in TOPK.items():
        if not name.startswith("attn/"):
            continue
        k = c["values"].shape[-1]
        values, indices = attention_topk(torch.from_numpy(c["q"]), torch.from_numpy(c["k"]), str(c["kernel"]), k)
        assert rel_err(values.numpy(), c["values"]) <= topk_ref.TOL
        topk_ref.check_topk(values.numpy(), indices.numpy(), topk_ref.dense_attention(c["q"], c["k"], str(c["kernel"])), k, name)


def test_attention_topk_upcasts_bfloat16_storage(topk_backend):
    from difformer_amd import attention_topk
    for kernel in ("simple", "sigmoid"):
        q, kk = (t.bfloat16() for t in _operands(kernel, 25, 40, 2, 12, seed=3))
        values, indices = attention_topk(q, kk, kernel, 8)            # (TopkBackend asserts float32 operands)
        assert values.dtype == torch.float32
        attn = topk_ref.dense_attention(q.float().numpy(), kk.float().numpy(), kernel)
        topk_ref.check_topk(values.numpy(), indices.numpy(), attn, 8, kernel + " bf16")


def test_attention_topk_value_errors_name_the_limit(topk_backend):
    from difformer_amd import attention_topk
    q, kk = _operands("simple", 10, 40, 1, 8)
    with pytest.raises(ValueError, match="32"):
        attention_topk(q, kk, "simple", 33)
    with pytest.raises(ValueError, match="L = 5"):
        attention_topk(q, kk[:5], "simple", 6)
    with pytest.raises(ValueError, match="at least 1"):
        attention_topk(q, kk, "simple", 0)
    with pytest.raises(ValueError, match="unknown attention kernel"):
        attention_topk(q, kk, "softmax", 3)
    with pytest.raises(ValueError, match="512"):
        attention_topk(torch.zeros(4, 1, 516), torch.zeros(4, 1, 516), "simple", 2)
    assert not getattr(topk_backend, "topk_calls", [])


def _model(kernel, heads, hidden=16, f_in=6, layers=2, **kw):
    from difformer_amd import DIFFormer
    torch.manual_seed(0)
    return DIFFormer(f_in, hidden, 3, num_layers=layers, num_heads=heads, kernel=kernel, use_graph=False, **kw).eval()


@pytest.mark.parametrize("kernel,heads", [("simple", 1), ("sigmoid", 1), ("sigmoid", 2)])
def test_top_attentions_is_topk_of_get_attentions(topk_backend, kernel, heads):
    model = _model(kernel, heads)
    x = torch.randn(23, 6, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        dense = model.get_attentions(x).numpy().astype(np.float64)        # [layers, N, N, H]
    values, indices = model.top_attentions(x, 5)
    assert values.shape == indices.shape == (2, 23, heads, 5) and indices.dtype == torch.int64 and not values.requires_grad
    for layer in range(2):
        topk_ref.check_topk(values[layer].numpy(), indices[layer].numpy(), dense[layer], 5, f"{kernel} layer {layer}")


def test_top_attentions_golden_model(topk_backend):
    from difformer_amd import DIFFormer
    c = TOPK["model/a_h2_nograph"]
    cfg, sd = split_model_case(c)
    args = {k: (v if not isinstance(v, np.generic) else v.item()) for k, v in cfg.items()}
    args = {k: (str(v) if k == "kernel" else v) for k, v in args.items()}
    model = DIFFormer(int(args.pop("in_channels")), int(args.pop("hidden_channels")), int(args.pop("out_channels")), **args).eval()
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    k = c["values"].shape[-1]
    values, indices = model.top_attentions(torch.from_numpy(c["x"]), k)
    assert values.shape == c["values"].shape
    e1 = rel_err(values.numpy(), c["values"])
    print(f"golden model: values {e1:.2e}")
    assert e1 <= topk_ref.TOL
    srt = np.sort(indices.numpy(), axis=-1)
    assert (srt[..., 1:] != srt[..., :-1]).all() and srt.min() >= 0 and srt.max() < c["x"].shape[0]
    assert (indices.numpy() == c["indices"]).mean() > 0.99       # (float32 layers in front of the scores: a near-tie may swap)


def test_top_attentions_refuses_a_row_sharded_model(topk_backend):
    model = _model("simple", 1)
    model.set_row_shard(object())
    with pytest.raises(NotImplementedError, match="row-sharded"):
        model.top_attentions(torch.randn(8, 6), 2)


def test_top_attentions_of_a_host_model_goes_through_its_device_twin(topk_backend, monkeypatch):
    """The staged path with the "device" forced to the host for the model's own call (the twin then computes unstaged)."""
    from difformer_amd import staging
    model = _model("sigmoid", 2)
    x = torch.randn(19, 6, generator=torch.Generator().manual_seed(2))
    plain_v, plain_i = model.top_attentions(x, 4)
    assert "_staged" not in model.__dict__
    real = staging.staging_device
    monkeypatch.setattr(staging, "staging_device",
                        lambda module, tensors: torch.device("cpu") if module is model else real(module, tensors))
    staging.operands.clear()
    values, indices = model.top_attentions(x, 4)
    staging.operands.clear()
    assert "_staged" in model.__dict__ and model.__dict__["_staged"][0].module is not model
    assert torch.equal(values, plain_v) and torch.equal(indices, plain_i)


# ---- generated code -----------------------------------------------------------------------------------------------------
def test_no_spills_and_no_scratch_in_any_kernel(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not installed")
    p = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-S", "--cuda-device-only",
                        "-Rpass-analysis=kernel-resource-usage", SOURCE, "-o", str(tmp_path / "attn_topk.s")],
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
    kernels = {n: u for n, u in usage.items() if "attn_topk_" in n}
    assert len(kernels) == 18, sorted(kernels)
    for n, u in kernels.items():
        assert u == {"VGPRs Spill": 0, "SGPRs Spill": 0, "ScratchSize [bytes/lane]": 0}, (n, u)
    text = open(tmp_path / "attn_topk.s").read()
    assert "v_mfma_f32_16x16x4_f32" in text and "scratch_" not in text


# ---- coverage -----------------------------------------------------------------------------------------------------------
def test_every_kernel_of_the_maps_library_is_launched_by_the_gpu_tests():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_symbols as ks
    from difformer_amd import _lib
    launched, unlaunched, section = {}, [], "launched"
    for line in open(os.path.join(ROOT, "profiles", "r08_maps_kernel_coverage.txt")):
        line = line.rstrip("\n")
        if not line or line.startswith("#"):
            continue
        if line.strip() == "UNLAUNCHED":
            section = "unlaunched"
            continue
        count, name = line.split(None, 1)
        (unlaunched.append(name.strip()) if section == "unlaunched" else launched.__setitem__(name.strip(), int(count)))
    assert not unlaunched, unlaunched
    have = set(ks.kernels(_lib.MAPS_LIB_PATH))
    assert have and have == set(launched) and all(v > 0 for v in launched.values()), sorted(have ^ set(launched))
