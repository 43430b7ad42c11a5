"""difformer_amd.Adam without a GPU: the long-double oracle pinned to torch.optim.Adam in float64, the eighth library's header and
argument checks, the CPU-parameter path, the argument errors, and -- with a backend that applies the oracle -- what step() hands
to the kernel and the version counters it bumps."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import adam_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_adam.h")
NAMES = ["dif_adam_last_error", "dif_adam_launches", "dif_adam_step_f32", "dif_adam_version"]


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("wd", [0.0, 5e-4])
def test_oracle_equals_torch_adam_in_float64_over_five_steps(t0, wd):
    """rtol 1e-11 on p, exp_avg and exp_avg_sq after each of 5 steps: float64 rounding (2^-53 = 1.1e-16) amplified by at most
    2^10 where 1 - beta2^t cancels at beta2 = 0.999 is 1.1e-13 per step; derived, not tuned.  The oracle's state is rounded to
    float64 between the steps, as torch's is."""
    rng = np.random.default_rng(5)
    n = 257
    p0 = rng.standard_normal(n)
    m0 = rng.standard_normal(n) * 0.05 if t0 else np.zeros(n)
    v0 = rng.uniform(0.2, 2.0, n) * 0.01 if t0 else np.zeros(n)
    grads = [10.0 ** rng.uniform(-6, 2, n) * rng.choice([-1.0, 1.0], n) for _ in range(5)]
    prm = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([prm], lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=wd)
    if t0:
        opt.state[prm] = dict(step=torch.tensor(float(t0)), exp_avg=torch.from_numpy(m0.copy()), exp_avg_sq=torch.from_numpy(v0.copy()))
    p, m, v = p0, m0, v0
    worst = 0.0
    for k, g in enumerate(grads):
        prm.grad = torch.from_numpy(g.copy())
        opt.step()
        p, m, v = (a.astype(np.float64) for a in adam_ref.step(p, g, m, v, t0 + k + 1, 1e-3, 0.9, 0.999, 1e-8, wd))
        st = opt.state[prm]
        for got, ref in ((prm.detach().numpy(), p), (st["exp_avg"].numpy(), m), (st["exp_avg_sq"].numpy(), v)):
            worst = max(worst, float(np.max(np.abs(got - ref) / np.abs(ref))))
        assert float(st["step"]) == t0 + k + 1
    print(f"oracle vs torch float64, t0={t0}, wd={wd}: worst relative difference {worst:.3e}")
    assert worst <= 1e-11


def test_oracle_helpers_and_the_case_table():
    assert adam_ref.ulp32(1.0) == 2.0 ** -23 and adam_ref.ulp32(-3.0) == 2.0 ** -22 and adam_ref.ulp32(0.0) == 2.0 ** -149
    assert adam_ref.ulp32(1e-40) == 2.0 ** -149 and adam_ref.ulp32(np.longdouble(2) - np.longdouble(2) ** -40) == 2.0 ** -23
    table = adam_ref.cases()
    assert adam_ref.MAX_TENSORS >= 32
    sizes = {int(np.prod(t["shape"], dtype=np.int64)) for t in table["sizes/t1/wd0"]["tensors"]}
    assert {0, 1, 3, 4, 5, adam_ref.CHUNK - 1, adam_ref.CHUNK, adam_ref.CHUNK + 1} <= sizes
    assert any(t["shape"] == () for t in table["sizes/t1/wd0"]["tensors"])
    assert {c["tensors"][0]["t0"] + 1 for n, c in table.items() if n.startswith("sizes/")} == {1, 2, 1000}
    assert {c["hyper"]["wd"] for n, c in table.items() if n.startswith("sizes/")} == {0.0, 5e-4}
    assert len(table[f"many/{adam_ref.MAX_TENSORS}"]["tensors"]) == adam_ref.MAX_TENSORS
    assert len(table[f"many/{adam_ref.MAX_TENSORS + 1}"]["tensors"]) == adam_ref.MAX_TENSORS + 1
    assert all(1 <= t["p"].size <= 7 for t in table[f"many/{adam_ref.MAX_TENSORS + 1}"]["tensors"])
    mid = [t["g"] is None for t in table["no_grad_in_the_middle"]["tensors"]]
    assert mid[0] is False and mid[1] is True and mid[-1] is False
    wide = np.abs(table["magnitudes/t1/wd0"]["tensors"][0]["g"])
    assert wide.min() <= 1.0001e-12 and wide.max() >= 0.9999e4
    assert table["groups/a"]["hyper"] != table["groups/b"]["hyper"] and table["flat_grads"]["flat_grads"]
    for name in table:                                                      # every case is well-posed: finite results, v' >= 0
        for ref in adam_ref.evaluate(name):
            if ref is not None:
                assert all(np.isfinite(a).all() for a in ref) and (ref[2] >= 0).all() and all((b > 0).all() for b in ref[3:]), name


# ---- header and library -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from difformer_amd import _lib
    if not os.path.exists(_lib.ADAM_LIB_PATH):
        pytest.skip("libdifformer_adam.so is not built")
    return _lib.load_adam()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(lib):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.ADAM_SIGNATURES) == NAMES
    for name in declared:
        assert getattr(lib, name) is not None
    others = (set(_lib.SIGNATURES) | set(_lib.MAPS_SIGNATURES) | set(_lib.EDGES_SIGNATURES) | set(_lib.KNN_SIGNATURES)
              | set(_lib.SLOTS_SIGNATURES) | set(_lib.METRICS_SIGNATURES) | set(_lib.LOSS_SIGNATURES))
    assert not set(_lib.ADAM_SIGNATURES) & others
    vp, i64, dbl = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double
    assert _lib.ADAM_SIGNATURES["dif_adam_step_f32"] == (ctypes.c_int, [vp, i64, dbl, dbl, dbl, dbl, dbl, vp, vp])
    assert _lib.ADAM_SIGNATURES["dif_adam_last_error"][0] is ctypes.c_char_p
    assert lib.dif_adam_version() == _lib.ADAM_VERSION == 1
    c = _lib.ADAM_CONSTANTS
    assert set(c) == {"DIF_ADAM_MAX_TENSORS", "DIF_ADAM_CHUNK", "DIF_ADAM_TABLE_FIELDS", "DIF_ADAM_TICKET_BYTES"}
    assert c["DIF_ADAM_MAX_TENSORS"] >= 32 and c["DIF_ADAM_TICKET_BYTES"] == 4 * c["DIF_ADAM_MAX_TENSORS"] and c["DIF_ADAM_TABLE_FIELDS"] == 6
    assert c["DIF_ADAM_MAX_TENSORS"] == adam_ref.MAX_TENSORS and c["DIF_ADAM_CHUNK"] == adam_ref.CHUNK
    assert '#include "difformer_hip.h"' in open(HEADER).read()
    M = c["DIF_ADAM_MAX_TENSORS"]
    assert [lib.dif_adam_launches(k) for k in (0, 1, M, M + 1, 2 * M, 2 * M + 1)] == [0, 1, 1, 2, 2, 3]
    assert lib.dif_adam_launches(-1) == -1 and lib.dif_adam_launches((1 << 20) + 1) == -1


def test_every_argument_check_returns_its_code_without_a_gpu(lib):
    """Made-up (never dereferenced) addresses: every rejection happens before any HIP call."""
    from difformer_amd import _lib
    bad, rng = _lib.ERROR_CODES["DIF_E_BADARG"], _lib.ERROR_CODES["DIF_E_RANGE"]
    good = [0x10004, 0x20004, 0x30004, 0x40004, 0x50004, 100]

    def call(rows, count=None, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, tickets=0x60004):
        flat = [x for r in rows for x in r]
        arr = (ctypes.c_int64 * max(len(flat), 1))(*flat)
        return lib.dif_adam_step_f32(arr, len(rows) if count is None else count, lr, b1, b2, eps, wd, tickets, None)

    assert call([], count=-1) == bad and call([], count=(1 << 20) + 1) == bad
    assert lib.dif_adam_step_f32(None, 1, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0x60004, None) == bad
    assert call([good], tickets=None) == bad and call([good], tickets=0x60002) == bad
    for k in range(5):
        row = list(good)
        row[k] = None or 0
        assert call([good, row]) == bad and b"tensor 1" in lib.dif_adam_last_error(), k
        row[k] = good[k] + 2
        assert call([good, row]) == bad and b"aligned" in lib.dif_adam_last_error(), k
    assert call([good[:5] + [-1]]) == bad
    for over in (dict(lr=-1.0), dict(lr=float("nan")), dict(lr=float("inf")), dict(eps=-1e-8), dict(wd=-0.1), dict(wd=float("nan")),
                 dict(b1=1.0), dict(b1=-0.1), dict(b2=1.0), dict(b2=float("nan"))):
        assert call([good], **over) == bad, over
        assert b"dif_adam_step_f32" in lib.dif_adam_last_error()                # this library's text, not another's
    huge = good[:5] + [adam_ref.CHUNK * ((1 << 31) - 1) + 1]                      # 2^31 chunks in one launch
    assert call([huge]) == rng
    assert call([good[:5] + [adam_ref.CHUNK * ((1 << 30))], good[:5] + [adam_ref.CHUNK * ((1 << 30))]]) == rng
    assert call([], count=0) == 0                                                # nothing to do, nothing launched
    assert call([], count=0, tickets=None) == bad


# ---- the public class on CPU parameters ------------------------------------------------------------------------------------------
def _bitwise(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _mlp(seed):
    torch.manual_seed(seed)
    return torch.nn.Sequential(torch.nn.Linear(6, 5), torch.nn.Tanh(), torch.nn.Linear(5, 3))


def test_cpu_parameters_take_torchs_step_bitwise():
    import difformer_amd
    a, b = _mlp(3), _mlp(3)
    oa = difformer_amd.Adam([dict(params=a[0].parameters(), lr=3e-3, betas=(0.8, 0.99)), dict(params=a[2].parameters())],
                            lr=1e-2, weight_decay=5e-4)
    ob = torch.optim.Adam([dict(params=b[0].parameters(), lr=3e-3, betas=(0.8, 0.99)), dict(params=b[2].parameters())],
                          lr=1e-2, weight_decay=5e-4)
    assert isinstance(oa, torch.optim.Adam) and [g["capturable"] for g in oa.param_groups] == [False, False]
    x = torch.randn(9, 6)
    for k in range(3):
        for model, opt in ((a, oa), (b, ob)):
            opt.zero_grad(set_to_none=True)
            model(x).square().sum().backward()
            if k == 1:
                model[2].bias.grad = None                                      # a parameter without a gradient is skipped
            opt.step()
        assert all(_bitwise(p.detach(), q.detach()) for p, q in zip(a.parameters(), b.parameters())), k
    for p, q in zip(a.parameters(), b.parameters()):
        sa, sb = oa.state[p], ob.state[q]
        assert float(sa["step"]) == float(sb["step"]) and _bitwise(sa["exp_avg"], sb["exp_avg"]) and _bitwise(sa["exp_avg_sq"], sb["exp_avg_sq"])
    ob.load_state_dict(oa.state_dict())                                        # and the state dicts are interchangeable
    oa.load_state_dict(ob.state_dict())
    assert float(oa.step(lambda: torch.tensor(2.5))) == 2.5                    # a closure's value is returned


def test_every_argument_error_raises_without_a_device(monkeypatch):
    import difformer_amd
    w = torch.nn.Parameter(torch.zeros(4, 3))
    meta = torch.device("meta")                                                # not a CPU tensor, and never touched
    for bad in (dict(amsgrad=True), dict(maximize=True), dict(differentiable=True), dict(lr=torch.tensor(1e-3))):
        with pytest.raises(ValueError, match="difformer_amd.Adam"):
            difformer_amd.Adam([w], **bad)
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(ValueError, match="float32"):
            difformer_amd.Adam([torch.nn.Parameter(torch.zeros(3, dtype=dtype, device=meta))])
    with pytest.raises(ValueError, match="mixes"):
        difformer_amd.Adam([w, torch.nn.Parameter(torch.zeros(3, device=meta))])
    with pytest.raises(ValueError, match="learning rate"):                              # torch's own range checks are still there
        difformer_amd.Adam([w], lr=-1.0)
    opt = difformer_amd.Adam([w])
    with pytest.raises(ValueError, match="float32"):
        opt.add_param_group(dict(params=[torch.nn.Parameter(torch.zeros(3, dtype=torch.float64, device=meta))]))
    assert len(opt.param_groups) == 1
    # options switched on later, in param_groups: caught at the step
    w.grad = torch.ones(4, 3)
    for key, value in (("amsgrad", True), ("maximize", True), ("lr", torch.tensor(1e-3)), ("decoupled_weight_decay", True)):
        opt = difformer_amd.Adam([w])
        opt.param_groups[0][key] = value
        with pytest.raises(ValueError, match="difformer_amd.Adam"):
            opt.step()
    assert torch.equal(w.detach(), torch.zeros(4, 3))
    # a sparse gradient of a "device" parameter (a CPU tensor standing in: the error comes before any backend is asked for)
    from difformer_amd import ops, optim
    monkeypatch.setattr(ops, "_BACKEND", None)
    monkeypatch.setattr(ops, "get_backend", lambda: pytest.fail("the backend was reached"))
    monkeypatch.setattr(optim, "_on_device", lambda t: True)
    d = torch.nn.Parameter(torch.zeros(4, 3))
    opt = difformer_amd.Adam([w, d])
    assert opt.param_groups[0]["capturable"] is True
    d.grad = torch.zeros(4, 3).to_sparse()
    with pytest.raises(ValueError, match="sparse"):
        opt.step()
    assert not opt.state[w] and not opt.state[d]                               # nothing was allocated, for either


# ---- what step() hands to the kernel -------------------------------------------------------------------------------------------------
class _OracleBackend:
    """adam_step of backend_hip.HipBackend on CPU tensors: the oracle, rounded once to float32."""

    def __init__(self):
        self.calls = []

    def adam_step(self, params, grads, exp_avgs, exp_avg_sqs, steps, lr, beta1, beta2, eps, weight_decay):
        self.calls.append(dict(params=list(params), numel=[p.numel() for p in params], grads=[g.clone() for g in grads],
                               hyper=(lr, beta1, beta2, eps, weight_decay), contiguous=all(g.is_contiguous() for g in grads)))
        for p, g, m, v, t in zip(params, grads, exp_avgs, exp_avg_sqs, steps, strict=True):
            assert t.dtype == torch.float32 and t.dim() == 0 and m.shape == p.shape and v.shape == p.shape
            p2, m2, v2 = adam_ref.step(p.detach().numpy(), g.numpy(), m.numpy(), v.numpy(), float(t) + 1, lr, beta1, beta2, eps, weight_decay)
            # written through the storage, as the kernel does through raw pointers: no version counter moves here
            for dst, src in ((p, p2), (m, m2), (v, v2)):
                np.copyto(dst.detach().numpy(), src.astype(np.float32))
            np.copyto(t.numpy(), np.float32(float(t) + 1))


@pytest.fixture
def oracle_backend(monkeypatch):
    from difformer_amd import ops, optim
    be = _OracleBackend()
    monkeypatch.setattr(ops, "_BACKEND", be)
    monkeypatch.setattr(optim, "_on_device", lambda t: True)                   # CPU tensors stand in for device tensors
    return be


def test_step_hands_the_groups_to_the_backend_in_order_and_bumps_versions(oracle_backend):
    import difformer_amd
    model, twin = _mlp(7), _mlp(7)
    groups = lambda m: [dict(params=list(m[0].parameters()), lr=3e-3, betas=(0.8, 0.99)), dict(params=list(m[2].parameters()))]
    opt = difformer_amd.Adam(groups(model), lr=1e-2, weight_decay=5e-4)
    ref = torch.optim.Adam(groups(twin), lr=1e-2, weight_decay=5e-4)
    assert [g["capturable"] for g in opt.param_groups] == [True, True]
    x = torch.randn(9, 6)
    skipped = model[2].bias
    for k in range(3):
        for m, o in ((model, opt), (twin, ref)):
            o.zero_grad(set_to_none=True)
            m(x).square().sum().backward()
        if k == 1:
            model[0].weight.grad = model[0].weight.grad.t().contiguous().t()   # a non-contiguous gradient is made contiguous
            assert not model[0].weight.grad.is_contiguous()
        if k < 2:
            skipped.grad = twin[2].bias.grad = None
        before = {p: p._version for p in model.parameters()}
        kept = (skipped.detach().clone(), copy.deepcopy(opt.state.get(skipped, {})))
        grads = [p.grad.clone() if p.grad is not None else None for p in model.parameters()]
        del oracle_backend.calls[:]
        opt.step()
        ref.step()
        # one call per group, tensors in param_groups order with their sizes, the group's own hyper-parameters
        calls = oracle_backend.calls
        assert len(calls) == 2 and all(c["contiguous"] for c in calls)
        want0 = list(model[0].parameters())
        want1 = [p for p in model[2].parameters() if p.grad is not None]
        assert [id(p) for p in calls[0]["params"]] == [id(p) for p in want0] and calls[0]["numel"] == [30, 5]
        assert [id(p) for p in calls[1]["params"]] == [id(p) for p in want1] and calls[1]["numel"] == ([15] if k < 2 else [15, 3])
        assert calls[0]["hyper"] == (3e-3, 0.8, 0.99, 1e-8, 5e-4) and calls[1]["hyper"] == (1e-2, 0.9, 0.999, 1e-8, 5e-4)
        assert all(torch.equal(g, p.grad) for c in calls for g, p in zip(c["grads"], c["params"]))
        # gradients are read, never written
        assert all((g is None and p.grad is None) or torch.equal(g, p.grad) for g, p in zip(grads, model.parameters()))
        for p in model.parameters():
            if p is skipped and k < 2:                                           # no gradient: value, state and version stay
                assert p._version == before[p] and _bitwise(p.detach(), kept[0])
                assert (skipped in opt.state and bool(opt.state[skipped])) == bool(kept[1])
            else:
                assert p._version >= before[p] + 1, k
    # a sanity check of the whole path: close to torch's own float32 steps (update size 1e-2, three steps)
    for p, q in zip(model.parameters(), twin.parameters()):
        assert torch.allclose(p, q, rtol=0, atol=1e-5)
    assert float(opt.state[model[0].weight]["step"]) == 3 and float(opt.state[skipped]["step"]) == 1
    # hyper-parameters are read at every step
    opt.param_groups[1]["lr"] = 0.5
    model(x).square().sum().backward()
    del oracle_backend.calls[:]
    opt.step()
    assert oracle_backend.calls[1]["hyper"][0] == 0.5


def test_state_dict_round_trip_with_a_capturable_torch_adam(oracle_backend):
    import difformer_amd
    model, twin = _mlp(8), _mlp(8)
    opt = difformer_amd.Adam(model.parameters(), lr=1e-2)
    x = torch.randn(4, 6)
    for _ in range(2):
        opt.zero_grad()
        model(x).square().sum().backward()
        opt.step()
    sd = opt.state_dict()
    assert all(s["step"].dtype == torch.float32 and s["step"].dim() == 0 and float(s["step"]) == 2 for s in sd["state"].values())
    assert set(next(iter(sd["state"].values()))) == {"step", "exp_avg", "exp_avg_sq"} and sd["param_groups"][0]["capturable"] is True
    other = torch.optim.Adam(twin.parameters(), lr=1e-2, capturable=True)
    other.load_state_dict(sd)
    assert all(torch.is_tensor(s["step"]) and float(s["step"]) == 2 for s in other.state.values())
    back = difformer_amd.Adam(model.parameters(), lr=1e-2)
    back.load_state_dict(other.state_dict())
    for p in model.parameters():
        assert _bitwise(back.state[p]["exp_avg"], opt.state[p]["exp_avg"]) and float(back.state[p]["step"]) == 2
    # a state_dict of a plain torch.optim.Adam (host step counters, capturable=False) loads too
    plain = torch.optim.Adam(twin.parameters(), lr=1e-2)
    twin(x).square().sum().backward()
    plain.step()
    back.load_state_dict(plain.state_dict())
    assert back.param_groups[0]["capturable"] is True
    assert all(s["step"].dtype == torch.float32 and float(s["step"]) == 1 for s in back.state.values())


def test_the_package_exports_adam_and_the_makefile_builds_the_library():
    import difformer_amd
    assert "Adam" in difformer_amd.__all__ and issubclass(difformer_amd.Adam, torch.optim.Adam)
    make = open(os.path.join(ROOT, "difformer_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(ADAM_OUT\)", make, flags=re.M) and re.search(r"^\trm -rf .*\$\(ADAM_OUT\)", make, flags=re.M)
    assert "-Wl,-Bsymbolic $(ADAM_OBJS)" in make
    src = open(os.path.join(ROOT, "difformer_amd", "csrc", "adam.hip")).read()
    assert "dif::launch(" in src and "<<<" not in src and "hipLaunchKernelGGL" not in src and "hipFuncSetAttribute" not in src
