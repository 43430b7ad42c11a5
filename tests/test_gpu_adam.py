"""The Adam update on the MI355X (csrc/adam.hip behind include/difformer_adam.h) and difformer_amd.Adam against the long-double
oracle of tests/adam_ref.py.

Bounds per element (adam_ref.bounds; one rounding to float32 of a float64 evaluation, not tuned):
    m', v'   |d| <= 1/2 ulp32(ref) + 2^-45 |ref|
    p'       |d| <= 1/2 ulp32(ref) + 2^-40 (|p| + |p - ref|)
Every tensor of a C-ABI call here starts one element past an aligned address (pointers are only promised aligned to their
element).  The case table (tests/adam_ref.py; tests/test_adam_host.py shows it well-posed): numel 0, 1, 3, 4, 5, chunk - 1 / + 0 /
+ 1 and a 0-d tensor; DIF_ADAM_MAX_TENSORS and one more tensors (one launch, two launches); gradients as views of a flat buffer; a
tensor without a gradient in the middle; t = 1, 2, 1,000; wd = 0 and 5e-4; two hyper-parameter sets; gradient magnitudes 1e-12 to
1e4 within one tensor.

Measured on the MI355X (profiles/r15_adam.md; test_zz_report_the_worst_cases prints them): worst p, exp_avg and exp_avg_sq
1.0000 x bound each (ties of the one rounding, never above 1).
"""
import copy
import ctypes
import gc

import numpy as np
import pytest
import torch

from guarded import GuardedArena
import adam_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {"p": 0.0, "m": 0.0, "v": 0.0}          # worst error / bound over everything held to the oracle, printed by the last test
GAP = {}                                        # measured against torch (state interchange), printed by the last test


@pytest.fixture(scope="module", autouse=True)
def leave_the_allocator_as_found():
    """torch keeps one BLAS workspace (214 MB here) per stream that ever ran one of its GEMMs, for the life of the process: the
    training steps below run them on the default stream and on the capture's side stream.  The peak-memory tests of the modules
    that run after this one count allocated bytes, so the workspaces are handed back when this module is done."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    getattr(torch._C, "_cuda_clearCublasWorkspaces", lambda: None)()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def lib():
    from difformer_amd import _lib
    return _lib.load_adam()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().copy()


def _run(lib, case, guarded=False):
    """One call of dif_adam_step_f32 on a case -> per tensor dict(p, m, v, step: numpy, bits of each, g_bits before/after)."""
    from difformer_amd import _lib
    arena = GuardedArena() if guarded else None

    def put(arr):
        t = torch.from_numpy(np.array(arr, dtype=np.float32, order="C"))      # (0-d stays 0-d)
        if arena is not None:
            d = arena.alloc(t.shape, torch.float32, DEV, offset_bytes=4)
        else:                                                   # one element past an aligned address
            d = torch.empty(t.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(t.shape)
        d.copy_(t)
        return d

    tensors = case["tensors"]
    flat = None
    if case["flat_grads"]:
        flat = put(np.concatenate([t["g"].ravel() for t in tensors if t["g"] is not None]))
    dev, rows, o = [], [], 0
    for t in tensors:
        d = dict(p=put(t["p"]), m=put(t["m"]), v=put(t["v"]), step=put(np.float32(t["t0"])), g=None)
        if t["g"] is not None:
            n = t["g"].size
            d["g"] = flat[o: o + n].view(t["shape"]) if flat is not None else put(t["g"])
            o += n if flat is not None else 0
            assert all(d[k].data_ptr() % 4 == 0 for k in "pmvg") and d["step"].dim() == 0
            rows += [d["p"].data_ptr(), d["g"].data_ptr(), d["m"].data_ptr(), d["v"].data_ptr(), d["step"].data_ptr(), n]
        dev.append(d)
    if case["flat_grads"]:
        assert any(d["g"] is not None and d["g"].data_ptr() % 16 for d in dev)       # views at 4-byte-only aligned offsets
    words = _lib.ADAM_CONSTANTS["DIF_ADAM_TICKET_BYTES"] // 4
    tickets = arena.alloc((words,), torch.int32, DEV, zero=True) if arena is not None else torch.zeros(words, dtype=torch.int32, device=DEV)
    before = [None if d["g"] is None else _bits(d["g"]) for d in dev]
    h = case["hyper"]
    table = (ctypes.c_int64 * max(len(rows), 1))(*rows)
    rc = lib.dif_adam_step_f32(table, len(rows) // 6, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"], tickets.data_ptr(), _stream())
    _lib.check_adam(rc, "dif_adam_step_f32")
    if arena is not None:
        arena.check()
    else:
        torch.cuda.synchronize()
    assert not tickets.cpu().any()                                                  # left all zero for the next call
    out = []
    for d, b in zip(dev, before):
        r = {k: d[k].detach().cpu().numpy() for k in ("p", "m", "v", "step")}
        r.update({k + "_bits": _bits(d[k]) for k in ("p", "m", "v", "step")})
        r["g_unchanged"] = b is None or bool((b == _bits(d["g"])).all())
        out.append(r)
    return out


def _hold(case, got, ref, name):
    """The bounds of the module docstring for every tensor with a gradient; the others bitwise as they were; step == t exactly."""
    for k, (ten, g, r) in enumerate(zip(case["tensors"], got, ref)):
        assert g["g_unchanged"], (name, k)
        if r is None:                                            # no gradient: not in the table, nothing moves
            for key in ("p", "m", "v"):
                assert (g[key + "_bits"] == np.ascontiguousarray(ten[key]).view(np.int32)).all(), (name, k, key)
            assert float(g["step"]) == ten["t0"], (name, k)
            continue
        ep, em, ev = adam_ref.worst_ratio(g["p"], g["m"], g["v"], r)
        for key, e in (("p", ep), ("m", em), ("v", ev)):
            WORST[key] = max(WORST[key], e)
        assert ep <= 1 and em <= 1 and ev <= 1, (name, k, ten["shape"], ep, em, ev)
        assert float(g["step"]) == ten["t0"] + 1, (name, k, float(g["step"]))


# ---- the C ABI against the oracle -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(adam_ref.cases()))
def test_every_case_is_within_one_rounding_of_the_oracle(lib, name):
    case = adam_ref.cases()[name]
    _hold(case, _run(lib, case), adam_ref.evaluate(name), name)


@pytest.mark.parametrize("name", list(adam_ref.cases()))
def test_every_case_between_guard_bands(lib, name):
    """p, grad, m, v, step and the tickets each between two checked bands of 0xFF: nothing outside the operands is written
    (_run checks the bands), and the results are those of the plain allocation, bitwise."""
    case = adam_ref.cases()[name]
    got = _run(lib, case, guarded=True)
    _hold(case, got, adam_ref.evaluate(name), name)
    plain = _run(lib, case)
    for a, b in zip(got, plain):
        assert all((a[k + "_bits"] == b[k + "_bits"]).all() for k in ("p", "m", "v", "step"))


def test_a_nan_and_an_infinite_gradient_stay_in_their_element(lib):
    base = adam_ref.cases()["magnitudes/t2/wd0.0005"]
    clean = _run(lib, base)
    case = copy.deepcopy(base)
    g = case["tensors"][0]["g"]
    hit = [7, adam_ref.CHUNK + 1]
    g[hit[0]], g[hit[1]] = np.nan, np.inf
    got = _run(lib, case)
    others = np.setdiff1d(np.arange(g.size), hit)
    for key in ("p", "m", "v"):
        assert not np.isfinite(got[0][key][hit]).any(), key
        assert (got[0][key + "_bits"][others] == clean[0][key + "_bits"][others]).all(), key
        assert (got[1][key + "_bits"] == clean[1][key + "_bits"]).all(), key
    assert float(got[0]["step"]) == 2 and float(got[1]["step"]) == 2


def test_the_same_step_twice_is_bitwise_equal(lib):
    for name in ("magnitudes/t2/wd0.0005", f"many/{adam_ref.MAX_TENSORS + 1}", "sizes/t1000/wd0.0005"):
        a, b = _run(lib, adam_ref.cases()[name]), _run(lib, adam_ref.cases()[name])
        for x, y in zip(a, b):
            assert all((x[k + "_bits"] == y[k + "_bits"]).all() for k in ("p", "m", "v", "step")), name


# ---- the public class -------------------------------------------------------------------------------------------------------------------
def _small_model(seed):
    from test_gpu_loss import _small_model as make               # 300 nodes, hidden 64, 2 layers, 7 classes
    return make(seed)


def _tiny_model(seed):
    """20 nodes, hidden 4: the whole-model kernels of tiny.py."""
    from difformer_amd import DIFFormer
    n, f_in, classes = 20, 14, 3
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, f_in, generator=g).to(DEV)
    pairs = torch.randint(0, n, (2, 40), generator=g)
    ei = torch.cat([pairs, pairs.flip(0), torch.arange(n).repeat(2, 1)], dim=1).to(DEV)
    y = torch.randint(0, classes, (n,), generator=g).to(DEV)
    mask = (torch.rand(n, generator=g) < 0.7).to(DEV)
    torch.manual_seed(seed)
    model = DIFFormer(f_in, 4, classes, num_layers=2, kernel="simple", dropout=0.0).to(DEV).train()
    return model, x, ei, y, mask


def _groups(model):
    """Two groups with different lr and betas: the layers' parameters and the rest."""
    convs = [p for n, p in model.named_parameters() if n.startswith("convs.")]
    rest = [p for n, p in model.named_parameters() if not n.startswith("convs.")]
    assert convs and rest
    return [dict(params=convs, lr=3e-3, betas=(0.8, 0.99)), dict(params=rest)]


def _train_step(model, opt, x, ei, y, mask):
    from difformer_amd import log_softmax_nll
    opt.zero_grad(set_to_none=True)
    loss = log_softmax_nll(model(x, ei), y, mask)
    loss.backward()
    return loss


@pytest.mark.parametrize("make", [_small_model, _tiny_model], ids=["hidden64", "tiny"])
def test_three_steps_of_the_public_class_equal_the_oracle(make):
    """Every step of difformer_amd.Adam against the oracle fed the state before the step and the gradients read back."""
    import difformer_amd
    model, x, ei, y, mask = make(31)
    opt = difformer_amd.Adam(_groups(model), lr=1e-2, weight_decay=5e-4)
    worst = [0.0, 0.0, 0.0]
    for k in range(3):
        _train_step(model, opt, x, ei, y, mask)
        state = {}
        for group in opt.param_groups:
            for p in group["params"]:
                st = opt.state.get(p) or {}
                zero = np.zeros(tuple(p.shape), dtype=np.float32)
                state[p] = (p.detach().cpu().numpy(), p.grad.cpu().numpy(), st["exp_avg"].cpu().numpy() if st else zero,
                            st["exp_avg_sq"].cpu().numpy() if st else zero, group)
        opt.step()
        for p, (p0, g, m0, v0, group) in state.items():
            ref = adam_ref.step(p0, g, m0, v0, k + 1, group["lr"], group["betas"][0], group["betas"][1], group["eps"], group["weight_decay"])
            st = opt.state[p]
            e = adam_ref.worst_ratio(p.detach().cpu().numpy(), st["exp_avg"].cpu().numpy(), st["exp_avg_sq"].cpu().numpy(),
                                     ref + adam_ref.bounds(p0, *ref))
            worst = [max(a, b) for a, b in zip(worst, e)]
            assert float(st["step"]) == k + 1 and st["step"].device == p.device and st["step"].dtype == torch.float32
            assert (p.grad.cpu().numpy() == g).all()
    print(f"public class, 3 steps: worst p {worst[0]:.4f}, m {worst[1]:.4f}, v {worst[2]:.4f} x bound")
    for key, e in zip("pmv", worst):
        WORST[key] = max(WORST[key], e)
    assert max(worst) <= 1, worst


@pytest.mark.parametrize("make", [_small_model, _tiny_model], ids=["hidden64", "tiny"])
def test_the_forward_after_a_step_sees_the_new_parameters(make):
    """The packed-weight memos are keyed on (data_ptr, _version) and the kernel writes through raw pointers: without the version
    bump of step() the eval forward after the step serves the weights from before it.  The twin gets the updated parameters
    through load_state_dict; two forwards on equal parameters are bitwise equal."""
    import difformer_amd
    from difformer_amd import tiny
    model, x, ei, y, mask = make(32)
    opt = difformer_amd.Adam(model.parameters(), lr=1e-2, weight_decay=5e-4)
    model.eval()
    with torch.no_grad():
        y0 = model(x, ei).clone()                                 # fills every memo with the parameters before the step
    took_tiny = tiny.stats["forward"]
    versions = [p._version for p in model.parameters()]
    model.train()
    _train_step(model, opt, x, ei, y, mask)
    opt.step()
    assert all(p._version > v for p, v in zip(model.parameters(), versions))
    model.eval()
    with torch.no_grad():
        y1 = model(x, ei).clone()
    assert (tiny.stats["forward"] > took_tiny) == (make is _tiny_model)
    twin = make(32)[0]
    twin.load_state_dict(model.state_dict())
    twin.eval()
    with torch.no_grad():
        y2 = twin(x, ei)
    assert not torch.equal(y0, y1)                               # the step did change the output
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32))


def test_a_parameter_without_a_gradient_and_a_strided_gradient():
    import difformer_amd
    torch.manual_seed(3)
    a = torch.nn.Parameter(torch.randn(37, 5, device=DEV))
    b = torch.nn.Parameter(torch.randn(11, device=DEV))
    c = torch.nn.Parameter(torch.randn(6, 4, device=DEV))
    opt = difformer_amd.Adam([a, b, c], lr=1e-2)
    a.grad, c.grad = torch.randn(37, 5, device=DEV), torch.randn(4, 6, device=DEV).t()
    assert not c.grad.is_contiguous()
    b0, vb = b.detach().clone(), b._version
    p0 = {p: p.detach().cpu().numpy() for p in (a, c)}
    opt.step()
    assert torch.equal(b.detach(), b0) and b._version == vb and not opt.state.get(b)
    for p in (a, c):
        g = p.grad.cpu().numpy()
        ref = adam_ref.step(p0[p], g, np.zeros_like(g), np.zeros_like(g), 1, 1e-2, 0.9, 0.999, 1e-8, 0.0)
        e = adam_ref.worst_ratio(p.detach().cpu().numpy(), opt.state[p]["exp_avg"].cpu().numpy(), opt.state[p]["exp_avg_sq"].cpu().numpy(),
                                 ref + adam_ref.bounds(p0[p], *ref))
        assert max(e) <= 1, e
    for bad in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(ValueError, match="float32"):
            difformer_amd.Adam([torch.nn.Parameter(torch.zeros(3, dtype=bad, device=DEV))])


def test_state_dict_loads_into_a_capturable_torch_adam_and_back():
    """Two steps of ours, the state into torch.optim.Adam(capturable=True) on a twin, one more step on each under the same
    gradients.  The unit is 4 ulp32 + 1e-7 |update|.  Measured on the MI355X: 33.96 units (profiles/r15_adam.md), all of it
    torch's: with capturable=True it evaluates 1 - beta2^t in float32 on the device, and at t = 3 that is 1 - 0.997003 = 0.003
    with an absolute error of 2^-24, a relative error of up to 2e-5 in the bias correction, 1e-5 = 100 units in the update.
    The bar is therefore twice the measurement against torch, 68 units; against the oracle the same step is held to one
    rounding (test_three_steps_of_the_public_class_equal_the_oracle)."""
    import difformer_amd
    model, x, ei, y, mask = _small_model(33)
    opt = difformer_amd.Adam(model.parameters(), lr=1e-2, weight_decay=5e-4)
    for _ in range(2):
        _train_step(model, opt, x, ei, y, mask)
        opt.step()
    twin = _small_model(33)[0]
    twin.load_state_dict(model.state_dict())
    other = torch.optim.Adam(twin.parameters(), lr=1e-2, weight_decay=5e-4, capturable=True)
    other.load_state_dict(copy.deepcopy(opt.state_dict()))                         # (load_state_dict keeps the tensors it is given)
    assert all(s["step"].is_cuda and float(s["step"]) == 2 for s in other.state.values())
    _train_step(model, opt, x, ei, y, mask)
    before = [p.detach().clone() for p in model.parameters()]
    for p, q in zip(model.parameters(), twin.parameters()):
        q.grad = p.grad.clone()
    opt.step()
    other.step()
    worst = 0.0
    for p, q, p0 in zip(model.parameters(), twin.parameters(), before):
        a, b, old = (t.detach().cpu().numpy().astype(np.float64) for t in (p, q, p0))
        bar = 4 * adam_ref.ulp32(b).astype(np.float64) + 1e-7 * np.abs(b - old)
        worst = max(worst, float(np.max(np.abs(a - b) / bar)))
    GAP["third step against torch.optim.Adam(capturable=True)"] = worst
    print(f"state interchange: worst |ours - torch| = {worst:.3f} x (4 ulp32 + 1e-7 |update|)")
    assert worst <= 68
    assert all(float(s["step"]) == 3 for s in other.state.values()) and all(float(s["step"]) == 3 for s in opt.state.values())
    back = difformer_amd.Adam(model.parameters(), lr=1e-2, weight_decay=5e-4)
    back.load_state_dict(other.state_dict())                                       # ... and back
    assert all(s["step"].is_cuda and s["step"].dtype == torch.float32 for s in back.state.values())
    _train_step(model, back, x, ei, y, mask)
    back.step()
    assert all(float(s["step"]) == 4 for s in back.state.values())


def test_a_whole_step_with_our_adam_is_captured_as_one_graph():
    """GraphedTrainStep with difformer_amd.Adam and no flag: three replays against six eager steps of a twin (three warm-up steps
    run before the capture), losses to the bar of test_a_step_with_a_boolean_mask_loss_is_captured_as_one_graph."""
    import difformer_amd
    from difformer_amd import log_softmax_nll
    eager, x, ei, y, mask = _small_model(34)
    twin = copy.deepcopy(eager)
    loss_fn = lambda out: log_softmax_nll(out, y, mask)
    opt_e = difformer_amd.Adam(eager.parameters(), lr=1e-3, weight_decay=5e-4)
    opt_g = difformer_amd.Adam(twin.parameters(), lr=1e-3, weight_decay=5e-4)
    step = difformer_amd.GraphedTrainStep(twin, opt_g, loss_fn, x, ei, warmup=3)
    losses_g = [float(step()) for _ in range(3)]
    losses_e = []
    for _ in range(3 + 3):
        opt_e.zero_grad(set_to_none=True)
        loss = loss_fn(eager(x, ei))
        loss.backward()
        opt_e.step()
        losses_e.append(float(loss.detach()))
    print("graphed", losses_g, "eager", losses_e[-3:])
    assert losses_g[0] != losses_g[2]                                            # the replays do train
    for a, b in zip(losses_g, losses_e[-3:]):
        assert abs(a - b) <= 2.0 ** -23 * abs(b) + 2.0 ** -50, (losses_g, losses_e)
    assert all(float(s["step"]) == 6 for s in opt_g.state.values())              # the device counters ran in the replays


def test_zz_report_the_worst_cases():
    """Prints what the tests above measured (profiles/r15_adam.md quotes it); run last in this module."""
    print(f"worst case against the oracle: p {WORST['p']:.4f}, exp_avg {WORST['m']:.4f}, exp_avg_sq {WORST['v']:.4f} x bound")
    for key, value in GAP.items():
        print(f"{key}: {value:.3f} x (4 ulp32 + 1e-7 |update|)")
    assert all(e <= 1 for e in WORST.values())
