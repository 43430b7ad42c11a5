"""The training losses without a GPU: the long-double oracle pinned to the reference's own expressions evaluated by torch in
float64, the well-posedness of the GPU tests' inputs, the seventh library's header and host arithmetic, the CPU-tensor path and
the argument errors."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_loss.h")
NLL_FWD = ("x", "ldx", "label", "ignore_index", "rows", "rows_kind", "index_status", "n", "C", "record", "workspace",
           "workspace_bytes", "stream")
NLL_BWD = ("x", "ldx", "label", "ignore_index", "rows", "rows_kind", "n", "C", "record", "upstream", "grad", "ldg", "stream")
BCE_FWD = ("x", "ldx", "target", "target_type", "ldt", "rows", "rows_kind", "index_status", "n", "C", "record", "workspace",
           "workspace_bytes", "stream")
BCE_BWD = ("x", "ldx", "target", "target_type", "ldt", "rows", "rows_kind", "n", "C", "record", "upstream", "grad", "ldg", "stream")
NAMES = ["dif_bce_with_logits_bwd_bf16", "dif_bce_with_logits_bwd_f32", "dif_bce_with_logits_fwd_bf16", "dif_bce_with_logits_fwd_f32",
         "dif_loss_last_error", "dif_loss_row_weights", "dif_loss_version", "dif_loss_workspace_bytes",
         "dif_nll_log_softmax_bwd_bf16", "dif_nll_log_softmax_bwd_f32", "dif_nll_log_softmax_fwd_bf16", "dif_nll_log_softmax_fwd_f32"]


# ---- the oracle ---------------------------------------------------------------------------------------------------------------------
def _torch_float64(case):
    """The reference's expression (main.py:121-129, main-batch.py:136-140) on float64 logits -> (loss, gradient)."""
    x = torch.from_numpy(case["x"]).double().requires_grad_()
    rows = case["rows"]
    second = torch.from_numpy(case["second"])
    if case["kind"] == "nll":
        logp = F.log_softmax(x, dim=1)
        if rows is not None:
            logp, second = logp[torch.from_numpy(rows)], second[torch.from_numpy(rows)]
        loss = F.nll_loss(logp, second, ignore_index=case["ignore_index"])
    else:
        out = x
        if rows is not None:
            out, second = x[torch.from_numpy(rows)], second[torch.from_numpy(rows)]
        loss = F.binary_cross_entropy_with_logits(out, second.double())
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


def test_oracle_equals_the_reference_expressions_in_float64():
    """Bounds of the issue: |d loss| <= 2^-50 + 2^-50 |loss|, every gradient element within 2^-45 / count.  Index, mask and
    duplicate indices, ignore_index and the three target dtypes are all in the table, at logit scales 1 to 30.  Measured
    worst cases over the 416 cases: 0.33 x the loss bound, 0.06 x the gradient bound."""
    worst_loss, worst_grad, seen = 0.0, 0.0, 0
    kinds = set()
    for name, case in loss_ref.cases().items():
        ref = loss_ref.evaluate(case, upstream=1.0)
        loss, grad = _torch_float64(case)
        dl = abs(loss - ref["loss"]) / (2.0 ** -50 * (1 + abs(ref["loss"])))
        dg = float(np.max(np.abs(grad - ref["grad"]))) / (2.0 ** -45 / ref["count"])
        worst_loss, worst_grad, seen = max(worst_loss, dl), max(worst_grad, dg), seen + 1
        assert dl <= 1 and dg <= 1, (name, dl, dg)
        kinds.add((case["kind"], "all" if case["rows"] is None else str(case["rows"].dtype), str(case["second"].dtype)))
    print(f"oracle vs torch float64 over {seen} cases: worst loss {worst_loss:.3f} x bound, worst gradient {worst_grad:.3f} x bound")
    assert seen > 400
    assert {("nll", s, "int64") for s in ("all", "bool", "int64")} <= kinds
    assert {("bce", s, t) for s in ("all", "bool", "int64") for t in ("int64", "float32", "uint8")} <= kinds


def test_oracle_keeps_what_float64_log_loses():
    """x = 83: the true BCE loss at t = 1 is log1p(exp(-83)) = 8.9e-37; log(1 + exp(-83)) is 0 in float64."""
    x = np.array([[83.0]], dtype=np.float32)
    got = loss_ref.bce(x, np.array([[1]], dtype=np.int64))
    assert 8.8e-37 < got["loss"] < 9.0e-37 and got["count"] == 1
    assert -9.0e-37 < got["grad"][0, 0] < -8.8e-37                        # -sigmoid(-x), not sigmoid(x) - 1 == 0
    got = loss_ref.nll(np.array([[83.0, 0.0]], dtype=np.float32), np.array([0]))
    assert 8.8e-37 < got["loss"] < 9.0e-37 and -9.0e-37 < got["grad"][0, 0] < -8.8e-37 and got["grad"][0, 1] == -got["grad"][0, 0]


def test_oracle_selection_and_edge_semantics():
    x = np.array([[0.0, 1.0], [np.nan, np.inf], [2.0, -1.0]], dtype=np.float32)
    lab = np.array([1, 0, 0])
    a = loss_ref.nll(x, lab, np.array([True, False, True]))
    b = loss_ref.nll(x[[0, 2]], lab[[0, 2]])
    assert a["loss"] == b["loss"] and a["count"] == 2 and (a["grad"][1] == 0).all() and (a["grad"][[0, 2]] == b["grad"]).all()
    c = loss_ref.nll(x, lab, np.array([2, 0, 2, 2], dtype=np.int64))              # multiplicity 3
    assert c["count"] == 4 and np.allclose(c["grad"][2], 3 * c["grad"][0] / a["grad"][0] * a["grad"][2], rtol=1e-12)
    assert np.isnan(loss_ref.nll(x, lab)["loss"])                                  # the NaN row selected
    empty = loss_ref.nll(x, lab, np.zeros(0, dtype=np.int64))
    assert np.isnan(empty["loss"]) and empty["count"] == 0 and (empty["grad"] == 0).all()
    bad = loss_ref.nll(x, np.array([1, 0, 5]), np.array([0, 2, 7, -1], dtype=np.int64))
    assert np.isnan(bad["loss"]) and bad["invalid"] == 3 and bad["count"] == 1
    ign = loss_ref.nll(x, np.array([1, -100, -100]))
    assert ign["count"] == 1 and ign["loss"] == loss_ref.nll(x[:1], lab[:1])["loss"]
    assert loss_ref.ulp(1.0) == 2.0 ** -23 and loss_ref.ulp(1.5, True) == 2.0 ** -7 and loss_ref.ulp(0.0) == 2.0 ** -149
    assert loss_ref.ulp(1e-40) == 2.0 ** -149 and loss_ref.ulp(1e-40, True) == 2.0 ** -133 and loss_ref.ulp(-3.0) == 2.0 ** -22
    r = loss_ref.to_bf16(np.array([1.00390625, 1.01171875, 3.0e-39], dtype=np.float32))    # ties to even, a denormal
    assert r[0] == 1.0 and r[1] == 1.015625 and r[2] == torch.tensor(3.0e-39).bfloat16().float().item()


def test_every_gpu_case_is_well_posed():
    table = loss_ref.cases()
    assert len(table) > 400
    for name, case in table.items():
        assert loss_ref.well_posed(case), name
        ref = loss_ref.evaluate(case)
        assert np.isfinite(ref["loss"]) and ref["count"] > 0 and ref["invalid"] == 0 and np.isfinite(ref["grad"]).all(), name
    for C in loss_ref.COLUMNS:
        assert len(loss_ref.rows_for(C)) >= 4 and {1, 2, 3} <= set(loss_ref.rows_for(C))
    # the mechanisms the table is there for
    assert -(-70001 // (256 // loss_ref.lanes(2))) > 256                          # more than one partial per finalising lane
    assert -(-4100 // (256 // loss_ref.lanes(65))) > loss_ref.MAX_GROUPS           # more than one pass per workgroup
    sat = loss_ref.evaluate(table["sweep/nll/C17/n9/s30"])["grad"]
    assert (np.abs(sat[sat != 0]) < 1e-30).any()                                  # saturated rows: entries far below float32's normals


# ---- header and library -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from difformer_amd import _lib
    return _lib.load_loss()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(lib):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.LOSS_SIGNATURES) == NAMES
    for name in declared:
        assert getattr(lib, name) is not None
    others = (set(_lib.SIGNATURES) | set(_lib.MAPS_SIGNATURES) | set(_lib.EDGES_SIGNATURES) | set(_lib.KNN_SIGNATURES)
              | set(_lib.SLOTS_SIGNATURES) | set(_lib.METRICS_SIGNATURES))
    assert not set(_lib.LOSS_SIGNATURES) & others
    assert len(_lib.SIGNATURES) == 101
    for sfx in ("f32", "bf16"):
        assert len(_lib.LOSS_SIGNATURES["dif_nll_log_softmax_fwd_" + sfx][1]) == len(NLL_FWD)
        assert len(_lib.LOSS_SIGNATURES["dif_nll_log_softmax_bwd_" + sfx][1]) == len(NLL_BWD)
        assert len(_lib.LOSS_SIGNATURES["dif_bce_with_logits_fwd_" + sfx][1]) == len(BCE_FWD)
        assert len(_lib.LOSS_SIGNATURES["dif_bce_with_logits_bwd_" + sfx][1]) == len(BCE_BWD)
    assert _lib.LOSS_SIGNATURES["dif_loss_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.LOSS_SIGNATURES["dif_loss_last_error"][0] is ctypes.c_char_p
    assert lib.dif_loss_version() == _lib.LOSS_VERSION == 1
    assert _lib.LOSS_CONSTANTS == dict(DIF_LOSS_ROWS_ALL=0, DIF_LOSS_ROWS_WEIGHTS=1, DIF_LOSS_ROWS_MASK=2, DIF_LOSS_TARGET_I64=0,
                                       DIF_LOSS_TARGET_F32=1, DIF_LOSS_TARGET_U8=2, DIF_LOSS_RECORD_BYTES=32)
    assert '#include "difformer_hip.h"' in open(HEADER).read()


def test_the_workspace_is_host_arithmetic_and_equals_the_documented_formula(lib):
    assert lib.dif_loss_workspace_bytes(0, 5) == 256 and lib.dif_loss_workspace_bytes(5, 0) == 0
    assert lib.dif_loss_workspace_bytes(5, 65537) == 0 and lib.dif_loss_workspace_bytes(-1, 5) == 0
    assert lib.dif_loss_workspace_bytes(70001, 2) == loss_ref.workspace_formula(70001, 2) == 13312
    assert lib.dif_loss_workspace_bytes(1 << 40, 65536) == 24 * 1024
    rng = np.random.default_rng(0)
    for _ in range(300):
        C = int(rng.integers(1, 300))
        n = int(10 ** rng.uniform(0, 8))
        assert lib.dif_loss_workspace_bytes(n, C) == loss_ref.workspace_formula(n, C), (n, C)
    for C in loss_ref.COLUMNS:
        for n in loss_ref.rows_for(C):
            assert lib.dif_loss_workspace_bytes(n, C) == loss_ref.workspace_formula(n, C) == 256


def _args(names, **over):
    """Made-up (never dereferenced) addresses: every rejection happens before any HIP call."""
    a = dict(x=0x10004, ldx=112, label=0x20008, ignore_index=-100, target=0x20008, target_type=0, ldt=112, rows=0x30004, rows_kind=1,
             index_status=None, n=100, C=112, record=0x40008, workspace=0x50010, workspace_bytes=1 << 20, upstream=0x60004,
             grad=0x70004, ldg=112, stream=None)
    a.update(over)
    return [a[k] for k in names]


COMMON = [(dict(x=None), "DIF_E_BADARG"), (dict(record=None), "DIF_E_BADARG"), (dict(x=0x10002), "DIF_E_BADARG"),
          (dict(record=0x40004), "DIF_E_BADARG"), (dict(ldx=111), "DIF_E_BADARG"), (dict(n=-1), "DIF_E_BADARG"),
          (dict(C=0), "DIF_E_SHAPE"), (dict(C=65537, ldx=65537, ldt=65537, ldg=65537), "DIF_E_SHAPE"),
          (dict(rows_kind=3), "DIF_E_BADARG"), (dict(rows_kind=-1), "DIF_E_BADARG"), (dict(rows=None), "DIF_E_BADARG"),
          (dict(rows=0x30002), "DIF_E_BADARG")]
FWD = [(dict(workspace=None), "DIF_E_BADARG"), (dict(workspace=0x50008), "DIF_E_BADARG"), (dict(workspace_bytes=255), "DIF_E_WORKSPACE"),
       (dict(workspace_bytes=-1), "DIF_E_WORKSPACE"), (dict(index_status=0x80002), "DIF_E_BADARG")]
BWD = [(dict(upstream=None), "DIF_E_BADARG"), (dict(grad=None), "DIF_E_BADARG"), (dict(ldg=111), "DIF_E_BADARG"),
       (dict(upstream=0x60002), "DIF_E_BADARG"), (dict(grad=0x70002), "DIF_E_BADARG")]
NLL = [(dict(label=None), "DIF_E_BADARG"), (dict(label=0x20004), "DIF_E_BADARG")]
BCE = [(dict(target=None), "DIF_E_BADARG"), (dict(target=0x20004), "DIF_E_BADARG"), (dict(target_type=3), "DIF_E_BADARG"),
       (dict(ldt=111), "DIF_E_BADARG"), (dict(target=0x20002, target_type=1), "DIF_E_BADARG")]


@pytest.mark.parametrize("symbol,names,table", [
    ("dif_nll_log_softmax_fwd_f32", NLL_FWD, COMMON + FWD + NLL), ("dif_nll_log_softmax_bwd_f32", NLL_BWD, COMMON + BWD + NLL),
    ("dif_bce_with_logits_fwd_f32", BCE_FWD, COMMON + FWD + BCE), ("dif_bce_with_logits_bwd_f32", BCE_BWD, COMMON + BWD + BCE)])
def test_every_argument_check_returns_its_code_without_a_gpu(lib, symbol, names, table):
    from difformer_amd import _lib
    for over, code in table:
        rc = getattr(lib, symbol)(*_args(names, **over))
        assert rc == _lib.ERROR_CODES[code], (symbol, over, rc, lib.dif_loss_last_error())
        assert symbol.encode() in lib.dif_loss_last_error()                      # this library's text, not another's
    # bfloat16 rows need 2-byte alignment only; an odd address is rejected
    twin = symbol.replace("f32", "bf16")
    assert getattr(lib, twin)(*_args(names, x=0x10001)) == _lib.ERROR_CODES["DIF_E_BADARG"] and twin.encode() in lib.dif_loss_last_error()
    assert getattr(lib, twin)(*_args(names, C=0, x=0x10002, grad=0x70002)) == _lib.ERROR_CODES["DIF_E_SHAPE"]
    # a mask needs no alignment, "all rows" no pointer: the next check (C) answers
    assert getattr(lib, symbol)(*_args(names, rows=0x30001, rows_kind=2, C=0)) == _lib.ERROR_CODES["DIF_E_SHAPE"]
    assert getattr(lib, symbol)(*_args(names, rows=None, rows_kind=0, ldx=1)) == _lib.ERROR_CODES["DIF_E_BADARG"]
    assert b"leading dimension" in lib.dif_loss_last_error()


def test_row_weights_argument_checks(lib):
    from difformer_amd import _lib
    bad = _lib.ERROR_CODES["DIF_E_BADARG"]
    f = lib.dif_loss_row_weights
    assert f(None, 5, 10, 0x1004, 0x2004, None) == bad and f(0x1008, 5, 10, None, 0x2004, None) == bad
    assert f(0x1008, 5, 10, 0x1004, None, None) == bad and f(0x1004, 5, 10, 0x1004, 0x2004, None) == bad
    assert f(0x1008, -1, 10, 0x1004, 0x2004, None) == bad and f(0x1008, 1 << 31, 10, 0x1004, 0x2004, None) == bad
    assert f(0x1008, 5, -1, 0x1004, 0x2004, None) == bad and f(0x1008, 5, 10, 0x1002, 0x2004, None) == bad
    assert b"dif_loss_row_weights" in lib.dif_loss_last_error()


# ---- the public functions on CPU tensors -------------------------------------------------------------------------------------------------
def _bitwise(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32 if a.dtype == torch.float32 else torch.int16),
                                                                     b.view(torch.int32 if b.dtype == torch.float32 else torch.int16))


@pytest.mark.parametrize("name", ["select/nll/all", "select/nll/mask", "select/nll/index", "sweep/nll/C17/n9/s30"])
def test_cpu_tensors_take_the_torch_expression_nll(name):
    from difformer_amd import log_softmax_nll
    case = loss_ref.cases()[name]
    rows = None if case["rows"] is None else torch.from_numpy(case["rows"])
    lab = torch.from_numpy(case["second"])
    for label in (lab, lab.view(-1, 1)):
        a = torch.from_numpy(case["x"]).requires_grad_()
        b = torch.from_numpy(case["x"]).requires_grad_()
        got = log_softmax_nll(a, label, rows)
        logp = F.log_softmax(b, dim=1)
        want = F.nll_loss(logp if rows is None else logp[rows], lab if rows is None else label.view(-1)[rows])
        (got * 3).backward()
        (want * 3).backward()
        assert got.dim() == 0 and _bitwise(got.detach(), want.detach()) and _bitwise(a.grad, b.grad)
    with torch.no_grad():
        assert _bitwise(log_softmax_nll(a.detach().bfloat16(), lab, rows), F.nll_loss(
            F.log_softmax(a.detach().bfloat16(), dim=1) if rows is None else F.log_softmax(a.detach().bfloat16(), dim=1)[rows],
            lab if rows is None else lab[rows]))
    lab0 = lab.clone()
    lab0[lab0 == -100] = 0
    got = log_softmax_nll(a.detach(), lab0, rows, ignore_index=0)
    logp = F.log_softmax(a.detach(), dim=1)
    assert _bitwise(got, F.nll_loss(logp if rows is None else logp[rows], lab0 if rows is None else lab0[rows], ignore_index=0))


@pytest.mark.parametrize("name", ["select/bce/all", "select/bce/mask", "select/bce/index", "target/bce/float32"])
def test_cpu_tensors_take_the_torch_expression_bce(name):
    from difformer_amd import bce_with_logits
    case = loss_ref.cases()[name]
    rows = None if case["rows"] is None else torch.from_numpy(case["rows"])
    target = torch.from_numpy(case["second"])
    for t in (target, target.bool()) if target.dtype != torch.float32 else (target,):
        a = torch.from_numpy(case["x"]).requires_grad_()
        b = torch.from_numpy(case["x"]).requires_grad_()
        got = bce_with_logits(a, t, rows)
        want = F.binary_cross_entropy_with_logits(b if rows is None else b[rows], (t if rows is None else t[rows]).float())
        (got * -0.5).backward()
        (want * -0.5).backward()
        assert got.dim() == 0 and _bitwise(got.detach(), want.detach()) and _bitwise(a.grad, b.grad)


def test_every_argument_error_raises():
    from difformer_amd import bce_with_logits, log_softmax_nll, loss_record
    x, lab, t = torch.zeros(6, 3), torch.zeros(6, dtype=torch.int64), torch.zeros(6, 3)
    meta = torch.device("meta")
    for bad in (dict(out=x.double()), dict(out=x.half()), dict(out=x[0]), dict(out=x.view(6, 3, 1)), dict(out=torch.zeros(6, 0)),
                dict(out=x.numpy()), dict(label=lab.numpy()), dict(label=lab.int()), dict(label=lab[:5]), dict(label=lab.view(3, 2)),
                dict(label=lab.view(6, 1, 1)), dict(label=lab.float()), dict(label=lab.to(meta)), dict(rows=[0, 1]),
                dict(rows=torch.zeros(6)), dict(rows=torch.zeros(6, dtype=torch.int32)), dict(rows=torch.zeros(5, dtype=torch.bool)),
                dict(rows=torch.zeros(6, 1, dtype=torch.bool)), dict(rows=torch.zeros((2, 2), dtype=torch.int64)),
                dict(rows=torch.zeros(2, dtype=torch.int64, device=meta))):
        with pytest.raises(ValueError, match="log_softmax_nll"):
            log_softmax_nll(**dict(dict(out=x, label=lab), **bad))
    for bad in (dict(out=x.double()), dict(out=x[0]), dict(target=t[:, :2]), dict(target=t[:5]), dict(target=t.double()),
                dict(target=t.to(torch.complex64)), dict(target=t.view(6, 3, 1)), dict(target=t.numpy()), dict(target=t.to(meta)),
                dict(rows=torch.zeros(7, dtype=torch.bool)), dict(rows=torch.zeros(6, dtype=torch.uint8))):
        with pytest.raises(ValueError, match="bce_with_logits"):
            bce_with_logits(**dict(dict(out=x, target=t), **bad))
    with pytest.raises(ValueError, match="float64"):
        log_softmax_nll(x.double(), lab)
    with pytest.raises(ValueError, match="CPU"):
        loss_record("nll", x, lab)
    with pytest.raises(ValueError, match="kind"):
        loss_record("mse", x, lab)
    wide = torch.zeros(1, 65537)
    with pytest.raises(ValueError, match="65536"):
        bce_with_logits(wide, wide)


def test_the_package_exports_the_losses_and_the_makefile_builds_the_library():
    import difformer_amd
    assert {"log_softmax_nll", "bce_with_logits", "loss_record"} <= set(difformer_amd.__all__)
    make = open(os.path.join(ROOT, "difformer_amd", "csrc", "Makefile")).read()
    assert re.search(r"^all:.*\$\(LOSS_OUT\)", make, flags=re.M) and re.search(r"^\trm -rf .*\$\(LOSS_OUT\)", make, flags=re.M)
    assert "-Wl,-Bsymbolic $(LOSS_OBJS)" in make
