"""The evaluation metrics without a GPU: the integer oracle pinned to sklearn and to the reference's loops, the well-posedness
of the GPU tests' inputs, the argument errors of the public functions, the sixth library's header, and its host arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import metrics_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "difformer_metrics.h")
ROC_ARGS = ("score", "lds", "cls", "ldc", "n", "C", "counts", "workspace", "workspace_bytes", "stream")
ACC_ARGS = ("pred", "ldp", "label", "labelled", "n", "K", "out", "stream")
SMALL = [name for name in metrics_ref.cases() if name != "long"]      # n <= 4,096: what the sklearn bound is derived for


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def test_oracle_equals_sklearn_roc_auc_score():
    """Bound 1e-12: both sides are float64 evaluations of the same rational U2 / (2 P N); the integer side rounds once
    (2^-53), sklearn's trapezoid sums at most n <= 4,096 terms of relative error 2^-53 each, so the difference stays below
    4,097 * 1.2e-16 < 1e-12.  Measured worst case over the 706 columns of the edge inputs: 1.1e-16."""
    metrics = pytest.importorskip("sklearn.metrics")
    worst, seen = 0.0, 0
    for name in SMALL:
        y, s, evaluated = metrics_ref.cases()[name]
        assert y.shape[0] <= 4096
        tab = metrics_ref.table(y, s)
        for c in evaluated:
            P, N, _, invalid, U2 = tab[c]
            assert invalid == 0, (name, c)
            lab = y[:, c] == y[:, c]
            want = metrics.roc_auc_score(y[lab, c], s[lab, c])
            worst = max(worst, abs(U2 / (2 * P * N) - want))
            seen += 1
    print(f"oracle vs roc_auc_score over {seen} columns: worst |difference| {worst:.3e}")
    assert seen > 400 and worst <= 1e-12
    y, s, _ = metrics_ref.cases()["ties/constant"]
    assert [U2 / (2 * P * N) for P, N, _, _, U2 in metrics_ref.table(y, s)] == [0.5] * 3
    y, s, _ = metrics_ref.cases()["ties/signed-zeros"]
    zeros = np.where(s == 0, np.float32(0.0), s)
    assert metrics_ref.table(y, s) == metrics_ref.table(y, zeros)            # -0.0 == +0.0


def test_oracle_equals_sklearn_micro_f1():
    """correct / n against f1_score(average='micro'); the same 1e-12 bound (one division against sklearn's tp / (tp + fp)
    arithmetic in float64).  Measured worst case: 0 (every quotient equal)."""
    metrics = pytest.importorskip("sklearn.metrics")
    worst = 0.0
    for n in metrics_ref.ARGMAX_ROWS:
        for K in metrics_ref.ARGMAX_COLUMNS:
            y, p = metrics_ref.argmax_case(n, K)
            y = np.nan_to_num(y, nan=0.0).astype(np.int64)
            want = metrics.f1_score(y, np.argmax(p, axis=-1)[:, None], average="micro")
            worst = max(worst, abs(metrics_ref.eval_f1(y, p) - want))
    print(f"oracle vs f1_score: worst |difference| {worst:.3e}")
    assert worst <= 1e-12


def _reference_eval_rocauc(y_true, y_pred, roc_auc_score):
    """data_utils.py:262-285, line for line, on torch tensors."""
    import torch.nn.functional as F
    rocauc_list = []
    y_true = y_true.detach().cpu().numpy()
    if y_true.shape[1] == 1:
        y_pred = F.softmax(y_pred, dim=-1)[:, 1].unsqueeze(1).cpu().numpy()
    else:
        y_pred = y_pred.detach().cpu().numpy()
    for i in range(y_true.shape[1]):
        if np.sum(y_true[:, i] == 1) > 0 and np.sum(y_true[:, i] == 0) > 0:
            is_labeled = y_true[:, i] == y_true[:, i]
            rocauc_list.append(roc_auc_score(y_true[is_labeled, i], y_pred[is_labeled, i]))
    if len(rocauc_list) == 0:
        raise RuntimeError('No positively labeled data available. Cannot compute ROC-AUC.')
    return sum(rocauc_list) / len(rocauc_list)


def _reference_eval_acc(y_true, y_pred):
    """data_utils.py:249-259."""
    acc_list = []
    y_true = y_true.detach().cpu().numpy()
    y_pred = y_pred.argmax(dim=-1, keepdim=True).detach().cpu().numpy()
    for i in range(y_true.shape[1]):
        is_labeled = y_true[:, i] == y_true[:, i]
        correct = y_true[is_labeled, i] == y_pred[is_labeled, i]
        acc_list.append(float(np.sum(correct)) / len(correct))
    return sum(acc_list) / len(acc_list)


def test_oracle_equals_the_reference_loops():
    metrics = pytest.importorskip("sklearn.metrics")
    # skipped columns, NaN labels, ignored non-finite scores: the mean runs over the evaluated columns only
    for name in ("labels/skipped-columns", "scores/ignored-non-finite", "ties/integer", "passes/C112", "chunk/C7/n74"):
        y, s, evaluated = metrics_ref.cases()[name]
        want = _reference_eval_rocauc(torch.from_numpy(y), torch.from_numpy(s), metrics.roc_auc_score)
        assert abs(metrics_ref.eval_rocauc(y, s) - want) <= 1e-12, name
        assert metrics_ref.evaluated_columns(metrics_ref.table(y, s)) == evaluated
    # the C == 1 branch: softmax(y_pred)[:, 1], saturated logits collapse to long ties
    rng = np.random.default_rng(5)
    logits = torch.from_numpy(np.where(rng.random((600, 2)) < 0.5, 40.0, -40.0).astype(np.float32) + rng.integers(-1, 2, (600, 2)).astype(np.float32))
    y = metrics_ref.labels(600, 1, 5)
    prob = torch.softmax(logits, dim=-1)[:, 1:2].numpy()
    assert len(np.unique(prob)) < 40
    want = _reference_eval_rocauc(torch.from_numpy(y), logits, metrics.roc_auc_score)
    assert abs(metrics_ref.eval_rocauc(y, prob) - want) <= 1e-12
    # nothing to evaluate: the reference's error and text
    none = np.ones((20, 3), dtype=np.float32)
    for fn in (lambda: metrics_ref.eval_rocauc(none, np.zeros((20, 3), dtype=np.float32)),
               lambda: _reference_eval_rocauc(torch.from_numpy(none), torch.zeros(20, 3), metrics.roc_auc_score)):
        with pytest.raises(RuntimeError, match="No positively labeled data available. Cannot compute ROC-AUC."):
            fn()
    with pytest.raises(ValueError):
        bad = metrics_ref.labels(30, 2, 6)
        bad[5, 1] = 2
        metrics_ref.eval_rocauc(bad, metrics_ref.normal_scores(30, 2, 6))


def test_oracle_equals_the_reference_eval_acc():
    for n in metrics_ref.ARGMAX_ROWS:
        for K in metrics_ref.ARGMAX_COLUMNS:
            y, p = metrics_ref.argmax_case(n, K)
            if (y == y).any():
                assert metrics_ref.eval_acc(y, p) == _reference_eval_acc(torch.from_numpy(y), torch.from_numpy(p)), (n, K)
            # torch.argmax and numpy.argmax agree on first maxima and NaN
            assert np.array_equal(torch.from_numpy(p).argmax(dim=-1).numpy(), np.argmax(p, axis=-1))
    y, p = metrics_ref.argmax_case(257, 7)
    assert np.isnan(p).sum() == 2 and (np.sort(p, axis=1)[:, -1] == np.sort(p, axis=1)[:, -2]).any()      # NaN row, equal maxima
    with pytest.raises(ZeroDivisionError):
        metrics_ref.eval_acc(np.full((4, 1), np.nan, dtype=np.float32), np.zeros((4, 3), dtype=np.float32))
    with pytest.raises(ZeroDivisionError):
        _reference_eval_acc(torch.full((4, 1), float("nan")), torch.zeros(4, 3))


@pytest.mark.parametrize("name", list(metrics_ref.cases()))
def test_the_gpu_tests_inputs_are_well_posed(name):
    """Every column a case claims is evaluated has P, N > 0 and nothing invalid under the oracle, and no other column has:
    the GPU test leaves out 0 cases."""
    y, s, evaluated = metrics_ref.cases()[name]
    tab = metrics_ref.table(y, s)
    assert metrics_ref.evaluated_columns(tab) == evaluated
    assert all(tab[c][3] == 0 for c in evaluated)
    assert all(sum(row[:4]) == y.shape[0] for row in tab)
    if name == "ties/700-across-a-chunk":
        order = np.sort(s[:, 0])
        assert (order[300:1000] == 0).all() and order[299] < 0 < order[1000]      # sorted positions 300..999 straddle 512
    if name == "ties/across-columns":
        merged = s.copy()
        merged[:, 1] += 0.5                                                       # the tie across the boundary is real:
        assert metrics_ref.table(y, s)[0] == metrics_ref.table(y, merged)[0]      # (columns are independent in the oracle)


def test_the_integer_formula_on_a_worked_example():
    # scores 1 2 2 3, labels 0 1 0 1: positives at 2 (one negative below, one tied) and 3 (two below) -> U2 = 3 + 4
    assert metrics_ref.column_counts(np.array([0, 1, 0, 1], dtype=np.uint8), np.array([1, 2, 2, 3], dtype=np.float32)) == (2, 2, 0, 0, 7)
    codes = metrics_ref.class_codes(np.array([[0.0], [1.0], [np.nan], [2.0], [1.0]], dtype=np.float32))
    assert codes[:, 0].tolist() == [0, 1, 2, 3, 1]
    assert metrics_ref.column_counts(codes[:, 0], np.array([0, np.inf, np.nan, 0, 1], dtype=np.float32)) == (1, 1, 1, 2, 2)


# ---- argument errors: before the device is touched ------------------------------------------------------------------------------
def test_value_errors_of_the_public_functions():
    import difformer_amd
    from difformer_amd import eval_acc, eval_f1, eval_rocauc, rocauc_counts
    assert {"eval_rocauc", "eval_acc", "eval_f1", "rocauc_counts"} <= set(difformer_amd.__all__)
    assert set(difformer_amd.metrics.__all__) >= {"eval_rocauc", "eval_acc", "eval_f1", "rocauc_counts"}
    y, p = torch.zeros(10, 3), torch.zeros(10, 3)
    for fn in (eval_rocauc, rocauc_counts, eval_acc, eval_f1):
        with pytest.raises(ValueError, match="2-d"):
            fn(torch.zeros(10), p)
        with pytest.raises(ValueError, match="2-d"):
            fn(y[:, :1], torch.zeros(10, 3, 1))
        with pytest.raises(ValueError, match="rows"):
            fn(y[:, :1], torch.zeros(9, 3))
        with pytest.raises(ValueError, match="float64"):
            fn(y[:, :1], p.double())
        with pytest.raises(ValueError, match="empty"):
            fn(torch.zeros(0, 1), torch.zeros(0, 3))
    for fn in (eval_rocauc, rocauc_counts):
        with pytest.raises(ValueError, match="columns"):
            fn(y, torch.zeros(10, 4))
        with pytest.raises(ValueError, match="at least 2 columns"):
            fn(y[:, :1], torch.zeros(10, 1))
    for fn in (eval_acc, eval_f1):
        with pytest.raises(ValueError, match=r"\[n, 1\]"):
            fn(y, p)


# ---- header and library ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def met():
    from difformer_amd import _lib
    if not os.path.exists(_lib.METRICS_LIB_PATH):
        pytest.skip("libdifformer_metrics.so not built")
    return _lib.load_metrics()


def test_header_names_equal_the_signature_table_and_the_library_exports_them(met):
    from difformer_amd import _lib
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(dif_[a-z0-9_]+)\s*\(", text)))
    assert declared == sorted(_lib.METRICS_SIGNATURES) == ["dif_argmax_correct_f32", "dif_metrics_last_error", "dif_metrics_version",
                                                           "dif_rocauc_counts_f32", "dif_rocauc_workspace_bytes"]
    for name in declared:
        assert getattr(met, name) is not None
    others = (set(_lib.SIGNATURES) | set(_lib.MAPS_SIGNATURES) | set(_lib.EDGES_SIGNATURES) | set(_lib.KNN_SIGNATURES)
              | set(_lib.SLOTS_SIGNATURES))
    assert not set(_lib.METRICS_SIGNATURES) & others
    assert len(_lib.METRICS_SIGNATURES["dif_rocauc_counts_f32"][1]) == len(ROC_ARGS)
    assert len(_lib.METRICS_SIGNATURES["dif_argmax_correct_f32"][1]) == len(ACC_ARGS)
    assert _lib.METRICS_SIGNATURES["dif_rocauc_workspace_bytes"][0] is ctypes.c_int64
    assert _lib.METRICS_SIGNATURES["dif_metrics_last_error"][0] is ctypes.c_char_p
    assert met.dif_metrics_version() == _lib.METRICS_VERSION == 1


def _roc(met, **over):
    """dif_rocauc_counts_f32 with made-up (never dereferenced) addresses: every rejection happens before any HIP call."""
    a = dict(score=0x10000, lds=112, cls=0x20001, ldc=112, n=100, C=112, counts=0x30000, workspace=0x40000, workspace_bytes=1 << 40,
             stream=None)
    a.update(over)
    return met.dif_rocauc_counts_f32(*[a[k] for k in ROC_ARGS])


def _acc(met, **over):
    a = dict(pred=0x10000, ldp=8, label=0x20000, labelled=0x30001, n=100, K=7, out=0x40000, stream=None)
    a.update(over)
    return met.dif_argmax_correct_f32(*[a[k] for k in ACC_ARGS])


@pytest.mark.parametrize("over,code", [
    (dict(score=None), "DIF_E_BADARG"), (dict(cls=None), "DIF_E_BADARG"), (dict(counts=None), "DIF_E_BADARG"),
    (dict(workspace=None), "DIF_E_BADARG"), (dict(score=0x10002), "DIF_E_BADARG"), (dict(counts=0x30004), "DIF_E_BADARG"),
    (dict(workspace=0x40008), "DIF_E_BADARG"), (dict(lds=111), "DIF_E_BADARG"), (dict(ldc=111), "DIF_E_BADARG"),
    (dict(n=0), "DIF_E_BADARG"), (dict(n=-5), "DIF_E_BADARG"), (dict(C=0), "DIF_E_SHAPE"),
    (dict(C=65537, lds=65537, ldc=65537, n=1), "DIF_E_SHAPE"), (dict(workspace_bytes=15), "DIF_E_WORKSPACE"),
    (dict(workspace_bytes=-1), "DIF_E_WORKSPACE"), (dict(n=(2 ** 31 - 1) // 112 + 1), "DIF_E_RANGE"), (dict(n=1 << 40), "DIF_E_RANGE"),
])
def test_every_argument_check_of_the_table_returns_its_code_without_a_gpu(met, over, code):
    from difformer_amd import _lib
    rc = _roc(met, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, met.dif_metrics_last_error())
    assert b"dif_rocauc_counts_f32" in met.dif_metrics_last_error()              # this library's text, not another's


@pytest.mark.parametrize("over,code", [
    (dict(pred=None), "DIF_E_BADARG"), (dict(label=None), "DIF_E_BADARG"), (dict(labelled=None), "DIF_E_BADARG"),
    (dict(out=None), "DIF_E_BADARG"), (dict(pred=0x10001), "DIF_E_BADARG"), (dict(label=0x20004), "DIF_E_BADARG"),
    (dict(out=0x40004), "DIF_E_BADARG"), (dict(ldp=6), "DIF_E_BADARG"), (dict(n=0), "DIF_E_BADARG"), (dict(K=0), "DIF_E_SHAPE"),
    (dict(K=65537, ldp=65537), "DIF_E_SHAPE"),
])
def test_every_argument_check_of_the_count_returns_its_code_without_a_gpu(met, over, code):
    from difformer_amd import _lib
    rc = _acc(met, **over)
    assert rc == _lib.ERROR_CODES[code], (rc, met.dif_metrics_last_error())
    assert b"dif_argmax_correct_f32" in met.dif_metrics_last_error()


def _workspace_formula(n, C):
    """The header's formula."""
    def A(x):
        return -(-x // 256) * 256
    m = n * C
    r = min(64, max(8, -(-m // 262144)))
    t = 256 * -(-m // (64 * r))
    s = max(m, t)
    return 5 * A(4 * m) + A(4 * t) + A(4 * (-(-s // 1024) + 1)) + 256


def test_the_workspace_is_host_arithmetic_one_byte_short_is_rejected_and_it_is_linear_in_the_pairs(met):
    from difformer_amd import _lib
    need = met.dif_rocauc_workspace_bytes(100, 112)
    assert need == _workspace_formula(100, 112) and need % 256 == 0
    assert _roc(met, workspace_bytes=need - 1) == _lib.ERROR_CODES["DIF_E_WORKSPACE"]
    assert b"workspace too small" in met.dif_metrics_last_error()
    # rejected shapes cost nothing
    assert met.dif_rocauc_workspace_bytes(0, 5) == 0 and met.dif_rocauc_workspace_bytes(5, 0) == 0
    assert met.dif_rocauc_workspace_bytes(5, 65537) == 0 and met.dif_rocauc_workspace_bytes(2 ** 31 - 1, 2) == 0
    assert met.dif_rocauc_workspace_bytes(2 ** 31 - 1, 1) == _workspace_formula(2 ** 31 - 1, 1)
    rng = np.random.default_rng(0)
    for _ in range(300):
        C = int(rng.integers(1, 300))
        n = int(10 ** rng.uniform(0, 7))
        if n * C <= 2 ** 31 - 1:
            assert met.dif_rocauc_workspace_bytes(n, C) == _workspace_formula(n, C), (n, C)
    # only the product matters, and the size is linear in it: 20 bytes per pair and at most 2 more for the table of the sort
    assert met.dif_rocauc_workspace_bytes(132534, 112) == met.dif_rocauc_workspace_bytes(132534 * 112, 1)
    sizes = [met.dif_rocauc_workspace_bytes(n, 112) for n in (1 << 18, 1 << 19, 1 << 20)]        # 64-round chunks throughout
    assert abs(sizes[1] - 2 * sizes[0]) <= 1024 and abs(sizes[2] - 2 * sizes[1]) <= 1024
    for n in (9, 20000, 132534, 1 << 20):
        assert 20 * n * 112 <= met.dif_rocauc_workspace_bytes(n, 112) <= 22 * n * 112 + 4096
