"""Evaluation metrics on the MI355X (csrc/eval_metrics.hip behind include/difformer_metrics.h): INTEGER equality of the whole
[C, 5] table {P, N, unlabelled, invalid, U2} with the oracle of tests/metrics_ref.py, and `==` of the float results (same
integers, same Python division, same summation order).  No tolerance anywhere.

Which case reaches which mechanism (tests/metrics_ref.py builds the inputs, tests/test_metrics_host.py shows them well-posed):
  sort chunks     n C in {1, 2, 3, 511, 512, 513, 2047, 2048, 2049} with one column: the 512-key wave chunk at 8 rounds and the
                  2,048-key block; with seven columns the nearest multiples of 7 on either side (7, 511, 518, 2044, 2051)
  scan tile       n C in {1023, 1024, 1025}; 7 n in {1022, 1029}
  longer chunks   20,000 x 112: 2.24 M pairs, 9 rounds per chunk
  column passes   C in {1, 2, 112, 256, 257} at n = 9: no pass, one pass, two passes on the column key
  tie groups      whole-number scores, constant scores (exactly 0.5), 700 equal scores across a chunk boundary, the last score of
                  a column equal to the first of the next, mixed signed zeros, denormals beside +-1e30
"""
import functools

import numpy as np
import pytest
import torch

from guarded import GuardedArena, guarded_inputs
import metrics_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def met():
    from difformer_amd import _lib
    return _lib.load_metrics()


@functools.lru_cache(maxsize=None)
def _oracle(name):
    """The oracle's table of a case, computed once and left unchanged."""
    y, s, _ = metrics_ref.cases()[name]
    return metrics_ref.table(y, s)


def _launch_table(met, sd, lds, cd, ldc, n, C, counts, ws):
    from difformer_amd import _lib
    rc = met.dif_rocauc_counts_f32(sd.data_ptr(), lds, cd.data_ptr(), ldc, n, C, counts.data_ptr(), ws.data_ptr(), ws.numel(),
                                   torch.cuda.current_stream().cuda_stream)
    _lib.check_metrics(rc, "dif_rocauc_counts_f32")


def _table(met, y, s):
    """The entry point on column slices of wider device tensors (lds, ldc > C; NaN scores and code 3 around them), the output
    and the workspace pre-filled with 0xFF."""
    n, C = s.shape
    wide_s = torch.full((n, C + 5), float("nan"))
    wide_s[:, 3:3 + C] = torch.from_numpy(s)
    wide_c = torch.full((n, C + 3), 3, dtype=torch.uint8)
    wide_c[:, 1:1 + C] = torch.from_numpy(metrics_ref.class_codes(y))
    sd, cd = wide_s.to(DEV), wide_c.to(DEV)
    counts = torch.full((C, 5), -1, dtype=torch.int64, device=DEV)
    ws = torch.full((met.dif_rocauc_workspace_bytes(n, C),), 0xFF, dtype=torch.uint8, device=DEV)
    _launch_table(met, sd[:, 3:], sd.stride(0), cd[:, 1:], cd.stride(0), n, C, counts, ws)
    torch.cuda.synchronize()
    return counts.cpu().tolist()


# ---- the table through the C ABI --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(metrics_ref.cases()))
def test_the_table_equals_the_oracle(met, name):
    y, s, _ = metrics_ref.cases()[name]
    assert _table(met, y, s) == _oracle(name)


@pytest.mark.parametrize("name", [f"chunk/C1/n{n}" for n in metrics_ref.ONE_COLUMN_ROWS])
def test_raw_scores_of_one_column_through_the_backend(name):
    from difformer_amd import ops
    y, s, _ = metrics_ref.cases()[name]
    got = ops.get_backend().rocauc_counts(torch.from_numpy(s).to(DEV), torch.from_numpy(metrics_ref.class_codes(y)).to(DEV))
    assert got.dtype == torch.int64 and got.device.type == "cuda" and got.cpu().tolist() == _oracle(name)


def test_two_calls_return_identical_tables(met):
    y, s, _ = metrics_ref.cases()["long"]
    first = _table(met, y, s)
    assert first == _table(met, y, s) == _oracle("long")


@pytest.mark.parametrize("name", ["chunk/C7/n74", "ties/700-across-a-chunk", "passes/C257", "ties/across-columns"])
def test_between_guard_bands(met, name):
    """Operands at their minimum alignment between poisoned bands (the tail of every row poisoned too), the output and the
    workspace poisoned (0xFF) between checked guard bands."""
    y, s, _ = metrics_ref.cases()[name]
    n, C = s.shape
    arena = GuardedArena()
    sd, = guarded_inputs(arena, DEV, 4, s=(torch.from_numpy(s), C + 3))
    cd, = guarded_inputs(arena, DEV, 1, c=(torch.from_numpy(metrics_ref.class_codes(y)), C + 1))
    counts = arena.alloc((C, 5), torch.int64, DEV, offset_bytes=8)
    ws = arena.alloc((met.dif_rocauc_workspace_bytes(n, C),), torch.uint8, DEV, offset_bytes=16)
    _launch_table(met, sd, C + 3, cd, C + 1, n, C, counts, ws)
    arena.check()
    assert counts.cpu().tolist() == _oracle(name)
    K = 7
    yl, p = metrics_ref.argmax_case(257, K)
    lab = yl[:, 0] == yl[:, 0]
    pd, = guarded_inputs(arena, DEV, 4, p=(torch.from_numpy(p), K + 2))
    ld, md = guarded_inputs(arena, DEV, 8, label=torch.from_numpy(np.where(lab, yl[:, 0], -1).astype(np.int64)),
                            mask=torch.from_numpy(lab.astype(np.uint8)))
    out = arena.alloc((2,), torch.int64, DEV, offset_bytes=8)
    from difformer_amd import _lib
    _lib.check_metrics(met.dif_argmax_correct_f32(pd.data_ptr(), K + 2, ld.data_ptr(), md.data_ptr(), 257, K, out.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream), "dif_argmax_correct_f32")
    arena.check()
    assert tuple(out.cpu().tolist()) == metrics_ref.argmax_counts(yl, p)


# ---- eval_rocauc ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["passes/C2", "passes/C112", "passes/C257", "ties/integer", "ties/integer-int64-labels", "ties/constant",
                                  "ties/across-columns", "ties/signed-zeros", "order/denormals", "labels/skipped-columns",
                                  "scores/ignored-non-finite", "chunk/C7/n293", "long"])
def test_eval_rocauc_equals_the_oracle(name):
    from difformer_amd import eval_rocauc, ops, rocauc_counts
    y, s, evaluated = metrics_ref.cases()[name]
    yd, sd = torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV)
    be = ops.get_backend()
    be.kernel_events = events = {}
    try:
        got = eval_rocauc(yd, sd)
    finally:
        be.kernel_events = None
    assert "dif_rocauc_counts_f32" in events
    assert isinstance(got, float) and got == metrics_ref.eval_rocauc(y, s)
    tab = rocauc_counts(yd, sd)
    assert tab.device.type == "cuda" and tab.dtype == torch.int64 and tab.cpu().tolist() == _oracle(name)
    if name == "ties/constant":
        assert got == 0.5 and all(U2 / (2 * P * N) == 0.5 for P, N, _, _, U2 in tab.cpu().tolist())
    if name == "ties/integer-int64-labels":
        assert yd.dtype == torch.int64


def test_eval_rocauc_errors_follow_the_reference():
    from difformer_amd import eval_rocauc
    y, s, _ = metrics_ref.cases()["labels/skipped-columns"]
    yd, sd = torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV)
    with pytest.raises(RuntimeError, match="No positively labeled data available. Cannot compute ROC-AUC."):
        eval_rocauc(yd[:, [1, 3, 4]], sd[:, [1, 3, 4]])                          # all 1s, all 0s, {1, 2}: nothing to evaluate
    assert eval_rocauc(yd, sd) == metrics_ref.eval_rocauc(y, s)                  # the value 2 in a skipped column: no error
    bad = yd.clone()
    bad[5, 2] = 2
    with pytest.raises(ValueError, match="column 2"):
        eval_rocauc(bad, sd)
    # a NaN or infinite score in a labelled row of an evaluated column raises, in an unlabelled row it is ignored
    y, s, _ = metrics_ref.cases()["scores/ignored-non-finite"]
    yd = torch.from_numpy(y).to(DEV)
    assert eval_rocauc(yd, torch.from_numpy(s).to(DEV)) == metrics_ref.eval_rocauc(y, s)
    for value in (float("nan"), float("inf"), float("-inf")):
        sb = torch.from_numpy(s).to(DEV)
        sb[0, 1] = value                                                         # (row 0 is labelled in every column)
        assert y[0, 1] == 1
        with pytest.raises(ValueError, match="column 1"):
            eval_rocauc(yd, sb)
    with pytest.raises(ValueError, match="float64"):
        eval_rocauc(yd, torch.from_numpy(s).to(DEV).double())


def test_eval_rocauc_dtypes_layouts_and_host_tensors():
    from difformer_amd import eval_rocauc, rocauc_counts
    y, s, _ = metrics_ref.cases()["passes/C112"]
    yd = torch.from_numpy(y).to(DEV)
    for dtype in (torch.bfloat16, torch.float16):                                # widened exactly: heavy ties at 8 / 11 bits
        low = torch.from_numpy(s).to(dtype)
        assert eval_rocauc(yd, low.to(DEV)) == metrics_ref.eval_rocauc(y, low.float().numpy())
    wide = torch.randn(9, 120)
    wide[:, 4:116] = torch.from_numpy(s)
    view = wide.to(DEV)[:, 4:116]                                                # a column slice: rows 120 apart
    assert not view.is_contiguous() and eval_rocauc(yd, view) == metrics_ref.eval_rocauc(y, s)
    stepped = torch.from_numpy(np.repeat(s, 2, axis=1)).to(DEV)[:, ::2]          # column stride 2: copied
    assert stepped.stride(1) == 2 and eval_rocauc(yd, stepped) == metrics_ref.eval_rocauc(y, s)
    want = eval_rocauc(yd, torch.from_numpy(s).to(DEV))
    host = eval_rocauc(torch.from_numpy(y), torch.from_numpy(s))                 # host tensors are staged: evaluate_cpu
    assert isinstance(host, float) and host == want
    tab = rocauc_counts(torch.from_numpy(y), torch.from_numpy(s))
    assert tab.device.type == "cpu" and tab.tolist() == _oracle("passes/C112")
    with pytest.raises(ValueError, match="y_true on"):
        eval_rocauc(torch.from_numpy(y), torch.from_numpy(s).to(DEV))
    grad = torch.from_numpy(s).to(DEV).requires_grad_()
    assert eval_rocauc(yd, grad * 1.0) == want                                   # detached


def test_wide_tables_go_in_column_groups(monkeypatch):
    from difformer_amd import metrics
    y, s, _ = metrics_ref.cases()["passes/C257"]
    monkeypatch.setattr(metrics, "MAX_PAIRS", 9 * 100)                           # 257 columns in groups of 100, 100, 57
    tab = metrics.rocauc_counts(torch.from_numpy(y).to(DEV), torch.from_numpy(s).to(DEV))
    assert tab.shape == (257, 5) and tab.cpu().tolist() == _oracle("passes/C257")


def test_one_label_column_takes_the_softmax_branch():
    """y_pred [n, 2] -> softmax(y_pred)[:, 1]; saturated logits (+-40) collapse to long tie groups.  The oracle is fed the
    softmax values read back from the device."""
    from difformer_amd import eval_rocauc, rocauc_counts
    rng = np.random.default_rng(7)
    n = 3000
    logits = rng.standard_normal((n, 2)).astype(np.float32)
    sat = rng.random(n) < 0.6
    logits[sat] = np.where(rng.random((int(sat.sum()), 2)) < 0.5, 40.0, -40.0)
    y = metrics_ref.labels(n, 1, 7)
    ld, yd = torch.from_numpy(logits).to(DEV), torch.from_numpy(y).to(DEV)
    prob = torch.softmax(ld, dim=-1)[:, 1:2].cpu().numpy()
    values, counts = np.unique(prob, return_counts=True)
    assert counts.max() > 500                                                    # tie groups of hundreds
    assert rocauc_counts(yd, ld).cpu().tolist() == metrics_ref.table(y, prob)
    assert eval_rocauc(yd, ld) == metrics_ref.eval_rocauc(y, prob)
    three = torch.from_numpy(rng.standard_normal((n, 3)).astype(np.float32)).to(DEV)        # column 1 of three classes
    assert eval_rocauc(yd, three) == metrics_ref.eval_rocauc(y, torch.softmax(three, dim=-1)[:, 1:2].cpu().numpy())


# ---- eval_acc / eval_f1 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", metrics_ref.ARGMAX_COLUMNS)
@pytest.mark.parametrize("n", metrics_ref.ARGMAX_ROWS)
def test_eval_acc_and_eval_f1_equal_the_oracle(n, K):
    from difformer_amd import eval_acc, eval_f1, ops
    y, p = metrics_ref.argmax_case(n, K)
    yd, pd = torch.from_numpy(y).to(DEV), torch.from_numpy(p).to(DEV)
    lab = y[:, 0] == y[:, 0]
    out = ops.get_backend().argmax_correct(pd, torch.from_numpy(np.where(lab, y[:, 0], -1).astype(np.int64)).to(DEV),
                                           torch.from_numpy(lab.astype(np.uint8)).to(DEV))
    assert tuple(out.cpu().tolist()) == metrics_ref.argmax_counts(y, p)
    if lab.any():
        assert eval_acc(yd, pd) == metrics_ref.eval_acc(y, p)
        assert eval_acc(torch.from_numpy(y), torch.from_numpy(p)) == metrics_ref.eval_acc(y, p)          # host tensors
    whole = np.where(lab[:, None], y, 0).astype(np.int64)                               # integer labels: nothing excluded
    assert eval_f1(torch.from_numpy(whole).to(DEV), pd) == metrics_ref.eval_f1(whole, p)
    assert eval_acc(torch.from_numpy(whole).to(DEV), pd.to(torch.bfloat16)) == metrics_ref.eval_acc(whole, p)   # whole numbers: exact
    if not lab.all():
        with pytest.raises(ValueError, match="NaN"):
            eval_f1(yd, pd)


def test_first_maximum_nan_rows_and_nothing_labelled():
    from difformer_amd import eval_acc
    p = torch.tensor([[1.0, 3.0, 3.0, 0.0], [float("nan"), 9.0, float("nan"), 0.0], [-0.0, 0.0, -1.0, -2.0], [5.0, 5.0, 5.0, 5.0]])
    for labels, want in (([1, 0, 0, 0], 1.0), ([2, 2, 1, 3], 0.0), ([1, 2, 0, 1], 0.5)):
        assert eval_acc(torch.tensor(labels).view(-1, 1).to(DEV), p.to(DEV)) == want
    wide = torch.zeros(3, 200)
    wide[0, 130], wide[0, 70] = 2.0, 2.0                                         # equal maxima in different lanes' strides
    wide[1, 199] = float("nan")
    wide[2, 64], wide[2, 0] = 1.0, 1.0
    assert eval_acc(torch.tensor([[70.0], [199.0], [0.0]]).to(DEV), wide.to(DEV)) == 1.0
    with pytest.raises(ZeroDivisionError):
        eval_acc(torch.full((5, 1), float("nan")).to(DEV), torch.zeros(5, 3).to(DEV))
