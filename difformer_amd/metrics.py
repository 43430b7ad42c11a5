"""The evaluation metrics of the reference's drivers, computed on the device as exact integers.

`node classification/data_utils.py:238-285` (copied in `image and text/data_utils.py:180-216`) moves the logits to the host
and evaluates there: `eval_rocauc` is a Python loop of one `sklearn.metrics.roc_auc_score` per label column, `eval_acc` and
`eval_f1` take an argmax and count.  `eval_rocauc`, `eval_acc` and `eval_f1` here take the same arguments in the same order
and return the same Python float from csrc/eval_metrics.hip (C ABI include/difformer_metrics.h); nothing of sklearn is used.
A driver switches by changing one import:

    from difformer_amd.metrics import eval_acc, eval_rocauc, eval_f1

The contract is on INTEGERS.  For one label column, restricted to its labelled rows, let P be the number of labels equal to
1 and N the number equal to 0, and compare scores as float32 values (so -0.0 == +0.0):

    U2 = sum over positive rows p of ( 2 #{negatives with score < s_p} + #{negatives with score == s_p} )

`roc_auc_score` is U2 / (2 P N): the Mann-Whitney statistic with mid-ranks, which is the trapezoid area under the ROC curve.
The device returns {P, N, unlabelled, invalid, U2} per column (`rocauc_counts`) and the host divides Python ints, so the
quotient is correctly rounded and the result is bitwise reproducible.  Accuracy is likewise `correct / labelled` of two
integers.

y_pred may be float32, bfloat16 or float16 (widened to float32, which is exact); float64 raises, because narrowing it would
create ties the reference does not have.  Host tensors are staged through the GPU (`evaluate_cpu` of eval.py:34-43 hands over
`out[split_idx]` on the host); mixed placements raise.  Everything is detached and runs on the current stream.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import ops
from . import staging

__all__ = ["eval_rocauc", "eval_acc", "eval_f1", "rocauc_counts"]

MAX_PAIRS = 2 ** 31 - 1     # (row, column) pairs of one sort (kMaxPairs of csrc/eval_metrics.hip): wider tables go in column groups
_PRED_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _check(who, y_true, y_pred, single):
    """The argument errors, before the device is touched -> (n, C_true, C_pred)."""
    for name, t in (("y_true", y_true), ("y_pred", y_pred)):
        if not torch.is_tensor(t) or t.dim() != 2:
            raise ValueError(f"{who}: {name} must be a 2-d tensor (got {tuple(t.shape) if torch.is_tensor(t) else type(t).__name__})")
    if y_pred.dtype not in _PRED_DTYPES:
        raise ValueError(f"{who}: y_pred must be float32, bfloat16 or float16 (got {y_pred.dtype}); float64 scores are not "
                         "narrowed: that would create ties the reference does not have")
    if y_true.dtype.is_complex:
        raise ValueError(f"{who}: y_true must be integer or floating (got {y_true.dtype})")
    n, ct = y_true.shape
    if y_pred.shape[0] != n:
        raise ValueError(f"{who}: y_true has {n} rows, y_pred {y_pred.shape[0]}")
    cp = y_pred.shape[1]
    if n < 1 or ct < 1 or cp < 1:
        raise ValueError(f"{who}: empty inputs (y_true {tuple(y_true.shape)}, y_pred {tuple(y_pred.shape)})")
    if single and ct != 1:
        raise ValueError(f"{who}: y_true must be [n, 1] (got {tuple(y_true.shape)}); the reference indexes the argmax column "
                         "out of range there")
    if not single:
        if ct == 1 and cp < 2:
            raise ValueError(f"{who}: y_true [n, 1] takes the probability of class 1: y_pred needs at least 2 columns (got {cp})")
        if ct > 1 and cp != ct:
            raise ValueError(f"{who}: y_pred has {cp} columns for {ct} label columns")
    if y_true.device != y_pred.device:
        raise ValueError(f"{who}: y_true on {y_true.device}, y_pred on {y_pred.device}")
    return n, ct, cp


def _class_codes(y_true):
    """uint8 codes of csrc/eval_metrics.hip: 0 = negative, 1 = positive, 2 = unlabelled (NaN), 3 = any other value."""
    other = torch.full((), 3, dtype=torch.uint8, device=y_true.device)
    codes = torch.where(y_true == 1, other - 2, torch.where(y_true == 0, other - 3, other))
    if y_true.is_floating_point():
        codes = torch.where(y_true != y_true, other - 1, codes)
    return codes


def _scores(y_true, y_pred):
    """data_utils.py:267-271: the probability of class 1 for a single label column, the raw outputs otherwise."""
    y_pred = y_pred.detach().float()
    if y_true.shape[1] == 1:
        return F.softmax(y_pred, dim=-1)[:, 1].unsqueeze(1)
    return y_pred


def _rocauc_counts(y_true, score):
    n, C = score.shape
    if n > MAX_PAIRS:
        raise ValueError(f"difformer_amd: {n} rows exceed the limit of {MAX_PAIRS} per column")
    codes = _class_codes(y_true.detach())
    be = ops.get_backend()
    per = MAX_PAIRS // n
    if C <= per:
        return be.rocauc_counts(score, codes)
    return torch.cat([be.rocauc_counts(score[:, a:a + per], codes[:, a:a + per]) for a in range(0, C, per)])


def rocauc_counts(y_true, y_pred):
    """y_true [n, C] (integer or floating; NaN = unlabelled), y_pred as for `eval_rocauc` -> int64 [C, 5] on the inputs'
    device: per label column {P, N, unlabelled, invalid, U2}.  P / N count the labels 1 / 0 with a finite score; `invalid`
    counts the labels that are neither 0, 1 nor NaN and the labelled rows whose score is NaN or infinite (sklearn raises for
    either).  roc_auc_score of the column is U2 / (2 P N).  No host synchronisation for device inputs."""
    _check("rocauc_counts", y_true, y_pred, False)
    dev = staging.staging_device(None, (y_true, y_pred))
    if dev is not None:      # host tensors: computed on the GPU, returned on the host
        return rocauc_counts(y_true.to(dev), y_pred.to(dev)).to(y_true.device)
    with torch.no_grad():
        return _rocauc_counts(y_true, _scores(y_true, y_pred))


def eval_rocauc(y_true, y_pred):
    """`eval_rocauc` of data_utils.py:262-285.  y_true [n, C]; with C == 1 the scores are `softmax(y_pred, -1)[:, 1]`
    (:267-269), otherwise y_pred is [n, C] (:271).  A column is evaluated iff it has a positive and a negative (:275), over
    its labelled rows (:276-277); the result is the Python `sum(list) / len(list)` of the evaluated columns' U2 / (2 P N) in
    ascending column order (:279, :285).  No evaluated column: the reference's RuntimeError (:281-283).  An evaluated column
    with a third label value or a non-finite score in a labelled row raises ValueError, as roc_auc_score does; non-finite
    scores in skipped columns or unlabelled rows are never shown to sklearn and are ignored here too.  (One corner differs:
    a column whose ONLY positives or negatives carry non-finite scores is skipped here, where sklearn raises.)"""
    _check("eval_rocauc", y_true, y_pred, False)
    table = rocauc_counts(y_true, y_pred).tolist()
    rocauc_list = []
    for i, (P, N, _, invalid, U2) in enumerate(table):
        if P > 0 and N > 0:
            if invalid > 0:
                raise ValueError(f"eval_rocauc: column {i} has {invalid} labelled rows with a label other than 0 / 1 or a "
                                 "NaN / infinite score")
            rocauc_list.append(U2 / (2 * P * N))
    if len(rocauc_list) == 0:
        raise RuntimeError('No positively labeled data available. Cannot compute ROC-AUC.')
    return sum(rocauc_list) / len(rocauc_list)


def _argmax_counts(who, y_true, y_pred):
    """-> (correct, labelled) as Python ints: rows whose label is not NaN, and those among them whose label equals the
    argmax of y_pred's row (first maximal index, NaN above every number: torch.argmax)."""
    _check(who, y_true, y_pred, True)
    dev = staging.staging_device(None, (y_true, y_pred))
    if dev is not None:
        y_true, y_pred = y_true.to(dev), y_pred.to(dev)
    with torch.no_grad():
        yt = y_true.detach()[:, 0]
        if yt.is_floating_point():
            labelled = yt == yt
            whole = labelled & torch.isfinite(yt) & (yt == yt.trunc())       # any other value equals no index
            label = torch.where(whole, yt, torch.full((), -1, dtype=yt.dtype, device=yt.device)).to(torch.int64)
        else:
            labelled = torch.ones_like(yt, dtype=torch.bool)
            label = yt.to(torch.int64)
        out = ops.get_backend().argmax_correct(y_pred.detach().float(), label, labelled.to(torch.uint8))
    correct, n_labelled = out.tolist()
    return correct, n_labelled


def eval_acc(y_true, y_pred):
    """`eval_acc` of data_utils.py:249-259: y_true [n, 1], y_pred [n, K]; rows whose label is NaN are excluded (:255), the
    result is correct / labelled (:256-257) and ZeroDivisionError when nothing is labelled, as there."""
    correct, labelled = _argmax_counts("eval_acc", y_true, y_pred)
    return correct / labelled


def eval_f1(y_true, y_pred):
    """`eval_f1` of data_utils.py:238-247: micro-F1 of single-label multiclass predictions, y_true [n, 1] of whole numbers,
    which is correct / n.  NaN labels raise ValueError, as sklearn's f1_score does."""
    correct, labelled = _argmax_counts("eval_f1", y_true, y_pred)
    if labelled != y_true.shape[0]:
        raise ValueError(f"eval_f1: y_true holds {y_true.shape[0] - labelled} NaN labels")
    return correct / y_true.shape[0]
