"""The two training losses of the reference's drivers, each one pass over the logits forward and one pass backward.

    log_softmax_nll(out, label, rows=None, ignore_index=-100)
        == F.nll_loss(F.log_softmax(out, dim=1)[rows], label.squeeze(1)[rows], ignore_index=ignore_index)
    bce_with_logits(out, target, rows=None)
        == F.binary_cross_entropy_with_logits(out[rows], target[rows].float())

`node classification/main.py:121-129` and `image and text/main.py:107-109` select the training rows with an index,
`main-batch.py:136-140` with a boolean mask, `eval.py:19-29` evaluates the same two expressions on the validation rows and
`physical particle/main.py:88` takes every row.  `rows` is accordingly None (all rows), an int64 index in any order (a row
counts as often as it occurs) or a bool mask of length n.  `label` is int64 [n] or [n, 1]; `target` is [n, C] and is read in
the type it is stored in (int64, float32, uint8 or bool; other integer and 16-bit float types are converted on the device), so
the `.to(torch.float)` of the scripts disappears.  A driver changes two lines:

    from difformer_amd.losses import log_softmax_nll
    loss = log_softmax_nll(out, dataset.label, train_idx)          # was: criterion(F.log_softmax(out, dim=1)[train_idx], ...)

Device tensors go through csrc/loss.hip (C ABI include/difformer_loss.h): every logit is widened to float64, the row is
evaluated in float64, the weighted sum runs in a fixed order and is divided by the count on the device, and the gradient
`weight * upstream / count * dl/dx` is rounded once to the logits' type.  The selection becomes a per-row weight -- nothing is
gathered, `out[mask]` (whose `nonzero` waits for the host in every step) is never formed, and NOTHING synchronises with the
host, so a step with a boolean-mask loss can be captured by `GraphedTrainStep`.  Two calls on equal operands return bitwise
equal results.

Returns a 0-d tensor in the logits' dtype (float32, or bfloat16 for bfloat16 logits, as torch), differentiable in `out`
(first derivatives only).  Edge semantics (include/difformer_loss.h): unselected and ignored rows are never read, so NaN or
infinite logits there change nothing and their gradient rows are +0; nothing selected gives NaN and a zero gradient; a label
outside [0, C) other than `ignore_index`, or an index outside [0, n), makes the loss NaN instead of aborting the process
(`loss_record` returns how many there were).

CPU tensors take the torch expression above, unchanged (`evaluate_cpu` of eval.py:34-43 calls the criterion on the host).
Mixed placements, float64 logits and wrong shapes raise ValueError before the device is touched.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

from . import ops

__all__ = ["log_softmax_nll", "bce_with_logits", "loss_record"]

MAX_COLUMNS = 65536         # kMaxColumns of csrc/loss.hip
_LOGIT_DTYPES = (torch.float32, torch.bfloat16)
_TARGET_DTYPES = (torch.int64, torch.float32, torch.uint8, torch.bool)
_CONVERTED_TARGET_DTYPES = (torch.int8, torch.int16, torch.int32, torch.float16, torch.bfloat16)      # exact in float32


def _check(who, out, second, second_name, rows):
    """The argument errors, before the device is touched -> (n, C)."""
    for name, t in (("out", out), (second_name, second)):
        if not torch.is_tensor(t):
            raise ValueError(f"{who}: {name} must be a tensor (got {type(t).__name__})")
    if out.dim() != 2:
        raise ValueError(f"{who}: out must be [n, C] (got {tuple(out.shape)})")
    if out.dtype not in _LOGIT_DTYPES:
        raise ValueError(f"{who}: out must be float32 or bfloat16 (got {out.dtype}); float64 logits are not narrowed")
    n, C = out.shape
    if not 1 <= C <= MAX_COLUMNS:
        raise ValueError(f"{who}: need 1 <= C <= {MAX_COLUMNS} columns (got {C})")
    if second.device != out.device:
        raise ValueError(f"{who}: out on {out.device}, {second_name} on {second.device}")
    if rows is not None:
        if not torch.is_tensor(rows) or rows.dim() != 1 or rows.dtype not in (torch.int64, torch.bool):
            raise ValueError(f"{who}: rows must be None, a 1-d int64 index or a 1-d bool mask (got "
                             f"{(rows.dtype, tuple(rows.shape)) if torch.is_tensor(rows) else type(rows).__name__})")
        if rows.dtype == torch.bool and rows.shape[0] != n:
            raise ValueError(f"{who}: the mask has {rows.shape[0]} entries for {n} rows")
        if rows.device != out.device:
            raise ValueError(f"{who}: out on {out.device}, rows on {rows.device}")
    return n, C


def _selection(rows, n):
    """rows -> (int32 weights | uint8 mask | None, the status word of the index or None); device work only."""
    if rows is None:
        return None, None
    if rows.dtype == torch.bool:
        return rows.contiguous().view(torch.uint8), None
    return ops.get_backend().loss_row_weights(rows.detach(), n)


class _Loss(torch.autograd.Function):
    """One loss of csrc/loss.hip: `kind` 'nll' (second = int64 labels [n]) or 'bce' (second = target [n, C])."""

    @staticmethod
    def forward(ctx, out, kind, second, rows, ignore_index):
        be = ops.get_backend()
        weights, status = _selection(rows, out.shape[0])
        x = out.detach()
        record = be.loss_forward(kind, x, second, weights, status, ignore_index)
        ctx.kind, ctx.ignore_index = kind, ignore_index
        ctx.save_for_backward(x, second, weights, record)
        loss = record.view(torch.float32)[2]
        return loss.clone() if out.dtype == torch.float32 else loss.to(out.dtype)

    @staticmethod
    @once_differentiable
    def backward(ctx, upstream):
        x, second, weights, record = ctx.saved_tensors
        grad = ops.get_backend().loss_backward(ctx.kind, x, second, record, upstream.detach().float().reshape(1), weights,
                                               ctx.ignore_index)
        return grad, None, None, None, None


def _labels(who, label, n):
    if label.dtype != torch.int64 or not (tuple(label.shape) == (n,) or tuple(label.shape) == (n, 1)):
        raise ValueError(f"{who}: label must be int64 [n] or [n, 1] with n = {n} (got {label.dtype}, {tuple(label.shape)})")
    return label.reshape(n)


def _target(who, target, n, C):
    if tuple(target.shape) != (n, C):
        raise ValueError(f"{who}: target must be {(n, C)} like out (got {tuple(target.shape)})")
    if target.dtype not in _TARGET_DTYPES + _CONVERTED_TARGET_DTYPES:
        raise ValueError(f"{who}: target must be int64, float32, uint8 or bool, or a narrower integer or 16-bit float type "
                         f"(got {target.dtype})")
    return target


def _device_target(target):
    target = target.detach()
    if target.dtype == torch.bool:
        return target.view(torch.uint8) if target.stride(-1) == 1 else target.to(torch.uint8)
    return target.float() if target.dtype in _CONVERTED_TARGET_DTYPES else target


def log_softmax_nll(out, label, rows=None, ignore_index=-100):
    """mean over the selected rows r whose label is not `ignore_index` of  logsumexp(out[r]) - out[r, label[r]]:
    `F.nll_loss(F.log_softmax(out, dim=1)[rows], label.squeeze(1)[rows], ignore_index=ignore_index)`.
    out [n, C] float32 or bfloat16, label int64 [n] or [n, 1], rows None | int64 index | bool mask [n]."""
    who = "log_softmax_nll"
    n, _ = _check(who, out, label, "label", rows)
    flat = _labels(who, label, n)
    if not out.is_cuda:
        logp = F.log_softmax(out, dim=1)
        return F.nll_loss(logp if rows is None else logp[rows], flat if rows is None else flat[rows], ignore_index=ignore_index)
    return _Loss.apply(out, "nll", flat.detach(), rows, int(ignore_index))


def bce_with_logits(out, target, rows=None):
    """mean over the selected rows and all C columns of  max(x, 0) - x t + log1p(exp(-|x|)):
    `F.binary_cross_entropy_with_logits(out[rows], target[rows].float())`.
    out [n, C] float32 or bfloat16, target [n, C], rows None | int64 index | bool mask [n]."""
    who = "bce_with_logits"
    n, C = _check(who, out, target, "target", rows)
    target = _target(who, target, n, C)
    if not out.is_cuda:
        if rows is None:
            return F.binary_cross_entropy_with_logits(out, target.float())
        return F.binary_cross_entropy_with_logits(out[rows], target[rows].float())
    return _Loss.apply(out, "bce", _device_target(target), rows, -100)


def loss_record(kind, out, second, rows=None, ignore_index=-100):
    """The forward's record for device tensors, without a host synchronisation: (float64 loss, int64 count, int64 invalid) as
    0-d device tensors.  kind 'nll' (second = label) or 'bce' (second = target); `count` is the divisor of the mean, `invalid`
    the number of labels outside [0, C) other than ignore_index plus the indices outside [0, n) (the loss is NaN if any)."""
    if kind not in ("nll", "bce"):
        raise ValueError(f"loss_record: kind must be 'nll' or 'bce' (got {kind!r})")
    n, C = _check("loss_record", out, second, "label" if kind == "nll" else "target", rows)
    second = _labels("loss_record", second, n).detach() if kind == "nll" else _device_target(_target("loss_record", second, n, C))
    if not out.is_cuda:
        raise ValueError("loss_record: the record is the device kernels' output; CPU tensors have none")
    with torch.no_grad():
        weights, status = _selection(rows, n)
        record = ops.get_backend().loss_forward(kind, out.detach(), second, weights, status, int(ignore_index))
    ints = record.view(torch.int64)
    return record[0], ints[2], ints[3]
