"""Oracle of the evaluation metrics (difformer_amd/metrics.py, csrc/eval_metrics.hip): plain numpy and Python ints.

Per label column the integers (P, N, unlabelled, invalid, U2) of include/difformer_metrics.h, the three metric functions
restated from the reference's loops (node classification/data_utils.py:238-285) with the integer formula in place of sklearn,
and the inputs of the GPU tests.  Scores are float32 and compared as float32 values (numpy keeps denormals and takes
-0.0 == +0.0), so the order is the one the device's integer keys give.
"""
import functools

import numpy as np

NO_DATA = "No positively labeled data available. Cannot compute ROC-AUC."


# ---- the integers ----------------------------------------------------------------------------------------------------------------
def class_codes(y_true):
    """0 = negative, 1 = positive, 2 = unlabelled (NaN), 3 = any other value."""
    y = np.asarray(y_true)
    codes = np.full(y.shape, 3, dtype=np.uint8)
    codes[y == 0] = 0
    codes[y == 1] = 1
    if y.dtype.kind == "f":
        codes[y != y] = 2
    return codes


def column_counts(codes, score):
    """One column -> (P, N, unlabelled, invalid, U2) as Python ints."""
    score = np.asarray(score, dtype=np.float32)
    fin = np.isfinite(score)
    pos, neg = (codes == 1) & fin, (codes == 0) & fin
    unlabelled = int((codes == 2).sum())
    P, N = int(pos.sum()), int(neg.sum())
    sn = np.sort(score[neg])
    lt = np.searchsorted(sn, score[pos], side="left")
    le = np.searchsorted(sn, score[pos], side="right")
    U2 = sum(int(v) for v in 2 * lt.astype(np.int64) + (le - lt))
    return P, N, unlabelled, len(codes) - P - N - unlabelled, U2


def table(y_true, score):
    """[C][5] Python ints for y_true [n, C] and float32 scores [n, C]."""
    codes = class_codes(y_true)
    score = np.asarray(score, dtype=np.float32)
    assert codes.shape == score.shape and codes.ndim == 2
    return [list(column_counts(codes[:, c], score[:, c])) for c in range(codes.shape[1])]


def evaluated_columns(tab):
    return [c for c, (P, N, *_rest) in enumerate(tab) if P > 0 and N > 0]


# ---- the metric functions, as the reference loops -----------------------------------------------------------------------------------
def eval_rocauc(y_true, score):
    """data_utils.py:262-285 on the scores the loop sees (for one label column: softmax(y_pred)[:, 1:2])."""
    rocauc_list = []
    for c, (P, N, _, invalid, U2) in enumerate(table(y_true, score)):
        if P > 0 and N > 0:
            if invalid:
                raise ValueError(f"column {c}")
            rocauc_list.append(U2 / (2 * P * N))
    if len(rocauc_list) == 0:
        raise RuntimeError(NO_DATA)
    return sum(rocauc_list) / len(rocauc_list)


def argmax_counts(y_true, y_pred):
    """-> (correct, labelled): rows of y_true [n, 1] that are not NaN, and those whose label equals numpy's argmax (first
    maximal index, NaN above every number)."""
    y = np.asarray(y_true)[:, 0]
    pred = np.argmax(np.asarray(y_pred, dtype=np.float32), axis=-1)
    labelled = y == y
    return int((y[labelled] == pred[labelled]).sum()), int(labelled.sum())


def eval_acc(y_true, y_pred):
    correct, labelled = argmax_counts(y_true, y_pred)
    return correct / labelled


def eval_f1(y_true, y_pred):
    y = np.asarray(y_true)
    if y.dtype.kind == "f" and (y != y).any():
        raise ValueError("NaN labels")
    return argmax_counts(y, y_pred)[0] / y.shape[0]


# ---- inputs ----------------------------------------------------------------------------------------------------------------------------
def labels(n, C, seed, nan_frac=0.15, positives=0.3, dtype=np.float32):
    """Labels [n, C] in {0, 1} (NaN rows with a floating dtype).  With n >= 2 every column holds a 1 (row 0) and a 0 (row 1)."""
    rng = np.random.default_rng(seed)
    y = (rng.random((n, C)) < positives).astype(dtype)
    if np.dtype(dtype).kind == "f" and nan_frac:
        y[rng.random((n, C)) < nan_frac] = np.nan
    if n >= 2:
        y[0], y[1] = 1, 0
    return y


def normal_scores(n, C, seed):
    return np.random.default_rng(seed + 1000).standard_normal((n, C)).astype(np.float32)


def integer_scores(n, C, seed):
    return np.random.default_rng(seed + 2000).integers(-2, 3, (n, C)).astype(np.float32)


# products n C around the sort's 512-key wave chunk and 2,048-key block and the scan's 1,024 tile, one column
ONE_COLUMN_ROWS = (1, 2, 3, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049)
# seven columns: 7 n = 7 | 511 | 518 | 1022 | 1029 | 2044 | 2051 -- 512, 1,024 and 2,048 are no multiples of 7: the nearest on either side
SEVEN_COLUMN_ROWS = (1, 73, 74, 146, 147, 292, 293)
KEY_PASS_COLUMNS = (1, 2, 112, 256, 257)          # n = 9: one pass on the column up to 256 columns, two from 257
LONG = (20000, 112)                               # 2.24 M pairs: 9 rounds per chunk


def _case(y, s, evaluated=None):
    """evaluated: the columns the case claims are evaluated (None: all of them)."""
    return y, np.ascontiguousarray(s, dtype=np.float32), list(range(y.shape[1])) if evaluated is None else list(evaluated)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (y_true [n, C], float32 scores [n, C], columns claimed evaluated).  Built once; treat as read-only."""
    out = {}
    for n in ONE_COLUMN_ROWS:
        out[f"chunk/C1/n{n}"] = _case(labels(n, 1, n), normal_scores(n, 1, n), None if n >= 2 else [])
    for n in SEVEN_COLUMN_ROWS:
        out[f"chunk/C7/n{n}"] = _case(labels(n, 7, n), normal_scores(n, 7, n), None if n >= 2 else [])
    for C in KEY_PASS_COLUMNS:
        out[f"passes/C{C}"] = _case(labels(9, C, C, nan_frac=0.1), normal_scores(9, C, C))
    out["ties/integer"] = _case(labels(300, 5, 11), integer_scores(300, 5, 11))
    out["ties/integer-int64-labels"] = _case(labels(300, 5, 12, dtype=np.int64), integer_scores(300, 5, 12))
    out["ties/constant"] = _case(labels(257, 3, 13), np.full((257, 3), 0.25))
    # one tie group of 700 across the 512-key chunk boundary: 300 distinct scores below it, 200 above, rows shuffled
    rng = np.random.default_rng(14)
    s = np.concatenate([-1.0 - rng.random(300), np.zeros(700), 1.0 + rng.random(200)]).astype(np.float32)[rng.permutation(1200)]
    out["ties/700-across-a-chunk"] = _case(labels(1200, 1, 14), s[:, None])
    # the last score of column c equals the first of column c + 1
    s = np.stack([c + rng.random(50) for c in range(3)], axis=1).astype(np.float32)
    s[7, 0], s[9, 1], s[3, 1], s[5, 2] = 1.0, 1.0, 2.0, 2.0
    assert s[:, 0].max() == s[:, 1].min() == 1.0 and s[:, 1].max() == s[:, 2].min() == 2.0
    y = labels(50, 3, 15, nan_frac=0)
    y[7, 0], y[9, 1], y[3, 1], y[5, 2] = 1, 0, 1, 0         # were the groups merged, these would tie
    out["ties/across-columns"] = _case(y, s)
    z = np.where(rng.random((200, 2)) < 0.5, -0.0, 0.0).astype(np.float32)
    z[::7] = 1.0
    z[3::11] = -1.0
    out["ties/signed-zeros"] = _case(labels(200, 2, 16), z)
    d = rng.choice(np.array([1e-45, -1e-45, 3e-39, -3e-39, 1.2e-38, -1.2e-38, 1e30, -1e30, 0.0, -0.0, 1.0, -1.0], dtype=np.float32),
                   (400, 2))
    out["order/denormals"] = _case(labels(400, 2, 17), d)
    # a column of all 1s and one of all 0s are skipped; so is the column with a third label value
    y = labels(120, 5, 18)
    y[:, 1], y[:, 3] = 1, 0
    y[:, 4] = np.where(np.arange(120) % 2 == 0, 2.0, 1.0)
    out["labels/skipped-columns"] = _case(y, normal_scores(120, 5, 18), [0, 2])
    # NaN / inf scores where nothing looks: unlabelled rows of an evaluated column, any row of a skipped one
    y = labels(90, 3, 19)
    s = normal_scores(90, 3, 19)
    y[:, 2] = 0
    s[10:20, 2] = np.inf
    y[20:30, 0] = np.nan
    s[20:25, 0], s[25:30, 0] = np.nan, -np.inf
    out["scores/ignored-non-finite"] = _case(y, s, [0, 1])
    out["long"] = _case(labels(LONG[0], LONG[1], 20, positives=0.1), normal_scores(LONG[0], LONG[1], 20))
    return out


ARGMAX_ROWS = (1, 63, 64, 65, 257)
ARGMAX_COLUMNS = (1, 2, 7, 64, 65)


@functools.lru_cache(maxsize=None)
def argmax_case(n, K):
    """(y_true float32 [n, 1] with NaN rows, y_pred float32 [n, K]): whole-number predictions so that rows hold several equal
    maxima, one row with a NaN (two of them where the row is wide enough), signed zeros."""
    rng = np.random.default_rng(100 * n + K)
    p = rng.integers(-3, 4, (n, K)).astype(np.float32)
    p[p == 0] = np.where(rng.random(int((p == 0).sum())) < 0.5, -0.0, 0.0)
    if K >= 2:
        p[n // 2, K // 2] = np.nan
    if K >= 7:
        p[n // 2, K - 1] = np.nan
    y = np.argmax(p, axis=-1).astype(np.float32)
    wrong = rng.random(n) < 0.4
    y[wrong] = rng.integers(0, K, int(wrong.sum()))
    if n >= 3:
        y[rng.random(n) < 0.2] = np.nan
        y[0] = np.argmax(p[0])
    return y[:, None], p
