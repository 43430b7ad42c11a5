"""Oracle of the training losses (difformer_amd/losses.py, csrc/loss.hip): numpy in long double (80-bit on x86-64), returned as
float64, and the case tables of tests/test_loss_host.py and tests/test_gpu_loss.py.

The oracle evaluates the header's formulas (include/difformer_loss.h) row by row over the SELECTED rows only:
    NLL   m = max x,  S' = sum_{c != label} exp(x_c - m),  d = x_label - m,  l = log1p(S') if d == 0 else log(S' + exp(d)) - d
          dl/dx_c = exp(x_c - m) / S (c != label),  -S' / S (c == label),  S = S' + exp(d)
    BCE   l = max(x, 0) - x t + log1p(exp(-|x|)),  dl/dx = -sigmoid(-x) (t == 1), sigmoid(x) (t == 0), sigmoid(x) - t (else)
    loss = sum_r w_r l_r / count,  grad = w_r * upstream / count * dl/dx
with w_r the multiplicity of row r.  A case is a dict; `cases()` builds every one once.
"""
import functools

import numpy as np

LD = np.longdouble

# ---- geometry of csrc/loss.hip: W lanes per row, 64 / W rows per wave, 256 / W rows per workgroup pass ----------------------------
COLUMNS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 63, 64, 65, 112, 128, 129, 257, 1000)
SCALES = (1, 30)
MAX_GROUPS = 1024


def lanes(C):
    W = 1
    while W < C and W < 64:
        W *= 2
    return W


def rows_for(C):
    """n in {1, 2, 3}, rows-per-wave +- 1 and rows-per-workgroup +- 1 of C's lane-group width."""
    W = lanes(C)
    return sorted({1, 2, 3, 64 // W - 1, 64 // W + 1, 256 // W - 1, 256 // W + 1} - {0})


def workspace_formula(n, C):
    """The header's formula of dif_loss_workspace_bytes."""
    R = 256 // lanes(C)
    G = min(MAX_GROUPS, max(1, -(-n // R)))
    return -(-24 * G // 256) * 256


# ---- number formats ---------------------------------------------------------------------------------------------------------------------
def to_bf16(x):
    """float32 array -> the nearest bfloat16 values (ties to even), held as float32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def ulp(g, bf16=False):
    """Spacing of the format at |g| (float64 array): 2^(e - 23) for float32, 2^(e - 7) for bfloat16, the spacing at 0 (2^-149,
    2^-133) for denormals."""
    g = np.abs(np.asarray(g, dtype=np.float64))
    e = np.where(g > 0, np.frexp(g)[1] - 1, -126)                # |g| in [2^e, 2^(e + 1))
    e = np.maximum(e, -126)
    return np.ldexp(1.0, e - (7 if bf16 else 23))


# ---- selection ----------------------------------------------------------------------------------------------------------------------------
def weights_of(rows, n):
    """rows None | bool mask [n] | int64 index -> (int64 multiplicities [n], number of indices outside [0, n))."""
    if rows is None:
        return np.ones(n, dtype=np.int64), 0
    rows = np.asarray(rows)
    if rows.dtype == np.bool_:
        return rows.astype(np.int64), 0
    ok = (rows >= 0) & (rows < n)
    return np.bincount(rows[ok], minlength=n).astype(np.int64), int((~ok).sum())


# ---- the oracle -----------------------------------------------------------------------------------------------------------------------------
def _sigmoid(z):
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(-np.abs(z))
        return np.where(z >= 0, 1 / (1 + e), e / (1 + e))


def nll(x, label, rows=None, ignore_index=-100, upstream=1.0):
    """-> dict(loss float64, count, invalid, grad float64 [n, C]); x float32 [n, C], label int64 [n]."""
    n, C = x.shape
    w, bad = weights_of(rows, n)
    label = np.asarray(label).reshape(n)
    picked = w > 0
    invalid_rows = picked & (label != ignore_index) & ((label < 0) | (label >= C))
    live = np.flatnonzero(picked & (label != ignore_index) & ~invalid_rows)
    count = int(w[live].sum())
    invalid = bad + int(w[invalid_rows].sum())
    grad = np.zeros((n, C), dtype=np.float64)
    total = LD(0)
    if live.size:
        with np.errstate(all="ignore"):
            X = x[live].astype(LD)
            lab = label[live]
            at = (np.arange(live.size), lab)
            m = np.fmax.reduce(X, axis=1)
            E = np.exp(X - m[:, None])
            el = E[at]
            Eo = E.copy()
            Eo[at] = 0
            so = Eo.sum(axis=1)
            so = np.where(np.isnan(E).any(axis=1), LD("nan"), so)
            d = X[at] - m
            loss_rows = np.where(d == 0, np.log1p(so), np.log(so + el) - d)
            total = (w[live].astype(LD) * loss_rows).sum()
            S = so + el
            G = E / S[:, None]
            G[at] = -(so / S)
            if count:
                grad[live] = (w[live].astype(LD)[:, None] * (LD(upstream) / LD(count)) * G).astype(np.float64)
    loss = float(total / LD(count)) if count and not invalid else float("nan")
    return dict(loss=loss, count=count, invalid=invalid, grad=grad)


def bce(x, target, rows=None, upstream=1.0):
    """-> dict(loss, count, invalid, grad); x float32 [n, C], target [n, C] of any real dtype."""
    n, C = x.shape
    w, bad = weights_of(rows, n)
    live = np.flatnonzero(w > 0)
    count = int(w[live].sum()) * C
    grad = np.zeros((n, C), dtype=np.float64)
    total = LD(0)
    if live.size:
        with np.errstate(all="ignore"):
            X = x[live].astype(LD)
            T = np.asarray(target)[live].astype(LD)
            L = (np.fmax(X, 0) - X * T) + np.log1p(np.exp(-np.abs(X)))
            total = (w[live].astype(LD) * L.sum(axis=1)).sum()
            G = np.where(T == 1, -_sigmoid(-X), np.where(T == 0, _sigmoid(X), _sigmoid(X) - T))
            G = np.where(np.isnan(X), LD("nan"), G)
            grad[live] = (w[live].astype(LD)[:, None] * (LD(upstream) / LD(count)) * G).astype(np.float64)
    loss = float(total / LD(count)) if count and not bad else float("nan")
    return dict(loss=loss, count=count, invalid=bad, grad=grad)


def evaluate(case, bf16=False, upstream=None):
    """The oracle on a case (on its logits rounded to bfloat16 when bf16)."""
    x = to_bf16(case["x"]) if bf16 else case["x"]
    up = case["upstream"] if upstream is None else upstream
    if case["kind"] == "nll":
        return nll(x, case["second"], case["rows"], case["ignore_index"], up)
    return bce(x, case["second"], case["rows"], up)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
SELECTIONS = ("all", "mask", "index")
TARGET_DTYPES = (np.int64, np.float32, np.uint8)


def make_case(kind, n, C, scale, seed, selection, target_dtype=np.int64, ignored=True, upstream=1.0):
    """A well-posed case: finite logits of the given scale, at least one selected row with a counted label.
    selection: 'all' | 'mask' | 'index' (unsorted, one row three times)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, C)) * scale).astype(np.float32)
    keep = int(rng.integers(n))                                   # a row that is selected and counted whatever else happens
    if selection == "all":
        rows = None
    elif selection == "mask":
        rows = rng.random(n) < 0.6
        rows[keep] = True
    else:
        picked = np.flatnonzero(rng.random(n) < 0.6)
        rows = rng.permutation(np.concatenate([picked, [keep, keep, keep]])).astype(np.int64)       # multiplicity >= 3 at `keep`
    if kind == "nll":
        second = rng.integers(0, C, n).astype(np.int64)
        if ignored:
            second[rng.random(n) < 0.15] = -100
            second[keep] = int(rng.integers(C))
    else:
        second = (rng.random((n, C)) < 0.5).astype(target_dtype)
        if target_dtype == np.float32:                           # soft targets too
            soft = rng.random((n, C)) < 0.3
            second[soft] = rng.random(int(soft.sum())).astype(np.float32)
    return dict(kind=kind, x=x, second=second, rows=rows, ignore_index=-100, upstream=upstream)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  'sweep/<kind>/C<C>/n<n>/s<scale>': both sides of every lane-group width; the selection and the BCE target
    dtype rotate with the position in the table, so that every combination occurs many times."""
    out = {}
    i = 0
    for kind in ("nll", "bce"):
        for C in COLUMNS:
            for n in rows_for(C):
                for scale in SCALES:
                    out[f"sweep/{kind}/C{C}/n{n}/s{scale}"] = make_case(kind, n, C, scale, 1000 + i, SELECTIONS[i % 3],
                                                                        TARGET_DTYPES[(i // 3) % 3])
                    i += 1
    # 547 workgroups of 128 rows: more than one partial per lane of the finalising workgroup (256 lanes)
    out["groups/nll/70001x2"] = make_case("nll", 70001, 2, 1, 7, "mask")
    out["groups/bce/70001x2"] = make_case("bce", 70001, 2, 30, 8, "index", np.uint8)
    # more workgroup passes than MAX_GROUPS: every workgroup takes two passes of 4 rows
    out["passes/nll/4100x65"] = make_case("nll", 4100, 65, 30, 9, "index")
    out["passes/bce/4100x112"] = make_case("bce", 4100, 112, 1, 10, "mask", np.float32)
    for kind in ("nll", "bce"):
        for j, sel in enumerate(SELECTIONS):
            out[f"select/{kind}/{sel}"] = make_case(kind, 300, 7, 3, 20 + j, sel, TARGET_DTYPES[j], upstream=-2.5)
        for j, dt in enumerate(TARGET_DTYPES):
            out[f"target/{kind}/{np.dtype(dt).name}"] = make_case(kind, 131, 112, 4, 30 + j, "mask", dt)
    return out


def sweep_names(kind, C):
    return [f"sweep/{kind}/C{C}/n{n}/s{s}" for n in rows_for(C) for s in SCALES]


def well_posed(case):
    """count > 0 and every logit of a selected (and, for NLL, counted) row finite."""
    n, C = case["x"].shape
    w, bad = weights_of(case["rows"], n)
    sel = w > 0
    if case["kind"] == "nll":
        lab = case["second"]
        sel &= lab != case["ignore_index"]
        if ((lab[sel] < 0) | (lab[sel] >= C)).any():
            return False
    return bad == 0 and sel.any() and bool(np.isfinite(case["x"][sel]).all())
