"""Long-double oracle of the graph read-out (global_add_pool / global_mean_pool / global_max_pool and their gradients) and the
case table that tests/test_readout_host.py and tests/test_gpu_readout.py share (plain helper module).

Semantics are those of include/difformer_readout.h: graph b is the rows [ptr[b], ptr[b+1]); an empty graph gives a row of +0 in
all three modes and has no gradient rows; `max` gives NaN for a column that holds one and splits the gradient evenly among
the rows that equal the maximum (torch's amax rule), none for a NaN column.

Every case carries two sets of node rows: `x32`, float32 values with a full mantissa, and `xb`, bfloat16-exact values.  Within
a column of a graph all values are distinct in BOTH sets (so `max` has no tie) except where `plant` names a graph, a column
and rows that are set to one value above all others (a tie of exactly that many rows).
"""
import functools

import numpy as np

MODES = ("add", "mean", "max")
COLUMNS = (1, 63, 64, 65, 255, 256, 257, 300, 1024)          # both sides of a wave, of the workgroup, a loop with a ragged tail
LENGTHS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 257, 1025)
# three graphs per column count: empty graphs first, last, in the middle and adjacent
TRIPLES = ((0, 5, 64), (1, 0, 65), (63, 2, 0), (4, 257, 1), (0, 0, 3), (65, 0, 0), (2, 63, 5), (3, 4, 64), (5, 1, 2))
SINGLES = (1, 2, 3, 4, 5, 63, 64, 65, 257)
PLANTED = 32.0                                                 # above every value of the pool below


def phases(H):
    """(columns in flight, row phases) of csrc/graph_readout.hip for H columns."""
    w = 1
    while w < H and w < 256:
        w *= 2
    return w, 256 // w


def _value_pool():
    """2,048 distinct bfloat16-exact values: +-(1 + m / 128) 2^e, m < 128, -4 <= e < 4 (|v| < 16)."""
    m = 1.0 + np.arange(128) / 128.0
    mags = np.concatenate([m * 2.0 ** e for e in range(-4, 4)])
    return np.concatenate([mags, -mags])


POOL = _value_pool()


def make_case(H, lengths, seed, plant=()):
    """-> dict(H, lengths, ptr int32 [B + 1], x32, xb float32 [N, H], g32, gb float32 [B, H], plant)."""
    rng = np.random.default_rng(seed)
    lengths = [int(v) for v in lengths]
    ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    N = int(ptr[-1])
    xb = np.zeros((N, H), dtype=np.float64)
    pool = rng.permutation(POOL)
    for b, n in enumerate(lengths):
        if n:                                                  # per column a walk with an odd stride: no two rows equal
            start, stride = rng.integers(0, POOL.size, H), 2 * rng.integers(0, POOL.size // 2, H) + 1
            xb[ptr[b]:ptr[b + 1]] = pool[(start + np.arange(n)[:, None] * stride) % POOL.size]
    # neighbours of the pool differ by >= 2^-8 relative; a perturbation below 2^-10 keeps them apart and in order
    x32 = (xb * (1.0 + rng.uniform(-1.0, 1.0, xb.shape) * 2.0 ** -10)).astype(np.float32)
    xb = xb.astype(np.float32)
    for b, col, rows in plant:
        for x in (x32, xb):
            x[ptr[b] + np.asarray(rows), col] = PLANTED
    g32 = rng.standard_normal((len(lengths), H)).astype(np.float32)
    gb = _to_bf16(g32)
    return dict(H=H, lengths=lengths, ptr=ptr, x32=x32, xb=xb, g32=g32, gb=gb, plant=tuple(plant))


def _to_bf16(a):
    """float32 -> the nearest bfloat16 value (ties to even), as float32."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(a))


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  The names say which mechanism a case is there for."""
    table = {}
    for i, H in enumerate(COLUMNS):
        table[f"triple/H{H}"] = make_case(H, TRIPLES[i], 100 + i)
        table[f"single/H{H}"] = make_case(H, (SINGLES[i],), 200 + i)
    rng = np.random.default_rng(7)
    many = rng.choice(LENGTHS[:9], size=257)                   # lengths up to 65
    many[[0, 100, 101, 256]] = 0                               # empty first, adjacent in the middle, last
    table["many/H300"] = make_case(300, many, 300)             # 257 workgroups, two column blocks of which one ragged
    table["many/H64"] = make_case(64, np.roll(many, 3), 301)
    table["long/H1024"] = make_case(1024, (1025,), 302)        # one graph: four column blocks, 1,025 rows in one phase
    table["long/H65"] = make_case(65, (1025, 257, 0), 303)     # two phases, lengths that are no multiple of them
    # planted ties: H = 64 has 4 row phases (rows r and r + 1 lie in different phases, r and r + 4 in the same one),
    # H = 300 one phase, H = 1 256 phases
    table["ties/H64"] = make_case(64, (63, 0, 5), 304, plant=((0, 0, (0, 1)), (0, 1, (0, 4)), (0, 2, (1, 5, 6)), (0, 3, (0, 1, 2)),
                                                              (0, 63, (30, 62)), (2, 63, (3, 4)), (2, 5, (0, 2, 4))))
    table["ties/H300"] = make_case(300, (5, 63), 305, plant=((0, 0, (0, 4)), (1, 255, (1, 2, 3)), (1, 256, (0, 62)), (1, 299, (2, 3, 6))))
    table["ties/H1"] = make_case(1, (257, 4), 306, plant=((0, 0, (0, 256)), (1, 0, (0, 1, 3))))
    return table


# ---- the oracle -------------------------------------------------------------------------------------------------------------------
def forward(x, ptr, mode):
    """-> long double [B, H]."""
    x = np.asarray(x, dtype=np.longdouble)
    B = len(ptr) - 1
    out = np.zeros((B, x.shape[1]), dtype=np.longdouble)
    for b in range(B):
        rows = x[ptr[b]:ptr[b + 1]]
        if not rows.shape[0]:
            continue
        if mode == "max":
            out[b] = np.where(np.isnan(rows).any(axis=0), np.nan, np.max(np.nan_to_num(rows, nan=-np.inf), axis=0))
        else:
            out[b] = rows.sum(axis=0) / (rows.shape[0] if mode == "mean" else 1)
    return out


def backward(x, ptr, mode, g):
    """-> long double [N, H]: the gradient in x of sum(forward(x) * g)."""
    x, g = np.asarray(x, dtype=np.longdouble), np.asarray(g, dtype=np.longdouble)
    gx = np.zeros_like(x)
    for b in range(len(ptr) - 1):
        rows = x[ptr[b]:ptr[b + 1]]
        n = rows.shape[0]
        if not n:
            continue
        if mode == "add":
            gx[ptr[b]:ptr[b + 1]] = g[b]
        elif mode == "mean":
            gx[ptr[b]:ptr[b + 1]] = g[b] / n
        else:
            with np.errstate(invalid="ignore"):
                hit = rows == np.max(rows, axis=0)                     # a NaN column: np.max is NaN, nothing equals it
            ties = hit.sum(axis=0)
            gx[ptr[b]:ptr[b + 1]] = np.where(hit, g[b] / np.maximum(ties, 1), 0)
    return gx


def sum_abs(x, ptr):
    """sum |x| per graph and column -> float64 [B, H]."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    return np.stack([a[ptr[b]:ptr[b + 1]].sum(axis=0) for b in range(len(ptr) - 1)]) if len(ptr) > 1 else a[:0]


def ulp(v, bf16=False):
    """Spacing of the storage type in the binade of |v| (at 0 and in the denormals: the smallest spacing)."""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -126)))
    return 2.0 ** (e - (7 if bf16 else 23))


def forward_bound(ref, case, mode, bf16=False):
    """add / mean: |out - ref| <= 1/2 ulp_storage(ref) + length * 2^-53 * sum |x| (for mean, over length)."""
    x = case["xb" if bf16 else "x32"]
    n = np.asarray(case["lengths"], dtype=np.float64)[:, None]
    slack = n * 2.0 ** -53 * sum_abs(x, case["ptr"])
    if mode == "mean":
        slack = slack / np.maximum(n, 1)
    return 0.5 * ulp(ref, bf16) + slack


def backward_bound(ref, bf16=False):
    """mean / max: 1/2 ulp_storage(ref) + 2^-53 |ref|."""
    return 0.5 * ulp(ref, bf16) + 2.0 ** -53 * np.abs(np.asarray(ref, dtype=np.float64))


@functools.lru_cache(maxsize=None)
def evaluate(name, bf16=False):
    """The oracle's results of a case, computed once and left unchanged: {mode: (out, grad_x)} in long double."""
    case = cases()[name]
    x, g = (case["xb"], case["gb"]) if bf16 else (case["x32"], case["g32"])
    res = {}
    for mode in MODES:
        out, gx = forward(x, case["ptr"], mode), backward(x, case["ptr"], mode, g)
        out.setflags(write=False)
        gx.setflags(write=False)
        res[mode] = (out, gx)
    return res
