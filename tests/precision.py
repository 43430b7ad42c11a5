"""Operands that make a split-bfloat16 product visible (tests/test_gpu_exact_fp32.py, tests/test_precision_helpers.py).

Every split path of the library forms a float32 product from bfloat16 pieces: x = hi + lo, hi = bf16(x), lo = bf16(x - hi),
and x.w ~ lo.hi' + hi.lo' + hi.hi' on the bf16 matrix core with float32 accumulation.  The helpers that split all read the
same: `split_bf16` (csrc/simple_layer.hip, skinny_linear.hip, simple_layer_wide.hip, simple_layer_xwide.hip), `sg_split8`
(sigmoid_attn.hip), `split8` (sigmoid_attn_bwd.hip), the row-GEMM fragments (rowgemm_split.h, simple_attn_bwd.hip) and the
Gram slab (simple_attn.hip) convert with __builtin_convertvector (round to nearest even on gfx950) and take the lo part of
the float32 difference x - hi, which is exact.  `split_planes<2>` (sigmoid_wide.hip) is the same two planes written as a
loop (subtract the plane in place, convert again).  What differs is WHAT gets split, not how:
  - rowgemm_split_kernel scales its resident operand by `mat_scale` (1 / (|Q| |K|) in the apply mode) in float32 first: a
    lo-heavy K^T V stays lo-heavy only when that scale is a power of two;
  - the sigmoid plane kernels split the centred values V - mean V (forward) and G / den (backward), not the caller's
    operands (sigw_pack_kernel).

On N(0, 1) operands the dropped terms (lo.lo', and what bf16(x - hi) leaves) have random signs: a split product moves by
~1e-6 of sum |a b| and a norm-wise test barely sees it.  `lo_heavy` builds positive values whose dropped terms are all
positive and ~1e-5 of every product, so a split product is low by ~1e-5 of sum |a b| at every depth, while a float32
chain stays below ~1e-6.
"""
import numpy as np

BF16_BITS = 8            # significant bits of bfloat16 (7 stored + the implicit one)


def bf16_rne(x):
    """float32 -> nearest bfloat16 (ties to even) as float32; a NaN stays a quiet NaN.  What __builtin_convertvector(float
    -> __bf16) gives on gfx950 and what dif::f32_to_bf16 (csrc/dif_common.h) computes."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    r = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    r = np.where(nan, ((u >> 16) | 0x40) << 16, r).astype(np.uint32)
    return r.view(np.float32).reshape(x.shape)


def split_bf16(x):
    """-> (hi, lo) float32 arrays of bfloat16 values: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in float32)."""
    x = np.asarray(x, dtype=np.float32)
    hi = bf16_rne(x)
    return hi, bf16_rne(x - hi)


def ulp_bf16(v):
    """Spacing of the bfloat16 numbers at |v| (normal, nonzero v)."""
    return np.ldexp(1.0, np.floor(np.log2(np.abs(np.asarray(v, dtype=np.float64)))).astype(np.int64) - (BF16_BITS - 1))


def _chain(pairs, shape):
    """Sequential float32 accumulation of exact float64 products, one rounding per step (a fused multiply-add)."""
    acc = np.zeros(shape, dtype=np.float32)
    for k in range(pairs[0][0].shape[-1]):
        for p, q in pairs:
            acc = (acc.astype(np.float64) + p[..., k].astype(np.float64) * q[..., k].astype(np.float64)).astype(np.float32)
    return acc.astype(np.float64)


def fp32_chain_dot(a, b):
    """sum_k a[..., k] b[..., k] as a sequential float32 FMA chain -> float64 array of the float32 results.  The fp32 MFMA
    adds in another order; this is the error scale of a float32 dot product of that depth."""
    a, b = np.broadcast_arrays(np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32))
    return _chain([(a, b)], a.shape[:-1])


def split3_dot(a, b):
    """The three-MFMA product of the split paths over the last axis: lo.hi' + hi.lo' + hi.hi', float32 accumulation (a
    bf16 x bf16 product is exact in float32; the small terms first, as the kernels issue them) -> float64 array of the
    float32 results."""
    ah, al = split_bf16(a)
    bh, bl = split_bf16(b)
    ah, al, bh, bl = np.broadcast_arrays(ah, al, bh, bl)
    return _chain([(al, bh), (ah, bl), (ah, bh)], ah.shape[:-1])


def lo_heavy(shape, seed, scale=1.0):
    """Positive float32 values x = h + l + r whose split drops as much as it can, all of it with one sign:
        h  a bfloat16 value in [0.5, 2)                                     -> bf16(x) == h
        l  a bfloat16 value at 0.2 .. 0.45 ulp(h): below half an ulp of h   -> bf16(x - h) == l
        r  ~0.45 ulp(l) (what float32 keeps of it)                          -> dropped by the split
    A split product of two such operands misses h.r' + r.h' + l.l' in every term: low by ~1e-5 of sum |a b|.
    `scale` multiplies the values and must be a power of two (the split then keeps its structure exactly)."""
    if np.frexp(float(scale))[0] != 0.5:
        raise ValueError(f"lo_heavy: scale must be a power of two (got {scale})")
    rng = np.random.default_rng(seed)
    h = bf16_rne(rng.uniform(0.5, 2.0, size=shape).astype(np.float32)).astype(np.float64)
    h = np.minimum(h, 2.0 - 2.0 ** -7)                                     # (rounding may reach 2.0: keep the binade)
    l = bf16_rne((rng.uniform(0.2, 0.45, size=shape) * ulp_bf16(h)).astype(np.float32)).astype(np.float64)
    x = (h + l + 0.45 * ulp_bf16(l)).astype(np.float32)
    return (x * np.float32(scale)).astype(np.float32)


def exact_bf16(shape, seed, scale=1.0):
    """Positive bfloat16 values in [0.5, 2) * scale as float32: lo == 0, a split product of two of them is exact."""
    rng = np.random.default_rng(seed)
    return (bf16_rne(rng.uniform(0.5, 2.0, size=shape).astype(np.float32)) * np.float32(scale)).astype(np.float32)


def mixed(shape, seed, which, axis=-1, scale=1.0):
    """lo_heavy entries in the slices `which` (indices or a boolean mask) along `axis`, exact bfloat16 values elsewhere.
    LayerNorm, the q / |q| normalisation of the simple kernel and the sigmoid normaliser cancel a UNIFORM relative scaling
    of a row: a split only shows through them when it moves some output features (or rows) and not the others."""
    sel = np.zeros(shape[axis], dtype=bool)
    sel[np.asarray(which)] = True
    bshape = [1] * len(shape)
    bshape[axis] = shape[axis]
    return np.where(sel.reshape(bshape), lo_heavy(shape, seed, scale), exact_bf16(shape, seed + 7919, scale)).astype(np.float32)


def dot_errors(got, a, b):
    """(got - a.b) / sum |a b| per dot product over the last axis, in float64."""
    a64, b64 = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return (np.asarray(got, dtype=np.float64) - (a64 * b64).sum(axis=-1)) / np.abs(a64 * b64).sum(axis=-1)
