"""Long-double oracle of one Adam step (include/difformer_adam.h) and the case table of the GPU tests.  No GPU, no torch.

    g  = grad + wd p
    m' = beta1 m + (1 - beta1) g
    v' = beta2 v + (1 - beta2) g^2
    p' = p - (lr / (1 - beta1^t)) m' / ( sqrt(v') / sqrt(1 - beta2^t) + eps )            t: the step count AFTER this step

evaluated in numpy.longdouble (64-bit mantissa on x86-64) from the state as it is stored, nothing rounded in between.  The
hyper-parameters are the float64 values the C ABI receives.

A case is one call of the C ABI: dict(hyper=dict(lr, beta1, beta2, eps, wd), tensors=[dict(shape, p, g | None, m, v, t0)],
flat_grads=bool).  `t0` is the step count BEFORE the step (the preset state); g None = a parameter without a gradient, which the
caller leaves out of the table; flat_grads = the gradients are views of one flat buffer that starts one element past an aligned
address (the whole-model path hands out such views).
"""
import functools
import os
import re

import numpy as np

L = np.longdouble
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_HEADER = open(os.path.join(ROOT, "include", "difformer_adam.h")).read()
MAX_TENSORS = int(re.search(r"#define DIF_ADAM_MAX_TENSORS (\d+)", _HEADER).group(1))
CHUNK = int(re.search(r"#define DIF_ADAM_CHUNK (\d+)", _HEADER).group(1))


def step(p, g, m, v, t, lr, beta1, beta2, eps, wd):
    """One step -> (p', m', v') as longdouble arrays, unrounded.  t: the count after this step."""
    p, g, m, v = (np.asarray(a).astype(L) for a in (p, g, m, v))
    b1, b2 = L(beta1), L(beta2)
    ge = g + L(wd) * p if wd != 0 else g
    m2 = b1 * m + (L(1) - b1) * ge
    v2 = b2 * v + (L(1) - b2) * (ge * ge)
    bc1 = L(1) - b1 ** L(t)
    bc2 = L(1) - b2 ** L(t)
    p2 = p - (L(lr) / bc1) * (m2 / (np.sqrt(v2) / np.sqrt(bc2) + L(eps)))
    return p2, m2, v2


def ulp32(x):
    """Spacing of float32 at |x| (x in any precision): 2^(e - 24) for |x| = f 2^e, f in [0.5, 1); 2^-149 at 0 and for denormals."""
    f, e = np.frexp(np.abs(np.asarray(x, dtype=L)))
    return np.ldexp(L(1), np.where(f == 0, -149, np.maximum(e.astype(np.int64) - 24, -149)))


def bounds(p_before, ref_p, ref_m, ref_v):
    """The three error bounds of the issue, per element:
        m', v'   1/2 ulp32(ref) + 2^-45 |ref|
        p'       1/2 ulp32(ref) + 2^-40 (|p| + |p - ref|)
    one rounding to float32 of a float64 evaluation; the second terms cover float64 against long double, with the error of pow
    amplified by at most 2^10 where 1 - beta2^t cancels at beta2 = 0.999."""
    p0 = np.asarray(p_before).astype(L)
    bm = ulp32(ref_m) / 2 + L(2) ** -45 * np.abs(ref_m)
    bv = ulp32(ref_v) / 2 + L(2) ** -45 * np.abs(ref_v)
    bp = ulp32(ref_p) / 2 + L(2) ** -40 * (np.abs(p0) + np.abs(p0 - ref_p))
    return bp, bm, bv


def _tensor(rng, shape, t0, grad="normal", has_grad=True):
    n = int(np.prod(shape, dtype=np.int64))
    p = rng.standard_normal(n).astype(np.float32)
    p[p == 0] = 0.5
    if grad == "normal":
        g = (rng.standard_normal(n) * 0.1).astype(np.float32)
    else:                                                       # magnitudes 1e-12 .. 1e4 within the tensor, both signs
        g = (10.0 ** rng.uniform(-12, 4, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
        if n >= 2:
            g[0], g[-1] = 1e-12, -1e4
    g[g == 0] = 0.01
    if t0 == 0:
        m, v = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
    else:                                                       # a plausible preset state: moments of gradients of that size
        m = (rng.standard_normal(n) * 0.05).astype(np.float32)
        v = (rng.uniform(0.2, 2.0, n) * 0.01).astype(np.float32)
    return dict(shape=tuple(shape), p=p.reshape(shape), g=g.reshape(shape) if has_grad else None, m=m.reshape(shape),
                v=v.reshape(shape), t0=int(t0))


def hyper(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=0.0):
    return dict(lr=lr, beta1=beta1, beta2=beta2, eps=eps, wd=wd)


SIZES = [(0,), (1,), (3,), (4,), (5,), (CHUNK - 1,), (CHUNK,), (CHUNK + 1,), ()]           # () is a 0-d tensor
STEPS_BEFORE = (0, 1, 999)                                                                  # t = 1, 2 and 1,000
DECAYS = (0.0, 5e-4)


@functools.lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(20261020)
    table = {}
    for t0 in STEPS_BEFORE:
        for wd in DECAYS:
            table[f"sizes/t{t0 + 1}/wd{wd:g}"] = dict(hyper=hyper(wd=wd), flat_grads=False,
                                                     tensors=[_tensor(rng, s, t0) for s in SIZES])
    for count in (MAX_TENSORS, MAX_TENSORS + 1):                 # one launch, two launches
        table[f"many/{count}"] = dict(hyper=hyper(lr=1e-2, wd=5e-4), flat_grads=False,
                                      tensors=[_tensor(rng, (1 + k % 7,), k % 3) for k in range(count)])
    table["flat_grads"] = dict(hyper=hyper(wd=5e-4), flat_grads=True,
                               tensors=[_tensor(rng, s, 1) for s in ((5,), (3, 7), (CHUNK + 1,), (2,))])
    table["no_grad_in_the_middle"] = dict(hyper=hyper(), flat_grads=False,
                                          tensors=[_tensor(rng, (6,), 1), _tensor(rng, (4, 3), 1, has_grad=False),
                                                   _tensor(rng, (9,), 1), _tensor(rng, (2,), 0, has_grad=False), _tensor(rng, (3,), 0)])
    for t0 in STEPS_BEFORE:
        for wd in DECAYS:
            table[f"magnitudes/t{t0 + 1}/wd{wd:g}"] = dict(hyper=hyper(wd=wd), flat_grads=False,
                                                          tensors=[_tensor(rng, (3 * CHUNK + 17,), t0, grad="wide"),
                                                                   _tensor(rng, (40,), t0, grad="wide")])
    for name, h in (("groups/a", hyper(lr=1e-2, beta1=0.8, beta2=0.99)), ("groups/b", hyper(lr=3e-4, beta1=0.95, beta2=0.9999, wd=5e-4))):
        table[name] = dict(hyper=h, flat_grads=False, tensors=[_tensor(rng, s, 1) for s in ((7,), (5, 5), (CHUNK + 3,))])
    return table


@functools.lru_cache(maxsize=None)
def evaluate(name):
    """The oracle's result of a case, computed once: [None | (p', m', v', bound_p, bound_m, bound_v)] per tensor."""
    case = cases()[name]
    out = []
    for ten in case["tensors"]:
        if ten["g"] is None:
            out.append(None)
            continue
        h = case["hyper"]
        ref = step(ten["p"], ten["g"], ten["m"], ten["v"], ten["t0"] + 1, h["lr"], h["beta1"], h["beta2"], h["eps"], h["wd"])
        out.append(ref + bounds(ten["p"], *ref))
    return out


def worst_ratio(got_p, got_m, got_v, ref):
    """max |got - ref| / bound over the elements of one tensor, for (p, m, v); 0 for an empty tensor."""
    rp, rm, rv, bp, bm, bv = ref
    out = []
    for got, r, b in ((got_p, rp, bp), (got_m, rm, bm), (got_v, rv, bv)):
        d = np.abs(np.asarray(got).astype(L) - r) / b
        out.append(float(d.max()) if d.size else 0.0)
    return tuple(out)
