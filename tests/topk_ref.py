"""float64 restatement (numpy) of the top-k attention maps, and the criterion the tests hold a result to.

The attention is the reference's visualisation output, `node classification/difformer.py:20-21,32-38,43` (`simple`) and
`:47-55` (`sigmoid`); tests/test_attn_topk_host.py pins `dense_attention` to the reference's own tensors
(tests/golden/golden_attnw.npz, tests/golden/golden_topk.npz).

Criterion.  Exact index equality against float64 cannot be asked of a float32 kernel: with Gaussian operands the smallest gap
between neighbouring top-k values is ~5e-8 of the row scale.  A result is correct when
  1. rel_err(values, float64 top-k values) <= TOL;
  2. the float64 attention AT the returned indices matches the returned values to the same TOL (an index points at its value);
  3. every row's indices are distinct and in [0, L).
TOL = 1e-4 is the project's parity bar (tests/conftest.py rel_err).  A float32 restatement sits at 1-3e-7 on 1 and 2; a
result that misses the last three keys of a row sits at 5e-3 .. 1e-1.
"""
import numpy as np

from conftest import rel_err

TOL = 1e-4


def dense_attention(q, k, kernel):
    """q [N,H,M], k [L,H,M] -> float64 [N,L,H]."""
    q, k = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64)
    if kernel == "simple":
        qn, kn = q / np.sqrt((q * q).sum()), k / np.sqrt((k * k).sum())                    # :20-21
        den = np.einsum("nhm,hm->nh", qn, kn.sum(axis=0)) + q.shape[0]                      # :32-38
        return np.einsum("nhm,lhm->nlh", qn, kn) / den[:, None, :]                          # :43 (no `+ 1`)
    assert kernel == "sigmoid"
    s = 1.0 / (1.0 + np.exp(-np.einsum("nhm,lhm->nlh", q, k)))                              # :47
    return s / s.sum(axis=1, keepdims=True)                                                 # :50-55


def topk_rows(attn, k, rank=None):
    """attn [N,L,H] -> (values [N,H,k] float64, indices [N,H,k] int64): the k largest of attn[n,:,h], descending, among
    equals the lower index first, NaN last.  rank: the tensor the order is taken on when it is not attn itself (the scores
    of the sigmoid kernel, where sigma saturates)."""
    key = attn if rank is None else rank
    order = np.argsort(-np.transpose(key, (0, 2, 1)), axis=2, kind="stable")[:, :, :k]      # stable: ties keep index order
    return np.take_along_axis(np.transpose(attn, (0, 2, 1)), order, axis=2), order.astype(np.int64)


def reference_topk(q, k, kernel, topk):
    return topk_rows(dense_attention(q, k, kernel), topk)


def figures(values, indices, attn, ref_values):
    """-> (criterion 1, criterion 2, criterion 3 as bool)."""
    values, indices = np.asarray(values, dtype=np.float64), np.asarray(indices).astype(np.int64)
    L = attn.shape[1]
    valid = bool(((indices >= 0) & (indices < L)).all())
    srt = np.sort(indices, axis=2)
    valid = valid and bool((srt[:, :, 1:] != srt[:, :, :-1]).all())
    at = np.take_along_axis(np.transpose(attn, (0, 2, 1)), np.clip(indices, 0, L - 1), axis=2)
    return rel_err(values, ref_values), rel_err(values, at), valid


def check_topk(values, indices, attn, topk, what=""):
    """Asserts the three criteria for a result against the float64 attention [N,L,H]; prints the figures first."""
    ref_values, _ = topk_rows(attn, topk)
    assert tuple(values.shape) == ref_values.shape and tuple(indices.shape) == ref_values.shape, (values.shape, ref_values.shape)
    e1, e2, valid = figures(values, indices, attn, ref_values)
    print(f"topk {what}: values {e1:.2e}, values at indices {e2:.2e}, indices valid {valid}")
    assert valid, f"{what}: a row's indices repeat or leave [0, {attn.shape[1]})"
    assert e1 <= TOL, f"{what}: top-k values off by {e1:.3e}"
    assert e2 <= TOL, f"{what}: indices do not point at their values ({e2:.3e})"
