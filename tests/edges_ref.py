"""float64 restatement (numpy) of the attention on graph edges.

`edge_values` / `edge_mass` are the reference's dense visualisation output (tests/topk_ref.py `dense_attention`, pinned to the
reference's own tensors) read at the edges: edge_index row 0 is the source (key) id, row 1 the target (query) id, as
`gcn_conv` reads it (node classification/difformer.py:65-75).  `raw_values` / `raw_mass` restate what the ENTRY POINTS of
include/difformer_edges.h compute from their operands (q, k, scale, mode), edge by edge, without a dense map.
"""
import numpy as np

import topk_ref

TOL = 1e-4          # the project's parity bar (tests/conftest.py rel_err)


def edge_values(q, k, kernel, edge_index):
    """q [N,H,M], k [L,H,M], edge_index [2,E] -> float64 [E,H] = dense_attention[col, row, :]."""
    ei = np.asarray(edge_index)
    return topk_ref.dense_attention(q, k, kernel)[ei[1], ei[0], :]


def sum_per_target(values, edge_index, n):
    """values [E,H] -> float64 [n,H]: per target node the sum over its in-edges (duplicates count as often as they occur)."""
    mass = np.zeros((n, values.shape[1]), dtype=np.float64)
    np.add.at(mass, np.asarray(edge_index)[1], np.asarray(values, dtype=np.float64))
    return mass


def edge_mass(q, k, kernel, edge_index):
    """-> float64 [N,H]: the part of every attention row that lies on the graph's edges."""
    return sum_per_target(edge_values(q, k, kernel, edge_index), edge_index, np.asarray(q).shape[0])


def raw_values(q, k, scale, mode, edge_index):
    """float64 [E,H]: f(q[col_e,h] . k[row_e,h]) scale[col_e,h], f the identity (mode 0) or sigma (mode 1); scale None = 1."""
    q, k, ei = np.asarray(q, dtype=np.float64), np.asarray(k, dtype=np.float64), np.asarray(edge_index)
    s = np.einsum("ehm,ehm->eh", q[ei[1]], k[ei[0]])
    if mode == 1:
        s = 1.0 / (1.0 + np.exp(-s))
    return s if scale is None else s * np.asarray(scale, dtype=np.float64)[ei[1]]


def raw_mass(q, k, scale, mode, edge_index):
    return sum_per_target(raw_values(q, k, scale, mode, edge_index), edge_index, np.asarray(q).shape[0])


def random_graph(n_q, n_k, E, seed=0, hubs=()):
    """int64 [2,E] with duplicates, self-loops and at least one target without in-edges where the sizes allow it; hubs: degrees
    of target rows that get that many in-edges (taken out of E)."""
    rng = np.random.default_rng(seed)
    targets = np.arange(n_q) if n_q < 3 else np.delete(np.arange(n_q), n_q // 2)          # node n_q // 2 stays isolated
    row, col = rng.integers(0, n_k, E), rng.choice(targets, E)
    at = 0
    for j, deg in enumerate(hubs):
        col[at: at + deg] = targets[(3 + 5 * j) % len(targets)]
        at += deg
    if E >= 4:
        row[-1], col[-1] = row[-2], col[-2]                                              # a duplicate
        loop = int(targets[targets < n_k][-1])
        row[-3] = col[-3] = loop                                                          # a self-loop
    perm = rng.permutation(E)
    return np.stack([row[perm], col[perm]]).astype(np.int64)
