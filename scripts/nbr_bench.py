"""Batched neighbour graphs on the MI355X: the numbers of profiles/r17_batched_neighbours.md.
    python scripts/nbr_bench.py [--out FILE] [--quick]
Per batch: the batched `knn_graph(..., n_nodes=)` / `radius_graph(..., n_nodes=)` of this package (one launch / two launches),
a loop of the single-graph `knn_graph` over the graphs with the indices offset (what a caller writes today), and the padded
tensor-operation restatement on the same GPU (rows gathered into [B, max n, M], `cdist` or a normalised `bmm`, a mask for the
padding, then `topk` or a `< r` mask; float32, no tie rule).  GPU times are device events around windows of calls on random
data, after a warm-up window, the median of the windows.  Nothing here is a pass bar.
--quick: the same code paths at toy sizes (a rehearsal, not a measurement)."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difformer_amd import knn_graph, radius_graph  # noqa: E402

DEV = "cuda:0"
K = 5
# name, graphs, smallest and largest graph (uniform), columns, cosine, radius or None.  The snapshot stacks of the spatial-temporal
# datasets (chickenpox 104 x 20 x 4, covid 50 x 129 x 8, wikimath 146 x 1,068 x 14) and the two batches of scripts/readout_bench.py
# with positions (3 columns) for features.
SHAPES = (("chickenpox snapshots", 104, 20, 20, 4, True, None), ("covid snapshots", 50, 129, 129, 8, True, None),
          ("wikimath snapshots", 146, 1068, 1068, 14, True, None), ("Tau3Mu-like", 8192, 8, 32, 3, False, 1.0),
          ("ActsTrack-like", 1024, 40, 180, 3, False, 1.0))
QUICK = (("toy snapshots", 6, 20, 20, 4, True, None), ("toy batch", 40, 8, 32, 3, False, 1.0))


WINDOW_MS = 20.0                   # a window holds at least this much work: shorter ones time the clock and the scheduler


def timed(fn, calls, windows):
    """median ms per call over `windows` windows between two device events, after a warm-up window; a window is `calls` calls,
    or more when those take less than WINDOW_MS (sized from the warm-up window)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    calls = max(calls, min(2000, int(WINDOW_MS * calls / max(a.elapsed_time(b), 1e-3)) + 1))
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return statistics.median(out), min(out), max(out)


class Padded:
    """The batch as the reference's padding machinery holds it: a gather index [B, max n] (built once per batch layout, not
    timed) and the validity mask."""

    def __init__(self, n_nodes):
        B, mx = n_nodes.numel(), int(n_nodes.max())
        first = torch.cumsum(n_nodes, 0) - n_nodes
        slot = torch.arange(mx, device=n_nodes.device)[None, :]
        self.valid = slot < n_nodes[:, None]                                  # [B, mx]
        self.index = torch.where(self.valid, first[:, None] + slot, torch.zeros_like(slot))
        self.pair = self.valid[:, :, None] & self.valid[:, None, :]
        self.first, self.B, self.mx = first, B, mx

    def distances(self, x, cosine):
        xp = x[self.index]                                                    # [B, mx, M]
        if cosine:
            xn = torch.nn.functional.normalize(xp, dim=2)
            d = 1.0 - torch.bmm(xn, xn.transpose(1, 2))
        else:
            d = torch.cdist(xp, xp)
        return d.masked_fill_(~self.pair, float("inf"))

    def knn(self, x, k, cosine):
        """loop=True, every graph larger than k: [2, N k], centres ascending."""
        idx = torch.topk(self.distances(x, cosine), k, dim=2, largest=False).indices + self.first[:, None, None]
        col = idx[self.valid].reshape(-1)
        return torch.stack([col, self.index[self.valid].repeat_interleave(k)])

    def radius(self, x, r):
        """loop=True, no cap, no order inside a centre: [2, E]."""
        b, i, j = (self.distances(x, False) < r).nonzero(as_tuple=True)
        return torch.stack([self.index[b, j], self.index[b, i]])


def per_graph(x, ptr, k, cosine):
    parts = [knn_graph(x[lo:hi], k, loop=True, cosine=cosine) + lo for lo, hi in zip(ptr[:-1], ptr[1:])]
    return torch.cat(parts, dim=1)


def one(name, B, lo, hi, m, cosine, r, quick):
    g = torch.Generator(device=DEV).manual_seed(B + 64)                      # the batches of scripts/readout_bench.py
    n_nodes = torch.randint(lo, hi + 1, (B,), device=DEV, generator=g)
    N = int(n_nodes.sum())
    x = torch.randn(N, m, device=DEV, generator=g)
    ptr = [0] + torch.cumsum(n_nodes, 0).tolist()
    pad = Padded(n_nodes)
    calls, windows = (2, 3) if quick else (20, 20)
    res = {"name": name, "B": B, "N": N, "m": m, "metric": "cosine" if cosine else "euclidean", "r": r}
    res["batched"] = timed(lambda: knn_graph(x, K, loop=True, cosine=cosine, n_nodes=n_nodes), calls, windows)
    res["loop"] = timed(lambda: per_graph(x, ptr, K, cosine), 1, 3 if quick or B > 1000 else 7)
    res["padded"] = timed(lambda: pad.knn(x, K, cosine), max(1, calls // 4), windows)
    mine, theirs = knn_graph(x, K, loop=True, cosine=cosine, n_nodes=n_nodes), per_graph(x, ptr, K, cosine)
    res["equal_to_loop"] = bool(torch.equal(mine, theirs))
    sa, sb = torch.sort(mine[0].view(N, K), dim=1).values, torch.sort(pad.knn(x, K, cosine)[0].view(N, K), dim=1).values
    res["same_rows_as_padded"] = float((sa == sb).all(dim=1).float().mean())
    if r is not None:
        res["radius"] = timed(lambda: radius_graph(x, r, loop=True, n_nodes=n_nodes), calls, windows)
        res["radius_padded"] = timed(lambda: pad.radius(x, r), max(1, calls // 4), windows)
        res["radius_edges"] = (int(radius_graph(x, r, loop=True, n_nodes=n_nodes).shape[1]), int(pad.radius(x, r).shape[1]))
    return res


def cell(ours, other):
    """`other` as median (min .. max) and ours / other; bold where the new call is the slower one"""
    ratio = ours[0] / other[0]
    text = f"{other[0]:.4f} ({other[1]:.4f} .. {other[2]:.4f})"
    return text, (f"**{ratio:.2f}**" if ratio > 1 else f"{ratio:.2f}")


def report(rows, quick):
    lines = ["# r17 -- batched neighbour graphs (`csrc/nbr_batched.hip`, `scripts/nbr_bench.py`)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Times in ms: median (min .. max) of the windows of calls between device events,",
             "random normal features, after a warm-up window (20 windows of at least 20 ms of calls; the per-graph loop: 3 or 7 windows of one pass).",
             "`batched`: `knn_graph(x, 5, loop=True, n_nodes=...)`, one launch.  `loop`: the single-graph `knn_graph` per graph, indices",
             "offset, concatenated.  `padded`: rows gathered into [B, max n, M], `cdist` / normalised `bmm`, padding masked, `topk`",
             "(float32, no tie rule; the gather index is built outside the timed region).  A ratio is batched / other; **bold**: the",
             "new call is the slower one.  Nothing here is a pass bar." +
             ("  **--quick rehearsal: toy sizes, not a measurement.**" if quick else ""), "",
             "## k-NN, k = 5, loop", "",
             "| batch | graphs | rows | M | metric | batched ms | loop ms | batched / loop | padded ms | batched / padded | equal to the loop | rows equal to padded |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        o = r["batched"]
        lp, lr = cell(o, r["loop"])
        pd, pr = cell(o, r["padded"])
        lines.append(f"| {r['name']} | {r['B']} | {r['N']} | {r['m']} | {r['metric']} | {o[0]:.4f} ({o[1]:.4f} .. {o[2]:.4f}) | {lp} | {lr} | "
                     f"{pd} | {pr} | {'bitwise' if r['equal_to_loop'] else 'NO'} | {r['same_rows_as_padded']:.4f} |")
    lines += ["", "## radius, r = 1, loop, max_num_neighbors = 32", "",
              "`radius_graph(x, 1.0, loop=True, n_nodes=...)`: two launches, a `cumsum` and the one host read of E, against the padded",
              "`cdist` + `< r` mask + `nonzero` (no cap, no order inside a centre; it reads E back too).", "",
              "| batch | graphs | rows | M | batched ms | padded ms | batched / padded | edges (ours, padded) |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        if r["r"] is not None:
            o = r["radius"]
            pd, pr = cell(o, r["radius_padded"])
            lines.append(f"| {r['name']} | {r['B']} | {r['N']} | {r['m']} | {o[0]:.4f} ({o[1]:.4f} .. {o[2]:.4f}) | {pd} | {pr} | "
                         f"{r['radius_edges'][0]}, {r['radius_edges'][1]} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "r17_batched_neighbours.md"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    rows = [one(*s, args.quick) for s in (QUICK if args.quick else SHAPES)]
    text = report(rows, args.quick)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
