"""k-nearest-neighbour graphs on the MI355X: the numbers of profiles/r11_knn_graph.md.
    python scripts/knn_bench.py [--out FILE] [--quick]
Per shape: `knn_graph` / `kneighbors_graph` of this package, the tensor-operation restatement on the same GPU (chunked
`torch.cdist` or normalised `mm`, then `topk`), and sklearn on the host CPUs.  GPU times are device events around windows of
calls on random data, after a warm-up, at least 20 windows, the median; the CPU time is the median of a few wall-clock calls.
For the sweep route the achieved TFLOP/s of 2 N^2 M is reported too.  Nothing here is a pass bar.
--quick: the same code paths at toy sizes (a rehearsal, not a measurement)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difformer_amd import _lib, kneighbors_graph, knn_graph  # noqa: E402

DEV = "cuda:0"
SNAPSHOT_US = (477, 651)          # one wikimath training snapshot of the spatial-temporal loop (profiles/, 1,068 nodes)


def timed(fn, calls, windows):
    """median ms per call over `windows` windows of `calls` calls between two device events, after a warm-up window"""
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
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


def restatement(x, k, loop, cosine, chunk=4096):
    """The same graph from tensor operations: [chunk, N] blocks of distances, topk per block (float32; no tie rule)."""
    n = x.shape[0]
    kk = min(k, n - (0 if loop else 1))
    xs = torch.nn.functional.normalize(x, dim=1) if cosine else x
    cols = []
    for r in range(0, n, chunk):
        d = 1.0 - xs[r:r + chunk] @ xs.t() if cosine else torch.cdist(xs[r:r + chunk], xs)
        if not loop:
            d[torch.arange(d.shape[0], device=x.device), torch.arange(r, r + d.shape[0], device=x.device)] = float("inf")
        cols.append(torch.topk(d, kk, dim=1, largest=False).indices)
    col = torch.cat(cols).reshape(-1)
    return torch.stack([col, torch.arange(n, device=x.device).repeat_interleave(kk)])


def cpu_jobs():
    """threads sklearn may use: OMP_NUM_THREADS where it is set, else the CPUs of the process, 16 at the most"""
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    return int(os.environ.get("OMP_NUM_THREADS", "0") or 0) or min(16, cores)


def sklearn_seconds(x, k, loop, cosine, reps):
    try:
        from sklearn.neighbors import kneighbors_graph as sk
    except ImportError:
        return None
    xs = x.cpu().numpy()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        sk(xs, n_neighbors=k, include_self=loop, metric="cosine" if cosine else "minkowski", n_jobs=cpu_jobs())
        times.append(time.perf_counter() - t)
    return statistics.median(times)


def same_rows(a, b, n):
    """share of rows with the same neighbour set (the restatement ranks float32 distances and has no tie rule)"""
    sa, sb = torch.sort(a[0].view(n, -1), dim=1).values, torch.sort(b[0].view(n, -1), dim=1).values
    return float((sa == sb).all(dim=1).float().mean())


def one(n, m, k, loop, cosine, calls, windows, cpu_reps):
    g = torch.Generator().manual_seed(n + m)
    x = torch.randn(n, m, generator=g).to(DEV)
    ours = (lambda: knn_graph(x, k, loop=loop, cosine=True)) if cosine else (lambda: kneighbors_graph(x, k, include_self=loop))
    res = {"n": n, "m": m, "k": k, "loop": loop, "metric": "cosine" if cosine else "euclidean"}
    knn = _lib.load_knn()
    mp = -(-m // 4) * 4
    res["route"] = "direct" if knn.dif_knn_route(n, mp, k) == 0 else "sweep"
    res["splits"] = knn.dif_knn_splits(n, mp, k, int(loop), -1)
    res["workspace_mb"] = knn.dif_knn_workspace_bytes(n, mp, k, int(loop), int(cosine), -1) / 1e6
    res["ours_ms"] = timed(ours, calls, windows)
    res["restatement_ms"] = timed(lambda: restatement(x, k, loop, cosine), max(1, calls // 4), windows)
    mine = ours() if cosine else ours().flip(0)
    res["same_rows_as_restatement"] = same_rows(mine, restatement(x, k, loop, cosine), n)
    res["sklearn_s"] = sklearn_seconds(x, k, loop, cosine, cpu_reps)
    res["tflops"] = 2.0 * n * n * m / (res["ours_ms"][0] * 1e-3) / 1e12
    return res


def report(rows, quick):
    lines = ["# r11 -- k-nearest-neighbour graphs (`csrc/knn_graph.hip`, `scripts/knn_bench.py`)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  GPU times: median (min .. max) of 20 windows of calls between device events, random",
             "normal features, after a warm-up window.  Restatement: chunked `torch.cdist` / normalised `mm` + `topk` on the same GPU",
             f"(float32, no tie rule).  sklearn: `kneighbors_graph(..., n_jobs={cpu_jobs()})` on the host, {cpu_jobs()} CPU cores; median of",
             "the repetitions.  Nothing here is a pass bar." +
             ("  **--quick rehearsal: toy sizes, not a measurement.**" if quick else ""), "",
             "| N | M | metric | k | route | ranges | workspace MB | ours ms | restatement ms | ours / restatement | sklearn s | TFLOP/s of 2·N²·M | rows equal to the restatement |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        o, t = r["ours_ms"], r["restatement_ms"]
        sk = "not installed" if r["sklearn_s"] is None else f"{r['sklearn_s']:.4f}"
        lines.append(f"| {r['n']} | {r['m']} | {r['metric']} | {r['k']} | {r['route']} | {r['splits']} | {r['workspace_mb']:.2f} | "
                     f"{o[0]:.4f} ({o[1]:.4f} .. {o[2]:.4f}) | {t[0]:.4f} ({t[1]:.4f} .. {t[2]:.4f}) | {o[0] / t[0]:.2f} | {sk} | "
                     f"{r['tflops']:.2f} | {r['same_rows_as_restatement']:.4f} |")
    lines.append("")
    for r in rows:
        if r["n"] == 1068:
            us = r["ours_ms"][0] * 1e3
            lines.append(f"The 1,068-node call takes {us:.1f} us: {100 * us / SNAPSHOT_US[1]:.1f} % .. {100 * us / SNAPSHOT_US[0]:.1f} % of the "
                         f"{SNAPSHOT_US[0]}-{SNAPSHOT_US[1]} us wikimath training snapshot.")
    lines.append("The sweep design measured for the top-k attention maps (`profiles/r08_attn_topk.md`): 33.0 ms / 68 TFLOP/s at N = L = 132,534, "
                 "M = 64, KMAX 16; this sweep always runs KMAX 32 (one wave per SIMD) and is followed by the float64 re-rank.")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r11_knn_graph.md"))
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    np.random.seed(0)
    if args.quick:
        shapes = [(20, 4, 5, True, True, 5, 3, 1), (300, 8, 5, True, True, 5, 3, 1), (1000, 64, 5, True, False, 2, 3, 1)]
    else:
        shapes = [(20, 4, 5, True, True, 200, 20, 5), (1068, 8, 5, True, True, 100, 20, 5), (15000, 64, 5, True, False, 4, 20, 3),
                  (15000, 512, 5, True, False, 2, 20, 3)]
    rows = [one(*s) for s in shapes]
    text = report(rows, args.quick)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
