"""Snapshot batches against the per-snapshot loop, in the same process and session (`spatial-temporal/main.py:94-121`, `eval.py:9-22`):

    python scripts/st_epoch_batched.py [--epochs 20] [--out profiles/r18_snapshot_batches.md]

  chickenpox  n = 20,   d = 4,  104 snapshots, static graph         cumulative epoch (forward, summed cost, ONE backward) + evaluation
  covid       n = 129,  d = 8,   50 snapshots, a graph per snapshot  cumulative epoch + evaluation
  wikimath    n = 1068, d = 14, 146 snapshots, static graph         evaluation only (its training steps per snapshot: not batched)

for `simple` and `sigmoid`, with and without the graph term, the scripts' configuration (hidden 4, two layers, no Wv, dropout 0.2).
`loop`: model(x, ei, ea) per snapshot on device tensors made once (the graph cache of tiny.py holds the static graph; covid's 50
graphs are rebuilt every epoch, as its fresh tensors make them in main.py).  `batched`: one SnapshotBatch made once (its
construction timed separately), model.forward_snapshots per epoch.  No optimiser step: the parameters, and so the numbers, stay
the same for both.  Times are wall-clock per epoch between device synchronisations after warm-up epochs: median (min .. max).
Also: the largest difference between the batched results and the per-snapshot one-workgroup calls (tiny.PLAN = 1).  Synthetic data."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from st_epoch import data  # noqa: E402


def timed(fn, epochs, warmup=3):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(epochs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), min(times), max(times)


def cell(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    from difformer_amd import DIFFormer, SnapshotBatch, snapshots, tiny
    dev = torch.device("cuda:0")
    shapes = [("chickenpox", 20, 4, 4, 104, False, True), ("covid", 129, 8, 12, 50, True, True), ("wikimath", 1068, 14, 10, 146, False, False)]
    lines = ["# r18 -- snapshot batches (`csrc/tiny_batched.hip`, `scripts/st_epoch_batched.py`)", "",
             f"Device: {torch.cuda.get_device_name(0)}.  Wall-clock ms per epoch between device synchronisations, median (min .. max) of "
             f"{args.epochs} epochs after 3 warm-up epochs; loop and batched in the same process, same parameters, no optimiser step.",
             "`loop`: `model(x, ei, ea)` per snapshot (difformer_amd/tiny.py, the plan it picks by size); `batched`: "
             "`model.forward_snapshots(batch)`.  A ratio is batched / loop; **bold**: the batched call is the slower one.  "
             "`build`: one `SnapshotBatch(...)` construction (once per split, not per epoch).  `max diff`: the largest absolute "
             "difference of Y, dx and the parameter gradients between the batched call and the per-snapshot one-workgroup calls "
             "(`tiny.PLAN = 1`) over the largest absolute entry of the tensor.  Nothing here is a pass bar.", "",
             "| dataset | kernel | graph | T | pass | loop ms | batched ms | batched / loop | build ms | max diff |", "|---|---|---|---|---|---|---|---|---|---|"]
    for name, n, d, deg, T, dynamic, cumulative in shapes:
        if args.only not in name:
            continue
        host = data(n, d, deg, T, dynamic, False)
        for kernel in ("simple", "sigmoid"):
            for use_graph in (True, False):
                torch.manual_seed(123)
                model = DIFFormer(d, 4, 1, num_layers=2, alpha=0.5, dropout=0.2, num_heads=1, kernel=kernel, use_bn=True,
                                  use_residual=True, use_graph=use_graph, use_weight=False).to(dev)
                model.reset_parameters()
                xs = [s[0].to(dev) for s in host]
                ys = torch.stack([s[3] for s in host]).to(dev)
                if dynamic:
                    eis, eas = [s[1].to(dev) for s in host], [s[2].to(dev) for s in host]
                else:
                    eis, eas = [host[0][1].to(dev)] * T, [host[0][2].to(dev)] * T

                def make_batch():
                    b = SnapshotBatch(xs, eis if dynamic else eis[0], eas if dynamic else eas[0])
                    torch.cuda.synchronize()
                    return b
                batch = make_batch()
                build = timed(make_batch, 5, warmup=1)

                def loop_train():
                    if dynamic:                                   # fresh tensors per epoch (main.py:96): the graphs are rebuilt
                        tiny.graphs.clear()
                    model.train()
                    cost_tr = 0
                    for t in range(T):
                        cost_tr = cost_tr + torch.mean((model(xs[t], eis[t], eas[t]) - ys[t]) ** 2)
                    (cost_tr / T).backward()
                    model.zero_grad(set_to_none=True)

                def batched_train():
                    model.train()
                    Y = model.forward_snapshots(batch)
                    ((Y.view(T, n, 1) - ys.view(T, 1, n)) ** 2).mean().backward()
                    model.zero_grad(set_to_none=True)

                @torch.no_grad()
                def loop_eval():
                    if dynamic:
                        tiny.graphs.clear()
                    model.eval()
                    cost = 0
                    for t in range(T):
                        cost = cost + torch.mean((model(xs[t], eis[t], eas[t]) - ys[t]) ** 2)
                    return cost / T

                @torch.no_grad()
                def batched_eval():
                    model.eval()
                    Y = model.forward_snapshots(batch)
                    return ((Y.view(T, n, 1) - ys.view(T, 1, n)) ** 2).mean()

                # the batched results against the per-snapshot ONE-WORKGROUP calls, dropout off
                model.dropout, plan = 0.0, tiny.PLAN
                tiny.PLAN = 1
                model.train()
                gos = torch.randn(T * n, 1, device=dev)
                xl = [x.clone().requires_grad_(True) for x in xs]
                torch.cat([model(xl[t], eis[t], eas[t]) for t in range(T)]).backward(gos)
                ref = [torch.cat([x.grad for x in xl])] + [p.grad.clone() for p in model.parameters()]
                with torch.no_grad():
                    ref_y = torch.cat([model(xs[t], eis[t], eas[t]) for t in range(T)])
                model.zero_grad(set_to_none=True)
                tiny.PLAN = plan
                batch.x.requires_grad_(True)
                Y = model.forward_snapshots(batch)
                Y.backward(gos)
                got = [batch.x.grad] + [p.grad for p in model.parameters()]
                diff = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip([Y.detach()] + got, [ref_y] + ref))
                model.zero_grad(set_to_none=True)
                batch.x.grad = None
                batch.x.requires_grad_(False)
                model.dropout = 0.2

                passes = ([("cumulative epoch", loop_train, batched_train)] if cumulative else []) + [("evaluation", loop_eval, batched_eval)]
                for what, lo, ba in passes:
                    before = dict(snapshots.stats)
                    tl, tb = timed(lo, args.epochs), timed(ba, args.epochs)
                    assert snapshots.stats["fallback"] == before["fallback"] and snapshots.stats["forward"] > before["forward"]
                    r = tb[0] / tl[0]
                    ratio = f"**{r:.2f}**" if r > 1.0 else f"{r:.2f}"
                    line = f"| {name} | {kernel} | {use_graph} | {T} | {what} | {cell(tl)} | {cell(tb)} | {ratio} | {cell(build)} | {diff:.1e} |"
                    print(line, flush=True)
                    lines.append(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
