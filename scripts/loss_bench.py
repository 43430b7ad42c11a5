"""Training losses on the MI355X: the numbers of profiles/r14_losses.md.
    python scripts/loss_bench.py [--out FILE] [--iters N] [--quick]
Forward + backward of `log_softmax_nll` / `bce_with_logits` (csrc/loss.hip) against the tensor-operation expression they
replace, `F.nll_loss(F.log_softmax(out, 1)[rows], label[rows])` / `F.binary_cross_entropy_with_logits(out[rows],
target[rows].float())`, at the shapes of the scripts.  The two are timed alternately in one process: HIP events around N
iterations (at least 100) after a warm-up, and the host clock around the same window (a boolean-mask selection in the torch
expression waits for the host in every iteration; the events see that as idle time on the stream).  Also compares the two
results (loss and gradient) so that a timing is never reported for a wrong answer.  Nothing here is a pass bar.
--quick: the same code paths at toy sizes (a rehearsal, not a measurement)."""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from difformer_amd import bce_with_logits, log_softmax_nll  # noqa: E402

# name, n, C, loss, selection, target dtype
SHAPES = (("ogbn-proteins batch", 10000, 112, "bce", "mask", torch.int64),
          ("ogbn-proteins full graph", 132534, 112, "bce", "index", torch.float32),
          ("Pokec batch", 100000, 2, "nll", "mask", None),
          ("image and text", 15000, 10, "nll", "index", None))


def make(n, C, loss, selection, tdtype, dev):
    g = torch.Generator(device=dev).manual_seed(n + C)
    out = torch.randn(n, C, device=dev, generator=g).requires_grad_()
    if loss == "bce":
        second = (torch.rand(n, C, device=dev, generator=g) > 0.5).to(tdtype)
    else:
        second = torch.randint(0, C, (n,), device=dev, generator=g)
    mask = torch.rand(n, device=dev, generator=g) < 0.5
    rows = mask if selection == "mask" else mask.nonzero().squeeze(1)[torch.randperm(int(mask.sum()), device=dev, generator=g)]
    if loss == "bce":
        new = lambda: bce_with_logits(out, second, rows)
        old = lambda: F.binary_cross_entropy_with_logits(out[rows], second[rows].float())
    else:
        new = lambda: log_softmax_nll(out, second, rows)
        old = lambda: F.nll_loss(F.log_softmax(out, dim=1)[rows], second[rows])
    return out, new, old


def step(out, fn):
    out.grad = None
    loss = fn()
    loss.backward()
    return loss


def timed(out, fn, iters):
    """-> (device ms per iteration from events, host ms per iteration)"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        step(out, fn)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters, (time.perf_counter() - t0) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("loss_bench: needs the MI355X; there is no CPU measurement")
    dev = torch.device("cuda:0")
    iters = max(100, args.iters) if not args.quick else 5
    lines = ["| shape | loss, selection | torch expression: device / host ms | device kernels: device / host ms | device-time ratio | "
             "loss difference | largest gradient difference |", "|---|---|---|---|---|---|---|"]
    for name, n, C, loss, selection, tdtype in SHAPES:
        if args.quick:
            n = max(n // 100, 50)
        out, new, old = make(n, C, loss, selection, tdtype, dev)
        l_new = step(out, new).detach().double()
        g_new = out.grad.clone()
        l_old = step(out, old).detach().double()
        g_old = out.grad.clone()
        dl = float((l_new - l_old).abs() / l_old.abs())
        dg = float((g_new - g_old).abs().max() / g_old.abs().max())
        for fn in (new, old):                                   # warm-up of every shape the window uses
            for _ in range(20 if not args.quick else 2):
                step(out, fn)
        t_new, t_old = [], []
        for _ in range(args.rounds):                            # alternate the two
            t_old.append(timed(out, old, iters))
            t_new.append(timed(out, new, iters))
        med = lambda ts, i: statistics.median(t[i] for t in ts)
        lines.append(f"| {n:,} x {C} ({name}) | {loss.upper()}, {selection}{', ' + str(tdtype).replace('torch.', '') + ' targets' if tdtype else ''} | "
                     f"{med(t_old, 0):.4f} / {med(t_old, 1):.4f} | {med(t_new, 0):.4f} / {med(t_new, 1):.4f} | "
                     f"{med(t_old, 0) / med(t_new, 0):.2f}x | {dl:.1e} | {dg:.1e} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + f"\n\nForward + backward per iteration, median of {args.rounds} windows of {iters} iterations each, alternated; " \
        f"{torch.cuda.get_device_name(0)}.\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
