"""optimizer.step() on the MI355X: the numbers of profiles/r15_adam.md.
    python scripts/adam_step.py [--out FILE] [--iters N] [--rounds R] [--quick]
Four optimisers over the parameter sets of four models of the scripts, each on its own copy of the parameters with the same
random non-zero gradients:
    torch          torch.optim.Adam (the default foreach path)
    fused          torch.optim.Adam(fused=True)
    capturable     torch.optim.Adam(capturable=True)
    difformer      difformer_amd.Adam (csrc/adam.hip: one launch per 48 tensors)
Timed alternately in one process after a warm-up: HIP events around a window of N steps (device time per step; a host-bound
window shows the host's pace here too), and the host clock from the first step() of the window to the return of the last, before
any synchronisation (what the Python thread spends per step).  Medians over R windows.  Also compares one step of every
candidate against torch's default, so that a timing is never reported for a wrong answer.  Nothing here is a pass bar.
--quick: two windows of 5 steps (a rehearsal, not a measurement)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import difformer_amd  # noqa: E402
from difformer_amd import DIFFormer  # noqa: E402

OPTIMIZERS = ("torch", "fused", "capturable", "difformer")


def make_optimizer(name, params, **kw):
    """The --optimizer option of st_epoch.py / it_epoch.py and the candidates here."""
    if name == "torch":
        return torch.optim.Adam(params, **kw)
    if name == "fused":
        return torch.optim.Adam(params, fused=True, **kw)
    if name == "capturable":
        return torch.optim.Adam(params, capturable=True, **kw)
    if name == "difformer":
        return difformer_amd.Adam(params, **kw)
    raise SystemExit(f"--optimizer must be one of {', '.join(OPTIMIZERS)} (got {name})")


def models():
    """name -> the model whose parameter set is stepped (configurations of the scripts)."""
    return (("wikimath (hidden 4, 14 features)", lambda: DIFFormer(14, 4, 1, num_layers=2, use_weight=False)),
            ("Cora (1,433 x 64, 2 layers)", lambda: DIFFormer(1433, 64, 7, num_layers=2)),
            ("ogbn-proteins (3 layers, hidden 64, 112 classes)", lambda: DIFFormer(8, 64, 112, num_layers=3)),
            ("cifar10 image-and-text (hidden 300)", lambda: DIFFormer(512, 300, 10, num_layers=2, use_graph=False, use_weight=False)))


def window(opt, iters):
    """-> (device ms per step from events, host ms per step before any synchronisation)"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    t0 = time.perf_counter()
    for _ in range(iters):
        opt.step()
    host = (time.perf_counter() - t0) * 1e3 / iters
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters, host


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adam_step: needs the MI355X; there is no CPU measurement")
    dev = torch.device("cuda:0")
    iters, rounds = (max(100, args.iters), args.rounds) if not args.quick else (5, 2)
    head = "| parameter set | tensors, elements | " + " | ".join(f"{n}: device / host ms" for n in OPTIMIZERS) + \
        " | host: torch / difformer | largest difference to torch after one step |"
    lines = [head, "|" + "---|" * (len(OPTIMIZERS) + 4)]
    for name, make in models():
        torch.manual_seed(0)
        base = [p.detach().clone() for p in make().to(dev).parameters()]
        g = torch.Generator(device=dev).manual_seed(1)
        grads = [torch.randn(p.shape, device=dev, generator=g) * 0.1 + 0.01 for p in base]
        opts, params = {}, {}
        for cand in OPTIMIZERS:
            params[cand] = [torch.nn.Parameter(p.clone()) for p in base]
            for p, gr in zip(params[cand], grads):
                p.grad = gr.clone()
            opts[cand] = make_optimizer(cand, params[cand], lr=0.01, weight_decay=5e-4)
            opts[cand].step()
        diff = max(float((a - b).abs().max()) for c in OPTIMIZERS[1:] for a, b in zip(params[c], params["torch"]))
        for cand in OPTIMIZERS:                                 # warm-up
            for _ in range(20 if not args.quick else 2):
                opts[cand].step()
        t = {c: [] for c in OPTIMIZERS}
        for _ in range(rounds):                                 # alternate the candidates
            for cand in OPTIMIZERS:
                t[cand].append(window(opts[cand], iters))
        med = lambda c, i: statistics.median(x[i] for x in t[c])
        lines.append(f"| {name} | {len(base)}, {sum(p.numel() for p in base):,} | "
                     + " | ".join(f"{med(c, 0):.4f} / {med(c, 1):.4f}" for c in OPTIMIZERS)
                     + f" | {med('torch', 1) / med('difformer', 1):.2f}x | {diff:.1e} |")
        print(lines[-1], flush=True)
    text = "\n".join(lines) + f"\n\nPer step(), median of {rounds} windows of {iters} steps each, alternated; lr 0.01, weight decay 5e-4; " \
        f"{torch.cuda.get_device_name(0)}.\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
