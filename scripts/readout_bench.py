"""Graph read-out on the MI355X: the numbers of profiles/r16_readout.md.
    python scripts/readout_bench.py [--out FILE] [--iters N] [--quick]
Forward + backward of global_add_pool / global_mean_pool / global_max_pool (csrc/graph_readout.hip) against the tensor-operation
restatement they replace (`index_add_` and a multiply, `scatter_reduce(amax)`: what scripts/pp_step.py --readout torch and
torch_geometric do) at the two batch shapes of the physical-particle folder, hidden 64.  The two are timed alternately in one
process: HIP events around N iterations (at least 100) after a warm-up, and the host clock around the same window.  Also
compares the two results, so that a timing is never reported for a wrong answer, and counts the kernels each side launches
with torch's profiler (in a pass of its own, after the timing).  Nothing here is a pass bar.
--quick: the same code paths at toy sizes (a rehearsal, not a measurement)."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import difformer_amd  # noqa: E402

# name, graphs, smallest and largest graph (uniform), columns: the batches of scripts/pp_step.py
SHAPES = (("ActsTrack-like", 1024, 40, 180, 64), ("Tau3Mu-like", 8192, 8, 32, 64))
POOLS = {"add": difformer_amd.global_add_pool, "mean": difformer_amd.global_mean_pool, "max": difformer_amd.global_max_pool}


def make(B, lo, hi, H, mode, dev):
    g = torch.Generator(device=dev).manual_seed(B + H)
    n_nodes = torch.randint(lo, hi + 1, (B,), device=dev, generator=g)
    N = int(n_nodes.sum())
    x = torch.randn(N, H, device=dev, generator=g).requires_grad_()
    up = torch.randn(B, H, device=dev, generator=g)
    gid = torch.repeat_interleave(torch.arange(B, device=dev), n_nodes)
    inv = (1.0 / n_nodes.float())[:, None]
    new = lambda: POOLS[mode](x, n_nodes=n_nodes)
    if mode == "max":
        index = gid[:, None].expand(-1, H)
        old = lambda: torch.zeros(B, H, device=dev).scatter_reduce(0, index, x, "amax", include_self=False)
    elif mode == "mean":
        old = lambda: torch.zeros(B, H, device=dev).index_add_(0, gid, x) * inv
    else:
        old = lambda: torch.zeros(B, H, device=dev).index_add_(0, gid, x)
    return x, up, new, old, N


def step(x, up, fn):
    x.grad = None
    out = fn()
    out.backward(up)
    return out


def timed(x, up, fn, iters):
    """-> (device ms per iteration from events, host ms per iteration)"""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    start.record()
    for _ in range(iters):
        step(x, up, fn)
    end.record()
    torch.cuda.synchronize()
    return start.elapsed_time(end) / iters, (time.perf_counter() - t0) * 1e3 / iters


def launches(x, up, fn):
    """Kernels (and memsets / copies) one forward + backward enqueues, or None where the profiler is not available."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step(x, up, fn)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as e:                                      # the count is a report, not a result
        print(f"launch count not measured: {e}", flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-launch-count", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("readout_bench: needs the MI355X; there is no CPU measurement")
    dev = torch.device("cuda:0")
    iters = max(100, args.iters) if not args.quick else 5
    lines = ["| shape | pool | tensor operations: device / host ms | device kernels: device / host ms | device-time ratio | "
             "largest output difference | largest gradient difference |", "|---|---|---|---|---|---|---|"]
    counts = []
    for name, B, lo, hi, H in SHAPES:
        if args.quick:
            B = max(B // 64, 4)
        for mode in POOLS:
            x, up, new, old, N = make(B, lo, hi, H, mode, dev)
            o_new = step(x, up, new).detach()
            g_new = x.grad.clone()
            o_old = step(x, up, old).detach()
            g_old = x.grad.clone()
            do = float((o_new - o_old).abs().max() / o_old.abs().max())
            dg = float((g_new - g_old).abs().max() / g_old.abs().max())
            for fn in (new, old):                                   # warm-up of every shape the window uses
                for _ in range(20 if not args.quick else 2):
                    step(x, up, fn)
            t_new, t_old = [], []
            for _ in range(args.rounds):                            # alternate the two
                t_old.append(timed(x, up, old, iters))
                t_new.append(timed(x, up, new, iters))
            med = lambda ts, i: statistics.median(t[i] for t in ts)
            lines.append(f"| {N:,} x {H} / {B:,} graphs ({name}) | {mode} | {med(t_old, 0):.4f} / {med(t_old, 1):.4f} | "
                         f"{med(t_new, 0):.4f} / {med(t_new, 1):.4f} | {med(t_old, 0) / med(t_new, 0):.2f}x | {do:.1e} | {dg:.1e} |")
            print(lines[-1], flush=True)
            counts.append((name, mode, x, up, old, new))
    # the profiler slows the host: after every timing window
    counts = [] if args.no_launch_count else [(n, m, launches(x, up, old), launches(x, up, new)) for n, m, x, up, old, new in counts]
    text = "\n".join(lines) + f"\n\nForward + backward per iteration, median of {args.rounds} windows of {iters} iterations each, alternated; " \
        f"{torch.cuda.get_device_name(0)}.\n"
    if counts:
        text += "\nDevice activities (kernels, memsets, copies) of one forward + backward, torch profiler:\n\n| shape | pool | tensor operations | device kernels |\n|---|---|---|---|\n"
        text += "".join(f"| {n} | {m} | {a if a is not None else 'not measured'} | {b if b is not None else 'not measured'} |\n" for n, m, a, b in counts)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
