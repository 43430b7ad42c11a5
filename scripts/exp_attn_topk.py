"""Top-k attention maps on the MI355X: the numbers of profiles/r08_attn_topk.md.
    python scripts/exp_attn_topk.py [--out FILE] [--quick]
(a) N = L = 132,534, M = 64, H = 1, k = 16, both modes: ms per call (device events, warmed up, several calls per window) and
    achieved TFLOP/s of 2 N L M, next to the fp32-chain sigmoid forward (dif_sigmoid_attn_f32 under dif_set_exact_fp32(1)) at
    the same shape in the same run, alternating the three.  That kernel forms the same score tiles plus a second contraction
    of the same size (4 N L M FLOP in all).
(b) N = 15,000, hidden 64 and hidden 300, 2 layers: DIFFormer.top_attentions against the only means there was,
    get_attentions followed by torch.topk: time per call and peak memory (torch.cuda.max_memory_allocated).
--quick: the same code paths at toy sizes (a rehearsal, not a measurement)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from difformer_amd import DIFFormer, ops  # noqa: E402


def timed(fn, calls):
    """ms per call over `calls` calls between two device events, after one warm-up call."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def headline(n, m, k, rounds, calls):
    dev = torch.device("cuda:0")
    be = ops.get_backend()
    g = torch.Generator().manual_seed(0)
    q = (torch.randn(n, 1, m, generator=g) * m ** -0.25).to(dev)
    kk = (torch.randn(n, 1, m, generator=g) * m ** -0.25).to(dev)
    v = torch.randn(n, 1, m, generator=g).to(dev)
    was = be.set_exact_fp32(True)
    runs = {"topk_simple": lambda: be.attn_topk(q, kk, 0, k), "topk_sigmoid": lambda: be.attn_topk(q, kk, 1, k),
            "sigmoid_attn_fp32_chain": lambda: be.sigmoid_attention(q, kk, v)}
    ms = {name: [] for name in runs}
    try:
        for _ in range(rounds):                      # alternating: a drift of the clock hits all three alike
            for name, fn in runs.items():
                ms[name].append(timed(fn, calls))
    finally:
        be.set_exact_fp32(was)
    from difformer_amd import _lib
    res = {"n": n, "m": m, "k": k, "splits": _lib.load_maps().dif_attn_topk_splits(n, n, 1, m, k)}
    for name, t in ms.items():
        best = min(t)
        flop = (4.0 if name.startswith("sigmoid_attn") else 2.0) * n * n * m
        res[name] = {"ms": [round(x, 3) for x in t], "ms_min": round(best, 3), "tflops": round(flop / best / 1e9, 2),
                     "ms_per_score_pass": round(best / (2.0 if name.startswith("sigmoid_attn") else 1.0), 3)}
    return res


def against_dense(n, hidden, k, calls):
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    res = {"n": n, "hidden": hidden, "k": k}
    for kernel in ("simple", "sigmoid"):
        model = DIFFormer(32, hidden, 4, num_layers=2, num_heads=1, kernel=kernel, use_graph=False).to(dev).eval()
        x = torch.randn(n, 32, device=dev)

        def dense():
            with torch.no_grad():
                return torch.topk(model.get_attentions(x).permute(0, 1, 3, 2), k)

        row = {}
        for name, fn in (("top_attentions", lambda: model.top_attentions(x, k)), ("get_attentions_topk", dense)):
            torch.cuda.synchronize()
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats()
            t = timed(fn, calls)
            row[name] = {"ms": round(t, 3), "peak_mb": round(torch.cuda.max_memory_allocated() / 1e6, 1)}
        tv, dv = model.top_attentions(x, k)[0], dense()[0]
        row["max_rel_diff_of_values"] = float(((tv - dv).abs().max() / dv.abs().max()).item())
        res[kernel] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    out = {"device": torch.cuda.get_device_name(0)}
    if args.quick:
        out["a"] = headline(4096, 64, 16, 1, 2)
        out["b"] = [against_dense(1000, 64, 16, 1)]
    else:
        out["a"] = headline(132534, 64, 16, 3, 3)
        out["b"] = [against_dense(15000, 64, 16, 3), against_dense(15000, 300, 16, 3)]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
