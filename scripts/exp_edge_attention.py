"""Attention on graph edges on the MI355X: the numbers of profiles/r10_edge_attention.md.
    python scripts/exp_edge_attention.py [--out FILE] [--quick]
Per shape and mode: ms per call (device events, warmed up, several calls per window, the variants alternating inside a round,
the minimum of the windows) of dif_edge_attn_f32 and dif_edge_attn_mass_f32, the bytes per second of
E (2 H M 4 + 16 + 4 H) resp. nnz (H M 4 + 4), and the same numbers from tensor operations in chunks on the same GPU:
`(q[col] * k[row]).sum(-1)` (which writes and re-reads both gathered operands), followed by index_add_ for the mass.
Shapes: (a) the ogbn-proteins-shaped graph as bench.py builds it (132,534 nodes, 79.3 M entries, M = 64, H = 1), with uniform and
with skewed degrees; (b) 15,000 nodes x 300 columns with 5 in-edges per node.  The longest row's cost is measured by itself: the
mass kernel on a CSR whose only row with entries is that one (one wave).
--quick: the same code paths at toy sizes (a rehearsal, not a measurement)."""
import argparse
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from difformer_amd import ops  # noqa: E402

CHUNK = 1 << 22          # edges per step of the tensor-operation restatement: 1 GB per gathered operand at M = 64


def make_graph(*args, **kw):
    spec = importlib.util.spec_from_file_location("bench", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench.make_graph(*args, **kw)


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


def windows(runs, rounds, calls):
    ms = {name: [] for name in runs}
    for _ in range(rounds):                          # alternating: a drift of the clock hits all variants alike
        for name, fn in runs.items():
            ms[name].append(timed(fn, calls))
    return ms


def tensor_ops_values(q, k, scale, ei, mode, mass_out=None):
    """The restatement in chunks: [E,H] values, and (mass_out given) their sum per target."""
    out = torch.empty((ei.shape[1], q.shape[1]), dtype=torch.float32, device=q.device)
    for e0 in range(0, ei.shape[1], CHUNK):
        row, col = ei[0, e0: e0 + CHUNK], ei[1, e0: e0 + CHUNK]
        s = (q[col] * k[row]).sum(-1)
        out[e0: e0 + CHUNK] = (torch.sigmoid(s) if mode else s) * scale[col]
        if mass_out is not None:
            mass_out.index_add_(0, col, out[e0: e0 + CHUNK])
    return out


def measure(name, ei, n, h, m, rounds, calls):
    dev = ei.device
    be = ops.get_backend()
    g = torch.Generator().manual_seed(0)
    q = (torch.randn(n, h, m, generator=g) * m ** -0.25).to(dev)
    k = (torch.randn(n, h, m, generator=g) * m ** -0.25).to(dev)
    scale = (torch.rand(n, h, generator=g) + 0.5).to(dev)
    E = ei.shape[1]
    csr = ops.GraphCSR.build(ei, None, n, 1)
    deg = (csr.rowptr[1:] - csr.rowptr[:-1]).long()
    hub = int(deg.argmax())
    # the longest row alone: every other row empty, the hub's entries where they are
    lone = torch.where(torch.arange(n + 1, device=dev) <= hub, csr.rowptr[hub], csr.rowptr[hub + 1]).to(torch.int32).contiguous()
    res = {"shape": name, "n": n, "E": E, "H": h, "M": m,
           "degree": {"max": int(deg.max()), "mean": round(E / n, 1), "median": int(deg.median()),
                      "rows_over_4x_mean": int((deg > 4 * E / n).sum())}}
    edge_bytes, mass_bytes = E * (2 * h * m * 4 + 16 + 4 * h), E * (h * m * 4 + 4)
    for mode, label in ((0, "simple"), (1, "sigmoid")):
        mass_buf = torch.zeros((n, h), dtype=torch.float32, device=dev)
        runs = {"edge_kernel": lambda: be.edge_attention(q, k, scale, ei, mode),
                "edge_tensor_ops": lambda: tensor_ops_values(q, k, scale, ei, mode),
                "mass_kernel": lambda: be.edge_attention_mass(q, k, scale, csr.rowptr, csr.src, mode),
                "mass_tensor_ops": lambda: tensor_ops_values(q, k, scale, ei, mode, mass_buf.zero_()),
                "mass_kernel_longest_row_alone": lambda: be.edge_attention_mass(q, k, scale, lone, csr.src, mode)}
        ms = windows(runs, rounds, calls)
        row = {r: {"ms": [round(x, 4) for x in t], "ms_min": round(min(t), 4)} for r, t in ms.items()}
        row["edge_kernel"]["TB_per_s"] = round(edge_bytes / min(ms["edge_kernel"]) / 1e9, 3)
        row["mass_kernel"]["TB_per_s"] = round(mass_bytes / min(ms["mass_kernel"]) / 1e9, 3)
        row["edge_speedup_over_tensor_ops"] = round(min(ms["edge_tensor_ops"]) / min(ms["edge_kernel"]), 2)
        row["mass_speedup_over_tensor_ops"] = round(min(ms["mass_tensor_ops"]) / min(ms["mass_kernel"]), 2)
        values, status = be.edge_attention(q, k, scale, ei, mode)
        ref = tensor_ops_values(q, k, scale, ei, mode, mass_buf.zero_())
        mass = be.edge_attention_mass(q, k, scale, csr.rowptr, csr.src, mode)
        row["status"] = status.tolist()
        row["max_rel_diff_of_values"] = float(((values - ref).abs().max() / ref.abs().max()).item())
        row["max_rel_diff_of_mass"] = float(((mass - mass_buf).abs().max() / mass_buf.abs().max()).item())
        res[label] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "shapes": []}
    n, pairs, small, rounds, calls = (132534, 39561252, 15000, 3, 3) if not args.quick else (3000, 40000, 500, 1, 1)
    for name, zipf in (("proteins-uniform", False), ("proteins-zipf", True)):
        ei = make_graph(n, pairs, dev, zipf=zipf)
        out["shapes"].append(measure(name, ei, n, 1, 64, rounds, calls))
        del ei
        torch.cuda.empty_cache()
    g = torch.Generator(device=dev).manual_seed(1)
    ei = torch.stack([torch.randint(0, small, (5 * small,), generator=g, device=dev),
                      torch.arange(small, device=dev).repeat_interleave(5)]).contiguous()
    out["shapes"].append(measure("15000x300-5-in-edges", ei, small, 1, 300, rounds, 10 * calls))
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    slow = [(s["shape"], lab, s[lab]["edge_speedup_over_tensor_ops"]) for s in out["shapes"] for lab in ("simple", "sigmoid")
            if s[lab]["edge_speedup_over_tensor_ops"] < 2.0]
    if slow and not args.quick:
        print("below the speed bar (2x the tensor-operation restatement):", slow)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
