"""Evaluation metrics on the MI355X: the numbers of profiles/r13_eval_metrics.md.
    python scripts/metrics_bench.py [--out FILE] [--quick]
Per shape: `eval_rocauc` / `eval_acc` of this package on device-resident and on host-resident inputs, and two baselines that
are never the code under test: (a) the reference's functions (node classification/data_utils.py:249-285) restated with
sklearn on the host CPUs (the numpy integer formula where sklearn is not installed; the report says which), and (b) a
tensor-operation restatement on the same GPU (`torch.sort` of every column, `cumsum`, `searchsorted`).

Every shape is one STEP: a child process of its own under `timeout`, which writes one JSON file.  The steps are chained: the
first one that fails (or runs into its limit) ends the run and nothing more is started on the GPU.  This process never opens
the GPU itself.  GPU times: at least 20 warm iterations after a warm-up; device events around the asynchronous table,
the host clock around calls that end in a read-back.  Nothing here is a pass bar.
--quick: the same code paths at toy sizes (a rehearsal, not a measurement)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPOCH_MS = (42.0, 45.0)           # one mini-batch training epoch of ogbn-proteins (profiles/r06_node_classification_epoch.txt)
FORWARD_MS = 1.4                  # the full-graph evaluation forward
EVAL_STEP = 9                     # run.sh:37-39: --eval_step 9
PROTEINS = (132534, 112, (86619, 21236, 24679))
POKEC = (1632803, 2)
IMAGE_TEXT = (15000, 10)
STEPS = (("proteins", 900), ("pokec", 300), ("image_text", 120))      # name, time limit in seconds


# ---- baselines ---------------------------------------------------------------------------------------------------------------------
def roc_auc_fn():
    """sklearn's roc_auc_score, or the integer formula in numpy -> (function, its name)"""
    try:
        from sklearn.metrics import roc_auc_score
        return roc_auc_score, "sklearn"
    except ImportError:
        import numpy as np

        def mann_whitney(y, s):
            neg = np.sort(s[y == 0])
            pos = s[y == 1]
            u2 = int(np.searchsorted(neg, pos, side="left").sum()) + int(np.searchsorted(neg, pos, side="right").sum())
            return u2 / (2 * len(pos) * len(neg))
        return mann_whitney, "numpy (sklearn not installed)"


def reference_eval_rocauc(y_true, y_pred, roc_auc_score):
    """data_utils.py:262-285 (more than one label column)"""
    import numpy as np
    rocauc_list = []
    y_true = y_true.detach().cpu().numpy()
    y_pred = y_pred.detach().cpu().numpy()
    for i in range(y_true.shape[1]):
        if np.sum(y_true[:, i] == 1) > 0 and np.sum(y_true[:, i] == 0) > 0:
            is_labeled = y_true[:, i] == y_true[:, i]
            rocauc_list.append(roc_auc_score(y_true[is_labeled, i], y_pred[is_labeled, i]))
    if len(rocauc_list) == 0:
        raise RuntimeError('No positively labeled data available. Cannot compute ROC-AUC.')
    return sum(rocauc_list) / len(rocauc_list)


def reference_eval_acc(y_true, y_pred):
    """data_utils.py:249-259"""
    import numpy as np
    acc_list = []
    y_true = y_true.detach().cpu().numpy()
    y_pred = y_pred.argmax(dim=-1, keepdim=True).detach().cpu().numpy()
    for i in range(y_true.shape[1]):
        is_labeled = y_true[:, i] == y_true[:, i]
        correct = y_true[is_labeled, i] == y_pred[is_labeled, i]
        acc_list.append(float(np.sum(correct)) / len(correct))
    return sum(acc_list) / len(acc_list)


def tensor_eval_rocauc(y_true, y_pred):
    """(b): every column sorted by torch.sort, negatives counted by cumsum, tie groups bounded by searchsorted; one read-back"""
    import torch
    ss, idx = torch.sort(y_pred.float(), dim=0)
    yy = y_true.gather(0, idx)
    neg, pos = yy == 0, yy == 1
    cn = torch.zeros((ss.shape[0] + 1, ss.shape[1]), dtype=torch.int64, device=ss.device)
    cn[1:] = torch.cumsum(neg, dim=0)
    st = ss.t().contiguous()
    left = torch.searchsorted(st, st, right=False).t()
    right = torch.searchsorted(st, st, right=True).t()
    u2 = ((cn.gather(0, left) + cn.gather(0, right)) * pos).sum(dim=0)
    table = torch.stack([pos.sum(dim=0), neg.sum(dim=0), u2]).t().tolist()
    aucs = [U2 / (2 * P * N) for P, N, U2 in table if P > 0 and N > 0]
    return sum(aucs) / len(aucs)


def tensor_eval_acc(y_true, y_pred):
    lab = y_true[:, 0] == y_true[:, 0]
    correct, n = torch_stack_tolist(((y_pred.argmax(dim=-1) == y_true[:, 0]) & lab).sum(), lab.sum())
    return correct / n


def torch_stack_tolist(*scalars):
    import torch
    return torch.stack(list(scalars)).tolist()


# ---- timing ------------------------------------------------------------------------------------------------------------------------------
def wall_ms(fn, iters, warm=3):
    """median (min, max) ms of `iters` calls that each end in a device read-back (or run on the host), after `warm` calls"""
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t) * 1e3)
    return [statistics.median(out), min(out), max(out)]


def event_ms(fn, iters, warm=3):
    """median (min, max) ms of `iters` asynchronous calls, each between two device events, after `warm` calls"""
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return [statistics.median(out), min(out), max(out)]


# ---- steps (child processes) ------------------------------------------------------------------------------------------------------------------
def step_proteins(quick):
    import torch
    from difformer_amd import _lib, eval_rocauc, rocauc_counts
    n, C, splits = (4000, 16, (2500, 700, 800)) if quick else PROTEINS
    iters, cpu_reps = (3, 1) if quick else (20, 2)
    g = torch.Generator().manual_seed(0)
    y = (torch.rand(n, C, generator=g) < 0.1).float()
    s = torch.randn(n, C, generator=g)
    perm = torch.randperm(n, generator=g)
    roc, roc_name = roc_auc_fn()
    rows, start = [], 0
    for m in splits:
        idx = perm[start:start + m]
        start += m
        yh, sh = y[idx].contiguous(), s[idx].contiguous()
        yd, sd = yh.cuda(), sh.cuda()
        ours = eval_rocauc(yd, sd)
        r = {"rows": m, "columns": C, "workspace_mb": _lib.load_metrics().dif_rocauc_workspace_bytes(m, C) / 1e6,
             "table_ms": event_ms(lambda: rocauc_counts(yd, sd), iters),
             "ours_device_ms": wall_ms(lambda: eval_rocauc(yd, sd), iters),
             "ours_host_ms": wall_ms(lambda: eval_rocauc(yh, sh), iters),
             "tensor_ms": wall_ms(lambda: tensor_eval_rocauc(yd, sd), iters),
             "reference_device_ms": wall_ms(lambda: reference_eval_rocauc(yd, sd, roc), cpu_reps, warm=0),
             "reference_host_ms": wall_ms(lambda: reference_eval_rocauc(yh, sh, roc), cpu_reps, warm=0),
             "equal_to_tensor_restatement": ours == tensor_eval_rocauc(yd, sd),
             "equal_on_host_tensors": ours == eval_rocauc(yh, sh),
             "difference_to_reference": abs(ours - reference_eval_rocauc(yh, sh, roc))}
        rows.append(r)
    return {"rows": rows, "reference": roc_name}


def step_acc(shape, quick, n_splits):
    import torch
    from difformer_amd import eval_acc
    n, K = (3000, shape[1]) if quick else shape
    iters, cpu_reps = (3, 1) if quick else (20, 5)
    g = torch.Generator().manual_seed(1)
    y = torch.randint(0, K, (n, 1), generator=g).float()
    p = torch.randn(n, K, generator=g)
    perm = torch.randperm(n, generator=g)
    cuts = [n // 2, n // 4, n - n // 2 - n // 4][:n_splits] if n_splits > 1 else [n]
    rows, start = [], 0
    for m in cuts:
        idx = perm[start:start + m]
        start += m
        yh, ph = y[idx].contiguous(), p[idx].contiguous()
        yd, pd = yh.cuda(), ph.cuda()
        ours = eval_acc(yd, pd)
        rows.append({"rows": m, "columns": K,
                     "ours_device_ms": wall_ms(lambda: eval_acc(yd, pd), iters),
                     "ours_host_ms": wall_ms(lambda: eval_acc(yh, ph), iters),
                     "tensor_ms": wall_ms(lambda: tensor_eval_acc(yd, pd), iters),
                     "reference_device_ms": wall_ms(lambda: reference_eval_acc(yd, pd), cpu_reps, warm=1),
                     "reference_host_ms": wall_ms(lambda: reference_eval_acc(yh, ph), cpu_reps, warm=1),
                     "equal_to_tensor_restatement": ours == tensor_eval_acc(yd, pd),
                     "equal_to_reference": ours == reference_eval_acc(yh, ph)})
    return {"rows": rows}


def run_step(name, quick):
    import torch
    assert torch.cuda.is_available(), "a measurement needs the MI355X"
    res = {"proteins": lambda: step_proteins(quick), "pokec": lambda: step_acc(POKEC, quick, 3),
           "image_text": lambda: step_acc(IMAGE_TEXT, quick, 1)}[name]()
    res["device"] = torch.cuda.get_device_name(0)
    return res


# ---- report ---------------------------------------------------------------------------------------------------------------------------------
def ms(t):
    return f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"


def share(metric_ms):
    """share of one scripted evaluation period (9 epochs + forward + metric) that the metric takes, for both epoch times"""
    return " .. ".join(f"{100 * metric_ms / (EVAL_STEP * e + FORWARD_MS + metric_ms):.1f} %" for e in EPOCH_MS)


def report(results, quick, failed):
    dev = next((r["device"] for r in results.values()), "no step finished")
    lines = ["# r13 -- evaluation metrics on the device (`csrc/eval_metrics.hip`, `scripts/metrics_bench.py`)", "",
             f"Device: {dev}.  Synthetic inputs (normal scores, 10 % positives, seeded).  Times in ms: median (min .. max).  `table`: device",
             "events around the asynchronous `rocauc_counts`; every other column: the host clock around a call that ends in a read-back,",
             "20 warm iterations (the host reference: 2 to 5 repetitions).  `device` / `host`: where the inputs live when the call starts",
             "-- the reference moves device tensors to the host first, this package stages host tensors through the GPU.",
             "Baselines: (a) the reference's loop restated, on the host CPUs; (b) `torch.sort` + `cumsum` + `searchsorted` on the same GPU.",
             "Nothing here is a pass bar." + ("  **--quick rehearsal: toy sizes, not a measurement.**" if quick else ""), ""]
    if "proteins" in results:
        p = results["proteins"]
        lines += [f"## `eval_rocauc`: the ogbn-proteins evaluation, three splits x 112 columns (reference (a): {p['reference']})", "",
                  "| rows | workspace MB | table | ours, device | ours, host | (b) tensor ops, device | (a) reference, device | (a) reference, host | ours / (b) | = (b) | = on host | abs. difference to (a) |",
                  "|---|---|---|---|---|---|---|---|---|---|---|---|"]
        for r in p["rows"]:
            lines.append(f"| {r['rows']} | {r['workspace_mb']:.1f} | {ms(r['table_ms'])} | {ms(r['ours_device_ms'])} | {ms(r['ours_host_ms'])} | "
                         f"{ms(r['tensor_ms'])} | {ms(r['reference_device_ms'])} | {ms(r['reference_host_ms'])} | "
                         f"{r['ours_device_ms'][0] / r['tensor_ms'][0]:.2f} | {r['equal_to_tensor_restatement']} | {r['equal_on_host_tensors']} | "
                         f"{r['difference_to_reference']:.1e} |")
        tot = {k: sum(r[k][0] for r in p["rows"]) for k in ("ours_device_ms", "ours_host_ms", "tensor_ms", "reference_device_ms", "reference_host_ms")}
        lines += ["", f"The three calls of one evaluation together: reference {tot['reference_device_ms']:.0f} ms from device tensors "
                      f"({tot['reference_host_ms']:.0f} ms from host tensors), tensor operations {tot['tensor_ms']:.2f} ms, this package "
                      f"{tot['ours_device_ms']:.2f} ms ({tot['ours_host_ms']:.2f} ms from host tensors).",
                  f"Share of one scripted evaluation period ({EVAL_STEP} epochs of {EPOCH_MS[0]:.0f}-{EPOCH_MS[1]:.0f} ms + a {FORWARD_MS} ms forward + the metric), "
                  f"at either epoch time: before {share(tot['reference_device_ms'])}, after {share(tot['ours_device_ms'])} "
                  f"(main-batch.py evaluates on host tensors: before {share(tot['reference_host_ms'])}, after {share(tot['ours_host_ms'])}).", ""]
    for name, title in (("pokec", "`eval_acc`: Pokec, 1,632,803 x 2 in three random splits"), ("image_text", "`eval_acc`: image and text, 15,000 x 10")):
        if name not in results:
            continue
        lines += [f"## {title}", "",
                  "| rows | columns | ours, device | ours, host | (b) tensor ops, device | (a) reference, device | (a) reference, host | ours / (b) | = (b) | = (a) |",
                  "|---|---|---|---|---|---|---|---|---|---|"]
        for r in results[name]["rows"]:
            lines.append(f"| {r['rows']} | {r['columns']} | {ms(r['ours_device_ms'])} | {ms(r['ours_host_ms'])} | {ms(r['tensor_ms'])} | "
                         f"{ms(r['reference_device_ms'])} | {ms(r['reference_host_ms'])} | {r['ours_device_ms'][0] / r['tensor_ms'][0]:.2f} | "
                         f"{r['equal_to_tensor_restatement']} | {r['equal_to_reference']} |")
        lines.append("")
    slower = [(n, r["rows"]) for n, res in results.items() for r in res["rows"] if r["ours_device_ms"][0] > r["tensor_ms"][0]]
    if slower:
        lines.append("**Slower than the tensor-operation restatement (b)** at: " + ", ".join(f"{n} {rows} rows" for n, rows in slower) +
                     ".  Not tuned in this round.")
    elif results:
        lines.append("The kernel path is faster than the tensor-operation restatement (b) at every listed shape.")
    if failed:
        lines.append(f"**The run ended at step `{failed}`: it failed or ran into its time limit; later steps were not started.**")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_eval_metrics.md"))
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--step", help="(internal) run one step in this process and write its JSON to --json")
    ap.add_argument("--json")
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, ROOT)
        res = run_step(args.step, args.quick)
        with open(args.json, "w") as f:
            json.dump(res, f)
        return 0
    results, failed = {}, None
    with tempfile.TemporaryDirectory() as tmp:
        for name, limit in STEPS:
            path = os.path.join(tmp, name + ".json")
            cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--json", path]
            print("step", name, flush=True)
            rc = subprocess.run(cmd + (["--quick"] if args.quick else [])).returncode
            if rc != 0 or not os.path.exists(path):
                failed = name
                print(f"step {name} ended with status {rc}: nothing more is started", flush=True)
                break
            with open(path) as f:
                results[name] = json.load(f)
    text = report(results, args.quick, failed)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
