"""Two builds of libdifformer_hip.so, bit for bit, on the whole-model kernels for tiny graphs (needs the GPU):

    python scripts/exp_tiny_bitwise.py LIB_A LIB_B [more libraries ...]

Every case of tests/test_gpu_tiny._cases() under tiny.PLAN = 1 (one workgroup) and 2 (grid), forward + backward once with the
seeds of _run_case (`sigmoid` on one workgroup capped at 700 nodes, as the test does; the dropout uniforms come from the seeded
device generator).  Each library runs in a fresh child process (DIFFORMER_HIP_LIB) under its own time limit; `out`, `dx` and every
parameter gradient are compared byte for byte on the host, every later library against the first.  Exit status 1 if any differ.

A build of another commit:  git worktree add W <commit>;  make -C W/difformer_amd/csrc OUT=$PWD/a.so OBJDIR=$PWD/obj_a $PWD/a.so
(add EXTRA=-fno-slp-vectorize to take the SLP vectoriser out: under -ffp-contract=fast it decides which multiply-add pairs of
these kernels end up fused, see profiles/tiny_stages_bitwise.txt).  Where scripts/device_asm_diff.py already says `identical`,
this run is not needed: it is for changes that move the device code."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(out_path):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import numpy as np
    import torch
    import test_gpu_tiny as tt
    from difformer_amd import DIFFormer, tiny
    dev = torch.device("cuda:0")
    saved = {}
    for plan in (1, 2):
        tiny.PLAN = plan
        for c in tt._cases():
            if plan == 1 and c["kernel"] == "sigmoid" and c["n"] > 700:
                c = dict(c, n=700)
            n, L = c["n"], c["layers"]
            torch.manual_seed(100 + c["seed"])
            model = DIFFormer(c["f_in"], c["hidden"], c["c"], num_layers=L, num_heads=1, kernel=c["kernel"], alpha=c["alpha"],
                              dropout=c["dropout"], use_bn=c["use_bn"], use_residual=c["use_residual"], use_weight=c["use_weight"],
                              use_graph=c["use_graph"], graph_weight=c["graph_weight"], use_source=c["use_source"])
            with torch.no_grad():
                for bn in model.bns:
                    bn.weight.add_(0.2 * torch.randn(bn.weight.shape))
                    bn.bias.add_(0.2 * torch.randn(bn.bias.shape))
            g = torch.Generator().manual_seed(c["seed"])
            x = torch.randn(n, c["f_in"], generator=g)
            iso = min(c["iso"], n - 1)
            ei = torch.cat([tt._graph(n, n * c["deg"], seed=c["seed"], isolated=iso), torch.arange(n - iso).repeat(2, 1)], dim=1)
            w = (torch.rand(ei.shape[1], generator=g) * 2 + 0.05) if c["weighted"] else None
            go = torch.randn(n, c["c"], generator=g)
            model = model.to(dev).train()
            xd = x.to(dev).requires_grad_(True)
            before = dict(tiny.stats)
            torch.manual_seed(4242)                  # one torch.rand((L + 1, n, d)) per forward from the device generator
            out = model(xd, ei.to(dev) if c["use_graph"] else None, w.to(dev) if (c["use_graph"] and w is not None) else None)
            out.backward(go.to(dev))
            assert tiny.stats["forward"] == before["forward"] + 1 and tiny.stats["backward"] == before["backward"] + 1
            tag = f"plan{plan}-{tt._ID(c)}"
            res = {"out": out.detach(), "dx": xd.grad}
            res.update({"grad." + k: p.grad for k, p in model.named_parameters() if p.grad is not None})
            for k, v in res.items():
                saved[f"{tag}/{k}"] = np.frombuffer(v.cpu().numpy().tobytes(), dtype=np.uint8)
    torch.cuda.synchronize()
    np.savez(out_path, **saved)


def compare(pa, pb):
    import numpy as np
    a, b = np.load(pa), np.load(pb)
    assert set(a.files) == set(b.files), sorted(set(a.files) ^ set(b.files))
    runs = {}
    for k in sorted(a.files):
        x, y = a[k], b[k]
        if not np.array_equal(x, y):
            d = float(np.max(np.abs(x.view(np.float32).astype(np.float64) - y.view(np.float32).astype(np.float64))))
            runs.setdefault(k.split("/")[0], []).append((k.split("/")[1], d))
    for run, ts in runs.items():
        worst = max(ts, key=lambda t: t[1])
        print(f"  {run}: {len(ts)} tensors differ{' (out among them)' if any(t[0] == 'out' for t in ts) else ''}; largest {worst[1]:.3g} in {worst[0]}")
    n_runs = len({k.split("/")[0] for k in a.files})
    print(f"  {sum(len(t) for t in runs.values())} of {len(a.files)} tensors differ, in {len(runs)} of {n_runs} runs")
    return not runs


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    libs = sys.argv[1:]
    if len(libs) < 2:
        sys.exit(__doc__)
    with tempfile.TemporaryDirectory() as tmp:
        outs = []
        for i, lib in enumerate(libs):
            outs.append(os.path.join(tmp, f"{i}.npz"))
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", outs[-1]], check=True, timeout=300, cwd=ROOT,
                           env=dict(os.environ, DIFFORMER_HIP_LIB=os.path.abspath(lib)))
        same = True
        for lib, out in zip(libs[1:], outs[1:]):
            print(f"{libs[0]} against {lib}:")
            same = compare(outs[0], out) and same
    sys.exit(0 if same else 1)


if __name__ == "__main__":
    main()
