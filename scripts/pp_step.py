"""Training step of the physical-particle folder's model (physical particle/run.sh: DIFFormer_v2, hidden 64, 2 layers, --use_bn
--use_residual --use_graph --use_weight, batches of 1,024 ActsTrack-sized / 8,192 Tau3Mu-sized graphs): forward over the batch of
graphs, mean pooling per graph + a linear read-out + BCE (main.py's loop), backward, Adam.  Synthetic batches.
    python scripts/pp_step.py [--readout {torch,device}] [--kernels simple,sigmoid] [--reps N]
--readout torch (the default: the recorded numbers of profiles/r06_physical_particle_step.txt) restates global_mean_pool with
tensor operations and steps with torch.optim.Adam and F.binary_cross_entropy_with_logits; --readout device is the folder's model
on this package alone: GraphGNN (csrc/graph_readout.hip), difformer_amd.bce_with_logits and difformer_amd.Adam."""
import argparse
import os, sys, time
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "scripts"))
import difformer_amd
from difformer_amd import DIFFormer_v2
from exp_v2_batch import batch
ap = argparse.ArgumentParser()
ap.add_argument("--readout", choices=("torch", "device"), default="torch")
ap.add_argument("--kernels", default="simple,sigmoid")
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()
dev = torch.device("cuda:0")
print(f"{'batch':30s} {'kernel':8s} {'nodes':>8s} {'train step ms':>14s} {'eval forward ms':>16s}   (--readout {args.readout})")
for name, B, lo, hi in (("actstrack-like 1024 x ~110", 1024, 40, 180), ("tau3mu-like 8192 x ~20", 8192, 8, 32)):
    for kernel in args.kernels.split(","):
        n_nodes, ei, n = batch(B, lo, hi)
        torch.manual_seed(0)
        model = DIFFormer_v2(7, 64, 64, num_layers=2, kernel=kernel, use_bn=True, use_residual=True, use_graph=True, use_weight=True,
                             dropout=0.4).to(dev)
        x = torch.randn(n, 7, device=dev)
        y = (torch.rand(B, device=dev) > 0.5).float()
        if args.readout == "device":
            graph_model = difformer_amd.GraphGNN(64, 1, model, "mean").to(dev)
            opt = difformer_amd.Adam(graph_model.parameters(), lr=1.5e-3, weight_decay=1e-3)
            target = y[:, None]

            def step():
                graph_model.train(); opt.zero_grad()
                loss = difformer_amd.bce_with_logits(graph_model(x, ei, n_nodes), target)
                loss.backward(); opt.step()
        else:
            head = torch.nn.Linear(64, 1).to(dev)
            opt = torch.optim.Adam(list(model.parameters()) + list(head.parameters()), lr=1.5e-3, weight_decay=1e-3)
            gid = torch.repeat_interleave(torch.arange(B, device=dev), n_nodes)
            inv = (1.0 / n_nodes.float())[:, None]

            def step():
                model.train(); opt.zero_grad()
                h = model(x, ei, n_nodes)
                pooled = torch.zeros(B, h.shape[1], device=dev).index_add_(0, gid, h) * inv          # global_mean_pool
                loss = F.binary_cross_entropy_with_logits(head(pooled)[:, 0], y)
                loss.backward(); opt.step()

        def ev():
            model.eval()
            with torch.no_grad():
                model(x, ei, n_nodes)

        def timed(fn, reps=args.reps):
            for _ in range(3): fn()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(reps): fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / reps * 1e3
        print(f"{name:30s} {kernel:8s} {n:8d} {timed(step):14.3f} {timed(ev):16.3f}", flush=True)
