"""Generate tests/golden/golden_topk.npz by RUNNING THE REFERENCE ITSELF (the pattern of make_golden.py: the reference file
`node classification/difformer.py` imported verbatim with the same three shims, run in float64).

    python tests/golden/make_golden_topk.py

Runs only where the reference checkout is present; the fixture it writes is committed.  Each case holds its inputs and the
float64 top-k (values, int32 indices; larger value first, among equals the lower index) of the reference's own dense attention:
  attn/*   `full_attention_conv(q, k, v, kernel, output_attn=True)[1]`.  `sigmoid` with H = 2 and N != L.  `simple` with
           H = 1 and N == L: the only shapes at which the reference's `simple` branch returns an attention (difformer.py:29
           adds an [L,H,D] tensor to an [N,H,D] one, and :43 divides [N,L,H] by [N,H,1]).
  model/*  one 2-layer `DIFFormer(kernel='sigmoid', num_heads=2, use_graph=False, use_source=False)` through the reference's
           `get_attentions` (:211-226).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import load_reference  # noqa: E402


def topk(attn, k):
    """attn [..., N, L, H] float64 tensor -> (values [..., N, H, k], indices int32): stable descending order."""
    a = attn.transpose(-1, -2)
    order = torch.sort(a, dim=-1, descending=True, stable=True).indices[..., :k]
    return torch.gather(a, -1, order).numpy(), order.numpy().astype(np.int32)


def main():
    ref = load_reference()
    g = torch.Generator().manual_seed(20261019)
    torch.set_default_dtype(torch.float64)          # the reference hard-codes default-dtype torch.ones (difformer.py:27,32,50)
    flat = {}
    shapes = [  # (tag, kernel, N, L, H, M, stored k)
        ("sigmoid_n30_l45_h2_m16", "sigmoid", 30, 45, 2, 16, 32),
        ("sigmoid_n300_l257_h2_m12", "sigmoid", 300, 257, 2, 12, 16),
        ("simple_n37_h1_m16", "simple", 37, 37, 1, 16, 32),
        ("simple_n300_h1_m20", "simple", 300, 300, 1, 20, 16),
    ]
    for tag, kern, n, l, h, m, k in shapes:
        scale = m ** -0.25 if kern == "sigmoid" else 1.0          # scores of unit variance: sigma does not saturate
        q = (torch.randn(n, h, m, generator=g, dtype=torch.float32) * scale)
        kk = (torch.randn(l, h, m, generator=g, dtype=torch.float32) * scale)
        v = torch.randn(l, h, m, generator=g, dtype=torch.float32)
        _, attn = ref.full_attention_conv(q.double(), kk.double(), v.double(), kern, True)
        vals, idx = topk(attn, k)
        flat.update({f"attn/{tag}::q": q.numpy(), f"attn/{tag}::k": kk.numpy(), f"attn/{tag}::kernel": np.array(kern),
                     f"attn/{tag}::values": vals, f"attn/{tag}::indices": idx})
    # ---- the model: parameters drawn in float32, run in float64 (as make_golden.py) ----
    n, f_in, hidden, c, k = 300, 12, 16, 4, 16
    cfg = dict(num_layers=2, num_heads=2, kernel="sigmoid", use_graph=False, use_source=False)
    x = torch.randn(n, f_in, generator=g, dtype=torch.float32)
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(123)
    model = ref.DIFFormer(f_in, hidden, c, **cfg)
    model.reset_parameters()
    with torch.no_grad():
        for bn in model.bns:
            bn.weight.add_(0.1 * torch.randn(bn.weight.shape, generator=torch.Generator().manual_seed(7)))
            bn.bias.add_(0.1 * torch.randn(bn.bias.shape, generator=torch.Generator().manual_seed(8)))
    sd = {name: t.float().numpy().copy() for name, t in model.state_dict().items()}
    torch.set_default_dtype(torch.float64)
    model = model.double().eval()
    with torch.no_grad():
        attn = model.get_attentions(x.double())                    # [layers, N, N, H]
    vals, idx = topk(attn, k)
    tag = "model/a_h2_nograph"
    flat.update({f"{tag}::x": x.numpy(), f"{tag}::values": vals, f"{tag}::indices": idx})
    full = dict(in_channels=f_in, hidden_channels=hidden, out_channels=c, alpha=0.5, use_bn=True, use_residual=True,
                use_weight=True, graph_weight=-1, **cfg)
    flat.update({f"{tag}::cfg/{name}": np.array(v) for name, v in full.items()})
    flat.update({f"{tag}::sd/{name}": v for name, v in sd.items()})
    torch.set_default_dtype(torch.float32)
    out = os.path.join(HERE, "golden_topk.npz")
    np.savez_compressed(out, **flat)
    print(len(flat), "arrays,", os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
