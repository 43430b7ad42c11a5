"""Snapshot batches on the GPU (csrc/tiny_batched.hip, difformer_amd/snapshots.py): one forward launch of T workgroups and one
backward for all snapshots of an epoch.  Output, dx and every parameter gradient against float64 autograd of the oracle at the
sizes where the kernels can go wrong, the reference's own cumulative-epoch fixtures, bitwise independence of a snapshot from the
composition of its batch, the ordered gradient sum bit for bit, dropout with supplied uniforms, the path counters, and guard bands
around every buffer the path allocates."""
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import guarded
from conftest import grad_err, grad_scale, rel_err
from oracle import difformer_oracle_grad as og
from st_common import ST, build_model, cases, cost_fn, snapshots as st_snapshots

pytestmark = pytest.mark.gpu
TOL = 1e-4


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _graph(n, e, seed, loops=True):
    g = torch.Generator().manual_seed(seed)
    ei = torch.randint(0, n, (2, e), generator=g)
    if e >= 20:
        ei[:, : e // 10] = ei[:, e // 10: 2 * (e // 10)]                       # duplicates
    return torch.cat([ei, torch.arange(n).repeat(2, 1)], dim=1) if loops else ei


def _oracle(p, x, ei, w, cfg, masks=None):
    """og.difformer_forward with the dropout masks of :192 / :204 applied where the reference applies them."""
    if masks is None:
        return og.difformer_forward(p, x, ei, w, cfg)
    alpha = cfg["alpha"]
    ln = lambda t, k: F.layer_norm(t, (t.shape[-1],), p[k + ".weight"], p[k + ".bias"], 1e-5)
    h = F.linear(x, p["fcs.0.weight"], p["fcs.0.bias"])
    if cfg["use_bn"]:
        h = ln(h, "bns.0")
    h = torch.relu(h) * masks[0]
    layers = [h]
    for i in range(cfg["num_layers"]):
        h = og.difformer_conv(p, f"convs.{i}.", h, h, ei, w, layers[0], cfg)
        if cfg["use_residual"]:
            h = alpha * h + (1 - alpha) * layers[i]
        if cfg["use_bn"]:
            h = ln(h, f"bns.{i + 1}")
        h = h * masks[i + 1]
        layers.append(h)
    return F.linear(h, p["fcs.1.weight"], p["fcs.1.bias"])


def _case(sizes, kernel, hidden=4, f_in=4, c=1, layers=2, use_bn=True, use_residual=True, use_weight=False, use_graph=True,
          use_source=False, graph_weight=-1.0, alpha=0.5, shared=False, weighted=True, deg=4, empty=None, dropout=0.0, seed=0):
    return dict(sizes=list(sizes), kernel=kernel, hidden=hidden, f_in=f_in, c=c, layers=layers, use_bn=use_bn, use_residual=use_residual,
                use_weight=use_weight, use_graph=use_graph, use_source=use_source, graph_weight=graph_weight, alpha=alpha, shared=shared,
                weighted=weighted, deg=deg, empty=empty, dropout=dropout, seed=seed)


MIXED = [1, 20, 65, 129, 513]          # blockDim comes from the largest; its rows loop beyond 512 threads
# A pruned table: every size both as an equal-n batch and inside the mixed one, T in {1, 2, 3, 257}, hidden {1, 4, 5, 8}, input
# features {1, 8, 64}, outputs {1, 8}, layers {1, 2, 8}, both kernels, every constructor flag on and off, graph_weight > 0, shared and
# per-snapshot graphs, a snapshot without edges, no graph at all.
CASES = [
    _case([1] * 3, "simple", hidden=4, f_in=1, layers=1, use_bn=False, deg=1, seed=1),
    _case([1] * 2, "sigmoid", hidden=4, f_in=8, use_bn=False, use_weight=True, deg=1, seed=2),
    _case([2] * 2, "sigmoid", hidden=5, f_in=8, c=8, use_weight=True, deg=1, seed=3),
    _case([2] * 3, "simple", hidden=8, f_in=64, c=8, layers=8, use_source=True, deg=1, seed=4),
    _case([20] * 257, "simple", shared=True, weighted=True, seed=5),                         # more workgroups than compute units
    _case([20] * 3, "sigmoid", hidden=8, f_in=64, c=8, layers=8, use_weight=True, use_source=True, graph_weight=0.3, seed=6),
    _case([64] * 2, "simple", use_weight=True, graph_weight=0.8, use_residual=False, seed=7),
    _case([64] * 3, "sigmoid", hidden=1, f_in=1, layers=1, use_bn=False, weighted=False, seed=8),
    _case([65] * 3, "sigmoid", hidden=5, f_in=8, use_source=True, alpha=0.2, seed=9),
    _case([65] * 1, "simple", hidden=5, f_in=1, c=8, layers=1, use_bn=False, use_residual=False, seed=10),
    _case([129] * 3, "simple", hidden=4, f_in=8, deg=12, seed=11),                            # covid: per-snapshot graphs
    _case([129] * 2, "sigmoid", hidden=4, f_in=8, deg=12, shared=True, weighted=False, seed=12),
    _case([513] * 2, "simple", hidden=4, f_in=8, empty=1, seed=13),
    _case([513] * 1, "sigmoid", hidden=8, f_in=8, layers=1, use_weight=True, seed=14),
    _case([1068] * 2, "simple", hidden=4, f_in=8, shared=True, deg=8, seed=15),               # wikimath's shape
    _case([1068] * 1, "sigmoid", hidden=4, f_in=8, layers=2, deg=8, seed=16),
    _case(MIXED, "simple", hidden=4, f_in=8, empty=2, seed=17),
    _case(MIXED, "sigmoid", hidden=8, f_in=8, c=8, use_weight=True, use_source=True, graph_weight=0.3, empty=0, seed=18),
    _case(MIXED[::-1], "simple", hidden=5, f_in=64, layers=8, use_weight=True, seed=19),
    _case([20, 64], "simple", use_graph=False, seed=20),
    _case([65, 20, 7], "sigmoid", hidden=5, use_graph=False, use_bn=False, seed=21),
]
_ID = lambda c: f"{c['kernel']}-n{'x'.join(map(str, sorted(set(c['sizes']))))}-T{len(c['sizes'])}-d{c['hidden']}-L{c['layers']}-s{c['seed']}"


def _build(c, dev, train=True):
    """-> (model on dev, oracle cfg, host snapshots [(x, ei, w, go)])."""
    from difformer_amd import DIFFormer
    d, L = c["hidden"], c["layers"]
    torch.manual_seed(100 + c["seed"])
    model = DIFFormer(c["f_in"], d, c["c"], num_layers=L, num_heads=1, kernel=c["kernel"], alpha=c["alpha"], dropout=c["dropout"],
                      use_bn=c["use_bn"], use_residual=c["use_residual"], use_weight=c["use_weight"], use_graph=c["use_graph"],
                      graph_weight=c["graph_weight"], use_source=c["use_source"])
    with torch.no_grad():
        for bn in model.bns:
            bn.weight.add_(0.2 * torch.randn(bn.weight.shape))
            bn.bias.add_(0.2 * torch.randn(bn.bias.shape))
    g = torch.Generator().manual_seed(c["seed"])
    host, first = [], None
    for b, n in enumerate(c["sizes"]):
        x = torch.randn(n, c["f_in"], generator=g)
        go = torch.randn(n, c["c"], generator=g)
        if not c["use_graph"]:
            host.append((x, None, None, go))
            continue
        if c["shared"] and first is not None:
            ei, w = first
        else:
            ei = _graph(n, 0 if c["empty"] == b else n * c["deg"], seed=31 * c["seed"] + b, loops=c["empty"] != b)
            w = (torch.rand(ei.shape[1], generator=g) * 2 + 0.05) if c["weighted"] else None
            first = first or (ei, w)
        host.append((x, ei, w, go))
    cfg = dict(in_channels=c["f_in"], hidden_channels=d, out_channels=c["c"], num_layers=L, num_heads=1, kernel=c["kernel"],
               alpha=c["alpha"], use_bn=c["use_bn"], use_residual=c["use_residual"], use_weight=c["use_weight"],
               use_graph=c["use_graph"], graph_weight=c["graph_weight"], use_source=c["use_source"])
    model = model.to(dev)
    return (model.train() if train else model.eval()), cfg, host


def _batch(host, dev, shared=False):
    """SnapshotBatch of the host snapshots: tensors that are the same object on the host are the same object on the device."""
    from difformer_amd import SnapshotBatch
    moved = {}

    def to(t):
        if t is None:
            return None
        if id(t) not in moved:
            moved[id(t)] = t.to(dev)
        return moved[id(t)]
    xs = [x.to(dev) for x, _, _, _ in host]
    eis, ws = [to(ei) for _, ei, _, _ in host], [to(w) for _, _, w, _ in host]
    if shared and len({id(e) for e in eis}) == 1 and len({id(w) for w in ws}) == 1:
        return SnapshotBatch(xs, eis[0], ws[0])                            # the one-tensor-pair form of the constructor
    return SnapshotBatch(xs, eis, ws)


def _oracle_batch(model, host, cfg, dtype=torch.float64, masks=None):
    """The per-snapshot loop in `dtype` on the CPU -> ([out_b], [dx_b], {parameter: summed gradient})."""
    p = og.leaves({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, dtype)
    outs, dxs = [], []
    for b, (x, ei, w, go) in enumerate(host):
        xb = x.to(dtype).requires_grad_(True)
        out = _oracle(p, xb, ei, None if w is None else w.to(dtype), cfg, None if masks is None else masks[b].to(dtype))
        out.backward(go.to(dtype))
        outs.append(out.detach().numpy())
        dxs.append(xb.grad.numpy())
    return outs, dxs, {k: (None if v.grad is None else v.grad.numpy()) for k, v in p.items()}


def _check_against_oracle(model, batch, Y, host, cfg, masks=None):
    """Y per snapshot, dx and every parameter gradient at the project's bar: 1e-4 per tensor (conftest.rel_err / grad_err), or --
    for the tensors a float32 backward cannot resolve to 1e-4 of themselves -- within 4x the error of the SAME oracle run in
    float32, exactly as tests/test_gpu_tiny.py::_run_case."""
    outs, dxs, grads = _oracle_batch(model, host, cfg, torch.float64, masks)
    outs32, dxs32, grads32 = _oracle_batch(model, host, cfg, torch.float32, masks)
    for got, ref in zip(batch.split(Y.detach()), outs):
        assert rel_err(got.cpu().numpy(), ref) < TOL
    gmax = max([float(np.abs(v).max()) for v in grads.values() if v is not None] + [1e-30])
    floor = 2e-6 if batch.max_n >= 16 else 2e-3          # (one node: sigma / sigma is exactly 1 on the CPU, p v / p in the kernel is not)

    def ok(got, r64, r32, what):
        e, e32 = grad_err(got, r64, gmax, floor), grad_err(r32, r64, gmax, floor)
        print(f"{what}: {e:.3e} (float32 oracle {e32:.3e})")
        assert e < TOL or e < 4.0 * e32, (what, e, e32)

    ok(batch.x.grad.cpu().numpy(), np.concatenate(dxs), np.concatenate(dxs32), "dx")
    for k, prm in model.named_parameters():
        if grads[k] is None:
            assert prm.grad is None or not prm.grad.any(), k
            continue
        assert prm.grad is not None and torch.isfinite(prm.grad).all(), k
        ok(prm.grad.cpu().numpy(), grads[k], grads32[k], k)


def _run(model, batch, host, dev, **kw):
    """One forward_snapshots + backward with the host snapshots' output gradients -> Y (batch.x.grad and the parameters' .grad set)."""
    model.zero_grad()
    batch.x.grad = None
    batch.x.requires_grad_(True)
    Y = model.forward_snapshots(batch, **kw)
    Y.backward(torch.cat([go for _, _, _, go in host]).to(dev))
    return Y


# ---- parity with the float64 oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", CASES, ids=_ID)
def test_forward_and_backward_against_the_oracle(c, dev):
    from difformer_amd import snapshots, tiny
    model, cfg, host = _build(c, dev)
    batch = _batch(host, dev, shared=c["shared"])
    assert len(batch) == len(host) and batch.node_ptr[-1] == sum(c["sizes"])
    if c["use_graph"]:
        assert len({id(g) for g in batch.graphs}) == (1 if c["shared"] else len(host))       # a shared graph is built once
    before, tiny_before = dict(snapshots.stats), dict(tiny.stats)
    Y = _run(model, batch, host, dev)
    assert snapshots.stats == dict(before, forward=before["forward"] + 1, backward=before["backward"] + 1)
    assert tiny.stats["forward"] == tiny_before["forward"] and tiny.stats["backward"] == tiny_before["backward"]
    assert Y.shape == (sum(c["sizes"]), c["c"]) and torch.isfinite(Y).all()
    _check_against_oracle(model, batch, Y, host, cfg)
    # two identical calls are bitwise equal
    g1 = [batch.x.grad.clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None]
    Y2 = _run(model, batch, host, dev)
    g2 = [batch.x.grad] + [p.grad for p in model.parameters() if p.grad is not None]
    assert torch.equal(Y, Y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))


# ---- the reference's own numbers ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases("cumul"))
def test_cumulative_epoch_fixtures(name, dev):
    """The cumul/ cases of tests/golden/golden_st.npz (spatial-temporal/main.py:94-119 run by the folder's own model in float64)
    through ONE forward_snapshots and ONE backward: outputs, the summed cost and all gradients."""
    from difformer_amd import DIFFormer, SnapshotBatch, snapshots
    c = ST[name]
    model, cfg = build_model(DIFFormer, c, dev)
    snaps = st_snapshots(c, dev)
    batch = SnapshotBatch([s[0] for s in snaps], [s[1] for s in snaps], [s[2] for s in snaps])
    before = dict(snapshots.stats)
    Y = model.forward_snapshots(batch)
    cost_tr = sum(cost_fn(y_hat, s[3]) for y_hat, s in zip(batch.split(Y), snaps)) / len(snaps)      # main.py:107-116
    cost_tr.backward()
    assert snapshots.stats == dict(before, forward=before["forward"] + 1, backward=before["backward"] + 1)
    for t, o in enumerate(batch.split(Y.detach())):
        assert rel_err(o.cpu().numpy(), c["out_f64"][t]) < TOL
    assert abs(float(cost_tr.detach()) - float(c["loss_f64"])) < TOL * abs(float(c["loss_f64"]))
    gmax = grad_scale(c)
    for k, p in model.named_parameters():
        ref = c["grad_f64/" + k]
        got = np.zeros_like(ref) if p.grad is None else p.grad.cpu().numpy()
        assert np.isfinite(got).all(), k
        assert grad_err(got, ref, gmax) < TOL, k


# ---- independence of the batch's composition, bitwise -------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,hidden", [("simple", 4), ("sigmoid", 4), ("simple", 8), ("sigmoid", 5)])
@pytest.mark.parametrize("sizes", [[20, 50, 64, 7], [513, 20, 600, 129]], ids=["one-wave", "eight-waves"])
def test_a_snapshot_does_not_depend_on_its_batch(sizes, kernel, hidden, dev):
    """Snapshot 0's and snapshot 1's rows of Y and dx, alone or first or last or beside other neighbours: the same bits wherever
    blockDim is the same (it follows the largest snapshot: every composition of the second list holds one beyond 448 nodes)."""
    c = _case(sizes, kernel, hidden=hidden, f_in=8, c=2, use_weight=hidden != 4, use_source=hidden == 8, empty=3, seed=40 + hidden)
    model, cfg, host = _build(c, dev)
    a, b, big, e = host
    orders = [[a, b, big, e], [e, big, b, a], [big, a], [b, big, e, a, a]]
    if sizes[0] <= 64:
        orders += [[a], [b], [e, a], [b, e]]                               # one wave whatever the composition
    else:
        orders += [[a], [a, b]]                                           # 513 nodes: 512 threads on its own too
    rows = {}
    for order in orders:
        batch = _batch(order, dev)
        Y = _run(model, batch, order, dev).detach()
        for s, y, dx in zip(order, batch.split(Y), batch.split(batch.x.grad)):
            rows.setdefault(id(s), []).append((y.clone(), dx.clone()))
    assert len(rows[id(a)]) >= 6 and len(rows[id(b)]) >= 4
    for seen in rows.values():
        for y, dx in seen[1:]:
            assert torch.equal(y, seen[0][0]) and torch.equal(dx, seen[0][1])


# ---- the gradient sum, bitwise ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 257])
@pytest.mark.parametrize("kernel", ["simple", "sigmoid"])
def test_the_gradient_is_the_ordered_float64_sum_of_the_snapshots(kernel, T, dev):
    """The parameter gradients of T batch-of-one backward calls, added on the host in float64 in the order b = 0 .. T - 1 and
    rounded once to float32, equal the batched gradient bit for bit (hidden 5: padding between the parameters)."""
    c = _case([20] * T, kernel, hidden=5, f_in=8, c=2, use_weight=True, shared=True, seed=50)
    model, cfg, host = _build(c, dev)
    _run(model, _batch(host, dev, shared=True), host, dev)
    batched = {k: p.grad.clone() for k, p in model.named_parameters()}
    total = {k: torch.zeros(p.shape, dtype=torch.float64) for k, p in model.named_parameters()}
    for s in host:
        _run(model, _batch([s], dev), [s], dev)
        for k, p in model.named_parameters():
            total[k] += p.grad.cpu().double()
    for k, v in total.items():
        assert torch.equal(v.float(), batched[k].cpu()), k


# ---- dropout ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,sizes", [("simple", [20, 65, 7]), ("sigmoid", [129, 20])])
def test_dropout_with_supplied_uniforms(kernel, sizes, dev):
    c = _case(sizes, kernel, hidden=5, f_in=8, c=2, dropout=0.2, seed=60)
    model, cfg, host = _build(c, dev)
    L, d, p = c["layers"], c["hidden"], c["dropout"]
    batch = _batch(host, dev)
    u = torch.rand((L + 1) * sum(sizes) * d, generator=torch.Generator().manual_seed(7))
    # snapshot b's [(L + 1), n_b, d] block sits at (L + 1) * d * node_ptr[b]
    masks = [(u[(L + 1) * d * lo: (L + 1) * d * hi].view(L + 1, hi - lo, d) >= p).double() / (1.0 - p)
             for lo, hi in zip(batch.node_ptr[:-1], batch.node_ptr[1:])]
    Y = _run(model, batch, host, dev, _uniforms=u.to(dev))
    _check_against_oracle(model, batch, Y, host, cfg, masks)
    with pytest.raises(ValueError, match="_uniforms"):
        model.forward_snapshots(batch, _uniforms=u[:-1].to(dev))
    drawn = model.forward_snapshots(batch)                                  # its own draw: one torch.rand for the batch
    assert torch.isfinite(drawn).all() and not torch.equal(drawn, Y)
    # eval mode: dropout is the identity, whatever p and whatever uniforms
    model.eval()
    with torch.no_grad():
        y_eval = model.forward_snapshots(batch, _uniforms=u.to(dev))
        model.dropout = 0.0
        assert torch.equal(y_eval, model.forward_snapshots(batch))


# ---- path and launches --------------------------------------------------------------------------------------------------------------
def test_configurations_outside_the_limits_take_the_loop_bitwise(dev, monkeypatch):
    from difformer_amd import DIFFormer, SnapshotBatch, snapshots, tiny
    g = torch.Generator().manual_seed(3)
    sizes = [300, 130, 200]
    xs = [torch.randn(n, 8, generator=g).to(dev) for n in sizes]
    eis = [_graph(n, 4 * n, n).to(dev) for n in sizes]
    batch = SnapshotBatch(xs, eis)
    torch.manual_seed(0)
    for kw in (dict(hidden=16), dict(hidden=4, heads=2)):
        model = DIFFormer(8, kw["hidden"], 2, num_heads=kw.get("heads", 1)).to(dev).eval()
        before = dict(snapshots.stats)
        with torch.no_grad():
            Y = model.forward_snapshots(batch)
            loop = torch.cat([model(x, ei) for x, ei in zip(batch.split(batch.x), eis)])
        assert snapshots.stats == dict(before, fallback=before["fallback"] + 1) and torch.equal(Y, loop)
    model = DIFFormer(8, 4, 2).to(dev).train()
    # dropout = 1 in training, an edge_weight that wants a gradient, the switch: the loop; and back on the kernels without them
    ws = [torch.rand(ei.shape[1], device=dev, requires_grad=True) for ei in eis]
    wbatch = SnapshotBatch(xs, eis, ws)
    before = dict(snapshots.stats)
    model.forward_snapshots(wbatch).sum().backward()
    assert all(w.grad is not None for w in ws)
    model.dropout = 1.0
    assert torch.isfinite(model.forward_snapshots(batch)).all()
    model.dropout = 0.0
    monkeypatch.setattr(tiny, "ENABLED", False)
    model.forward_snapshots(batch)
    monkeypatch.setattr(tiny, "ENABLED", True)
    assert snapshots.stats == dict(before, fallback=before["fallback"] + 3)
    model.forward_snapshots(batch).sum().backward()
    assert snapshots.stats == dict(before, fallback=before["fallback"] + 3, forward=before["forward"] + 1, backward=before["backward"] + 1)
    with torch.no_grad():                                                   # frozen or not, eval or not: one forward launch
        model.eval()
        model.forward_snapshots(batch)
    assert snapshots.stats["forward"] == before["forward"] + 2 and snapshots.stats["backward"] == before["backward"] + 1


def test_a_bad_edge_index_raises_at_construction(dev):
    from difformer_amd import SnapshotBatch, tiny
    tiny._poll_status(wait=True)
    xs = [torch.randn(10, 4, device=dev), torch.randn(12, 4, device=dev)]
    bad = _graph(12, 30, 1)
    bad[1, 5] = 12
    with pytest.raises(ValueError, match="outside"):
        SnapshotBatch(xs, [_graph(10, 30, 0).to(dev), bad.to(dev)])
    tiny._poll_status(wait=True)                                            # reported once


@pytest.mark.parametrize("kernel,n,d,T,shared", [("simple", 20, 4, 104, True), ("sigmoid", 129, 8, 50, False)])
def test_steady_state_epochs_neither_wait_nor_grow(kernel, n, d, T, shared, dev):
    """main.py:86-121 on a batch: from the second epoch on nothing synchronises with the device (torch's sync debug mode raises if
    anything does), and across four epochs with an Adam step neither the allocated memory nor the CSR cache grows -- the check of
    tests/test_gpu_st.py::test_cumulative_epochs."""
    from difformer_amd import DIFFormer, SnapshotBatch, ops
    torch.manual_seed(123)
    model = DIFFormer(d, 4, 1, num_layers=2, alpha=0.5, dropout=0.0, num_heads=1, kernel=kernel, use_bn=True, use_residual=True,
                      use_graph=True, use_weight=False).to(dev).train()
    g = torch.Generator().manual_seed(17)
    xs, ys = torch.randn(T, n, d, generator=g).to(dev), torch.randn(T, n, generator=g).to(dev)
    if shared:
        batch = SnapshotBatch(xs, _graph(n, 4 * n, 0).to(dev))
    else:
        batch = SnapshotBatch(xs, [_graph(n, 12 * n, t).to(dev) for t in range(T)])
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=0.0)    # main.py:80

    def epoch():
        Y = model.forward_snapshots(batch)
        cost_tr = ((Y.view(T, n, 1) - ys.view(T, 1, n)) ** 2).mean()        # main.py:107-116, the costs of equal-n snapshots
        cost_tr.backward()
        return cost_tr

    def state():
        gc.collect()
        torch.cuda.synchronize()
        return len(ops.csr_cache), torch.cuda.memory_allocated(dev)

    states, costs = [], []
    for e in range(4):
        if e >= 1:
            torch.cuda.set_sync_debug_mode("error")
        try:
            cost = epoch()
        finally:
            torch.cuda.set_sync_debug_mode("default")
        opt.step()
        opt.zero_grad()
        costs.append(float(cost.detach()))
        del cost
        states.append(state())
    assert np.isfinite(costs).all()
    assert states[-1][0] <= states[1][0] and states[-1][1] <= states[1][1] + (1 << 20), states


# ---- guard bands ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel,sizes,hidden", [("simple", [20, 65, 7], 5), ("sigmoid", [129, 1, 20], 4), ("simple", [513, 20], 8)])
def test_guard_bands_and_poisoned_buffers(kernel, sizes, hidden, dev, monkeypatch):
    """Y, dx, tape, scratch, slabs and the gradient buffer come out of a guarded arena, 0xFF inside and around: the bands stay intact
    and no NaN reaches a result -- the padding between the parameters of the flat gradient included (zero)."""
    from difformer_amd import snapshots, tiny
    c = _case(sizes, kernel, hidden=hidden, f_in=8, c=2, use_weight=True, use_source=True, empty=1, seed=70)
    model, cfg, host = _build(c, dev)
    batch = _batch(host, dev)
    arena = guarded.GuardedArena()
    monkeypatch.setattr(snapshots, "torch", guarded.TorchProxy(arena))
    Y = _run(model, batch, host, dev)
    assert len(arena.blocks) == 6                                          # tape, y; slabs, gradient, dx, scratch
    live = [p for p in snapshots._plan(model, batch)[1] if p is not None]
    offs, P = tiny._layout(live)
    assert P > sum(p.numel() for p in live) and all(o % 4 == 0 for o in offs)      # there IS padding, and every offset is 16-byte aligned
    blk = arena.blocks[3]                                                  # the flat gradient [P] the slab sum writes
    assert blk.shape == (P,) and arena.blocks[2].shape == (len(host) * P,)
    flat = blk.buf[blk.start: blk.start + blk.nbytes].view(torch.float32)
    arena.check()
    assert torch.isfinite(Y).all() and torch.isfinite(batch.x.grad).all() and torch.isfinite(flat).all()
    used = torch.zeros(P, dtype=torch.bool, device=dev)
    for o, p in zip(offs, live):
        assert p.grad is not None and torch.equal(p.grad.reshape(-1), flat[o: o + p.numel()])
        used[o: o + p.numel()] = True
    assert not flat[~used].any()                                           # the padding between parameters: zero
    _check_against_oracle(model, batch, Y, host, cfg)
