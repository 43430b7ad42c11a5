"""What the tests of the feature-sliced product share (csrc/gcn_sliced.hip, difformer_amd/sliced.py): the lane groups and the
snake deal of the format, the graphs, the fixtures that set its three switches, and ONE decoder of a built format.

Integer work is checked exactly: the format must hold, for every row position and source tile, exactly its share of the CSR
group (as tile-local row numbers), every other cell a zero-row read.  The bank rule depends on the schedule (sl.quad_cap).
Strict: the 16 lanes that share an LDS cycle hit 16 different bank quads in every step.  Packed: at most 2 lanes on a quad,
and a zero-row read shares none."""
import numpy as np
import pytest
import torch

# lane sets that share one LDS cycle of ds_read_b128 (MI355X_MICROARCH.md, LDS table)
HW_GROUPS = [
    [0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27],
    [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
    [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59],
    [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63],
]


def slot_of(j, pw, PW):
    """The slot that (panel, wave) pair `pw` takes in round j: the rounds are dealt back and forth over the PW pairs."""
    return j * PW + ((PW - 1 - pw) if (j & 1) else pw)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need the MI355X"
    return torch.device("cuda:0")


def _switches(monkeypatch):
    from difformer_amd import ops

    def set_(schedule=None, slots=None, positions=None):
        for name, v in (("DIFFORMER_SLICED_SCHEDULE", schedule), ("DIFFORMER_SLICED_SLOTS", slots),
                        ("DIFFORMER_SLICED_POSITIONS", positions)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
        ops.csr_cache.clear()
    yield set_
    ops.csr_cache.clear()


@pytest.fixture
def env(monkeypatch):
    """env(schedule=None, slots=None, positions=None): the three switches of the format (None = unset), on a cold CSR cache."""
    yield from _switches(monkeypatch)


@pytest.fixture
def schedule(monkeypatch):
    """schedule(mode): `env` under the name of the one switch most tests force."""
    yield from _switches(monkeypatch)


def dense_graph(n, deg, seed, self_loops=True, duplicates=True):
    g = torch.Generator().manual_seed(seed)
    e = n * deg
    ei = torch.randint(0, n, (2, e), generator=g)
    if duplicates:
        ei[:, : e // 50] = ei[:, e // 50: 2 * (e // 50)]         # repeated edges must be summed twice
    if self_loops:
        ei = torch.cat([ei, torch.arange(n).repeat(2, 1)], dim=1)
    return ei


def skewed_graph(n, deg, seed, hubs=40, base=None):
    """Half of the entries land on `hubs` destination rows (max degree ~ n * deg / (2 * hubs) >> mean)."""
    ei = dense_graph(n, deg, seed) if base is None else base
    g = torch.Generator().manual_seed(seed + 1)
    half = ei.shape[1] // 2
    ei[1, :half] = torch.randint(0, hubs, (half,), generator=g) * (n // hubs)
    return ei


def ragged_graph(n, lo, hi, seed, orphan=None):
    """Every node receives lo..hi entries from random sources (repeats included) and its self loop; `orphan` receives
    nothing at all (no self loop either), so its degree is 0."""
    g = torch.Generator().manual_seed(seed)
    deg = torch.randint(lo, hi + 1, (n,), generator=g)
    if orphan is not None:
        deg[orphan] = 0
    dst = torch.repeat_interleave(torch.arange(n), deg)
    src = torch.randint(0, n, (dst.numel(),), generator=g)
    loops = torch.arange(n)
    if orphan is not None:
        loops = loops[loops != orphan]
    return torch.stack([torch.cat([src, loops]), torch.cat([dst, loops])])


def records(sl):
    """The records in front of sl.entries -> (row int32 [G * 64], scale float32 [G * 64])."""
    G = int(sl.plan[2])
    off = sl.entries.storage_offset()
    assert off >= G * 256
    raw = torch.empty(0, dtype=torch.int16, device=sl.entries.device).set_(sl.entries.untyped_storage(), off - G * 256, (G * 256,))
    rec = raw.view(torch.int32).view(G * 64, 2)
    return rec[:, 0].clone(), rec[:, 1].clone().view(torch.float32)


def check_format(sl, ei, n, csr):
    """Decodes `sl` (device or host copies of entries and table) against the CSR and the edge list it was built from;
    -> the number of (block, step, lane group, quad) cells that two lanes share (0 under the strict schedule)."""
    slices, panels, G, PW, W, R, T, NT = (int(v) for v in sl.plan)
    n_pos = n if sl.n_pos is None else int(sl.n_pos)
    assert NT == csr.n_blocks and T % 16 == 0 and PW == panels * W and G == -(-n_pos // 64) and (R - 1) * PW < G <= R * PW
    order = np.arange(n) if sl.order is None else sl.order.cpu().numpy().astype(np.int64)
    assert order.size == n_pos
    if sl.parts is None:
        part, nparts = np.zeros(n_pos, np.int64), np.ones(n_pos, np.int64)
        assert np.array_equal(np.sort(order), np.arange(n)), "order is a permutation of the rows"
    else:
        pp = sl.parts.cpu().numpy().view(np.uint16).astype(np.int64)
        part, nparts = pp & 0xFF, pp >> 8
        live = order >= 0
        assert np.array_equal(np.sort(order[live & (part == 0)]), np.arange(n)), "every row has exactly one part 0"
        assert np.all((nparts >= 1) & (nparts <= 64) & (part < nparts))
        # the parts of a row: consecutive positions of one slot, in part order
        heads = np.nonzero(live & (part == 0))[0]
        for h in heads[nparts[heads] > 1]:
            P = nparts[h]
            assert h // 64 == (h + P - 1) // 64 and np.all(order[h:h + P] == order[h]) and np.array_equal(part[h:h + P], np.arange(P))
            assert np.all(nparts[h:h + P] == P)
        assert int(nparts[heads].sum()) == int(live.sum())
    table = sl.table.cpu().numpy()
    n_ptw = panels * NT * W
    n_blocks = int(table[-1])
    rows = table[:-1].reshape(n_ptw, R + 1)
    ent = sl.entries.cpu().numpy().view(np.uint16).reshape(-1, 64, 8)[:n_blocks]
    assert ent.max() < T + 16
    quads = (ent & 15).transpose(0, 2, 1).astype(np.int64)       # [block, step, lane]
    zero = (ent >= T).transpose(0, 2, 1)
    assert sl.quad_cap in (1, 2)
    shared = 0
    for grp in HW_GROUPS:
        q = quads[:, :, grp]
        if sl.quad_cap == 1:
            # every step of every block: the 16 lanes of a hardware group read 16 different bank quads
            q = np.sort(q, axis=2)
            assert np.array_equal(q, np.broadcast_to(np.arange(16), q.shape)), "bank conflict in the schedule"
            continue
        # every step of every block: a hardware lane group puts at most 2 lanes on a bank quad; a zero-row read shares none
        per_quad = (q[..., None] == np.arange(16)).sum(axis=2)   # [block, step, quad]
        assert per_quad.max() <= 2, "more than two lanes of a lane group on one bank quad"
        own = np.take_along_axis(per_quad, q, axis=2)            # lanes on the quad each lane reads
        assert np.all(own[zero[:, :, grp]] == 1), "a zero-row read shares its bank quad"
        shared += int((per_quad == 2).sum())
    # the real entries of (row position, tile) == its share of the CSR group
    src, dst = ei[0].numpy(), ei[1].numpy()
    perm = np.lexsort((src, dst))
    src_s, dst_s = src[perm], dst[perm]
    rowptr = np.searchsorted(dst_s, np.arange(n + 1))
    assert np.array_equal(rowptr, csr.rowptr.cpu().numpy())
    if sl.quad_cap == 1 and sl.order is not None and sl.parts is None:
        deg = np.diff(rowptr)[order]
        assert np.all(deg[:-1] >= deg[1:]), "slots are formed in descending-degree order"
    # a part takes its share of the group in CSR order (entries of a (row, tile) group are filed by edge id)
    csr_src = csr.src.cpu().numpy().astype(np.int64)
    blkptr = csr.blkptr.cpu().numpy().reshape(NT + 1, n) if NT > 1 else None
    total_real, expect_start, seen_slots = 0, 0, 0
    for p in range(panels):
        for t in range(NT):
            for w in range(W):
                start, nb = int(rows[(p * NT + t) * W + w, 0]), rows[(p * NT + t) * W + w, 1:].astype(np.int64)
                assert start == expect_start and np.all(nb[:-1] >= nb[1:]), "round lengths must not increase"
                expect_start += int(nb.sum())
                for j in range(R):
                    g = slot_of(j, w * panels + p, PW)
                    if g >= G:
                        assert nb[j] == 0
                        continue
                    seen_slots += (t == 0)
                    blocks = [start + int(np.minimum(nb, k).sum()) + j for k in range(int(nb[j]))]
                    lists = ent[blocks].transpose(1, 0, 2).reshape(64, -1) if blocks else np.zeros((64, 0), np.uint16)
                    for lane in range(64):
                        pos = g * 64 + lane
                        got = np.sort(lists[lane][lists[lane] < T].astype(np.int64))
                        if pos >= n_pos or order[pos] < 0:
                            assert got.size == 0
                            continue
                        row = order[pos]
                        seg = src_s[rowptr[row]: rowptr[row + 1]]
                        e0, e1 = (rowptr[row], rowptr[row + 1]) if NT == 1 else (blkptr[t, row], blkptr[t + 1, row])
                        grp_e = csr_src[e0:e1] - t * T
                        assert np.array_equal(np.sort(grp_e), seg[(seg >= t * T) & (seg < (t + 1) * T)] - t * T)
                        c = grp_e.size
                        want = np.sort(grp_e[c * part[pos] // nparts[pos]: c * (part[pos] + 1) // nparts[pos]])
                        assert np.array_equal(got, want), (p, t, w, j, lane)
                        total_real += got.size
    assert expect_start == n_blocks and seen_slots == G and total_real == ei.shape[1]
    return shared


def product_vs_oracle(mode, dev, schedule):
    """Forward, adjoint and both ranks of a 2-way row shard under DIFFORMER_SLICED_SCHEDULE = mode, against the float64 oracle
    at 1e-5 (the bound of test_gpu_sliced.py); two products and two builds bit-identical."""
    from conftest import rel_err
    from oracle import difformer_oracle as orc
    from difformer_amd import gcn_conv, ops
    from difformer_amd.dist import RowShard
    schedule(mode)
    cap = 2 if mode == "packed" else 1
    n, deg, d = 50000, 60, 64
    ei = dense_graph(n, deg, seed=3 * n + d)
    # out-degrees != in-degrees, both near-uniform (the first half of the nodes sends ~2 more entries each)
    ei[0, : n] = torch.randint(0, n // 2, (n,), generator=torch.Generator().manual_seed(3))
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, 1, d, generator=g)
    gout = torch.randn(n, 1, d, generator=g)
    eid = ei.to(dev)
    xd = x.to(dev).requires_grad_(True)
    csr = ops.csr_cache.get(eid, None, n, d * 4)
    assert csr.sliced(0, n, d).quad_cap == cap
    out = gcn_conv(xd, eid, None)
    ref = orc.gcn_conv(x.double().numpy(), ei.numpy(), None)
    assert rel_err(out.detach().cpu().numpy(), ref) < 1e-5
    assert torch.equal(gcn_conv(xd, eid, None), out)                                           # deterministic
    out.backward(gout.to(dev))
    adj = csr.adjoint()
    assert adj.sliced(0, n, d) is not None and adj.sliced(0, n, d).quad_cap == cap
    row, col = ei[0].numpy(), ei[1].numpy()                       # difformer.py:63-75 in float64
    degs = np.bincount(col, minlength=n).astype(np.float64)
    dinv = np.where(degs > 0, 1.0 / np.sqrt(np.maximum(degs, 1)), 0.0)
    want = np.zeros((n, d))
    np.add.at(want, row, (dinv[col] * dinv[row])[:, None] * gout[:, 0, :].double().numpy()[col])
    assert rel_err(xd.grad[:, 0, :].cpu().numpy(), want) < 1e-5
    # a 2-way row shard: each rank's rows through the same builder and the same rule
    be = ops.get_backend()
    x2 = x[:, 0, :].to(dev).contiguous()
    for rank in (0, 1):
        sh = RowShard(n, rank=rank, world=2)
        lo, cnt = sh.row_begin, sh.n_local
        scsr = ops.csr_cache.get(eid, None, n, d * 4, sh)
        sl = scsr.sliced(lo, cnt, d)
        assert sl is not None and sl.quad_cap == cap
        ys = be.sliced_prescale(x2, scsr.rowptr, n, sl.plan)
        got = be.sliced_spmm(sl, ys, scsr.rowptr, n, lo, cnt, d)
        assert rel_err(got.cpu().numpy(), ref[lo: lo + cnt, 0, :]) < 1e-5, rank
        assert torch.equal(be.sliced_spmm(sl, ys, scsr.rowptr, n, lo, cnt, d), got)
        again = scsr._build_sliced(lo, cnt, d)
        assert torch.equal(again.entries, sl.entries) and torch.equal(again.table, sl.table)


def headline_stats(sl, csr, n, dev):
    """-> (built blocks, row-envelope prediction in blocks, shared cells, their minimum for this build)"""
    slices, panels, G, PW, W, R, T, NT = (int(v) for v in sl.plan)
    order = sl.order.long()
    cnt = csr.blkptr.view(NT + 1, n)
    cnt = (cnt[1:] - cnt[:-1]).t().contiguous()                                   # [row, tile]
    o = torch.full((G * 64,), -1, dtype=torch.int64, device=dev)
    o[:n] = order
    c = torch.where(o[:, None] >= 0, cnt[o.clamp(min=0)], torch.zeros_like(cnt[:1])).view(G, 64, NT)
    nb = (c.max(dim=1).values + 7) // 8
    j = torch.arange(R, device=dev)[:, None]
    pw = torch.arange(PW, device=dev)[None, :]
    s = j * PW + torch.where(j % 2 == 1, PW - 1 - pw, pw)
    r = torch.where((s < G)[..., None], nb[s.clamp(max=G - 1)], torch.zeros_like(nb[:1]))
    predicted = int(torch.flip(torch.cummax(torch.flip(r, [0]), 0).values, [0]).sum())
    n_blocks = int(sl.table[-1])
    # shared cells of the built format: per (block, step, lane group) the lanes beyond the first on a quad, real reads only
    ent = sl.entries[: n_blocks * 512].view(n_blocks, 64, 8).to(torch.int32) & 0xFFFF
    groups = torch.tensor(HW_GROUPS, device=dev)
    shared = 0
    for b0 in range(0, n_blocks, 16384):
        e = ent[b0: b0 + 16384][:, groups, :]                                      # [block, group, 16 lanes, step]
        q = torch.where(e < T, e & 15, 16 + torch.arange(16, device=dev)[None, None, :, None])      # zero rows never match
        qs = torch.sort(q, dim=2).values
        shared += int((qs[:, :, 1:, :] == qs[:, :, :-1, :]).sum())
    # minimum: columns of every (slot, tile, lane group) against the built length of the round
    rows = sl.table[:-1].view(panels * NT * W, R + 1).long()
    g = torch.arange(G, device=dev)
    jj, idx = g // PW, g % PW
    pwg = torch.where(jj % 2 == 1, PW - 1 - idx, idx)
    p, w = pwg % panels, pwg // panels
    t = torch.arange(NT, device=dev)
    K = 8 * rows[(p[:, None] * NT + t[None, :]) * W + w[:, None], 1 + jj[:, None]]          # [slot, tile] steps
    inv = torch.empty(n, dtype=torch.int64, device=dev)
    inv[order] = torch.arange(n, device=dev)
    group_of = torch.empty(64, dtype=torch.int64, device=dev)
    group_of[groups.flatten()] = torch.arange(64, device=dev) // 16
    dst = torch.repeat_interleave(torch.arange(n, device=dev), (csr.rowptr[1:] - csr.rowptr[:-1]).long())
    pos = inv[dst]
    srcl = csr.src.long()
    key = (((pos // 64) * NT + srcl // T) * 4 + group_of[pos % 64]) * 16 + (srcl % T) % 16
    col = torch.bincount(key, minlength=G * NT * 64).view(G, NT, 4, 16)
    minimum = int((col - K[:, :, None, None]).clamp(min=0).sum())
    return n_blocks, predicted, shared, minimum
