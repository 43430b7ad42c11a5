"""The device-side slot order of the packed schedule (csrc/sliced_slots.hip, include/difformer_slots.h).

`dealt_order` below restates stages a-d of the header in numpy with the same tie rules; the device order must equal it
entry for entry.  The restatement alone is checked on the CPU (it places every row once, and twice the same); the GPU
tests hold the call to it, to the permutation property at every geometry edge (one tile, rows that do not fill the last
slot, a last round that is partly empty, a row shard), to the guards of tests/test_gpu_sliced_packed.py on the built
format, and the products under it to the float64 oracle at the packed tests' 1e-5.
"""
import numpy as np
import pytest
import torch

from sliced_format import dense_graph, dev, env, headline_stats, product_vs_oracle, ragged_graph, slot_of  # noqa: F401  (dev, env: fixtures)

WINDOW = 1024
MAX_BLOCKS = 4095


# ---- the restatement ------------------------------------------------------------------------------------------------
def block_vectors(rowptr, blkptr, n_src, NT, row_begin, n_rows):
    """a. b[row][tile] = min((entries + 7) // 8, 4095)"""
    if NT > 1:
        cnt = blkptr.reshape(NT + 1, n_src)[:, row_begin: row_begin + n_rows].astype(np.int64)
        b = ((cnt[1:] - cnt[:-1] + 7) // 8).T.copy()
    else:
        rp = rowptr.astype(np.int64)
        b = ((rp[row_begin + 1: row_begin + n_rows + 1] - rp[row_begin: row_begin + n_rows] + 7) // 8)[:, None]
    return np.minimum(b, MAX_BLOCKS)


def profile_order(b):
    """a. rows by the largest count descending, then the set of tiles that reach it, stable"""
    NT = b.shape[1]
    top = b.max(axis=1)
    hot = ((b == top[:, None]) * (1 << np.arange(NT, dtype=np.int64))[None, :]).sum(axis=1)
    return np.argsort((MAX_BLOCKS - top) * (1 << NT) + hot, kind="stable")


def greedy_slots(b, srt):
    """b. -> the rows, 64 per slot in pick order, window by window"""
    n = b.shape[0]
    tot = b.sum(axis=1)
    out = np.empty(n, dtype=np.int64)
    o = 0
    for w0 in range(0, n, WINDOW):
        rows = srt[w0: w0 + WINDOW]
        bw, tw = b[rows], tot[rows]
        alive = np.ones(len(rows), dtype=bool)
        left = len(rows)
        while left:
            k = min(64, left)
            cand = np.flatnonzero(alive)
            i = cand[np.lexsort((rows[cand], -tw[cand]))[0]]              # seed: largest total, then lower row
            m = bw[i].copy()
            alive[i] = False
            out[o] = rows[i]
            o += 1
            for _ in range(k - 1):
                cand = np.flatnonzero(alive)
                cost = np.maximum(bw[cand] - m[None, :], 0).sum(axis=1)
                i = cand[np.lexsort((rows[cand], -tw[cand], cost))[0]]    # least raise, larger total, lower row
                np.maximum(m, bw[i], out=m)
                alive[i] = False
                out[o] = rows[i]
                o += 1
            left -= k
    return out


def deal(b, slotrows, PW, R):
    """c. -> src[position] = the formed slot dealt to that slot position"""
    n, NT = b.shape
    G = (n + 63) // 64
    M = np.stack([b[slotrows[g * 64: (g + 1) * 64]].max(axis=0) for g in range(G)])
    partial = n % 64 != 0
    last = np.zeros(G, dtype=np.int64)
    last[G - 1] = int(partial)
    srt = np.lexsort((np.arange(G), -M.sum(axis=1), last))               # partial slot last, total descending, slot id
    env = np.zeros((PW, NT), dtype=np.int64)
    src = np.full(G, -1, dtype=np.int64)
    for j in range(R - 1, -1, -1):
        stratum = srt[j * PW: min((j + 1) * PW, G)]
        free = np.ones(len(stratum), dtype=bool)
        pairs = [pw for pw in range(PW) if slot_of(j, pw, PW) < G]
        assert len(pairs) == len(stratum)
        if j == R - 1 and partial:
            pstar = next(pw for pw in pairs if slot_of(j, pw, PW) == G - 1)
            assert stratum[-1] == G - 1
            free[-1] = False
            src[G - 1] = G - 1
            env[pstar] = np.maximum(env[pstar], M[G - 1])
            pairs.remove(pstar)
        et = env.sum(axis=1)
        pairs.sort(key=lambda p: (-et[p], p))
        Ms = M[stratum]
        for p in pairs:
            cand = np.flatnonzero(free)
            i = cand[np.argmin(np.maximum(Ms[cand] - env[p][None, :], 0).sum(axis=1))]     # first minimum of the stratum
            free[i] = False
            src[slot_of(j, p, PW)] = stratum[i]
            np.maximum(env[p], Ms[i], out=env[p])
    return src


def emit(slotrows, src):
    """d."""
    out = np.empty(len(slotrows), dtype=np.int64)
    for g, s in enumerate(src):
        chunk = slotrows[s * 64: (s + 1) * 64]
        out[g * 64: g * 64 + len(chunk)] = chunk
    return out


def dealt_order(b, PW, R):
    slotrows = greedy_slots(b, profile_order(b))
    return emit(slotrows, deal(b, slotrows, PW, R))


def envelope_blocks(b, order, PW, R):
    """blocks the table kernel stores for `order` if the quad columns do not bind: per (pair, tile) the slot maxima, padded
    to a non-increasing sequence over the rounds"""
    n, NT = b.shape
    G = (n + 63) // 64
    M = np.stack([b[order[g * 64: (g + 1) * 64]].max(axis=0) for g in range(G)])
    total = 0
    for pw in range(PW):
        env = np.zeros(NT, dtype=np.int64)
        for j in range(R - 1, -1, -1):
            g = slot_of(j, pw, PW)
            if g < G:
                env = np.maximum(env, M[g])
            total += int(env.sum())
    return total


# ---- CPU: the restatement alone -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,NT,PW,R", [(8205, 1, 80, 2), (5000, 4, 32, 3), (4096, 3, 64, 1), (3001, 5, 16, 3)])
def test_restatement_places_every_row_once_and_repeats_itself(n, NT, PW, R):
    rng = np.random.default_rng(n + NT)
    b = (rng.poisson(52.0 / NT * 4, size=(n, NT)) + 7) // 8
    G = (n + 63) // 64
    assert (R - 1) * PW < G <= R * PW
    order = dealt_order(b, PW, R)
    assert np.array_equal(np.sort(order), np.arange(n)), "every row exactly once"
    assert np.array_equal(order, dealt_order(b.copy(), PW, R)), "deterministic"
    if n % 64:
        tail = order[(G - 1) * 64:]
        slotrows = greedy_slots(b, profile_order(b))
        assert np.array_equal(tail, slotrows[(G - 1) * 64:]), "the partial slot keeps the last slot position"
    # the deal moves whole slots: every 64-row chunk of the order is a chunk of the greedy list
    slotrows = greedy_slots(b, profile_order(b))
    chunks = {tuple(slotrows[g * 64: (g + 1) * 64]) for g in range(G)}
    assert all(tuple(order[g * 64: (g + 1) * 64]) in chunks for g in range(G))


def test_restatement_pads_less_than_the_profile_order_on_poisson_rows():
    """Poisson (row, tile) counts at a scaled-down headline geometry: 13 tiles, 9 rounds.  The profile order dealt in order
    is what sliced.packed_slot_order gives; the dealt order must store clearly fewer blocks (the model of the headline graph:
    1.247 -> 1.198 lane-steps per entry)."""
    rng = np.random.default_rng(0)
    n, NT, PW, R = 64 * 9 * 24, 13, 24, 9
    cnt = rng.poisson(46.0, size=(n, NT))
    b = (cnt + 7) // 8
    profile = envelope_blocks(b, profile_order(b), PW, R)
    dealt = envelope_blocks(b, dealt_order(b, PW, R), PW, R)
    print(f"lane-steps per entry: profile {profile * 512 / cnt.sum():.4f}, dealt {dealt * 512 / cnt.sum():.4f}")
    assert dealt < 0.98 * profile


def test_slots_switch_rejects_unknown_values(monkeypatch):
    from difformer_amd import sliced
    monkeypatch.setenv("DIFFORMER_SLICED_SLOTS", "best")
    with pytest.raises(ValueError):
        sliced.sliced_slots()
    monkeypatch.setenv("DIFFORMER_SLICED_SLOTS", "profile")
    assert sliced.sliced_slots() == "profile"
    monkeypatch.delenv("DIFFORMER_SLICED_SLOTS")
    assert sliced.sliced_slots() == "dealt"


# ---- GPU ------------------------------------------------------------------------------------------------------------
def _graph(name):
    if name == "one_tile":
        return 8205, ragged_graph(8205, 47, 59, seed=1)        # 48-60 entries with the self loop
    if name == "four_tiles":
        return 40000, dense_graph(40000, 60, seed=7)
    return 84000, dense_graph(84000, 48, seed=84000 + 64)      # the graph of test_gpu_sliced_packed.py


def _device_order(be, csr, n, lo, cnt, F=64):
    plan = be.sliced_plan(n, cnt, F)
    order = be.sliced_slot_order(csr.rowptr, csr.blkptr, n, lo, cnt, plan)
    assert order is not None and order.dtype == torch.int32 and order.shape == (cnt,)
    return plan, order


def _restated(csr, n, lo, cnt, plan):
    PW, R, NT = int(plan[3]), int(plan[5]), int(plan[7])
    blkptr = csr.blkptr.cpu().numpy() if NT > 1 else None
    b = block_vectors(csr.rowptr.cpu().numpy(), blkptr, n, NT, lo, cnt)
    return b, dealt_order(b, PW, R)


@pytest.mark.gpu
@pytest.mark.parametrize("name,world", [("one_tile", 1), ("four_tiles", 1), ("nine_tiles", 1), ("four_tiles", 2)])
def test_order_is_a_permutation_and_repeats_bit_for_bit(name, world, dev, env):
    from difformer_amd import ops
    from difformer_amd.dist import RowShard
    env("packed")
    n, ei = _graph(name)
    be = ops.get_backend()
    eid = ei.to(dev)
    seen = set()
    for rank in range(world):
        sh = RowShard(n, rank=rank, world=world) if world > 1 else None
        lo, cnt = (sh.row_begin, sh.n_local) if sh else (0, n)
        csr = ops.csr_cache.get(eid, None, n, 256, sh) if sh else ops.csr_cache.get(eid, None, n, 256)
        plan, order = _device_order(be, csr, n, lo, cnt)
        G, PW, R, NT = int(plan[2]), int(plan[3]), int(plan[5]), int(plan[7])
        seen.add((NT, R, cnt % 64 != 0, G % PW != 0, lo > 0))
        got = order.cpu().numpy().astype(np.int64)
        assert np.array_equal(np.sort(got), np.arange(cnt)), "order is a permutation of the shard's rows"
        assert torch.equal(be.sliced_slot_order(csr.rowptr, csr.blkptr, n, lo, cnt, plan), order), "two calls, identical bytes"
    # the geometry this case is here for
    if name == "one_tile":
        assert all(s[0] == 1 and s[2] and s[3] for s in seen), seen     # 1 tile, rows % 64 != 0, last round partly empty
    if name == "four_tiles" and world == 1:
        assert all(s[0] == 4 and s[1] == 3 for s in seen), seen
    if name == "nine_tiles":
        assert all(s[0] == 9 and s[2] for s in seen), seen
    if world == 2:
        assert any(s[4] for s in seen), seen


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["one_tile", "four_tiles"])
def test_device_order_equals_the_restatement(name, dev, env):
    from difformer_amd import ops
    env("packed")
    n, ei = _graph(name)
    be = ops.get_backend()
    csr = ops.csr_cache.get(ei.to(dev), None, n, 256)
    plan, order = _device_order(be, csr, n, 0, n)
    _, want = _restated(csr, n, 0, n, plan)
    got = order.cpu().numpy().astype(np.int64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} of {n} entries differ, first at {bad[:1]}: {got[bad[:4]]} vs {want[bad[:4]]}"


@pytest.mark.gpu
def test_built_format_under_dealt_against_profile_and_the_packed_guards(dev, env):
    """84,000 rows, 9 tiles.  The guards are those of test_gpu_sliced_packed.py's headline test."""
    from difformer_amd import ops, sliced
    n, ei = _graph("nine_tiles")
    eid = ei.to(dev)
    blocks = {}
    for slots in ("profile", "dealt"):
        env("packed", slots)
        csr = ops.csr_cache.get(eid, None, n, 256)
        sl = csr.sliced(0, n, 64)
        assert sl is not None and sl.quad_cap == 2 and sl.order is not None
        built, predicted, shared, minimum = headline_stats(sl, csr, n, dev)
        print(f"{slots}: built {built} blocks ({built * 512 / csr.nnz:.4f} lane-steps per entry), row envelope {predicted}, "
              f"shared cells {shared}, minimum {minimum}")
        blocks[slots] = built
        if slots == "profile":
            assert torch.equal(sl.order, sliced.packed_slot_order(csr.rowptr, csr.blkptr, n, int(sl.plan[7]), 0, n))
        else:
            assert built <= 1.05 * predicted
            assert shared <= 2 * minimum
    assert blocks["dealt"] <= blocks["profile"]


@pytest.mark.gpu
def test_profile_reproduces_the_order_and_format_of_packed_slot_order(dev, env):
    """DIFFORMER_SLICED_SLOTS=profile is the format from before the device-side order, bit for bit: the same order, and the
    builder called with it directly gives the same entries and table."""
    from difformer_amd import ops, sliced
    env("packed", "profile")
    n, ei = _graph("four_tiles")
    csr = ops.csr_cache.get(ei.to(dev), None, n, 256)
    sl = csr.sliced(0, n, 64)
    be = ops.get_backend()
    plan = be.sliced_plan(n, n, 64)
    order = sliced.packed_slot_order(csr.rowptr, csr.blkptr, n, int(plan[7]), 0, n)
    entries, table = be.sliced_build(csr.rowptr, csr.blkptr, csr.src, n, csr.nnz, 0, n, 64, plan, order, None, None, 2)
    assert torch.equal(sl.order, order) and torch.equal(sl.entries, entries) and torch.equal(sl.table, table)


@pytest.mark.gpu
def test_products_under_dealt_vs_oracle_forward_adjoint_and_row_shard(dev, env):
    """The packed tests' product check (forward, adjoint, 2-way shard at 1e-5 of the float64 oracle; two products and two
    builds bit-identical) with the dealt order asked for by name, and the order really the device's."""
    from difformer_amd import ops, sliced
    env("packed", "dealt")
    product_vs_oracle("packed", dev, lambda mode: env(mode, "dealt"))
    env("packed", "dealt")
    n, ei = _graph("four_tiles")
    csr = ops.csr_cache.get(ei.to(dev), None, n, 256)
    sl = csr.sliced(0, n, 64)
    assert not torch.equal(sl.order, sliced.packed_slot_order(csr.rowptr, csr.blkptr, n, int(sl.plan[7]), 0, n))
    again = csr._build_sliced(0, n, 64)
    assert torch.equal(again.order, sl.order) and torch.equal(again.entries, sl.entries) and torch.equal(again.table, sl.table)


@pytest.mark.gpu
@pytest.mark.parametrize("name,world", [("one_tile", 1), ("four_tiles", 2)])
def test_slot_order_between_guard_bands(name, world, dev, env, monkeypatch):
    """`order` and the workspace poisoned and between guard bands (tests/guarded.py): nothing is written outside them, and
    nothing the result depends on is read from what they held before."""
    import guarded
    from difformer_amd import ops
    from difformer_amd.dist import RowShard
    env("packed")
    n, ei = _graph(name)
    be = ops.get_backend()
    eid = ei.to(dev)
    sh = RowShard(n, rank=world - 1, world=world) if world > 1 else None
    lo, cnt = (sh.row_begin, sh.n_local) if sh else (0, n)
    csr = ops.csr_cache.get(eid, None, n, 256, sh) if sh else ops.csr_cache.get(eid, None, n, 256)
    plan, plain = _device_order(be, csr, n, lo, cnt)
    arena = guarded.install(monkeypatch)
    _, order = _device_order(be, csr, n, lo, cnt)
    handed_out = len(arena.blocks)
    arena.check()
    assert handed_out >= 2 and torch.equal(order, plain), "order and workspace came from the arena"
